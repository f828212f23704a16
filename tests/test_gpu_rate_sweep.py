"""Seeded sweep of the frequency-translating decimators, the rational resamplers and the frequency-translating interpolators on the
GPU (tests/rate_cases.py: "translate", "rational", "translate_tx"), as tests/test_gpu_band_sweep.py sweeps the six band kinds: any
legal tap count, ratio, mixer, channel count, format, call split, kernel request, placement of input and output and START POSITION
in the 64-bit stream must give the bits of the float32 reference of the whole stream, move the plan's position by the arithmetic,
take the kernel the headers say, refuse what they say is refused, and write nothing but the call's outputs.  The translating
interpolators' S32 plans store convert_tx wire words under a keying threshold that leaves both keying states in the reference."""
import numpy as np
import pytest

import sxxcvr_amd
import rate_cases as rc
from band_cases import AUTO, GUARD, TILED
from gpu_util import OUT_FILL, assert_bit_exact, to_cpu, to_gpu
from rate_cases import KINDS, SWEEP_COUNT, SWEEP_SEED

pytestmark = pytest.mark.gpu

FILL = np.uint32(OUT_FILL)
SWEEP = [pytest.param(k, c, id="%s-%s" % (k, c.ident)) for k in KINDS if k != "bank"         # (tests/test_gpu_bank_sweep.py: K x nchan rows per call)
         for c in rc.cases(k, SWEEP_SEED, SWEEP_COUNT)]


@pytest.mark.parametrize("kind,case", SWEEP)
def test_rate_sweep(oracle, kind, case):
    import torch
    K = KINDS[kind]
    nchan = case.nchan
    h = rc.taps_of(kind, case)
    raw, xs = rc.stream_input(kind, case, oracle)
    refs = [rc.reference(kind, oracle, case, h, xs[c]) for c in range(nchan)]
    plan = rc.make_plan(kind, case, h)
    assert tuple(plan.contract) == tuple(rc.contract(kind, case)) and plan.contract.rot == 0
    if kind != "rational":
        assert (plan.num, plan.den) == (case.num % case.den, case.den)
    thr2 = None
    if case.fmt == "S32" and K.tx:
        # wire words out: a threshold with outputs on both sides of the keying rule
        thr2 = rc.keying_threshold(refs[0])
        plan.set_tx_threshold(float(thr2))
    want = [rc.stored_words(oracle, case.fmt, r, thr2) for r in refs]
    if thr2 is not None:
        keyed = (np.concatenate(want).view(np.int32)[:, 0] & 3) == 3
        assert 0 < keyed.sum() < keyed.size, (case.ident, int(keyed.sum()), keyed.size)
    wi, wo = raw.shape[-1], want[0].shape[-1]              # 32-bit words per input / output sample
    stream = torch.cuda.current_stream().cuda_stream
    lead = rc.lead_of(case)
    pos_in, pos_out = case.c0, rc.outputs_for(case, 0, case.c0)
    if case.place != "start":
        # the samples in front of the stream become the plan's history, then the plan is placed
        lg = to_gpu(np.ascontiguousarray(raw[:, :lead]))
        plan.set_history_ptr(lg.data_ptr(), lead, lead, stream)
        plan.set_position(case.c0)
        torch.cuda.synchronize()
    assert plan.position == (pos_in, pos_out), case.ident
    got = [[] for _ in range(nchan)]
    at_data = lead
    for i, call in enumerate(case.calls):
        n = call.n
        n_out = rc.outputs_for(case, pos_in, n)
        what = "%s call %d %r" % (case.ident, i, call)
        # the input: a view `skew` samples into a buffer of fill, rows at the call's stride
        at_in = [call.skew + c * call.in_stride for c in range(nchan)]
        xin = np.full((at_in[-1] + n + 3, wi), FILL, dtype=np.uint32)
        for c, at in enumerate(at_in):
            xin[at:at + n] = raw[c, at_data:at_data + n].view(np.uint32)
        xg = to_gpu(xin.view(np.int32))
        # the output: larger than needed, prefilled, the first output GUARD + out_off samples in
        at_out = [GUARD + call.out_off + c * call.out_stride for c in range(nchan)]
        yg = torch.full((at_out[-1] + n_out + 5, wo), int(FILL), dtype=torch.int32, device="cuda")
        assert xg.data_ptr() % 16 == 0 and yg.data_ptr() % 16 == 0
        in_ptr = xg.data_ptr() + 4 * wi * call.skew
        out_ptr = yg.data_ptr() + 4 * wo * (GUARD + call.out_off)
        assert plan.outputs_for(n) == n_out, what
        label = rc.expected_kernel(kind, case, i)
        request = call.request
        if label == "refused":
            if rc.has_form(kind, case):
                plan.set_kernel(TILED)
                asked = rc.expected_kernel(kind, case, i, assume_aligned=True)
                assert plan.geometry(n)["kernel"] == (K.tiled if asked == "tiled" else K.generic), what
                with pytest.raises(sxxcvr_amd.NativeError) as ei:
                    plan.process_ptr(in_ptr, n, call.in_stride, out_ptr, call.out_stride, stream)
            else:
                with pytest.raises(sxxcvr_amd.NativeError) as ei:          # no tiled kernel for the shape or format at all
                    plan.set_kernel(TILED)
            assert ei.value.code == -4, what
            assert plan.position == (pos_in, pos_out), what
            torch.cuda.synchronize()
            assert int((yg != int(FILL)).sum()) == 0, "a refused call wrote something: " + what
            request = AUTO
        plan.set_kernel(request)
        label = rc.expected_kernel(kind, case, i, request=request)
        assert label in ("tiled", "generic", "history only"), what
        if n_out > 0:
            asked = rc.expected_kernel(kind, case, i, request=request, assume_aligned=True)
            g = plan.geometry(n)
            assert g["kernel"] == (K.tiled if asked == "tiled" else K.generic) and g["tiled"] == (asked == "tiled"), (what, g)
        assert plan.process_ptr(in_ptr, n, call.in_stride, out_ptr, call.out_stride, stream) == n_out, what
        pos_in += n
        pos_out += n_out
        at_data += n
        assert plan.position == (pos_in, pos_out), what
        torch.cuda.synchronize()
        y = to_cpu(yg).view(np.uint32)
        written = np.zeros(y.shape[0], dtype=bool)
        for c, at in enumerate(at_out):
            got[c].append(y[at:at + n_out].copy())
            written[at:at + n_out] = True
        assert np.all(y[~written] == FILL), "something outside the call's outputs was written (%s): sample %d of the buffer, the first " \
            "output at %d" % (what, int(np.nonzero((y != FILL).any(axis=1) & ~written)[0][0]), GUARD + call.out_off)
    assert at_data == xs.shape[-1]
    for c in range(nchan):
        g, w = np.concatenate(got[c]), want[c]
        where = "%s channel %d" % (case.ident, c)
        assert g.shape == w.shape, (where, g.shape, w.shape)
        if wo == 2 and thr2 is None:
            assert_bit_exact(g.view(np.complex64).ravel(), w.view(np.complex64).ravel(), where)
        else:                                               # CF16: the half words; S32 out: the wire words
            bad = np.nonzero((g != w).any(axis=1))[0]
            assert bad.size == 0, "%s: %d of %d outputs differ, first at %d: got %r want %r" % (where, bad.size, g.shape[0], bad[0], g[bad[0]], w[bad[0]])
    plan.close()
