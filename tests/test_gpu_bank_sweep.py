"""Seeded sweep of the tuner banks on the GPU (tests/rate_cases.py: "bank"), as tests/test_gpu_rate_sweep.py sweeps the translating
decimators a bank is made of: any legal tap count, ratio, band count, centres, channel count, format, call split, kernel request,
placement of the input, layout of the output -- bands inside channels or channels inside bands, drawn per call -- and START
POSITION in the 64-bit stream must give, per band and channel, the bits of the float32 reference of the whole stream
(bank_cases.bank_ref through rate_cases.reference), move the plan's position by the arithmetic, take the kernel the header says,
refuse what it says is refused, and write nothing but the call's K x nchan rows."""
import numpy as np
import pytest

import sxxcvr_amd
import rate_cases as rc
from band_cases import AUTO, GUARD, TILED
from gpu_util import OUT_FILL, assert_bit_exact, to_cpu, to_gpu
from rate_cases import KINDS, SWEEP_COUNT, SWEEP_SEED

pytestmark = pytest.mark.gpu

FILL = np.uint32(OUT_FILL)
KIND = "bank"
SWEEP = [pytest.param(c, id=c.ident) for c in rc.cases(KIND, SWEEP_SEED, SWEEP_COUNT)]


def test_the_sweep_is_whole():
    assert len(SWEEP) == SWEEP_COUNT == 36


@pytest.mark.parametrize("case", SWEEP)
def test_bank_sweep(oracle, case):
    import torch
    K = KINDS[KIND]
    nchan, nb = case.nchan, rc.nbands_of(case)
    h = rc.taps_of(KIND, case)
    raw, xs = rc.stream_input(KIND, case, oracle)
    refs = [rc.reference(KIND, oracle, case, h, xs[c]) for c in range(nchan)]                # [K, n_out] each
    plan = rc.make_plan(KIND, case, h)
    assert tuple(plan.contract) == tuple(rc.contract(KIND, case)) and plan.contract.rot == 0
    assert plan.nbands == nb and plan.centres == [(n % d, d) for n, d in case.centres]
    want = [rc.stored_words(oracle, case.fmt, r) for r in refs]                              # [K, n_out, words] each
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
    got = [[[] for _ in range(nb)] for _ in range(nchan)]
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
        # the output: larger than needed, prefilled, the first output GUARD + out_off samples in; K x nchan rows under the call's nesting
        at_out = [[GUARD + call.out_off + c * call.out_stride + k * call.band_stride for k in range(nb)] for c in range(nchan)]
        rows = sorted(at for r in at_out for at in r)
        assert all(b - a >= n_out for a, b in zip(rows, rows[1:])), what                     # (no two rows overlap: the generator's promise)
        yg = torch.full((rows[-1] + n_out + 5, wo), int(FILL), dtype=torch.int32, device="cuda")
        assert xg.data_ptr() % 16 == 0 and yg.data_ptr() % 16 == 0
        in_ptr = xg.data_ptr() + 4 * wi * call.skew
        out_ptr = yg.data_ptr() + 4 * wo * (GUARD + call.out_off)
        args = (in_ptr, n, call.in_stride, out_ptr, call.out_stride, call.band_stride, stream)
        assert plan.outputs_for(n) == n_out, what
        label = rc.expected_kernel(KIND, case, i)
        request = call.request
        if label == "refused":
            if rc.has_form(KIND, case):
                plan.set_kernel(TILED)
                asked = rc.expected_kernel(KIND, case, i, assume_aligned=True)
                assert plan.geometry(n)["kernel"] == (K.tiled if asked == "tiled" else K.generic), what
                with pytest.raises(sxxcvr_amd.NativeError) as ei:
                    plan.process_ptr(*args)
            else:
                with pytest.raises(sxxcvr_amd.NativeError) as ei:          # no tiled kernel for the shape or format at all
                    plan.set_kernel(TILED)
            assert ei.value.code == -4, what
            assert plan.position == (pos_in, pos_out), what
            torch.cuda.synchronize()
            assert int((yg != int(FILL)).sum()) == 0, "a refused call wrote something: " + what
            request = AUTO
        plan.set_kernel(request)
        label = rc.expected_kernel(KIND, case, i, request=request)
        assert label in ("tiled", "generic", "history only"), what
        if n_out > 0:
            asked = rc.expected_kernel(KIND, case, i, request=request, assume_aligned=True)
            g = plan.geometry(n)
            assert g["kernel"] == (K.tiled if asked == "tiled" else K.generic) and g["tiled"] == (asked == "tiled"), (what, g)
        assert plan.process_ptr(*args) == n_out, what
        pos_in += n
        pos_out += n_out
        at_data += n
        assert plan.position == (pos_in, pos_out), what
        torch.cuda.synchronize()
        y = to_cpu(yg).view(np.uint32)
        written = np.zeros(y.shape[0], dtype=bool)
        for c in range(nchan):
            for k in range(nb):
                at = at_out[c][k]
                got[c][k].append(y[at:at + n_out].copy())
                written[at:at + n_out] = True
        assert np.all(y[~written] == FILL), "something outside the call's %d x %d rows was written (%s): sample %d of the buffer, the first " \
            "output at %d" % (nb, nchan, what, int(np.nonzero((y != FILL).any(axis=1) & ~written)[0][0]), GUARD + call.out_off)
    assert at_data == xs.shape[-1]
    for c in range(nchan):
        for k in range(nb):
            g, w = np.concatenate(got[c][k]), want[c][k]
            where = "%s channel %d band %d" % (case.ident, c, k)
            assert g.shape == w.shape, (where, g.shape, w.shape)
            if wo == 2:
                assert_bit_exact(g.view(np.complex64).ravel(), w.view(np.complex64).ravel(), where)
            else:                                           # CF16: the half words
                bad = np.nonzero((g != w).any(axis=1))[0]
                assert bad.size == 0, "%s: %d of %d outputs differ, first at %d: got %r want %r" % (where, bad.size, g.shape[0], bad[0], g[bad[0]], w[bad[0]])
        if case.twin:
            a, b = (np.concatenate(got[c][k]) for k in case.twin)
            assert np.array_equal(a, b), "%s channel %d: the rows of the twin bands %r differ" % (case.ident, c, case.twin)
    plan.close()
