"""Seeded sweep of the arbitrary-rate resamplers on the GPU (tests/arb_sweep_cases.py), as tests/test_gpu_rate_sweep.py sweeps the
rate-changing kinds: any legal phase count, taps per phase, step -- the ends of the tiled and of the allowed range among them, changed
in mid-stream --, channel count, format, call split, kernel request, placement of input and output and PLACE in the 64-bit stream
(sxfir_set_history + sxfir_set_time: far, through 2^31 and 2^32, ahead of the stream, on the last phase) must give the bits of the
float32 reference of the whole stream, move the plan's position and time by the model's arithmetic, take the kernel the header says,
refuse what it says is refused, and write nothing but the call's outputs."""
import numpy as np
import pytest

import sxxcvr_amd
import arb_sweep_cases as ac
from arb_cases import MASK
from arb_sweep_cases import GENERIC_KERNEL, SWEEP_COUNT, SWEEP_SEED, TILED_KERNEL
from band_cases import AUTO, GUARD, TILED
from gpu_util import OUT_FILL, assert_bit_exact, to_cpu, to_gpu

pytestmark = pytest.mark.gpu

FILL = np.uint32(OUT_FILL)
SWEEP = [pytest.param(c, id=c.ident) for c in ac.cases(SWEEP_SEED, SWEEP_COUNT)]


def test_the_sweep_is_whole():
    assert len(SWEEP) == SWEEP_COUNT == 36


@pytest.mark.parametrize("case", SWEEP)
def test_arb_sweep(oracle, case):
    import torch
    nchan = case.nchan
    h = ac.taps_of(case)
    raw, xs = ac.stream_input(case, oracle)
    want = [ac.stored_words(oracle, case.fmt, ac.reference(oracle, case, h, xs[c])) for c in range(nchan)]
    plan = ac.make_plan(case, h)
    assert tuple(plan.contract) == (ac.jsplit_of(case), 1) and plan.contract.rot == 0 and plan.nphases == case.P
    wi = wo = raw.shape[-1]                                 # 32-bit words per sample: the same storage in and out
    stream = torch.cuda.current_stream().cuda_stream
    if case.place != "start":
        # the samples in front of the stream become the plan's history, then the plan is placed
        lg = to_gpu(np.ascontiguousarray(raw[:, :case.lead]))
        plan.set_history_ptr(lg.data_ptr(), case.lead, case.lead, stream)
        plan.set_time(case.consumed, case.t_index, case.t_frac)
        torch.cuda.synchronize()
    produced = 0

    def check_state(st, what):
        """the model in front of the call `st` against the plan"""
        assert plan.position == (st.consumed, produced), what
        assert plan.time == (st.t >> 32, st.t & MASK) and plan.step == st.step, (what, plan.time, plan.step)
        assert (st.t >> 32) >= st.consumed - 1, what

    got = [[] for _ in range(nchan)]
    at_data = case.lead
    steps = ac.walk(case)
    for i, st in enumerate(steps):
        call, n, n_out = st.call, st.call.n, st.n_out
        what = "%s call %d %r at step %#x" % (case.ident, i, call, st.step)
        if plan.step != st.step:
            # a new segment: the step changes, the time of the next output stays
            assert i > 0 and st.segment == steps[i - 1].segment + 1, what
            before = plan.time
            plan.set_rate(step=st.step)
            assert plan.time == before, what
        check_state(st, what)
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
        label = ac.expected_kernel(case, st)
        request = call.request
        if label == "refused":
            if ac.has_form(case):
                plan.set_kernel(TILED)
                asked = ac.expected_kernel(case, st, assume_aligned=True)
                assert plan.geometry(n)["kernel"] == (TILED_KERNEL if asked == "tiled" else GENERIC_KERNEL), what
                with pytest.raises(sxxcvr_amd.NativeError) as ei:
                    plan.process_ptr(in_ptr, n, call.in_stride, out_ptr, call.out_stride, stream)
            else:
                with pytest.raises(sxxcvr_amd.NativeError) as ei:          # no tiled kernel for the shape or format at all
                    plan.set_kernel(TILED)
            assert ei.value.code == -4, what
            check_state(st, "after the refusal: " + what)
            torch.cuda.synchronize()
            assert int((yg != int(FILL)).sum()) == 0, "a refused call wrote something: " + what
            request = AUTO
        plan.set_kernel(request)
        label = ac.expected_kernel(case, st, request=request)
        assert label in ("tiled", "generic", "history only"), what
        if n_out > 0:
            asked = ac.expected_kernel(case, st, request=request, assume_aligned=True)
            g = plan.geometry(n)
            assert g["kernel"] == (TILED_KERNEL if asked == "tiled" else GENERIC_KERNEL) and g["tiled"] == (asked == "tiled"), (what, g)
        assert plan.process_ptr(in_ptr, n, call.in_stride, out_ptr, call.out_stride, stream) == n_out, what
        produced += n_out
        at_data += n
        after = st.t + n_out * st.step
        assert plan.position == (st.consumed + n, produced) and plan.time == (after >> 32, after & MASK) and plan.step == st.step, what
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
        if wo == 2:
            assert_bit_exact(g.view(np.complex64).ravel(), w.view(np.complex64).ravel(), where)
        else:                                               # CF16: the half words
            bad = np.nonzero((g != w).any(axis=1))[0]
            assert bad.size == 0, "%s: %d of %d outputs differ, first at %d: got %r want %r" % (where, bad.size, g.shape[0], bad[0], g[bad[0]], w[bad[0]])
    plan.close()
