"""Seeded sweep of the six band-plan kinds on the GPU (tests/band_cases.py: complex-tap decimator and interpolator, 4-band channelizer
and synthesizer, critically sampled and 2x oversampled): any legal tap count, channel count, format, call split, kernel request and
placement of input and output must give the bits of the float32 reference of the whole stream, move the plan's position by the
arithmetic, take the kernel the headers say, refuse what they say is refused, and write nothing but the call's outputs.  Then three
anchors per kind, through the tiled and the generic kernel: the fp64 definition of the header (no oracle), non-finite samples, and
subnormal products."""
import numpy as np
import pytest

import sxxcvr_amd
import band_cases as bc
from band_cases import AUTO, GUARD, KINDS, SWEEP_COUNT, SWEEP_SEED, TILED
from gpu_util import OUT_FILL, assert_bit_exact, to_cpu, to_gpu

pytestmark = pytest.mark.gpu

FILL = np.uint32(OUT_FILL)
ANCHORS = [pytest.param(k, *s, id="%s-%s" % (k, s[0])) for k in KINDS for s in bc.anchor_shapes(k)]
SWEEP = [pytest.param(k, c, id="%s-%s" % (k, c.ident)) for k in KINDS for c in bc.cases(k, SWEEP_SEED, SWEEP_COUNT)]


def _rows(K, nchan, banded):
    return [(c, k) for c in range(nchan) for k in range(bc.BANDS if banded else 1)]


def _call(kind, plan, in_ptr, n, call, out_ptr, stream):
    K = KINDS[kind]
    if K.banded_out:
        return plan.process_ptr(in_ptr, n, call.in_stride, out_ptr, call.out_stride, call.band_stride, stream)
    if K.banded_in:
        return plan.process_ptr(in_ptr, n, call.in_stride, call.band_stride, out_ptr, call.out_stride, stream)
    return plan.process_ptr(in_ptr, n, call.in_stride, out_ptr, call.out_stride, stream)


@pytest.mark.parametrize("kind,case", SWEEP)
def test_band_sweep(oracle, kind, case):
    import torch
    K = KINDS[kind]
    nchan = case.nchan
    h = bc.taps_of(kind, case.ntaps, case.tap_seed)
    raw, xs = bc.stream_input(kind, case, oracle)
    refs = [bc.reference(kind, oracle, h, case.ratio, xs[c]) for c in range(nchan)]
    plan = bc.make_plan(kind, h, case.ratio, nchan=nchan, fmt=case.fmt)
    assert tuple(plan.contract) == tuple(bc.contract(kind, case.ntaps, case.ratio)) and plan.contract.rot == 0
    thr2 = None
    if case.fmt == "S32" and not K.decim:
        thr2 = bc.keying_threshold(np.concatenate([r.ravel() for r in refs]))
        plan.set_tx_threshold(float(thr2))
    want = [bc.stored_words(kind, oracle, case.fmt, r, thr2) for r in refs]
    wi, wo = raw.shape[-1], want[0].shape[-1]              # 32-bit words per input / output sample
    rows_in, rows_out = _rows(K, nchan, K.banded_in), _rows(K, nchan, K.banded_out)
    got = {row: [] for row in rows_out}
    stream = torch.cuda.current_stream().cuda_stream
    pos_in = pos_out = 0
    for i, call in enumerate(case.calls):
        n = call.n
        n_out = bc.outputs_for(kind, case.ratio, pos_in, n)
        what = "%s call %d %r" % (case.ident, i, call)
        # the input: a view `skew` samples into a buffer of fill, rows at the call's strides
        in_band = call.band_stride if K.banded_in else 0
        at_in = {(c, k): call.skew + c * call.in_stride + k * in_band for c, k in rows_in}
        xin = np.full((max(at_in.values()) + n + 3, wi), FILL, dtype=np.uint32)
        for (c, k), at in at_in.items():
            xin[at:at + n] = (raw[c, k] if K.banded_in else raw[c])[pos_in:pos_in + n].view(np.uint32)
        xg = to_gpu(xin.view(np.int32))
        # the output: larger than needed, prefilled, the first output GUARD + out_off samples in
        out_band = call.band_stride if K.banded_out else 0
        at_out = {(c, k): GUARD + call.out_off + c * call.out_stride + k * out_band for c, k in rows_out}
        yg = torch.full((max(at_out.values()) + n_out + 5, wo), int(FILL), dtype=torch.int32, device="cuda")
        assert xg.data_ptr() % 16 == 0 and yg.data_ptr() % 16 == 0
        in_ptr = xg.data_ptr() + 4 * wi * call.skew
        out_ptr = yg.data_ptr() + 4 * wo * (GUARD + call.out_off)
        assert plan.outputs_for(n) == n_out, what
        label = bc.expected_kernel(kind, case, i)
        request = call.request
        if label == "refused":
            if bc.has_form(kind, case):
                plan.set_kernel(TILED)
                asked = bc.expected_kernel(kind, case, i, assume_aligned=True)
                assert plan.geometry(n)["kernel"] == (K.tiled if asked == "tiled" else K.generic), what
                with pytest.raises(sxxcvr_amd.NativeError) as ei:
                    _call(kind, plan, in_ptr, n, call, out_ptr, stream)
            else:
                with pytest.raises(sxxcvr_amd.NativeError) as ei:          # no tiled kernel for the shape or format at all
                    plan.set_kernel(TILED)
            assert ei.value.code == -4, what
            assert plan.position == (pos_in, pos_out), what
            torch.cuda.synchronize()
            assert int((yg != int(FILL)).sum()) == 0, "a refused call wrote something: " + what
            request = AUTO
        plan.set_kernel(request)
        label = bc.expected_kernel(kind, case, i, request=request)
        assert label in ("tiled", "generic", "history only"), what
        if n_out > 0:
            asked = bc.expected_kernel(kind, case, i, request=request, assume_aligned=True)
            g = plan.geometry(n)
            assert g["kernel"] == (K.tiled if asked == "tiled" else K.generic) and g["tiled"] == (asked == "tiled"), (what, g)
        assert _call(kind, plan, in_ptr, n, call, out_ptr, stream) == n_out, what
        pos_in += n
        pos_out += n_out
        assert plan.position == (pos_in, pos_out), what
        torch.cuda.synchronize()
        y = to_cpu(yg).view(np.uint32)
        written = np.zeros(y.shape[0], dtype=bool)
        for row, at in at_out.items():
            got[row].append(y[at:at + n_out].copy())
            written[at:at + n_out] = True
        assert np.all(y[~written] == FILL), "something outside the call's outputs was written (%s): sample %d of the buffer, the first " \
            "output at %d" % (what, int(np.nonzero((y != FILL).any(axis=1) & ~written)[0][0]), GUARD + call.out_off)
    assert pos_in == xs.shape[-1]
    for c, k in rows_out:
        g = np.concatenate(got[c, k])
        w = want[c][k] if K.banded_out else want[c]
        where = "%s channel %d band %d" % (case.ident, c, k)
        assert g.shape == w.shape, (where, g.shape, w.shape)
        if wo == 2 and thr2 is None:
            assert_bit_exact(g.view(np.complex64).ravel(), w.view(np.complex64).ravel(), where)
        else:                                               # CF16: the half words; S32 out: the wire words
            bad = np.nonzero((g != w).any(axis=1))[0]
            assert bad.size == 0, "%s: %d of %d outputs differ, first at %d: got %r want %r" % (where, bad.size, g.shape[0], bad[0], g[bad[0]], w[bad[0]])
    plan.close()


def _anchor_plan(kind, label, h, ratio, n, fmt="CF32"):
    """A one-channel plan on the kernel the label names: the tiled one forced, or the generic one of a shape without a tiled one."""
    K = KINDS[kind]
    plan = bc.make_plan(kind, h, ratio, fmt=fmt)
    tiled = label.startswith("tiled") and fmt == "CF32"
    if tiled:
        plan.set_kernel(TILED)
    g = plan.geometry(n)
    assert g["kernel"] == (K.tiled if tiled else K.generic) and g["tiled"] == tiled, g
    return plan


def _process(plan, x):
    import torch
    y = plan.process(to_gpu(x))
    torch.cuda.synchronize()
    return to_cpu(y)


def _random_input(kind, N, seed):
    rng = np.random.default_rng(seed)
    shape = (4, N) if KINDS[kind].banded_in else (N,)
    return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(np.complex64)


@pytest.mark.parametrize("fmt", ["CF32", "CF16"])
@pytest.mark.parametrize("kind,label,ntaps,ratio", ANCHORS)
def test_band_plans_against_fp64(kind, label, ntaps, ratio, fmt):
    """An anchor that does not pass through the oracle: the header's formula in fp64 by np.convolve alone (band_cases.definition_fp64)
    against the GPU, on random input with components uniform in [-1, 1).  Bound 2e-6 sum|h| B, which the float32 reference itself
    meets 31 times over at the least (tests/test_band_cases_host.py); CF16 filters the stored halves exactly and adds 2^-11 max|want|
    for the one rounding of each output to half, as test_every_configuration_against_scipy_fp64 does."""
    h = bc.taps_of(kind, ntaps, 5)
    N = bc.anchor_length(kind, ratio)
    x = _random_input(kind, N, 1234 + ntaps + ratio)
    plan = _anchor_plan(kind, label, h, ratio, N, fmt)
    if fmt == "CF16":
        x16 = x.view(np.float32).astype(np.float16)
        x_used = x16.astype(np.float32).view(np.complex64)          # what the kernel filters: the stored halves, exactly
        y = _process(plan, x16.view(np.int32)).view(np.float16).astype(np.float64)
        got = y[..., 0::2] + 1j * y[..., 1::2]
    else:
        x_used = x
        got = _process(plan, x).astype(np.complex128)
    want = bc.definition_fp64(kind, h, ratio, x_used)
    assert got.shape == want.shape
    tol = bc.fp64_bound(kind, h)
    if fmt == "CF16":
        tol += 2.0 ** -11 * float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print("%s %s %s: max |GPU - fp64 definition| = %.3g, bound %.3g" % (kind, label, fmt, err, tol))
    assert err <= tol


@pytest.mark.parametrize("kind,label,ntaps,ratio", ANCHORS)
def test_non_finite_samples(oracle, kind, label, ntaps, ratio):
    """+inf and a NaN in the first tile, -inf deep inside the second, each in the I component of one sample (band 1 of a
    synthesizer's input) and further apart than the filter is long, and a run of 40 samples of -0.0: the outputs that are NaN in the
    reference are NaN, every other output has the reference's bits (the rule of test_cf16_dense_kernel_edges).  The channelizers'
    reference takes each branch sum over its own phase's taps (band_cases.chan_ref_phase_taps), as the headers state it."""
    K = KINDS[kind]
    T, hist = bc.tile_of(kind, ratio), bc.hist_of(kind, ntaps, ratio)
    N = 2 * T + T // 2 + 3
    marks = {3: np.inf, T // 2 + 7: np.nan, T + T // 2 + 1: -np.inf}
    at = sorted(marks)
    assert at[1] < T < at[2] < 2 * T and min(np.diff(at)) > hist
    x = _random_input(kind, N, 77 + ntaps + ratio)
    row = x[1] if K.banded_in else x
    for smp, v in marks.items():
        row[smp] = complex(v, row[smp].imag)
    x[..., 2 * T + 10:2 * T + 50] = complex(-0.0, -0.0)
    assert np.signbit(x[..., 2 * T + 10].real).all() and np.isnan(x.real).sum() == 1 and np.isinf(x.real).sum() == 2
    h = bc.taps_of(kind, ntaps, 5)
    plan = _anchor_plan(kind, label, h, ratio, N)
    got = _process(plan, x)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = bc.chan_ref_phase_taps(oracle, h, x, ratio) if K.banded_out else bc.reference(kind, oracle, h, ratio, x)
    assert got.shape == ref.shape
    gf, wf = np.ascontiguousarray(got).view(np.float32), np.ascontiguousarray(ref).view(np.float32)
    nan = np.isnan(wf)
    assert nan.any() and np.isinf(wf[~nan]).any(), "the case is empty"
    assert np.array_equal(np.isnan(gf), nan), "%d components are NaN on one side only" % int((np.isnan(gf) != nan).sum())
    assert np.array_equal(gf.view(np.uint32)[~nan], wf.view(np.uint32)[~nan])


@pytest.mark.parametrize("kind,label,ntaps,ratio", ANCHORS)
def test_subnormal_products(oracle, kind, label, ntaps, ratio):
    """The input times 2^-120: products and partial sums are subnormal.  The contract is an fmaf chain and float32 adds, which keep
    subnormals: bit-exact against the reference on the same input, which holds subnormal, non-zero outputs."""
    N = bc.anchor_length(kind, ratio)
    x = (_random_input(kind, N, 99 + ntaps + ratio).view(np.float32) * np.float32(2.0 ** -120)).view(np.complex64)
    h = bc.taps_of(kind, ntaps, 5)
    ref = bc.reference(kind, oracle, h, ratio, x)
    mag = np.abs(np.ascontiguousarray(ref).view(np.float32))
    tiny = (mag > 0) & (mag < np.finfo(np.float32).tiny)
    print("%s %s: %d of %d output components of the reference are subnormal and not zero" % (kind, label, int(tiny.sum()), tiny.size))
    assert tiny.sum() >= 20, "the reference holds too few subnormal outputs: %d of %d" % (int(tiny.sum()), tiny.size)
    plan = _anchor_plan(kind, label, h, ratio, N)
    got = _process(plan, x)
    assert got.shape == ref.shape
    assert_bit_exact(got.ravel(), ref.ravel(), "%s %s on subnormal products" % (kind, label))
