"""Arbitrary-rate resamplers on the GPU (include/sxfir_arbitrary.h), bit for bit against the oracle as it stands (tests/arb_cases.py:
two samples of the oracle's interpolator pass per output, blended in float32).

Every call goes through `Rig.call`: the output lands between two guards of fill words that must come back untouched, and the plan's
position, time, step and outputs_for are checked against the big-integer model around it."""
import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import ArbitraryResampler, RationalResampler, Resampler, design_arbitrary
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED
from arb_cases import MASK, ONE, STEP_MAX, STEP_MIN, STEPS, Stream, arb_f64, arb_ref, arb_taps, blend_at, bound, count, position, times_of
from rational_cases import gaussian_stream, rational_taps

pytestmark = pytest.mark.gpu

FILL = 0x7FC07FC0               # a NaN as one fp32 word and as two halves: no output of these streams is this word
GUARD = 8                       # samples of fill words on either side of a row's outputs (whole 16-byte units in both formats)
TILE = 256                      # outputs per tile of resample_arb_kernel
TILED, GENERIC = "resample_arb_kernel", "resample_arb_generic_kernel"
EINVAL, EUNSUPPORTED = -1, -4
SQRT2 = 0x16A09E667
TILED_STEPS = [1 << 31, 1 << 33, ONE + 4295, SQRT2]


def _i32(word):
    return word - (1 << 32) if word >= 1 << 31 else word


class Rig:
    """One stream [nchan, n] on the GPU (rows `pad` samples longer than the stream: strides larger than the block) and its CPU twin
    as the plan sees it (CF16: quantised to half)."""

    def __init__(self, oracle, x, fmt="CF32", pad=41):
        import torch
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex64)
        self.oracle, self.fmt, self.nchan, self.n = oracle, fmt, x.shape[0], x.shape[1]
        self.sb, self.wps = (4, 1) if fmt == "CF16" else (8, 2)          # bytes, 32-bit words per sample
        self.stride = self.n + pad
        if fmt == "CF16":
            h16 = oracle.f32_to_f16(x.view(np.float32))
            self.x = oracle.f16_to_f32(h16).view(np.complex64)
            words = np.ascontiguousarray(h16).view(np.int32)
        else:
            self.x = x
            words = x.view(np.int32)
        buf = np.zeros((self.nchan, self.stride * self.wps), dtype=np.int32)
        buf[:, :words.shape[1]] = words
        self.xg = torch.from_numpy(buf).cuda()

    def words(self, y):
        """complex64 [.., n] reference -> the 32-bit words the plan stores"""
        y = np.ascontiguousarray(y, dtype=np.complex64)
        if self.fmt == "CF16":
            return np.ascontiguousarray(self.oracle.f32_to_f16(y.view(np.float32))).view(np.uint32)
        return y.view(np.uint32)

    def ref(self, h, P, steps, jsplit, consumed=0, t=None, first=0):
        """[nchan, words] of the stream's inputs [first, n) -- sample `first` at the absolute index `consumed`, zeros in front"""
        return np.stack([self.words(arb_ref(self.oracle, h, P, steps, self.x[c, first:], jsplit, consumed, t)) for c in range(self.nchan)])

    def check_state(self, plan, model):
        assert plan.position == (model.consumed, model.produced), (plan.position, model.consumed, model.produced)
        assert plan.time == (model.t >> 32, model.t & MASK) and plan.step == model.step
        assert (model.t >> 32) >= model.consumed - 1

    def call(self, plan, model, pos, n, kernel=None, offset=0, expect=None, odd_stride=False):
        """sxfir_resample_arbitrary over inputs [pos, pos + n) of every row; `model`: the Stream that mirrors the plan.  Returns
        [nchan, words]; with `expect` (an error code) the call must fail with it and leave the plan and the output buffer alone."""
        import torch
        self.check_state(plan, model)
        n_out = count(model.t, model.step, model.consumed, n)[0]
        assert plan.outputs_for(n) == n_out
        if kernel is not None:
            assert plan.geometry(n)["kernel"] == kernel, (plan.geometry(n), kernel)
        row = 2 * GUARD + offset + n_out + (offset + n_out) % 2               # an even stride, larger than the block
        row += 1 if odd_stride else 0
        buf = torch.full((self.nchan, row * self.wps), _i32(FILL), dtype=torch.int32, device="cuda")
        args = (self.xg.data_ptr() + self.sb * pos, n, self.stride, buf.data_ptr() + self.sb * (GUARD + offset), row,
                torch.cuda.current_stream().cuda_stream)
        if expect is not None:
            with pytest.raises(sxxcvr_amd.NativeError) as ei:
                plan.process_ptr(*args)
            torch.cuda.synchronize()
            assert ei.value.code == expect
            self.check_state(plan, model)
            assert np.all(buf.cpu().numpy().view(np.uint32) == FILL), "a refused call wrote to the output"
            return None
        assert plan.process_ptr(*args) == n_out
        torch.cuda.synchronize()
        assert len(model.call(n)) == n_out
        self.check_state(plan, model)
        got = buf.cpu().numpy().view(np.uint32).reshape(self.nchan, row, self.wps)
        lo, hi = GUARD + offset, GUARD + offset + n_out
        assert np.all(got[:, :lo] == FILL) and np.all(got[:, hi:] == FILL), "the guard around the outputs was written"
        return np.ascontiguousarray(got[:, lo:hi]).reshape(self.nchan, n_out * self.wps)

    def stream(self, plan, model, blocks, kernels=None, pos=0):
        outs = []
        for i, b in enumerate(blocks):
            outs.append(self.call(plan, model, pos, b, None if kernels is None else kernels[i]))
            pos += b
        return np.concatenate(outs, axis=1)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.ravel() != want.ravel())[0]
    assert not bad.size, "%s: %d of %d words differ, first at %d: got %08x want %08x" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def streams(nchan, n, seed=3):
    return np.stack([gaussian_stream(n, seed + 17 * c) for c in range(nchan)])


def wraps(times, P):
    """how many of the outputs at `times` have p == P - 1: their second chain is phase 0 of the next input"""
    return sum(1 for t in times if position(t, P)[1] == P - 1)


def has_tiled(P, T, fmt):
    return (P, T, fmt) == (128, 32, "CF32")


# ---- 1. the generic kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("fmt", ["CF32", "CF16"])
@pytest.mark.parametrize("T", [8, 32, 33])
@pytest.mark.parametrize("P", [4, 7, 128])
def test_generic(oracle, P, T, fmt, nchan):
    """Per step one call, and six calls: 3 samples, a single sample, no sample, a single sample, a few hundred and the rest."""
    h = arb_taps(P, T)
    no_output = 0
    for step in STEPS:
        n = 300 if step == STEP_MIN else 1203
        rig = Rig(oracle, streams(nchan, n, 3 + (step & 15)), fmt)
        plans = [ArbitraryResampler(h, P, step=step, nchan=nchan, fmt=fmt) for _ in range(2)]
        plan = plans[0]
        assert (plan.nphases, plan.step, plan.time) == (P, step, (0, 0)) and plan.mode == INTERPOLATE and not plan.complex_taps
        assert tuple(plan.contract) == ((2, 1) if T % 2 == 0 else (1, 1)) and plan.contract.rot == 0
        for q in plans:
            if has_tiled(P, T, fmt):
                q.set_kernel(KERNEL_GENERIC)
            else:
                with pytest.raises(sxxcvr_amd.NativeError) as ei:
                    q.set_kernel(KERNEL_TILED)
                assert ei.value.code == EUNSUPPORTED
        ref = rig.ref(h, P, step, plan.contract[0])
        assert ref.shape[1] == count(0, step, 0, n)[0] * rig.wps > 0
        same(rig.stream(plans[0], Stream(step), [n], [GENERIC]), ref, "step %#x, one call" % step)
        blocks = [3, 1, 0, 1, 101 if step == STEP_MIN else 401]
        blocks.append(n - sum(blocks))
        model = Stream(step)
        outs = [rig.call(plans[1], model, sum(blocks[:i]), b, GENERIC) for i, b in enumerate(blocks)]
        no_output += sum(1 for o, b in zip(outs, blocks) if b and o.shape[1] == 0)
        same(np.concatenate(outs, axis=1), ref, "step %#x, calls %r" % (step, blocks))
    assert no_output >= 2, "no call of samples without an output"


# ---- 2. the wrap case: p == P - 1 ----------------------------------------------------------------------------------------------
def test_wrap_is_exercised_by_the_streams_that_claim_it():
    """From the model: 5/4 and 1 + 1e-6 from t = 0 never reach the last phase in 4096 outputs at 128 phases; sqrt(2) does, 32 times."""
    for step, want in [(5 << 30, 0), (ONE + 4295, 0), (SQRT2, 32)]:
        assert wraps([m * step for m in range(4096)], 128) == want, hex(step)


@pytest.mark.parametrize("P,T,kernel,name", [(128, 32, KERNEL_TILED, TILED), (128, 32, KERNEL_GENERIC, GENERIC), (4, 8, KERNEL_AUTO, GENERIC),
                                             (7, 33, KERNEL_AUTO, GENERIC)])
def test_wrap_placed(oracle, P, T, kernel, name):
    """A stream placed with sxfir_set_time(.., t_frac = 0xFF800000) at unit step: EVERY output is of the last phase, alpha 3/4 at
    128 phases; then sqrt(2) from there."""
    h = arb_taps(P, T)
    n = 900
    rig = Rig(oracle, streams(1, n, 21))
    for step in (ONE, SQRT2):
        plan = ArbitraryResampler(h, P, step=step)
        plan.set_kernel(kernel)
        plan.set_time(0, 0, 0xFF800000)
        model = Stream(step, 0, 0xFF800000)
        times = times_of(step, n, 0, 0xFF800000)
        assert wraps(times, P) == (len(times) if step == ONE else wraps(times, P)) > 0
        if P == 128:
            assert position(times[0], P)[1:] == (127, 3 << 22)
        want = rig.ref(h, P, step, plan.contract[0], 0, 0xFF800000)
        same(rig.stream(plan, model, [n // 3, n - n // 3], [name, name]), want, "placed on the last phase, step %#x" % step)


# ---- 3. the tiled kernel, 128 x 32 on CF32 ---------------------------------------------------------------------------------------
def plan128(h, step, kernel=KERNEL_AUTO, nchan=1):
    plan = ArbitraryResampler(h, 128, step=step, nchan=nchan)
    assert tuple(plan.contract) == (2, 1)
    plan.set_kernel(kernel)
    return plan


def inputs_for(n_out, step, t0=0):
    """(inputs, outputs) of the smallest call of a fresh stream, its first output at t0, that yields at least n_out outputs"""
    n = ((t0 + (n_out - 1) * step) >> 32) + 2       # the last output's look-ahead sample
    got = count(t0, step, 0, n)[0]                  # (steps below 1: an input completes several outputs)
    assert got >= n_out > count(t0, step, 0, n - 1)[0]
    return n, got


def wraps_from(t0, step, m0, cnt, P=128):
    """the indices in [m0, m0 + cnt) of the outputs at t0 + m step whose phase is the last one -- the model's locate rule on numpy's
    64-bit integers: the fraction is the low 32 bits of the time, which a product that wraps at 2^64 keeps"""
    m = np.arange(m0, m0 + cnt, dtype=np.uint64)
    frac = (np.uint64(t0 & MASK) + m * np.uint64(step)) & np.uint64(MASK)
    hit = m[((frac * np.uint64(P)) >> np.uint64(32)) == np.uint64(P - 1)].astype(np.int64)
    assert all(position(t0 + int(i) * step, P)[1] == P - 1 for i in hit[:50])           # (the big-integer model agrees)
    return hit


@pytest.mark.parametrize("step", TILED_STEPS)
def test_tiled_auto_tiled_generic(oracle, step):
    """Less than a tile, whole tiles, a partial last tile: AUTO, forced TILED and forced GENERIC, each against the reference."""
    h = arb_taps(128, 32)
    for outs in (TILE - 5, TILE, 2 * TILE + 35, 5 * TILE + 7):
        n, n_out = inputs_for(outs, step)
        rig = Rig(oracle, streams(1, n, 5))
        ref = rig.ref(h, 128, step, 2)
        assert ref.shape[1] == 2 * n_out
        g = plan128(h, step).geometry(n)
        assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == -(-n_out // TILE) and g["tile_samples"] == TILE, g
        same(rig.stream(plan128(h, step), Stream(step), [n], [TILED]), ref, "auto, %d outputs" % n_out)
        same(rig.stream(plan128(h, step, KERNEL_TILED), Stream(step), [n], [TILED]), ref, "tiled, %d outputs" % n_out)
        same(rig.stream(plan128(h, step, KERNEL_GENERIC), Stream(step), [n], [GENERIC]), ref, "generic, %d outputs" % n_out)


@pytest.mark.parametrize("step", TILED_STEPS)
def test_tiled_splits_three_channels(oracle, step):
    """Three channels, any split: 3 samples, 1, 0, several tiles, the rest -- no start rule, the position is computed.  Calls whose
    first output lies in the history (floor(t) = consumed - 1) are among them: asserted from the model."""
    h = arb_taps(128, 32)
    n = 2300
    rig = Rig(oracle, streams(3, n, 6))
    ref = rig.ref(h, 128, step, 2)
    blocks = [3, 1, 0, 1411, 1, 700]
    # the fourth call as long as it takes for the call after it to start in the history, at this step (from the model)
    while True:
        probe = Stream(step)
        for b in blocks[:4]:
            probe.call(b)
        if (probe.t >> 32) == probe.consumed - 1:
            break
        blocks[3] += 1
    assert blocks[3] < 1500
    blocks.append(n - sum(blocks))
    plan, model = plan128(h, step, KERNEL_TILED, nchan=3), Stream(step)
    outs, in_history, pos = [], 0, 0
    for b in blocks:
        first_in_history = (model.t >> 32) == model.consumed - 1
        o = rig.call(plan, model, pos, b, TILED)
        in_history += 1 if first_in_history and o.shape[1] else 0
        outs.append(o)
        pos += b
    assert in_history >= 2, "no call started in the history"
    got = np.concatenate(outs, axis=1)
    # (rows of three channels of different length in words: compare channel by channel)
    same(got, ref, "three channels, calls %r" % blocks)


def test_tiled_set_rate_and_refusals(oracle):
    """set_rate between calls inside the range stays tiled; to 2^33 + 1: AUTO runs the generic kernel, the same bits as the reference;
    forced TILED answers SXFIR_EUNSUPPORTED, position and time untouched.  A misaligned output or an odd channel stride likewise."""
    h = arb_taps(128, 32)
    n = 3000
    out_of_range = (1 << 33) + 1
    segs = [(700, ONE + 4295), (900, SQRT2), (600, out_of_range), (800, 1 << 31)]
    for nchan in (1, 3):
        rig = Rig(oracle, streams(nchan, n, 8))
        ref = rig.ref(h, 128, segs, 2)
        plan, model = plan128(h, segs[0][1], nchan=nchan), Stream(segs[0][1])
        outs, pos = [], 0
        for k, step in segs:
            plan.set_rate(step=step)
            model.step = step
            assert plan.step == step
            name = GENERIC if step == out_of_range else TILED
            if step == out_of_range:
                plan.set_kernel(KERNEL_TILED)
                rig.call(plan, model, pos, k, GENERIC, expect=EUNSUPPORTED)
                assert b"step" in plan._lib.sxfir_last_error()
                plan.set_kernel(KERNEL_AUTO)
            outs.append(rig.call(plan, model, pos, k, name))
            pos += k
        same(np.concatenate(outs, axis=1), ref, "set_rate in mid-stream, %d channel(s)" % nchan)
    # an output pointer offset by one sample (8 bytes); an odd channel stride
    for nchan, kw in ((1, {"offset": 1}), (3, {"odd_stride": True})):
        rig = Rig(oracle, streams(nchan, 1200, 9))
        ref = rig.ref(h, 128, SQRT2, 2)
        plan = plan128(h, SQRT2, KERNEL_TILED, nchan=nchan)
        rig.call(plan, Stream(SQRT2), 0, 1200, expect=EUNSUPPORTED, **kw)          # (geometry() speaks of an aligned call)
        assert b"aligned" in plan._lib.sxfir_last_error()
        same(rig.call(plan, Stream(SQRT2), 0, 1200, TILED), ref, "the call after the refused one")
        plan = plan128(h, SQRT2, nchan=nchan)
        same(rig.call(plan, Stream(SQRT2), 0, 1200, **kw), ref, "auto: the generic kernel, the same bits")
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_rate(step=STEP_MAX + 1)
    assert ei.value.code == EINVAL and plan.step == SQRT2


WALK_SEED = 0x7A1C


# steps whose fraction keeps moving through all phases: near unity, near 2 (0x9E3779B / 2^32 = 0.0386 of a sample per output)
WALKS = [(1, SQRT2, 0), (3, ONE + 0x9E3779B, 0xFF800000), (1, (1 << 33) - 0x9E3779B, 0)]


@pytest.mark.parametrize("nchan,step,t0", WALKS)
def test_tiled_walk(oracle, nchan, step, t0):
    """More tiles than twice the grid's waves: a wave's second and third tile.  The whole call against the generic kernel on the GPU
    (test_generic holds that one to the oracle), windows of 200 outputs against the reference, from inputs regenerated for each
    window alone; then a second call against the reference.  Every stream holds outputs of the LAST phase (their second chain is
    phase 0 of the next input) on second and third tiles, and the windows there are laid around such outputs: asserted from the
    model.  The three-channel stream is placed with set_time on the last phase."""
    import torch
    h = arb_taps(128, 32)
    plans = [plan128(h, step, k, nchan) for k in (KERNEL_TILED, KERNEL_GENERIC)]
    for plan in plans:
        plan.set_time(0, 0, t0)
    per = plans[0].geometry(4096)["resident"] // nchan          # workgroups per channel of a small call; four waves each
    n_out = (8 * per + 5) * TILE + 140
    n, n_out = inputs_for(n_out, step, t0)
    n2 = 900
    x = torch.empty((nchan, n + n2), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, WALK_SEED, 60, 0)
    stream = torch.cuda.current_stream().cuda_stream
    g = plans[0].geometry(n)
    G = g["workgroups"] // nchan
    assert g["kernel"] == TILED and g["tiled"] and g["n_tiles"] == -(-n_out // TILE), g
    assert G == per and g["n_tiles"] > 8 * G, "no wave walks to a third tile: %r" % (g,)
    assert plans[1].geometry(n)["kernel"] == GENERIC

    def call(plan, pos, cnt, want_out):
        row = 2 * GUARD + want_out + want_out % 2
        buf = torch.full((nchan, row, 2), _i32(FILL), dtype=torch.int32, device="cuda")
        assert plan.outputs_for(cnt) == want_out
        assert plan.process_ptr(x.data_ptr() + 8 * pos, cnt, x.stride(0), buf.data_ptr() + 8 * GUARD, row, stream) == want_out
        assert bool((buf[:, :GUARD] == _i32(FILL)).all()) and bool((buf[:, GUARD + want_out:] == _i32(FILL)).all()), "the guard around the outputs was written"
        return buf

    def window(c, t_list):
        """words [cnt, 2] of the outputs at the absolute times t_list, channel c"""
        lo = max((t_list[0] >> 32) - 40, 0)
        hi = (t_list[-1] >> 32) + 2
        xw = oracle.synth_iq(WALK_SEED, 60 + c, lo, hi - lo)
        # (below `lo` the stream is not zero: 40 samples in front cover the 32 the chains read)
        return blend_at(oracle, h, 128, t_list, xw, 2, lo).view(np.uint32).reshape(len(t_list), 2)

    got = call(plans[0], 0, n, n_out)
    other = call(plans[1], 0, n, n_out)
    torch.cuda.synchronize()
    assert torch.equal(got, other), "the tiled and the generic kernel differ: first at output %d of channel %d" % (
        int((got != other).any(dim=2).nonzero()[0, 1]) - GUARD, int((got != other).any(dim=2).nonzero()[0, 0]))
    waves = 4 * G
    second, third = waves * TILE, 2 * waves * TILE              # the first output of the waves' second / third tiles
    assert n_out % TILE and n_out - 200 > third + 2 * TILE
    # the last phase: all over the stream, and on the waves' second and third tiles; a window there starts 5 outputs in front of one
    hits = wraps_from(t0, step, 0, n_out)
    assert hits.size > n_out // 1024 and (hits >= third).sum() > 0, "the stream hardly reaches the last phase"
    on_second, on_third = wraps_from(t0, step, second, 4 * TILE), wraps_from(t0, step, third + 30, 4 * TILE)
    assert on_second.size and on_third.size, "no output of the last phase on a wave's second / third tile"
    starts = {"the stream's start": 0, "a wave's second tile": second, "the seam in front of it": second - 100,
              "the last phase on a second tile": int(on_second[0]) - 5, "a wave's third tile": third + 30,
              "the last phase on a third tile": int(on_third[0]) - 5, "the last, ragged tile": n_out - 200}
    for what, m0 in starts.items():
        assert 0 <= m0 and m0 + 200 <= n_out
        if "last phase" in what:
            lo, hi = (second, third) if "second" in what else (third, 3 * waves * TILE)
            assert lo <= m0 + 5 and m0 + 200 <= hi and wraps_from(t0, step, m0, 200).size > 0, what
        for c in range(nchan):
            same(got[c, GUARD + m0:GUARD + m0 + 200].cpu().numpy().view(np.uint32), window(c, [t0 + m * step for m in range(m0, m0 + 200)]),
                 "%s, channel %d" % (what, c))
    # the call after it: the history and the time were carried over
    t_after = t0 + n_out * step
    assert plans[0].time == (t_after >> 32, t_after & MASK) and plans[0].position == (n, n_out)
    n_out2 = count(t_after, step, n, n2)[0]
    after = call(plans[0], n, n2, n_out2)
    torch.cuda.synchronize()
    for c in range(nchan):
        same(after[c, GUARD:GUARD + n_out2].cpu().numpy().view(np.uint32), window(c, [t_after + m * step for m in range(n_out2)]),
             "the call after it, channel %d" % c)
    print("step %#x x %d ch: resident %d, %d workgroups per channel, %d tiles, %d inputs" % (step, nchan, g["resident"], G, g["n_tiles"], n))


# ---- 4. stream rules -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,T,kernel,name", [(128, 32, KERNEL_AUTO, TILED), (7, 8, KERNEL_AUTO, GENERIC)])
def test_reset_set_position_set_time(oracle, P, T, kernel, name):
    h = arb_taps(P, T)
    n = 1500
    rig = Rig(oracle, streams(1, n, 12))
    step = SQRT2
    plan = ArbitraryResampler(h, P, step=step)
    plan.set_kernel(kernel)
    ref = rig.ref(h, P, step, plan.contract[0])
    same(rig.stream(plan, Stream(step), [700, 800], [name] * 2), ref, "a fresh plan")
    assert plan.time != (0, 0)
    plan.reset()
    assert plan.position == (0, 0) and plan.time == (0, 0) and plan.step == step
    same(rig.stream(plan, Stream(step), [n], [name]), ref, "after reset")
    # set_position(c): t = c * 2^32, produced = 0; it is not an error
    plan.reset()
    c = (1 << 31) - 200
    plan.set_position(c)
    assert plan.position == (c, 0) and plan.time == (c, 0)
    want = rig.ref(h, P, step, plan.contract[0], consumed=c)
    same(rig.stream(plan, Stream(step, c), [600, 900], [name] * 2), want, "placed with set_position, through 2^31")
    same(want, ref, "the same samples, the same time within a sample: the same bits")
    # set_time refuses a time below consumed - 1 and leaves the plan alone
    state = (plan.position, plan.time)
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_time(100, 98, 0)
    assert ei.value.code == EINVAL and (plan.position, plan.time) == state
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_time(-1, 5, 0)
    assert ei.value.code == EINVAL and (plan.position, plan.time) == state
    # ... and takes consumed - 1: the first output lies in the (zero) history
    plan.reset()
    plan.set_time(100, 99, 0x40000000)
    t0 = (99 << 32) | 0x40000000
    assert plan.position == (100, 0) and plan.time == (99, 0x40000000)
    want = rig.ref(h, P, step, plan.contract[0], consumed=100, t=t0)
    same(rig.stream(plan, Stream(step, 100, t0), [n], [name]), want, "placed with set_time, the first output in the history")
    # every other plan answers zeros to the query, and refuses the two setters
    other = RationalResampler(rational_taps(4, 32), 4, 5)
    import ctypes as C
    a, b, ti, tf = C.c_int(7), C.c_uint64(7), C.c_int64(7), C.c_uint32(7)
    assert other._lib.sxfir_plan_arbitrary(other._plan, C.byref(a), C.byref(b), C.byref(ti), C.byref(tf)) == 0
    assert (a.value, b.value, ti.value, tf.value) == (0, 0, 0, 0)
    assert other._lib.sxfir_set_rate(other._plan, ONE) == EINVAL and other._lib.sxfir_set_time(other._plan, 0, 0, 0) == EINVAL
    u, d = C.c_int(7), C.c_int(7)
    assert plan._lib.sxfir_plan_rational(plan._plan, C.byref(u), C.byref(d)) == 0 and (u.value, d.value) == (0, 0)


@pytest.mark.parametrize("P,T,kernel,name", [(128, 32, KERNEL_AUTO, TILED), (7, 8, KERNEL_AUTO, GENERIC)])
def test_placed_at_2_32(oracle, P, T, kernel, name):
    """A stream placed at consumed = 2^32 - 3 with set_history gives the bits of the same samples unplaced."""
    import torch
    h = arb_taps(P, T)
    n, a = 1400, 300
    rig = Rig(oracle, streams(1, n, 13))
    step = ONE + 4295
    plan = ArbitraryResampler(h, P, step=step)
    plan.set_kernel(kernel)
    ref = rig.ref(h, P, step, plan.contract[0])
    model = Stream(step)
    first = rig.call(plan, model, 0, a, name)
    rest = rig.call(plan, model, a, n - a, name)
    same(np.concatenate([first, rest], axis=1), ref, "unplaced")
    c = (1 << 32) - 3
    unplaced = Stream(step)
    unplaced.call(a)
    t = unplaced.t + ((c - a) << 32)
    placed = ArbitraryResampler(h, P, step=step)
    placed.set_kernel(kernel)
    placed.set_history_ptr(rig.xg.data_ptr(), a, rig.stride, torch.cuda.current_stream().cuda_stream)
    placed.set_time(c, t >> 32, t & MASK)
    assert (t >> 32) >= c - 1
    same(rig.call(placed, Stream(step, c, t), a, n - a, name), rest, "placed at 2^32 - 3")
    assert placed.position[0] == c + n - a > 1 << 32


@pytest.mark.parametrize("P,T,fmt,nchan,name", [(128, 32, "CF32", 1, TILED), (128, 32, "CF32", 3, TILED), (7, 8, "CF16", 2, GENERIC)])
def test_process_takes_tensors(oracle, P, T, fmt, nchan, name):
    """ArbitraryResampler.process, the torch tensor path: [nchan, n] and [n] tensors, a caller's `out`, set_rate between calls."""
    import torch
    h = arb_taps(P, T)
    n, a = 1500, 640
    rig = Rig(oracle, streams(nchan, n, 31), fmt, pad=0)
    segs = [(a, SQRT2), (n - a, ONE + 4295)]
    want = rig.ref(h, P, segs, 2)
    plan = ArbitraryResampler(h, P, rate=ONE / SQRT2, nchan=nchan, fmt=fmt)
    assert plan.step == SQRT2 and plan.geometry(a)["kernel"] == name
    xg = rig.xg if fmt == "CF16" else torch.view_as_complex(rig.xg.view(torch.float32).reshape(nchan, n, 2))
    xg = xg[0] if nchan == 1 else xg
    first = plan.process(xg[..., :a].contiguous())
    assert first.shape[-1] == count(0, SQRT2, 0, a)[0] and first.dim() == xg.dim()
    plan.set_rate(step=ONE + 4295)
    k = plan.outputs_for(n - a)
    out = torch.zeros((nchan, k + 6) if nchan > 1 else (k + 6,), dtype=first.dtype, device="cuda")
    rest = plan.process(xg[..., a:].contiguous(), out=out)
    torch.cuda.synchronize()
    assert rest.shape[-1] == k and rest.data_ptr() == out.data_ptr() and bool((out[..., k:] == 0).all())
    got = torch.cat([first, rest], dim=-1).reshape(nchan, -1).cpu().numpy()
    got = got.view(np.uint32) if fmt == "CF16" else np.ascontiguousarray(got).view(np.uint32)
    same(got, want, "process() over two calls")


@pytest.mark.parametrize("P,T,kernel,name", [(128, 32, KERNEL_AUTO, TILED), (7, 8, KERNEL_AUTO, GENERIC)])
def test_timed_pass_in_mid_stream(oracle, P, T, kernel, name):
    """sxfir_time_resample_arbitrary in the middle of a stream: two back-to-back passes write the words of the call that the
    stream makes next, between guards that stay; position, time and step are as they were; and the real call after it gives the
    reference's bits -- the history was left alone."""
    import torch
    h = arb_taps(P, T)
    n, a, b = 2300, 700, 900
    rig = Rig(oracle, streams(2, n, 27))
    plan = ArbitraryResampler(h, P, step=SQRT2, nchan=2)
    plan.set_kernel(kernel)
    ref = rig.ref(h, P, SQRT2, plan.contract[0])
    model = Stream(SQRT2)
    first = rig.call(plan, model, 0, a, name)
    k0 = first.shape[1]
    n_out = count(model.t, model.step, model.consumed, b)[0]
    assert plan.outputs_for(b) == n_out > 0 and plan.geometry(b)["kernel"] == name
    row = 2 * GUARD + n_out + n_out % 2
    buf = torch.full((2, row * rig.wps), _i32(FILL), dtype=torch.int32, device="cuda")
    ms = plan.time_resample_ptr(rig.xg.data_ptr() + rig.sb * a, b, rig.stride, buf.data_ptr() + rig.sb * GUARD, row, 2,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ms > 0.0
    rig.check_state(plan, model)
    got = buf.cpu().numpy().view(np.uint32).reshape(2, row, rig.wps)
    assert np.all(got[:, :GUARD] == FILL) and np.all(got[:, GUARD + n_out:] == FILL), "the guard around the timed passes' outputs was written"
    want = ref[:, k0:k0 + n_out * rig.wps]
    same(np.ascontiguousarray(got[:, GUARD:GUARD + n_out]).reshape(2, -1), want, "what the timed passes wrote")
    second = rig.call(plan, model, a, b, name)
    same(second, want, "the call after the timed passes")
    same(np.concatenate([first, second, rig.call(plan, model, a + b, n - a - b, name)], axis=1), ref, "the whole stream")


@pytest.mark.parametrize("P,T", [(2, 1), (2, 2), (4096, 1), (4096, 2)])
def test_create_at_the_ends_of_the_range(oracle, P, T):
    """The fewest and the most phases the header allows with one and two taps per phase: a history of 2 samples, the contracts
    (1, 1) and (2, 1), z = frac * P at its 44 bits.  One short stream at sqrt(2), placed on the last 2^-14 of a sample so that its
    first output is of the last phase at either P (asserted from the model), in two calls, against the reference."""
    h = arb_taps(P, T)
    n, t0 = 600, 0xFFFC0000
    rig = Rig(oracle, streams(2, n, 28))
    plan = ArbitraryResampler(h, P, step=SQRT2, nchan=2)
    assert plan.nphases == P and tuple(plan.contract) == ((2, 1) if T == 2 else (1, 1)) and plan.contract.rot == 0
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == EUNSUPPORTED
    plan.set_time(0, 0, t0)
    times = times_of(SQRT2, n, 0, t0)
    assert position(times[0], P)[1] == P - 1 and wraps(times, P) >= 1 and len(times) > 400
    want = rig.ref(h, P, SQRT2, plan.contract[0], 0, t0)
    same(rig.stream(plan, Stream(SQRT2, 0, t0), [n // 3, n - n // 3], [GENERIC] * 2), want, "%d phases x %d taps" % (P, T))


# ---- 5. against code that already ships ----------------------------------------------------------------------------------------
def test_against_the_rational_plan(oracle):
    """4 phases at step 5/4 from t = 0: alpha = 0 throughout, so the outputs are those of sxfir_create_rational(4, 5) over the same
    input, as values (fmaf(0, d, a) may turn -0 into +0): compared with ==."""
    h = rational_taps(4, 32)
    n = 2311
    x = streams(1, n, 16)
    rig = Rig(oracle, x)
    arb = ArbitraryResampler(h, 4, rate=0.8)
    assert arb.step == 5 << 30
    got = rig.stream(arb, Stream(5 << 30), [1000, n - 1000], [GENERIC] * 2).view(np.complex64)[0]
    rat = RationalResampler(h, 4, 5)
    import torch
    y = rat.process(torch.from_numpy(x[0]).cuda())
    torch.cuda.synchronize()
    want = y.cpu().numpy()
    assert 0 < want.size - got.size <= 2          # (the look-ahead sample: the last outputs wait for the next call)
    assert not np.isnan(want).any() and bool(np.all(got == want[:got.size]))


# ---- 6. anchors --------------------------------------------------------------------------------------------------------------------
ANCHORS = [(128, 32, KERNEL_TILED, TILED), (128, 32, KERNEL_GENERIC, GENERIC), (7, 33, KERNEL_AUTO, GENERIC)]


@pytest.mark.parametrize("P,T,kernel,name", ANCHORS)
def test_anchor_non_finite(oracle, P, T, kernel, name):
    """One +Inf and one NaN sample: non-finite outputs exactly where the reference has them (NaNs compared as NaNs, not by
    payload), the same bits everywhere else."""
    h = arb_taps(P, T)
    n = 2000
    x = streams(1, n, 14)
    x[0, 700] = np.complex64(complex(np.inf, 0.25))
    x[0, 1500] = np.complex64(complex(-0.5, np.nan))
    rig = Rig(oracle, x)
    plan = ArbitraryResampler(h, P, step=SQRT2)
    plan.set_kernel(kernel)
    got = rig.stream(plan, Stream(SQRT2), [n], [name]).view(np.float32)[0]
    want = rig.ref(h, P, SQRT2, plan.contract[0]).view(np.float32)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    # (an Inf sample that both chains of an output see leaves the blend as Inf - Inf: a NaN.  Inf outputs are the few whose second
    # chain alone reaches it)
    assert np.array_equal(np.isinf(got), np.isinf(want))
    # each of the two samples lies in the T-sample window of at least floor(T / step) outputs, in one component
    assert int(np.isnan(want).sum()) >= 2 * (T * ONE // SQRT2)
    ok = ~np.isnan(want)
    same(got.view(np.uint32)[ok], want.view(np.uint32)[ok], "around the non-finite samples")


@pytest.mark.parametrize("P,T,kernel,name", ANCHORS)
def test_anchor_subnormals(oracle, P, T, kernel, name):
    """A stream scaled into the subnormals: bit-exact, nothing is flushed."""
    h = arb_taps(P, T)
    n = 2000
    x = (streams(1, n, 15) * np.float32(2.0 ** -130)).astype(np.complex64)
    assert 0 < np.abs(x.view(np.float32)).max() < np.finfo(np.float32).tiny
    rig = Rig(oracle, x)
    plan = ArbitraryResampler(h, P, step=SQRT2)
    plan.set_kernel(kernel)
    want = rig.ref(h, P, SQRT2, plan.contract[0])
    assert np.count_nonzero(want.view(np.float32)) > want.size // 2
    same(rig.stream(plan, Stream(SQRT2), [n], [name]), want, "subnormal stream")


@pytest.mark.parametrize("kernel,name", [(KERNEL_TILED, TILED), (KERNEL_GENERIC, GENERIC)])
def test_anchor_fp64(oracle, kernel, name):
    """The fp64 definition within (2e-6 + 3 * 2^-24) sum|h| max|x| on one 128 x 32 stream, unit-gain taps."""
    h = design_arbitrary(128, 32, rate=1.0)
    n = 3000
    x = streams(1, n, 19)
    rig = Rig(oracle, x)
    plan = ArbitraryResampler(h, 128, step=SQRT2)
    plan.set_kernel(kernel)
    y = rig.stream(plan, Stream(SQRT2), [n], [name]).view(np.complex64)[0].astype(np.complex128)
    err = float(np.abs(y - arb_f64(h, 128, SQRT2, x[0])).max())
    print("128 x 32 %s: error %.3g, bound %.3g" % (name, err, bound(h, x[0])))
    assert err <= bound(h, x[0])


# ---- 7. every entry point takes its own kind alone ------------------------------------------------------------------------------
def test_entry_points_refuse_the_other_kinds(oracle):
    import ctypes as C
    import torch
    lib = sxxcvr_amd.load_sxfir()
    x = torch.zeros(4096, dtype=torch.complex64, device="cuda")
    y = torch.full((8192,), float("nan"), dtype=torch.complex64, device="cuda")
    n_out = C.c_size_t(7)
    ms = C.c_float()
    lp = sxxcvr_amd.design_lowpass(128, 4, 8.0, 1.0)
    others = [Resampler(DECIMATE, lp, 4), Resampler(INTERPOLATE, lp, 4), RationalResampler(rational_taps(4, 32), 4, 5),
              sxxcvr_amd.Channelizer(lp), sxxcvr_amd.Synthesizer(lp),
              Resampler(DECIMATE, sxxcvr_amd.design_bandpass(128, 4, 1, 4), 4)]
    for q in others:
        before = q.position
        n_out.value = 7
        assert lib.sxfir_resample_arbitrary(q._plan, x.data_ptr(), 1024, 1024, y.data_ptr(), 4096, C.byref(n_out), None) == EINVAL
        assert n_out.value == 0 and q.position == before and b"arbitrary-rate plan" in lib.sxfir_last_error()
        assert lib.sxfir_time_resample_arbitrary(q._plan, x.data_ptr(), 1024, 1024, y.data_ptr(), 4096, 1, None, C.byref(ms)) == EINVAL
    arb = ArbitraryResampler(arb_taps(128, 32), 128, step=SQRT2)
    state = (arb.position, arb.time)
    P = C.c_void_p
    calls = {"sxfir_resample": (arb._plan, P(x.data_ptr()), 1024, 1024, P(y.data_ptr()), 4096, C.byref(n_out), None),
             "sxfir_interpolate": (arb._plan, P(x.data_ptr()), 1024, 1024, P(y.data_ptr()), 4096, C.byref(n_out), None),
             "sxfir_decimate": (arb._plan, P(x.data_ptr()), 1024, 1024, P(y.data_ptr()), 4096, C.byref(n_out), None),
             "sxfir_channelize": (arb._plan, P(x.data_ptr()), 1024, 1024, P(y.data_ptr()), 4096, 1024, C.byref(n_out), None),
             "sxfir_synthesize": (arb._plan, P(x.data_ptr()), 256, 1024, 256, P(y.data_ptr()), 4096, C.byref(n_out), None),
             "sxfir_time_resample": (arb._plan, P(x.data_ptr()), 1024, 1024, P(y.data_ptr()), 4096, 1, None, C.byref(ms)),
             "sxfir_time_interpolate": (arb._plan, P(x.data_ptr()), 1024, 1024, P(y.data_ptr()), 4096, 1, None, C.byref(ms)),
             "sxfir_time_decimate": (arb._plan, P(x.data_ptr()), 1024, 1024, P(y.data_ptr()), 4096, 1, None, C.byref(ms))}
    for name, args in calls.items():
        n_out.value = 7
        assert getattr(lib, name)(*args) == EINVAL, name
        assert (arb.position, arb.time) == state, name
        if "time" not in name:
            assert n_out.value == 0, name
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert lib.sxfir_interpolate_keyed(arb._plan, P(x.data_ptr()), 1024, 1024, P(y.data_ptr()), 4096, C.byref(n_out), 0, 16, P(ctr.data_ptr()), None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.real).all()), "a refused call wrote to the output"
    # a call of 2^31 inputs or more is refused in front of either kernel (the call's relative time is 64 bits of Q32.32): nothing runs
    for kernel in (KERNEL_AUTO, KERNEL_GENERIC):
        arb.set_kernel(kernel)
        n_out.value = 7
        assert lib.sxfir_resample_arbitrary(arb._plan, x.data_ptr(), 1 << 31, 1 << 31, y.data_ptr(), 1 << 31, C.byref(n_out), None) == EINVAL
        assert n_out.value == 0 and (arb.position, arb.time) == state and b"too large" in lib.sxfir_last_error()
        assert lib.sxfir_time_resample_arbitrary(arb._plan, x.data_ptr(), 1 << 31, 1 << 31, y.data_ptr(), 1 << 31, 1, None, C.byref(ms)) == EINVAL
    arb.set_kernel(KERNEL_AUTO)
    # the timed entry point runs, and leaves position, time and history alone
    assert arb.time_resample_ptr(x.data_ptr(), 4096, 4096, y.data_ptr(), 8192, 2) > 0
    assert (arb.position, arb.time) == state
