"""Rational up / down resamplers on the GPU (include/sxfir_rational.h), bit for bit against the oracle as it stands
(tests/rational_cases.py: the oracle's interpolator pass, every down-th sample).

Every call goes through `Rig.call`: the output lands between two guards of fill words that must come back untouched, and the
plan's position, outputs_for and geometry(...)["kernel"] are checked around it."""
import ctypes as C

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import RationalResampler, Resampler, design_rational
from sxxcvr_amd.resampler import INTERPOLATE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED
from rational_cases import bound, gaussian_stream, n_out_for, rational_f64, rational_ref, rational_taps

pytestmark = pytest.mark.gpu

FILL = 0x7FC07FC0               # a NaN as one fp32 word and as two halves: no output of these streams is this word
GUARD = 8                       # samples of fill words on either side of a row's outputs (whole 16-byte units in both formats)
TILE = 1280                     # inputs per tile of resample45_kernel
TILED, GENERIC = "resample45_kernel", "resample_generic_kernel"
EINVAL, EUNSUPPORTED = -1, -4


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

    def ref(self, h, up, down, jsplit, first=0, count=None):
        """[nchan, words] of one pass over inputs [0, first + count) from zero history, the outputs of inputs [first, ..) alone"""
        count = self.n - first if count is None else count
        skip = n_out_for(first, up, down)
        return np.stack([self.words(rational_ref(self.oracle, h, up, down, self.x[c, :first + count], jsplit)[skip:]) for c in range(self.nchan)])

    def call(self, plan, pos, n, kernel=None, offset=0, expect=None, odd_stride=False):
        """sxfir_resample over inputs [pos, pos + n) of every row.  Returns [nchan, words]; with `expect` (an error code) the call
        must fail with it and leave the plan and the output buffer alone."""
        import torch
        up, down = plan.up, plan.down
        c0, p0 = plan.position
        assert p0 == n_out_for(c0, up, down)
        n_out = n_out_for(n, up, down, c0)
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
            assert plan.position == (c0, p0)
            assert np.all(buf.cpu().numpy().view(np.uint32) == FILL), "a refused call wrote to the output"
            return None
        assert plan.process_ptr(*args) == n_out
        torch.cuda.synchronize()
        assert plan.position == (c0 + n, p0 + n_out) and plan.position[1] == n_out_for(c0 + n, up, down)
        got = buf.cpu().numpy().view(np.uint32).reshape(self.nchan, row, self.wps)
        lo, hi = GUARD + offset, GUARD + offset + n_out
        assert np.all(got[:, :lo] == FILL) and np.all(got[:, hi:] == FILL), "the guard around the outputs was written"
        return np.ascontiguousarray(got[:, lo:hi]).reshape(self.nchan, n_out * self.wps)

    def stream(self, plan, blocks, kernels=None, pos=0):
        outs = []
        for i, b in enumerate(blocks):
            outs.append(self.call(plan, pos, b, None if kernels is None else kernels[i]))
            pos += b
        return np.concatenate(outs, axis=1)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.ravel() != want.ravel())[0]
    assert not bad.size, "%s: %d of %d words differ, first at %d: got %08x want %08x" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def streams(nchan, n, seed=3):
    return np.stack([gaussian_stream(n, seed + 17 * c) for c in range(nchan)])


# ---- 5. the generic kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("fmt", ["CF32", "CF16"])
@pytest.mark.parametrize("up,down,T", [(2, 3, 32), (3, 4, 8), (5, 4, 32), (3, 2, 16), (7, 5, 4), (4, 5, 16)])
def test_generic(oracle, up, down, T, fmt, nchan):
    """One call, and five calls: down - 1 samples, a single sample (which completes no output when up < down), another single
    sample (up > down: a call of no samples), 701 and the rest -- sizes that are no multiples of down."""
    h = rational_taps(up, T)
    n = 2311
    rig = Rig(oracle, streams(nchan, n), fmt)
    plan = RationalResampler(h, up, down, nchan=nchan, fmt=fmt)
    assert (plan.up, plan.down) == (up, down) and plan.mode == INTERPOLATE and not plan.complex_taps
    assert tuple(plan.contract) == ((2, 1) if T % 2 == 0 else (1, 1)) and plan.contract.rot == 0
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == EUNSUPPORTED
    ref = rig.ref(h, up, down, plan.contract[0])
    assert ref.shape[1] == n_out_for(n, up, down) * rig.wps
    same(rig.stream(plan, [n], [GENERIC]), ref, "one call")
    blocks = [down - 1, 1, 1 if up < down else 0, 701]
    if (n - sum(blocks)) % down == 0:
        blocks[3] += 1                      # (the last call is no multiple of down either)
    blocks.append(n - sum(blocks))
    assert blocks[0] % down and blocks[-1] % down
    if up < down:
        assert n_out_for(1, up, down, down - 1) == 0
    again = RationalResampler(h, up, down, nchan=nchan, fmt=fmt)
    same(rig.stream(again, blocks, [GENERIC] * 5), ref, "five calls %r" % blocks)


# ---- 6. the tiled kernel, 4/5 x 128 on CF32 ------------------------------------------------------------------------------------
TOTALS = [TILE - 5, TILE, 2 * TILE + 35, 3 * TILE + 7]


def plan45(h, kernel=KERNEL_AUTO, nchan=1):
    plan = RationalResampler(h, 4, 5, nchan=nchan)
    assert tuple(plan.contract) == (2, 1)
    plan.set_kernel(kernel)
    return plan


@pytest.mark.parametrize("n", TOTALS)
def test_tiled_auto_tiled_generic(oracle, n):
    h = rational_taps(4, 32)
    rig = Rig(oracle, streams(1, n, 5))
    ref = rig.ref(h, 4, 5, 2)
    g = plan45(h).geometry(n)
    assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == -(-n // TILE) and g["tile_samples"] == TILE, g
    same(rig.stream(plan45(h), [n], [TILED]), ref, "auto")
    same(rig.stream(plan45(h, KERNEL_TILED), [n], [TILED]), ref, "tiled")
    same(rig.stream(plan45(h, KERNEL_GENERIC), [n], [GENERIC]), ref, "generic")


@pytest.mark.parametrize("n", TOTALS)
def test_tiled_splits(oracle, n):
    """A stream split at multiples of 5 stays tiled; a split elsewhere runs the generic kernel for the call that starts off the
    period; a first call shorter than the history (3 samples), then the rest."""
    h = rational_taps(4, 32)
    rig = Rig(oracle, streams(1, n, 6))
    ref = rig.ref(h, 4, 5, 2)
    a, b = 5 * 77, 5 * 131
    same(rig.stream(plan45(h), [a, b, n - a - b], [TILED] * 3), ref, "split at multiples of 5")
    same(rig.stream(plan45(h), [a + 2, b, n - a - b - 2], [TILED, GENERIC, GENERIC]), ref, "split off the period")
    same(rig.stream(plan45(h), [a + 2, 3, n - a - 5], [TILED, GENERIC, TILED]), ref, "back on the period")
    same(rig.stream(plan45(h), [3, n - 3], [TILED, GENERIC]), ref, "3 samples, then the rest")


def test_tiled_refusals_change_nothing(oracle):
    """A forced TILED call that starts off the period, or whose output is offset by one sample: SXFIR_EUNSUPPORTED, the position
    and the next call's output as without it.  The same calls under AUTO: the generic kernel, the same bits."""
    h = rational_taps(4, 32)
    n = 2 * TILE + 35
    rig = Rig(oracle, streams(1, n, 7))
    ref = rig.ref(h, 4, 5, 2)
    n1 = 5 * 101 + 3
    k1 = n_out_for(n1, 4, 5) * rig.wps
    plan = plan45(h)
    same(rig.call(plan, 0, n1, TILED), ref[:, :k1], "first block")
    plan.set_kernel(KERNEL_TILED)
    rig.call(plan, n1, n - n1, GENERIC, expect=EUNSUPPORTED)
    assert b"multiple of 5" in plan._lib.sxfir_last_error()
    plan.set_kernel(KERNEL_AUTO)
    same(rig.call(plan, n1, n - n1, GENERIC), ref[:, k1:], "the call after the refused one")
    # an output pointer offset by one sample (8 bytes)
    plan = plan45(h, KERNEL_TILED)
    rig.call(plan, 0, n, TILED, offset=1, expect=EUNSUPPORTED)
    same(rig.call(plan, 0, n, TILED), ref, "the call after the refused one (offset output)")
    plan = plan45(h)
    same(rig.call(plan, 0, n, offset=1), ref, "offset output under AUTO")


@pytest.mark.parametrize("n", TOTALS)
def test_tiled_three_channels(oracle, n):
    h = rational_taps(4, 32)
    rig = Rig(oracle, streams(3, n, 8))
    ref = rig.ref(h, 4, 5, 2)
    same(rig.stream(plan45(h, KERNEL_TILED, nchan=3), [n], [TILED]), ref, "tiled")
    same(rig.stream(plan45(h, KERNEL_GENERIC, nchan=3), [5 * 33, n - 5 * 33], [GENERIC] * 2), ref, "generic")


def test_tiled_odd_output_stride(oracle):
    """Three channels whose output rows lie an odd number of samples apart break the 16-byte stores: the generic kernel under
    AUTO, the same bits; SXFIR_EUNSUPPORTED, plan untouched, under a forced TILED."""
    h = rational_taps(4, 32)
    n = TILE + 35
    rig = Rig(oracle, streams(3, n, 16))
    ref = rig.ref(h, 4, 5, 2)
    same(rig.call(plan45(h, nchan=3), 0, n, odd_stride=True), ref, "odd stride under AUTO")
    plan = plan45(h, KERNEL_TILED, nchan=3)
    rig.call(plan, 0, n, TILED, odd_stride=True, expect=EUNSUPPORTED)
    same(rig.call(plan, 0, n, TILED), ref, "the call after the refused one")


# ---- 6b. more tiles than waves: the tile loop's second iteration -------------------------------------------------------------
WALK_SEED = 0x45A7


def _walk(oracle, nchan=1, where=0):
    """One tiled call of 3 tiles and 35 samples more than the grid has waves (per channel), so that four waves walk on to a second
    tile -- the next tile's staging lands on an image the transposed stores have just read -- and the wave that carries the history
    over owns two tiles.  FORM_RAT45 has no heavy prologue: the grid is the plan's generations of resident waves, shared among the
    channels, whatever the call's size; geometry() of a very long call tells it.  The whole call is compared on the GPU with
    the plan's generic kernel over the same input (the sweep holds that one to the oracle); five windows of 200 outputs and the
    whole of a second tiled call of TILE + 8 samples are compared with the oracle's reference, from inputs regenerated for each
    window alone.  Returns the first call's geometry and size."""
    import torch
    h = rational_taps(4, 32)
    lead = 40 if where else 0                                   # (a placed plan: the samples in front are its history)
    assert where % 5 == 0 and lead % 5 == 0
    plans = [plan45(h, k, nchan) for k in (KERNEL_TILED, KERNEL_GENERIC)]
    per = plans[0].geometry(TILE << 20)["workgroups"] // nchan
    n, n2 = (per + 3) * TILE + 35, TILE + 8
    x = torch.empty((nchan, lead + n + n2), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, WALK_SEED, 50, 0)
    stream = torch.cuda.current_stream().cuda_stream
    for plan in plans:
        if where:
            plan.set_history_ptr(x.data_ptr(), lead, x.stride(0), stream)
            plan.set_position(where)
        assert plan.position == (where, where // 5 * 4)
    g = plans[0].geometry(n)
    G = g["workgroups"] // nchan                                # waves per channel: the first tile a wave reaches in its second iteration
    assert g["kernel"] == TILED and g["tiled"] and g["tile_samples"] == TILE and g["n_tiles"] == per + 4, g
    assert G < g["n_tiles"] and G == per, "no wave walks to a second tile: %r" % (g,)
    assert plans[1].geometry(n)["kernel"] == GENERIC

    def call(plan, pos, count):
        """sxfir_resample over inputs [pos, pos + count) of the stream (pos a multiple of 5), between guards of fill: the rows as
        int32 [nchan, row, 2]"""
        n_out = n_out_for(count, 4, 5)
        row = 2 * GUARD + n_out + n_out % 2
        buf = torch.full((nchan, row, 2), _i32(FILL), dtype=torch.int32, device="cuda")
        c0, p0 = plan.position
        assert plan.outputs_for(count) == n_out
        assert plan.process_ptr(x.data_ptr() + 8 * (lead + pos), count, x.stride(0), buf.data_ptr() + 8 * GUARD, row, stream) == n_out
        assert plan.position == (c0 + count, p0 + n_out)
        assert bool((buf[:, :GUARD] == _i32(FILL)).all()) and bool((buf[:, GUARD + n_out:] == _i32(FILL)).all()), "the guard around the outputs was written"
        return buf, n_out

    def window(c, m0, cnt):
        """[cnt, 2] words of outputs [m0, m0 + cnt) of the stream, m0 a multiple of 4 (a period's first), channel c: output 4 q + p
        reads inputs 5 q + p - 31 .. 5 q + p"""
        assert m0 % 4 == 0
        at = 5 * (m0 // 4)
        pre = min(35, lead + at)                                # whole periods in front of the window: the filter's reach, or all there are
        assert pre == 35 or (pre == at and lead == 0)
        count = min(5 * (cnt + 3) // 4 + 2, n + n2 - at)
        xw = oracle.synth_iq(WALK_SEED, 50 + c, lead + at - pre, pre + count)
        skip = pre // 5 * 4
        ref = rational_ref(oracle, h, 4, 5, xw, 2)[skip:skip + cnt]
        assert ref.size == cnt
        return ref.view(np.uint32).reshape(cnt, 2)

    got, n_out = call(plans[0], 0, n)
    other, _ = call(plans[1], 0, n)
    torch.cuda.synchronize()
    assert torch.equal(got, other), "the tiled and the generic kernel differ: first at output %d of channel %d" % (
        int((got != other).any(dim=2).nonzero()[0, 1]) - GUARD, int((got != other).any(dim=2).nonzero()[0, 0]))
    assert n_out == (per + 3) * 1024 + 28
    starts = {"the stream's start": 0, "the first tile of a second iteration": G * 1024, "the seam in front of it": G * 1024 - 100,
              "the middle": n_out // 2 // 4 * 4 + 4, "the last, ragged tile": n_out - 200}
    for what, m0 in starts.items():
        for c in range(nchan):
            same(got[c, GUARD + m0:GUARD + m0 + 200].cpu().numpy().view(np.uint32), window(c, m0, 200), "%s, channel %d" % (what, c))
    # the history was carried over by a wave that owned more than one tile
    assert (g["n_tiles"] - 1) % G < g["n_tiles"] - G
    assert plans[0].geometry(n2)["kernel"] == TILED
    second, n_out2 = call(plans[0], n, n2)
    torch.cuda.synchronize()
    for c in range(nchan):
        same(second[c, GUARD:GUARD + n_out2].cpu().numpy().view(np.uint32), window(c, n_out, n_out2), "the call after it, channel %d" % c)
    print("4/5 x %d ch from %d: resident %d, grid %d per channel, %d tiles, %d samples" % (nchan, where, g["resident"], G, g["n_tiles"], n))
    return g, n


def test_more_tiles_than_resident_workgroups(oracle):
    """One channel: the grid, whole generations of the chip's resident waves, is a multiple of 8 -- the XCD-blocked dealing."""
    g, n = _walk(oracle)
    assert g["workgroups"] % g["resident"] == 0 and g["workgroups"] % 8 == 0, g


def test_more_tiles_than_workgroups_plainly_strided(oracle):
    """The smallest channel count above one whose share of the grid is no multiple of 8: the tiles are dealt plainly strided."""
    grid = plan45(rational_taps(4, 32)).geometry(TILE << 20)["workgroups"]
    nchan = next(c for c in range(2, 64) if (grid // c) % 8)
    g, n = _walk(oracle, nchan=nchan)
    assert (g["workgroups"] // nchan) % 8 != 0, g


def test_more_tiles_than_resident_workgroups_far(oracle):
    """The same many-tile call on a plan placed at input 5 (2^40 + 3): a start on the period that is no small multiple of 5."""
    _walk(oracle, where=5 * ((1 << 40) + 3))


# ---- 7. without the oracle: every down-th output of the interpolator plan --------------------------------------------------
@pytest.mark.parametrize("fmt", ["CF32", "CF16"])
@pytest.mark.parametrize("up,down,T", [(4, 5, 32), (3, 4, 8)])
def test_equals_the_interpolator_decimated(oracle, up, down, T, fmt):
    import torch
    h = design_rational(up, down, T)
    n = 2 * TILE + 35
    rig = Rig(oracle, streams(1, n, 9), fmt)
    interp = Resampler(INTERPOLATE, h, up, fmt=fmt)
    x = rig.xg[0, :n * rig.wps]
    y = interp.process(torch.view_as_complex(x.view(torch.float32).view(-1, 2)) if fmt == "CF32" else x)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    want = (y.view(np.uint32).reshape(-1, 2) if fmt == "CF32" else y.view(np.uint32).reshape(-1, 1))[::down][:n_out_for(n, up, down)]
    plan = RationalResampler(h, up, down, fmt=fmt)
    name = TILED if (up, down, T, fmt) == (4, 5, 32, "CF32") else GENERIC
    same(rig.stream(plan, [n], [name]), want.reshape(1, -1), "%d/%d against x%d" % (up, down, up))


# ---- 8. take-over --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down,T", [(4, 5, 32), (3, 4, 8)])
def test_take_over_and_reset(oracle, up, down, T):
    """A second plan, given the tail of the consumed input as its history and the stream position, goes on with the bits of the
    uninterrupted run; sxfir_reset puts a plan back at the stream's start."""
    import torch
    h = rational_taps(up, T)
    n, consumed = 2 * TILE + 35, 1003
    assert consumed % down and consumed % 5
    rig = Rig(oracle, streams(2, n, 10))
    jsplit = 2 if T % 2 == 0 else 1
    ref = rig.ref(h, up, down, jsplit)
    whole = RationalResampler(h, up, down, nchan=2)
    same(rig.stream(whole, [n]), ref, "uninterrupted")
    k = n_out_for(consumed, up, down) * rig.wps
    second = RationalResampler(h, up, down, nchan=2)
    second.set_history_ptr(rig.xg.data_ptr(), consumed, rig.stride, torch.cuda.current_stream().cuda_stream)
    second.set_position(consumed)
    assert second.position == (consumed, n_out_for(consumed, up, down))
    same(rig.call(second, consumed, n - consumed, GENERIC), ref[:, k:], "taken over at %d" % consumed)
    whole.reset()
    assert whole.position == (0, 0)
    same(rig.call(whole, 0, consumed), ref[:, :k], "after reset")


# ---- 9. the frame --------------------------------------------------------------------------------------------------------------
def test_frame(oracle):
    import torch
    lib = sxxcvr_amd.load_sxfir()
    vp = C.c_void_p
    h = rational_taps(4, 32)
    n = TILE + 35
    rig = Rig(oracle, streams(3, n, 12))
    ref = rig.ref(h, 4, 5, 2)
    plan = RationalResampler(h, 4, 5, nchan=3)
    n1 = 5 * 61
    k1 = n_out_for(n1, 4, 5) * rig.wps
    same(rig.call(plan, 0, n1, TILED), ref[:, :k1], "first block")
    pos = plan.position
    out = torch.full((3, 8 * n), 0.0, dtype=torch.complex64, device="cuda")
    got, ms, counter = C.c_size_t(77), C.c_float(), torch.zeros(1, dtype=torch.int64, device="cuda")
    io = (plan._plan, vp(rig.xg.data_ptr() + 8 * n1), n - n1, rig.stride, vp(out.data_ptr()), 8 * n)
    refused = {
        "sxfir_decimate": lambda: lib.sxfir_decimate(*io, C.byref(got), None),
        "sxfir_interpolate": lambda: lib.sxfir_interpolate(*io, C.byref(got), None),
        "sxfir_interpolate_keyed": lambda: lib.sxfir_interpolate_keyed(*io, C.byref(got), 0, 8, vp(counter.data_ptr()), None),
        "sxfir_time_decimate": lambda: lib.sxfir_time_decimate(*io, 1, None, C.byref(ms)),
        "sxfir_time_interpolate": lambda: lib.sxfir_time_interpolate(*io, 1, None, C.byref(ms)),
        "sxfir_channelize": lambda: lib.sxfir_channelize(*io, 2 * n, C.byref(got), None),
        "sxfir_synthesize": lambda: lib.sxfir_synthesize(*io[:4], 2 * n, *io[4:], C.byref(got), None),
    }
    for name, fn in refused.items():
        got.value = 77
        assert fn() == EINVAL, name
        assert b"sxfir_resample" in lib.sxfir_last_error(), (name, lib.sxfir_last_error())
        assert plan.position == pos, name
        assert got.value in (0, 77), name
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and float(out.abs().max().item()) == 0.0
    # a NULL buffer with samples to read, and rows of three channels that would overlap
    assert lib.sxfir_resample(plan._plan, None, n - n1, rig.stride, vp(out.data_ptr()), 8 * n, C.byref(got), None) == EINVAL
    assert lib.sxfir_resample(plan._plan, io[1], n - n1, rig.stride, None, 8 * n, C.byref(got), None) == EINVAL
    assert lib.sxfir_resample(plan._plan, io[1], n - n1, rig.stride, vp(out.data_ptr()), plan.outputs_for(n - n1) - 1, C.byref(got), None) == EINVAL
    assert plan.position == pos
    # sxfir_time_resample leaves the position (and the history) as it was
    assert plan.time_resample_ptr(io[1].value, n - n1, rig.stride, out.data_ptr(), 8 * n, 2) > 0.0
    torch.cuda.synchronize()
    assert plan.position == pos
    same(rig.call(plan, n1, n - n1, TILED), ref[:, k1:], "the call after the refused ones")
    # sxfir_resample takes no other kind; sxfir_plan_rational tells them apart
    h4 = sxxcvr_amd.design_lowpass(128, 4)
    others = {"real": Resampler(0, h4, 4), "complex": Resampler(0, sxxcvr_amd.design_bandpass(128, 4, 1, 4), 4),
              "channelizer": sxxcvr_amd.Channelizer(h4)}
    up, down = C.c_int(-1), C.c_int(-1)
    for name, p in others.items():
        got.value = 77
        assert lib.sxfir_resample(p._plan, vp(rig.xg.data_ptr()), 64, rig.stride, vp(out.data_ptr()), 8 * n, C.byref(got), None) == EINVAL, name
        assert got.value == 0 and p.position == (0, 0), name
        assert lib.sxfir_time_resample(p._plan, vp(rig.xg.data_ptr()), 64, rig.stride, vp(out.data_ptr()), 8 * n, 1, None, C.byref(ms)) == EINVAL, name
        assert lib.sxfir_plan_rational(p._plan, C.byref(up), C.byref(down)) == 0 and (up.value, down.value) == (0, 0), name
    assert lib.sxfir_plan_rational(plan._plan, C.byref(up), C.byref(down)) == 0 and (up.value, down.value) == (4, 5)
    assert lib.sxfir_plan_rational(plan._plan, None, C.byref(down)) == EINVAL
    rot, bands, cx = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.sxfir_contract_rotation(plan._plan, C.byref(rot)) == 0 and rot.value == 0
    for query in ("sxfir_plan_bands", "sxfir_plan_oversampling", "sxfir_plan_synthesis_bands", "sxfir_plan_synthesis_oversampling"):
        assert getattr(lib, query)(plan._plan, C.byref(bands)) == 0 and bands.value == 0, query
    assert lib.sxfir_taps_are_complex(plan._plan, C.byref(cx)) == 0 and cx.value == 0
    # no tiled kernel but at 4/5 x 128 on CF32
    for args, kw in (((rational_taps(2, 32), 2, 3), {}), ((h, 4, 5), {"fmt": "CF16"})):
        p = RationalResampler(*args, **kw)
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            p.set_kernel(KERNEL_TILED)
        assert ei.value.code == EUNSUPPORTED
        assert p.geometry(TILE)["kernel"] == GENERIC


# ---- 10. anchors ---------------------------------------------------------------------------------------------------------------
ANCHORS = [(4, 5, 32, KERNEL_TILED, TILED), (4, 5, 32, KERNEL_GENERIC, GENERIC), (3, 4, 8, KERNEL_GENERIC, GENERIC)]


@pytest.mark.parametrize("up,down,T,kernel,name", ANCHORS)
def test_anchor_fp64(oracle, up, down, T, kernel, name):
    h = design_rational(up, down, T)
    n = 2 * TILE + 35
    x = streams(1, n, 13)
    rig = Rig(oracle, x)
    plan = RationalResampler(h, up, down)
    plan.set_kernel(kernel)
    y = rig.stream(plan, [n], [name]).view(np.complex64)[0].astype(np.complex128)
    err = float(np.abs(y - rational_f64(h, up, down, x[0])).max())
    print("%d/%d x %d %s: error %.3g, bound %.3g" % (up, down, T, name, err, bound(h, x[0])))
    assert err <= bound(h, x[0])


@pytest.mark.parametrize("up,down,T,kernel,name", ANCHORS)
def test_anchor_non_finite(oracle, up, down, T, kernel, name):
    """One +Inf and one NaN sample: non-finite outputs exactly where the reference has them (NaNs compared as NaNs, not by
    payload), the same bits everywhere else."""
    h = rational_taps(up, T)
    n = 2 * TILE + 35
    x = streams(1, n, 14)
    x[0, 700] = np.complex64(complex(np.inf, 0.25))
    x[0, 1900] = np.complex64(complex(-0.5, np.nan))
    rig = Rig(oracle, x)
    plan = RationalResampler(h, up, down)
    plan.set_kernel(kernel)
    got = rig.stream(plan, [n], [name]).view(np.float32)[0]
    want = rig.ref(h, up, down, plan.contract[0]).view(np.float32)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.isinf(want).any()
    ok = ~np.isnan(want)
    same(got.view(np.uint32)[ok], want.view(np.uint32)[ok], "around the non-finite samples")


@pytest.mark.parametrize("up,down,T,kernel,name", ANCHORS)
def test_anchor_subnormals(oracle, up, down, T, kernel, name):
    """A stream scaled into the subnormals: bit-exact, nothing is flushed."""
    h = rational_taps(up, T)
    n = 2 * TILE + 35
    x = (streams(1, n, 15) * np.float32(2.0 ** -130)).astype(np.complex64)
    assert 0 < np.abs(x.view(np.float32)).max() < np.finfo(np.float32).tiny
    rig = Rig(oracle, x)
    plan = RationalResampler(h, up, down)
    plan.set_kernel(kernel)
    want = rig.ref(h, up, down, plan.contract[0])
    assert np.count_nonzero(want.view(np.float32)) > want.size // 2
    same(rig.stream(plan, [n], [name]), want, "subnormal stream")
