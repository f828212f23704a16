"""Frequency-translating decimators on the GPU (include/sxfir_translate.h), bit for bit against tests/mix_cases.py: the complex-tap
decimator's oracle reference, rotated in float32 on the table of sxfir_design_rotator.

Every call goes through `Rig.call`: the output lands between two guards of fill words that must come back untouched, and the
plan's position, outputs_for and geometry(...)["kernel"] are checked around it."""
import ctypes as C

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import Resampler, TranslatingDecimator, design_bandpass, design_rotator
from sxxcvr_amd.resampler import DECIMATE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED
from gpu_util import random_taps_cx
from mix_cases import bound, mix_f64, mix_ref, rotate_f32, step
from rational_cases import gaussian_stream

pytestmark = pytest.mark.gpu

FILL = 0x7FC07FC0               # a NaN as one fp32 word and as two halves: no output of these streams is this word
GUARD = 8                       # samples of fill words on either side of a row's outputs (whole 16-byte units in both formats)
TILE = 2048                     # inputs per tile of decim4_mix_kernel
TILED, GENERIC = "decim4_mix_kernel", "decim_mix_generic_kernel"
EINVAL, EUNSUPPORTED = -1, -4
PAIRS = [(3, 7), (123, 1000), (12345, 65536), (1, 4)]         # (3, 7): the table wraps inside a lane's eight outputs; (1, 4): s = 0 at /4
TOTALS = [TILE - 4, TILE, 2 * TILE + 140, 3 * TILE + 28]


def _i32(word):
    return word - (1 << 32) if word >= 1 << 31 else word


def cdiv(a, b):
    return -(-a // b)


class Rig:
    """One stream [nchan, n] on the GPU (rows `pad` samples longer than the stream: strides larger than the block) and its CPU twin
    as the plan sees it (CF16: quantised to half; S32: wire words, the twin what convert_rx makes of them)."""

    def __init__(self, oracle, x, fmt="CF32", pad=41):
        import torch
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex64)
        self.oracle, self.fmt, self.nchan, self.n = oracle, fmt, x.shape[0], x.shape[1]
        self.sb_in, self.wps_in = (4, 1) if fmt == "CF16" else (8, 2)          # input: bytes, 32-bit words per sample
        self.sb, self.wps = self.sb_in, self.wps_in                           # output (S32 words in: CF32 out, 8 bytes too)
        self.stride = self.n + pad
        if fmt == "CF16":
            h16 = oracle.f32_to_f16(x.view(np.float32))
            self.x = oracle.f16_to_f32(h16).view(np.complex64)
            words = np.ascontiguousarray(h16).view(np.int32)
        elif fmt == "S32":
            rng = np.random.default_rng(77)                                    # (x gives the shape alone: any word is a sample)
            words = rng.integers(-2 ** 31, 2 ** 31, size=(self.nchan, 2 * self.n), dtype=np.int64).astype(np.int32)
            self.x = np.stack([oracle.convert_rx(words[c]) for c in range(self.nchan)])
        else:
            self.x = x
            words = x.view(np.int32)
        buf = np.zeros((self.nchan, self.stride * self.wps_in), dtype=np.int32)
        buf[:, :words.shape[1]] = words
        self.xg = torch.from_numpy(buf).cuda()

    def words(self, y):
        """complex64 [.., n] reference -> the 32-bit words the plan stores"""
        y = np.ascontiguousarray(y, dtype=np.complex64)
        if self.fmt == "CF16":
            return np.ascontiguousarray(self.oracle.f32_to_f16(y.view(np.float32))).view(np.uint32)
        return y.view(np.uint32)

    def ref(self, h, ratio, contract, num, den, first=0, count=None, m_first=None):
        """[nchan, words] of one pass over inputs [0, first + count) from zero history, the outputs of inputs [first, ..) alone; the
        first of THOSE has the absolute index m_first (default: its index in this stream)."""
        count = self.n - first if count is None else count
        skip = cdiv(first, ratio)
        m0 = 0 if m_first is None else m_first - skip
        return np.stack([self.words(mix_ref(self.oracle, h, ratio, self.x[c, :first + count], contract, num, den, m0)[skip:])
                         for c in range(self.nchan)])

    def call(self, plan, pos, n, kernel=None, offset=0, expect=None, odd_stride=False):
        """sxfir_decimate over inputs [pos, pos + n) of every row.  Returns [nchan, words]; with `expect` (an error code) the call
        must fail with it and leave the plan and the output buffer alone."""
        import torch
        D = plan.ratio
        c0, p0 = plan.position
        assert p0 == cdiv(c0, D)
        n_out = cdiv(c0 + n, D) - p0
        assert plan.outputs_for(n) == n_out
        if kernel is not None:
            assert plan.geometry(n)["kernel"] == kernel, (plan.geometry(n), kernel)
        row = 2 * GUARD + offset + n_out + (offset + n_out) % 2               # an even stride, larger than the block
        row += 1 if odd_stride else 0
        buf = torch.full((self.nchan, row * self.wps), _i32(FILL), dtype=torch.int32, device="cuda")
        args = (self.xg.data_ptr() + self.sb_in * pos, n, self.stride, buf.data_ptr() + self.sb * (GUARD + offset), row,
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
        assert plan.position == (c0 + n, p0 + n_out)
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


def plan4(h, num, den, kernel=KERNEL_AUTO, nchan=1):
    plan = TranslatingDecimator(h, 4, num, den, nchan=nchan)
    assert plan.complex_taps and plan.mode == DECIMATE and tuple(plan.contract) == (2, 4) and plan.contract.rot == 0
    assert (plan.num, plan.den) == (num % den, den)
    plan.set_kernel(kernel)
    return plan


H4 = random_taps_cx(128, 31)


# ---- the tiled kernel, /4 x 128 on CF32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("num,den", PAIRS)
@pytest.mark.parametrize("n", TOTALS)
def test_tiled_auto_tiled_generic(oracle, n, num, den):
    rig = Rig(oracle, streams(1, n, 5))
    g = plan4(H4, num, den).geometry(n)
    assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == cdiv(n, TILE) and g["tile_samples"] == TILE, g
    ref = rig.ref(H4, 4, plan4(H4, num, den).contract, num, den)
    assert ref.shape[1] == 2 * (n // 4)
    same(rig.stream(plan4(H4, num, den), [n], [TILED]), ref, "auto")
    same(rig.stream(plan4(H4, num, den, KERNEL_TILED), [n], [TILED]), ref, "tiled")
    same(rig.stream(plan4(H4, num, den, KERNEL_GENERIC), [n], [GENERIC]), ref, "generic")


def test_negative_num_is_reduced(oracle):
    n = TILE + 140
    rig = Rig(oracle, streams(1, n, 4))
    plan = TranslatingDecimator(H4, 4, -4 - 7 * 1000, 7)
    assert (plan.num, plan.den) == (3, 7)
    same(rig.stream(plan, [n], [TILED]), rig.ref(H4, 4, plan.contract, 3, 7), "num = -7004 is 3 mod 7")


@pytest.mark.parametrize("num,den", [(123, 1000), (3, 7)])
@pytest.mark.parametrize("n", [TOTALS[0], TOTALS[3]])
def test_splits(oracle, n, num, den):
    """A stream cut at multiples of 4 stays tiled; a cut elsewhere runs the generic kernel for the call that starts off the output
    boundary and the stream comes back; a first call shorter than the 128-sample history; five calls through both kernels give the
    bits of one call: the phase is continuous."""
    rig = Rig(oracle, streams(1, n, 6))
    ref = rig.ref(H4, 4, plan4(H4, num, den).contract, num, den)
    a, b = 4 * 77, 4 * 131
    same(rig.stream(plan4(H4, num, den), [a, b, n - a - b], [TILED] * 3), ref, "cut at multiples of 4")
    same(rig.stream(plan4(H4, num, den), [a + 2, b, n - a - b - 2], [TILED, GENERIC, GENERIC]), ref, "cut off the boundary")
    same(rig.stream(plan4(H4, num, den), [a + 2, 2, n - a - 4], [TILED, GENERIC, TILED]), ref, "back on the boundary")
    same(rig.stream(plan4(H4, num, den), [100, n - 100], [TILED, TILED]), ref, "100 samples, then the rest")
    same(rig.stream(plan4(H4, num, den), [a + 2, 2, 100, 3, n - a - 107], [TILED, GENERIC, TILED, TILED, GENERIC]), ref, "five calls")


@pytest.mark.parametrize("num,den", [(12345, 65536), (3, 7)])
def test_far_positions(oracle, num, den):
    """A plan placed at input 2^40 + 4 k with the history of the samples in front: one tiled and one generic call carry the phase of
    output 2^38 + k -- the 64-bit phase, without a long stream.  sxfir_reset returns the phase to 0."""
    import torch
    lead, n1 = 256, TILE + 6
    n = lead + n1 + TILE + 30
    where = (1 << 40) + 4 * 5
    rig = Rig(oracle, streams(1, n, 7))
    plan = plan4(H4, num, den)
    plan.set_history_ptr(rig.xg.data_ptr(), lead, rig.stride, torch.cuda.current_stream().cuda_stream)
    plan.set_position(where)
    assert plan.position == (where, where // 4)
    ref = rig.ref(H4, 4, plan.contract, num, den, first=lead, m_first=where // 4)
    got = rig.stream(plan, [n1, n - lead - n1], [TILED, GENERIC], pos=lead)
    same(got, ref, "from input 2^40 + 20")
    near = rig.ref(H4, 4, plan.contract, num, den, first=lead)
    assert np.count_nonzero(near != ref) > ref.size // 2, "the far phase is not the near one"
    plan.reset()
    assert plan.position == (0, 0)
    same(rig.call(plan, 0, TILE + 8, TILED), rig.ref(H4, 4, plan.contract, num, den, count=TILE + 8), "after reset")


@pytest.mark.parametrize("n", [TOTALS[2]])
def test_three_channels(oracle, n):
    num, den = 123, 1000
    rig = Rig(oracle, streams(3, n, 8))
    ref = rig.ref(H4, 4, plan4(H4, num, den).contract, num, den)
    same(rig.stream(plan4(H4, num, den, KERNEL_TILED, nchan=3), [n], [TILED]), ref, "tiled")
    same(rig.stream(plan4(H4, num, den, KERNEL_GENERIC, nchan=3), [4 * 33 + 1, n - 4 * 33 - 1], [GENERIC] * 2), ref, "generic")


def test_odd_stride_and_offset_output(oracle):
    """Output rows an odd number of samples apart, or an output offset by one sample, break the 16-byte stores: the generic kernel
    under AUTO, the same bits; SXFIR_EUNSUPPORTED, plan and output untouched, under a forced TILED."""
    num, den = 3, 7
    n = TILE + 140
    rig = Rig(oracle, streams(3, n, 16))
    ref = rig.ref(H4, 4, plan4(H4, num, den).contract, num, den)
    same(rig.call(plan4(H4, num, den, nchan=3), 0, n, odd_stride=True), ref, "odd stride under AUTO")
    same(rig.call(plan4(H4, num, den, nchan=3), 0, n, offset=1), ref, "offset output under AUTO")
    plan = plan4(H4, num, den, KERNEL_TILED, nchan=3)
    rig.call(plan, 0, n, TILED, odd_stride=True, expect=EUNSUPPORTED)
    rig.call(plan, 0, n, TILED, offset=1, expect=EUNSUPPORTED)
    same(rig.call(plan, 0, n, TILED), ref, "the call after the refused ones")
    # a forced TILED call that starts off the output boundary
    plan = plan4(H4, num, den, nchan=3)
    k1 = 2 * cdiv(4 * 50 + 1, 4)
    same(rig.call(plan, 0, 4 * 50 + 1, TILED), ref[:, :k1], "first block")
    plan.set_kernel(KERNEL_TILED)
    rig.call(plan, 4 * 50 + 1, n - 4 * 50 - 1, GENERIC, expect=EUNSUPPORTED)
    plan.set_kernel(KERNEL_AUTO)
    same(rig.call(plan, 4 * 50 + 1, n - 4 * 50 - 1, GENERIC), ref[:, k1:], "the call after the refused one")


# ---- more tiles than waves: the tile loop's second iteration ----------------------------------------------------------------------
WALK_SEED = 0x3A1C


def _walk(oracle, num, den, nchan=1, where=0):
    """One tiled call of 3 tiles and 140 samples more than the grid has waves (per channel), so that four waves walk on to a second
    tile -- `tile_ph += stride_step` and its wrap, the next tile's staging over an image the stores have just read -- and the wave
    that carries the history over owns two tiles.  FORM_MIX has the heavy prologue: a call this small is dealt as one generation,
    the grid per channel is resident / nchan.  The whole call is compared on the GPU with the plan's generic kernel over the same
    input (the sweep holds that one to the oracle); five windows of 200 outputs and the whole of a second tiled call of TILE + 8
    samples are compared with the oracle's reference, from inputs regenerated for each window alone.  Returns the first call's
    geometry and size."""
    import torch
    lead = 256 if where else 0                                  # (a placed plan: the samples in front are its history)
    assert where % 4 == 0 and lead % 4 == 0
    plans = [plan4(H4, num, den, k, nchan) for k in (KERNEL_TILED, KERNEL_GENERIC)]
    contract = plans[0].contract
    per = plans[0].geometry(TILE)["resident"] // nchan
    n, n2 = (per + 3) * TILE + 140, TILE + 8
    x = torch.empty((nchan, lead + n + n2), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, WALK_SEED, 40, 0)
    stream = torch.cuda.current_stream().cuda_stream
    for plan in plans:
        if where:
            plan.set_history_ptr(x.data_ptr(), lead, x.stride(0), stream)
            plan.set_position(where)
        assert plan.position == (where, where // 4)
    g = plans[0].geometry(n)
    G = g["workgroups"] // nchan                                # waves per channel: the first tile a wave reaches in its second iteration
    assert g["kernel"] == TILED and g["tiled"] and g["tile_samples"] == TILE and g["n_tiles"] == per + 4, g
    assert G < g["n_tiles"] and G == per, "no wave walks to a second tile: %r" % (g,)
    assert plans[1].geometry(n)["kernel"] == GENERIC

    def call(plan, pos, count):
        """sxfir_decimate over inputs [pos, pos + count) of the stream, between guards of fill: the rows as int32 [nchan, row, 2]"""
        n_out = count // 4
        row = 2 * GUARD + n_out + n_out % 2
        buf = torch.full((nchan, row, 2), _i32(FILL), dtype=torch.int32, device="cuda")
        c0, p0 = plan.position
        assert plan.outputs_for(count) == n_out
        assert plan.process_ptr(x.data_ptr() + 8 * (lead + pos), count, x.stride(0), buf.data_ptr() + 8 * GUARD, row, stream) == n_out
        assert plan.position == (c0 + count, p0 + n_out)
        assert bool((buf[:, :GUARD] == _i32(FILL)).all()) and bool((buf[:, GUARD + n_out:] == _i32(FILL)).all()), "the guard around the outputs was written"
        return buf, n_out

    def window(c, m0, cnt):
        """[cnt, 2] words of outputs [m0, m0 + cnt) of the stream (its first output: the absolute where / 4), channel c"""
        pre = min(128, lead + 4 * m0)                           # samples in front of the window: the filter's reach, or all there are
        assert pre == 128 or (pre == 4 * m0 and lead == 0)
        xw = oracle.synth_iq(WALK_SEED, 40 + c, lead + 4 * m0 - pre, pre + 4 * cnt)
        return mix_ref(oracle, H4, 4, xw, contract, num, den, where // 4 + m0 - pre // 4)[pre // 4:].view(np.uint32).reshape(cnt, 2)

    got, n_out = call(plans[0], 0, n)
    other, _ = call(plans[1], 0, n)
    torch.cuda.synchronize()
    assert torch.equal(got, other), "the tiled and the generic kernel differ: first at output %d of channel %d" % (
        int((got != other).any(dim=2).nonzero()[0, 1]) - GUARD, int((got != other).any(dim=2).nonzero()[0, 0]))
    starts = {"the stream's start": 0, "the first tile of a second iteration": G * 512, "the seam in front of it": G * 512 - 100,
              "the middle": n_out // 2 + 3, "the last, ragged tile": n_out - 200}
    assert n_out % 512 == 35
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
    print("%d/%d x %d ch from %d: resident %d, grid %d per channel, %d tiles, %d samples" % (num, den, nchan, where, g["resident"], G, g["n_tiles"], n))
    return g, n


@pytest.mark.parametrize("num,den,s", [(3, 7, 5), (65535, 65536, 65532), (65534, 65535, 65531), (1, 3, 1)])
def test_more_tiles_than_resident_workgroups(oracle, num, den, s):
    """One channel: the grid is the chip's resident waves, a multiple of 8 -- the XCD-blocked dealing (w8 != 0).  (3, 7) and (1, 3):
    more tiles than table entries, so `tile % den` wraps for an s that is not 0, and a lane's index wraps inside its eight reads;
    (65535, 65536) and (65534, 65535): s at the top of the table (the largest /4 allows; den - 4 on the odd den)."""
    assert step(num, den, 4) == s
    g, n = _walk(oracle, num, den)
    assert g["workgroups"] == g["resident"] and g["resident"] % 8 == 0, g
    assert den > 8 or g["n_tiles"] > den


def test_more_tiles_than_workgroups_three_channels(oracle):
    """Three channels (or the count in 2..5 that does it): the grid per channel is no multiple of 8, so the tiles are dealt plainly
    strided (w8 = 0)."""
    resident = plan4(H4, 123, 1000).geometry(TILE)["resident"]
    nchan = next(c for c in (3, 2, 4, 5) if (resident // c) % 8 and (resident // c * c) % 8)
    g, n = _walk(oracle, 123, 1000, nchan=nchan)
    assert (g["workgroups"] // nchan) % 8 != 0 and g["workgroups"] % 8 != 0, g


def test_more_tiles_than_resident_workgroups_far(oracle):
    """The same many-tile call on a plan placed at input 2^40 + 20: the call's phase comes from a 64-bit position."""
    _walk(oracle, 12345, 65536, where=(1 << 40) + 20)


# ---- the generic kernel at the shapes and formats without a tiled one ----------------------------------------------------------
@pytest.mark.parametrize("ntaps,D,fmt,contract", [(256, 8, "CF32", (2, 4, 0)), (35, 5, "CF32", (1, 5, 0)), (1536, 48, "CF32", (2, 4, 1)),
                                                  (128, 4, "CF16", (2, 4, 0)), (128, 4, "S32", (2, 4, 0))])
@pytest.mark.parametrize("num,den", [(123, 1000), (3, 7)])
def test_generic_shapes(oracle, ntaps, D, fmt, contract, num, den):
    h = random_taps_cx(ntaps, 9)
    n = D * 300 + 3
    rig = Rig(oracle, streams(2, n, 9), fmt)
    plan = TranslatingDecimator(h, D, num, den, nchan=2, fmt=fmt)
    c = plan.contract
    assert c.rot == contract[2] and tuple(c) == contract[:2], (tuple(c), c.rot)
    assert plan.complex_taps
    g = plan.geometry(n)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == EUNSUPPORTED
    ref = rig.ref(h, D, plan.contract, num, den)
    same(rig.stream(plan, [n], [GENERIC]), ref, "one call")
    again = TranslatingDecimator(h, D, num, den, nchan=2, fmt=fmt)
    same(rig.stream(again, [D * 7 + 1, 1, n - D * 7 - 2], [GENERIC] * 3), ref, "three calls")


# ---- without the oracle: the complex plan's output on the GPU, rotated ----------------------------------------------------------
@pytest.mark.parametrize("ntaps,D,name", [(128, 4, TILED), (35, 5, GENERIC)])
@pytest.mark.parametrize("num,den", [(12345, 65536), (1, 4)])
def test_equals_the_complex_plan_rotated(oracle, ntaps, D, name, num, den):
    import torch
    h = random_taps_cx(ntaps, 12)
    n = 2 * TILE + 140
    rig = Rig(oracle, streams(1, n, 10))
    cx = Resampler(DECIMATE, h, D)
    z = cx.process(torch.view_as_complex(rig.xg[0, :2 * n].view(torch.float32).view(-1, 2)))
    torch.cuda.synchronize()
    want = rotate_f32(z.cpu().numpy(), design_rotator(den), 0, step(num, den, D), den)
    plan = TranslatingDecimator(h, D, num, den)
    same(rig.stream(plan, [n], [name]), want.view(np.uint32).reshape(1, -1), "/%d x %d against the complex plan" % (D, ntaps))


# ---- the frame -----------------------------------------------------------------------------------------------------------------
def test_frame(oracle):
    import torch
    lib = sxxcvr_amd.load_sxfir()
    vp = C.c_void_p
    num, den = 123, 1000
    n = TILE + 140
    rig = Rig(oracle, streams(3, n, 12))
    plan = plan4(H4, num, den, nchan=3)
    ref = rig.ref(H4, 4, plan.contract, num, den)
    n1 = 4 * 61
    k1 = 2 * (n1 // 4)
    same(rig.call(plan, 0, n1, TILED), ref[:, :k1], "first block")
    pos = plan.position
    out = torch.full((3, 8 * n), 0.0, dtype=torch.complex64, device="cuda")
    got, ms, counter = C.c_size_t(77), C.c_float(), torch.zeros(1, dtype=torch.int64, device="cuda")
    io = (plan._plan, vp(rig.xg.data_ptr() + 8 * n1), n - n1, rig.stride, vp(out.data_ptr()), 8 * n)
    refused = {
        "sxfir_interpolate": lambda: lib.sxfir_interpolate(*io, C.byref(got), None),
        "sxfir_interpolate_keyed": lambda: lib.sxfir_interpolate_keyed(*io, C.byref(got), 0, 8, vp(counter.data_ptr()), None),
        "sxfir_time_interpolate": lambda: lib.sxfir_time_interpolate(*io, 1, None, C.byref(ms)),
        "sxfir_channelize": lambda: lib.sxfir_channelize(*io, 2 * n, C.byref(got), None),
        "sxfir_synthesize": lambda: lib.sxfir_synthesize(*io[:4], 2 * n, *io[4:], C.byref(got), None),
        "sxfir_resample": lambda: lib.sxfir_resample(*io, C.byref(got), None),
        "sxfir_time_resample": lambda: lib.sxfir_time_resample(*io, 1, None, C.byref(ms)),
    }
    for name, fn in refused.items():
        got.value = 77
        assert fn() == EINVAL, name
        assert plan.position == pos, name
        assert got.value in (0, 77), name
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and float(out.abs().max().item()) == 0.0
    # sxfir_time_decimate leaves the position, the history and the phase as they were
    assert plan.time_decimate_ptr(io[1].value, n - n1, rig.stride, out.data_ptr(), 8 * n, 2) > 0.0
    torch.cuda.synchronize()
    assert plan.position == pos
    timed = out.cpu().numpy()[:, :(n - n1) // 4]
    same(np.ascontiguousarray(timed).view(np.uint32), ref[:, k1:], "what the timed passes wrote")
    same(rig.call(plan, n1, n - n1, TILED), ref[:, k1:], "the call after the refused and the timed ones")
    # sxfir_plan_translation tells the kinds apart
    h4 = sxxcvr_amd.design_lowpass(128, 4)
    others = {"real": Resampler(DECIMATE, h4, 4), "complex": Resampler(DECIMATE, design_bandpass(128, 4, 1, 4), 4),
              "complex interpolator": sxxcvr_amd.ComplexInterpolator(design_bandpass(128, 4, 1, 4), 4),
              "channelizer": sxxcvr_amd.Channelizer(h4), "rational": sxxcvr_amd.RationalResampler(sxxcvr_amd.design_rational(4, 5), 4, 5)}
    a, b = C.c_int(-1), C.c_int(-1)
    for name, p in others.items():
        assert lib.sxfir_plan_translation(p._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0), name
    assert lib.sxfir_plan_translation(plan._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (num, den)
    assert lib.sxfir_plan_translation(plan._plan, None, C.byref(b)) == EINVAL
    q = C.c_int(-1)
    for query in ("sxfir_plan_bands", "sxfir_plan_oversampling", "sxfir_plan_synthesis_bands", "sxfir_plan_synthesis_oversampling"):
        assert getattr(lib, query)(plan._plan, C.byref(q)) == 0 and q.value == 0, query
    assert lib.sxfir_plan_rational(plan._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert lib.sxfir_taps_are_complex(plan._plan, C.byref(q)) == 0 and q.value == 1
    # den = 1: a table of one entry, every output times (1, +0)
    one = TranslatingDecimator(H4, 4, 5, 1)
    assert (one.num, one.den) == (0, 1)
    same(rig.call(one, 0, n, TILED)[:1], rig.ref(H4, 4, one.contract, 0, 1)[:1], "den 1")


# ---- anchors -------------------------------------------------------------------------------------------------------------------
ANCHORS = [(128, 4, KERNEL_TILED, TILED), (128, 4, KERNEL_GENERIC, GENERIC), (35, 5, KERNEL_GENERIC, GENERIC)]


def anchor_taps(ntaps, D, num, den, designed):
    return design_bandpass(ntaps, D, num, den) if designed and ntaps == 128 else random_taps_cx(ntaps, 9)


@pytest.mark.parametrize("ntaps,D,kernel,name", ANCHORS)
def test_anchor_fp64(oracle, ntaps, D, kernel, name):
    num, den = 123, 1000
    h = anchor_taps(ntaps, D, num, den, True)
    n = 2 * TILE + 140
    x = streams(1, n, 13)
    rig = Rig(oracle, x)
    plan = TranslatingDecimator(h, D, num, den)
    plan.set_kernel(kernel)
    y = rig.stream(plan, [n], [name]).view(np.complex64)[0].astype(np.complex128)
    want = mix_f64(h, D, num, den, x[0])
    b = bound(h, x[0], want)
    err = np.maximum(np.abs(y.real - want.real), np.abs(y.imag - want.imag))
    print("/%d x %d %s: worst error %.3g, bound there %.3g" % (D, ntaps, name, err.max(), b[err.argmax()]))
    assert np.all(err <= b)


@pytest.mark.parametrize("ntaps,D,kernel,name", ANCHORS)
def test_anchor_non_finite(oracle, ntaps, D, kernel, name):
    """One +Inf and one NaN sample: non-finite outputs exactly where the reference has them (NaNs compared as NaNs, not by
    payload), the same bits everywhere else."""
    num, den = 3, 7
    h = anchor_taps(ntaps, D, num, den, False)
    n = 2 * TILE + 140
    x = streams(1, n, 14)
    x[0, 700] = np.complex64(complex(np.inf, 0.25))
    x[0, 2900] = np.complex64(complex(-0.5, np.nan))
    rig = Rig(oracle, x)
    plan = TranslatingDecimator(h, D, num, den)
    plan.set_kernel(kernel)
    got = rig.stream(plan, [n], [name]).view(np.float32)[0]
    want = rig.ref(h, D, plan.contract, num, den).view(np.float32)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    assert np.array_equal(np.isinf(got), np.isinf(want))
    ok = ~np.isnan(want)
    same(got.view(np.uint32)[ok], want.view(np.uint32)[ok], "around the non-finite samples")


@pytest.mark.parametrize("ntaps,D,kernel,name", ANCHORS)
def test_anchor_subnormals(oracle, ntaps, D, kernel, name):
    """A stream scaled into the subnormals: bit-exact, nothing is flushed."""
    num, den = 123, 1000
    h = anchor_taps(ntaps, D, num, den, False)
    n = 2 * TILE + 140
    x = (streams(1, n, 15) * np.float32(2.0 ** -130)).astype(np.complex64)
    assert 0 < np.abs(x.view(np.float32)).max() < np.finfo(np.float32).tiny
    rig = Rig(oracle, x)
    plan = TranslatingDecimator(h, D, num, den)
    plan.set_kernel(kernel)
    want = rig.ref(h, D, plan.contract, num, den)
    assert np.count_nonzero(want.view(np.float32)) > want.size // 2
    same(rig.stream(plan, [n], [name]), want, "subnormal stream")
