"""Frequency-translating interpolators on the GPU (include/sxfir_translate_tx.h), bit for bit against tests/mix_tx_cases.py: the
input rotated in float32 on the table of sxfir_design_rotator, then the complex-tap interpolator's oracle reference.

Every call goes through `Rig.call`: the output lands between two guards of fill words that must come back untouched, and the
plan's position, outputs_for and geometry(...)["kernel"] are checked around it."""
import ctypes as C

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import ComplexInterpolator, Resampler, TranslatingDecimator, TranslatingInterpolator, design_bandpass
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED
from gpu_util import random_taps_cx
import rate_cases as rc
from mix_tx_cases import back_step, bound, mix_tx_f64, mix_tx_ref, rotate_in_f32, step
from rational_cases import gaussian_stream

pytestmark = pytest.mark.gpu

FILL = 0x7FC07FC0               # a NaN as one fp32 word and as two halves: no output of these streams is this word
GUARD = 8                       # samples of fill words on either side of a row's outputs (whole 16-byte units in both formats)
TILE_IN = {4: 256, 8: 128}      # inputs per tile of interp_mix_pass_kernel
TILED, GENERIC = "interp_mix_pass_kernel", "interp_mix_generic_kernel"
EINVAL, EUNSUPPORTED = -1, -4
PAIRS = [(123, 1000), (3, 7), (65535, 65536), (1, 4), (0, 1)]


def _i32(word):
    return word - (1 << 32) if word >= 1 << 31 else word


def totals(L):
    T = TILE_IN[L]
    return [1, T - 1, T, T + 1, 3 * T + 5]


class Rig:
    """One stream [nchan, n] on the GPU (rows `pad` samples longer than the stream: strides larger than the block) and its CPU twin
    as the plan sees it (CF16: quantised to half; S32: CF32 in, wire words out)."""

    def __init__(self, oracle, x, fmt="CF32", pad=41, thr2=None):
        import torch
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex64)
        self.oracle, self.fmt, self.nchan, self.n, self.thr2 = oracle, fmt, x.shape[0], x.shape[1], thr2
        self.sb_in, self.wps_in = (4, 1) if fmt == "CF16" else (8, 2)          # input: bytes, 32-bit words per sample
        self.sb, self.wps = self.sb_in, self.wps_in                           # output (S32: wire words, 8 bytes too)
        self.stride = self.n + pad
        if fmt == "CF16":
            h16 = oracle.f32_to_f16(x.view(np.float32))
            self.x = oracle.f16_to_f32(h16).view(np.complex64)
            words = np.ascontiguousarray(h16).view(np.int32)
        else:
            self.x = x
            words = x.view(np.int32)
        buf = np.zeros((self.nchan, self.stride * self.wps_in), dtype=np.int32)
        buf[:, :words.shape[1]] = words
        self.xg = torch.from_numpy(buf).cuda()

    def words(self, y):
        """complex64 [n] reference -> the 32-bit words the plan stores"""
        y = np.ascontiguousarray(y, dtype=np.complex64)
        if self.fmt == "CF16":
            return np.ascontiguousarray(self.oracle.f32_to_f16(y.view(np.float32))).view(np.uint32)
        if self.fmt == "S32":
            return self.oracle.convert_tx(y, np.float32(self.thr2)).view(np.uint32)
        return y.view(np.uint32)

    def ref(self, h, L, jsplit, num, den, first=0, count=None, m_first=None, threads=None):
        """[nchan, words] of one pass over inputs [0, first + count) from zero history, the outputs of inputs [first, ..) alone;
        input `first` has the absolute index m_first (default: its index in this stream)."""
        count = self.n - first if count is None else count
        m0 = 0 if m_first is None else m_first - first
        return np.stack([self.words(mix_tx_ref(self.oracle, h, L, self.x[c, :first + count], jsplit, num, den, m0, threads=threads)[L * first:])
                         for c in range(self.nchan)])

    def call(self, plan, pos, n, kernel=None, offset=0, expect=None, odd_stride=False):
        """sxfir_interpolate over inputs [pos, pos + n) of every row.  Returns [nchan, words]; with `expect` (an error code) the call
        must fail with it and leave the plan and the output buffer alone."""
        import torch
        L = plan.ratio
        c0, p0 = plan.position
        assert p0 == L * c0
        n_out = L * n
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


H = {4: random_taps_cx(128, 31), 8: random_taps_cx(256, 33)}


def plan_of(L, num, den, kernel=KERNEL_AUTO, nchan=1):
    plan = TranslatingInterpolator(H[L], L, num, den, nchan=nchan)
    assert plan.complex_taps and plan.mode == INTERPOLATE and tuple(plan.contract) == (2, 1) and plan.contract.rot == 0
    assert (plan.num, plan.den) == (num % den, den)
    plan.set_kernel(kernel)
    return plan


# ---- the tiled kernel, x4 x 128 and x8 x 256 on CF32 ----------------------------------------------------------------------------
@pytest.mark.parametrize("num,den", PAIRS)
@pytest.mark.parametrize("L", [4, 8])
def test_tiled_auto_generic(oracle, L, num, den):
    """1, tile - 1, tile, tile + 1 and 3 tiles + 5 inputs through the tiled kernel (forced and under AUTO) and the generic one."""
    T = TILE_IN[L]
    for n in totals(L):
        rig = Rig(oracle, streams(1, n, 5))
        g = plan_of(L, num, den).geometry(n)
        assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == -(-n // T) and g["tile_samples"] == L * T, g
        ref = rig.ref(H[L], L, 2, num, den)
        assert ref.shape[1] == 2 * L * n
        same(rig.stream(plan_of(L, num, den), [n], [TILED]), ref, "auto, %d inputs" % n)
        same(rig.stream(plan_of(L, num, den, KERNEL_TILED), [n], [TILED]), ref, "tiled, %d inputs" % n)
        same(rig.stream(plan_of(L, num, den, KERNEL_GENERIC), [n], [GENERIC]), ref, "generic, %d inputs" % n)


@pytest.mark.parametrize("L", [4, 8])
def test_negative_num_is_reduced(oracle, L):
    n = TILE_IN[L] + 40
    rig = Rig(oracle, streams(1, n, 4))
    plan = TranslatingInterpolator(H[L], L, -4 - 7 * 1000, 7)
    assert (plan.num, plan.den) == (3, 7)
    same(rig.stream(plan, [n], [TILED]), rig.ref(H[L], L, 2, 3, 7), "num = -7004 is 3 mod 7")


@pytest.mark.parametrize("num,den", [(123, 1000), (3, 7)])
@pytest.mark.parametrize("L", [4, 8])
def test_splits(oracle, L, num, den):
    """One stream cut into calls of odd sizes, a 1-sample call and one shorter than the 32-sample history among them, through
    either kernel and through both in turn: the bits of one call -- the phase is continuous."""
    T = TILE_IN[L]
    n = 3 * T + 5
    rig = Rig(oracle, streams(1, n, 6))
    ref = rig.ref(H[L], L, 2, num, den)
    same(rig.stream(plan_of(L, num, den), [n], [TILED]), ref, "one call")
    blocks = [T + 3, 1, 31, T - 1, n - 2 * T - 34]
    assert sum(blocks) == n
    same(rig.stream(plan_of(L, num, den), blocks, [TILED] * 5), ref, "five calls, tiled")
    same(rig.stream(plan_of(L, num, den, KERNEL_GENERIC), blocks, [GENERIC] * 5), ref, "five calls, generic")
    plan = plan_of(L, num, den)
    outs, pos = [], 0
    for i, b in enumerate(blocks):
        plan.set_kernel(KERNEL_GENERIC if i % 2 else KERNEL_TILED)
        outs.append(rig.call(plan, pos, b, GENERIC if i % 2 else TILED))
        pos += b
    same(np.concatenate(outs, axis=1), ref, "five calls, the kernels in turn")


@pytest.mark.parametrize("num,den", [(12345, 65536), (3, 7)])
@pytest.mark.parametrize("L", [4, 8])
def test_far_positions(oracle, L, num, den):
    """A plan placed at input 2^40 + 21 with the history of the samples in front: one tiled and one generic call carry the phase of
    that input -- the 64-bit phase, without a long stream.  sxfir_reset returns the phase to 0."""
    import torch
    T = TILE_IN[L]
    lead, n1 = 64, T + 6
    n = lead + n1 + T + 30
    where = (1 << 40) + 21                      # (where - lead is no multiple of 7: the far phase differs from the near one)
    rig = Rig(oracle, streams(1, n, 7))
    plan = plan_of(L, num, den)
    plan.set_history_ptr(rig.xg.data_ptr(), lead, rig.stride, torch.cuda.current_stream().cuda_stream)
    plan.set_position(where)
    assert plan.position == (where, L * where)
    ref = rig.ref(H[L], L, 2, num, den, first=lead, m_first=where)
    plan.set_kernel(KERNEL_TILED)
    a = rig.call(plan, lead, n1, TILED)
    plan.set_kernel(KERNEL_GENERIC)
    b = rig.call(plan, lead + n1, n - lead - n1, GENERIC)
    same(np.concatenate([a, b], axis=1), ref, "from input 2^40 + 21")
    near = rig.ref(H[L], L, 2, num, den, first=lead)
    assert np.count_nonzero(near != ref) > ref.size // 2, "the far phase is not the near one"
    plan.set_kernel(KERNEL_AUTO)
    plan.reset()
    assert plan.position == (0, 0)
    same(rig.call(plan, 0, T + 8, TILED), rig.ref(H[L], L, 2, num, den, count=T + 8), "after reset")


@pytest.mark.parametrize("kernel,name", [(KERNEL_TILED, TILED), (KERNEL_GENERIC, GENERIC)])
@pytest.mark.parametrize("L", [4, 8])
def test_history_at_position_0(oracle, L, kernel, name):
    """sxfir_set_history with non-zero, RAW history at position 0: the history samples have the negative indices -lead .. -1 and get
    the table entries of those indices reduced into [0, den)."""
    import torch
    lead, n = 40, TILE_IN[L] + 9
    num, den = 123, 1000
    rig = Rig(oracle, streams(1, lead + n, 17))
    plan = plan_of(L, num, den, kernel)
    plan.set_history_ptr(rig.xg.data_ptr(), lead, rig.stride, torch.cuda.current_stream().cuda_stream)
    assert plan.position == (0, 0)
    ref = rig.ref(H[L], L, 2, num, den, first=lead, m_first=0)
    same(rig.call(plan, lead, n, name), ref, "history at negative indices")
    assert np.count_nonzero(ref != rig.ref(H[L], L, 2, num, den, first=lead)) > ref.size // 2


# ---- more tiles than resident workgroups: the tile loop's second iteration ------------------------------------------------------
@pytest.mark.parametrize("num,den,s4", [(3, 7, 5), (65535, 65536, 65532), (65534, 65535, 65531), (1, 3, 1)])
@pytest.mark.parametrize("L", [4, 8])
def test_more_tiles_than_resident_workgroups(oracle, L, num, den, s4):
    """resident + 3 tiles: a call this small is dealt as ONE generation of waves, so the grid is the chip's resident waves and three
    waves walk on to a second tile -- `tile_ph += stride_step` and its wrap, the table reads in front of the next tile's DMAs, the
    counted wait behind a tile's own stores.  The (num, den) rows of tests/test_gpu_mix.py (s4: their step at ratio 4)."""
    assert step(num, den, 4) == s4
    plan = plan_of(L, num, den, KERNEL_TILED)
    resident = plan.geometry(TILE_IN[L])["resident"]
    n = (resident + 3) * TILE_IN[L]
    g = plan.geometry(n)
    assert g["kernel"] == TILED and g["n_tiles"] == resident + 3 and g["workgroups"] == resident, g
    rig = Rig(oracle, streams(1, n, 19), pad=0)
    same(rig.call(plan, 0, n, TILED), rig.ref(H[L], L, 2, num, den, threads=oracle.max_threads()), "resident + 3 tiles")


def _walk_size(n_tiles, L):
    """Inputs of a call of n_tiles tiles whose last tile is ragged (half a tile and five samples)."""
    return (n_tiles - 1) * TILE_IN[L] + TILE_IN[L] // 2 + 5


@pytest.mark.parametrize("num,den", [(3, 7), (1, 3), (65535, 65536), (65534, 65535)])
@pytest.mark.parametrize("L", [4, 8])
def test_a_waves_third_tile(oracle, L, num, den):
    """2 resident + 3 tiles under a forced TILED: still one generation of waves, so every wave walks to a second tile and three to a
    THIRD -- `stride_step` applied twice and wrapped twice, a second interior-to-interior hand-over under the counted wait with the
    table registers in flight, the history carried over by a wave on its third tile.  (3, 7) and (1, 3): more tiles than table
    entries; (65535, 65536) and (65534, 65535): the smallest steps t above 0 on the largest tables (t = L and t = L)."""
    plan = plan_of(L, num, den, KERNEL_TILED)
    resident = plan.geometry(TILE_IN[L])["resident"]
    n = _walk_size(2 * resident + 3, L)
    g = plan.geometry(n)
    print("x%d %d/%d: resident %d, workgroups %d, %d tiles, %d inputs, %d outputs" % (L, num, den, resident, g["workgroups"], g["n_tiles"], n, L * n))
    assert g["kernel"] == TILED and g["workgroups"] == resident and g["n_tiles"] == 2 * resident + 3, g
    assert (g["n_tiles"] - 1) % resident == 2                   # (the last tile is the third of the wave that carries the history over)
    rig = Rig(oracle, streams(1, n + TILE_IN[L] + 8, 19), pad=0)
    ref = rig.ref(H[L], L, 2, num, den, threads=oracle.max_threads())
    same(rig.call(plan, 0, n, TILED), ref[:, :2 * L * n], "2 resident + 3 tiles")
    same(rig.call(plan, n, TILE_IN[L] + 8, TILED), ref[:, 2 * L * n:], "the call after it: the history a third tile's wave left")


@pytest.mark.parametrize("L,skew", [(4, 1), (8, 3)])
def test_more_tiles_than_workgroups_three_channels(oracle, L, skew):
    """Three channels: the grid per channel is a third of the resident waves -- at x4 no multiple of 8, so the tiles are dealt plainly
    strided (682 of 2048 on the MI355X; x8: 1024 of 3072, XCD-blocked) -- and a call of that many tiles + 4 per channel has more
    tiles than waves at a figure the one-channel tests never reach.  The input is a view `skew` samples into rows of an odd, padded stride (the DMA source of every other row is 8-byte
    aligned only), the output rows lie an even, padded stride apart."""
    num, den = 123, 1000
    plan = plan_of(L, num, den, KERNEL_TILED, nchan=3)
    per = plan.geometry(TILE_IN[L])["resident"] // 3
    n = _walk_size(per + 4, L)
    g = plan.geometry(n)
    G = g["workgroups"] // 3
    print("x%d, 3 channels: resident %d, %d workgroups per channel, %d tiles per channel, %d inputs per channel" % (L, g["resident"], G, g["n_tiles"], n))
    assert g["kernel"] == TILED and g["workgroups"] == 3 * G and G == per and g["n_tiles"] == G + 4 and G < g["n_tiles"], g
    rig = Rig(oracle, streams(3, skew + n, 29), pad=41 - (skew + n) % 2)
    assert rig.stride % 2 == 1 and rig.stride > skew + n
    ref = np.stack([rig.words(mix_tx_ref(oracle, H[L], L, rig.x[c, skew:], 2, num, den, threads=oracle.max_threads())) for c in range(3)])
    same(rig.call(plan, skew, n, TILED), ref, "three channels, groups + 4 tiles each")


PLACED = [((1 << 40) + 21, 64, "max", 65535), ((1 << 40) + 21, 64, "one", 7), (5, 40, "one", 65535)]       # (rate_cases.MIXERS' classes)


@pytest.mark.parametrize("where,lead,cls,den", PLACED)
@pytest.mark.parametrize("L", [4, 8])
def test_more_tiles_than_resident_workgroups_placed(oracle, L, where, lead, cls, den):
    """resident + 3 tiles from a PLACED, odd position, the samples in front handed to sxfir_set_history raw: the 64-bit reduction of
    `mix.phase`, the image's halo 32 samples in front of the call and `stride_step` in one call.  From 2^40 + 21 on den 65535 (t = 1,
    the smallest step) and den 7 (t = 6, more tiles than entries); from position 5 with 40 history samples on den 65535 with s = 1 (the
    largest t, 65534): the halo's indices -27 .. 4 are reduced from below 0 while the walk wraps at nearly every step."""
    import torch
    num = rc.mixer_num(cls, den, None, L)
    t = back_step(num, den, L)
    assert t == {"max": 1, "one": den - 1}[cls] and (where - lead) * t % den != 0       # (the far phase is not the near one)
    plan = plan_of(L, num, den, KERNEL_TILED)
    resident = plan.geometry(TILE_IN[L])["resident"]
    n = _walk_size(resident + 3, L)
    rig = Rig(oracle, streams(1, lead + n, 23), pad=0)
    plan.set_history_ptr(rig.xg.data_ptr(), lead, rig.stride, torch.cuda.current_stream().cuda_stream)
    plan.set_position(where)
    assert plan.position == (where, L * where)
    g = plan.geometry(n)
    print("x%d %d/%d from %d: resident %d, workgroups %d, %d tiles, %d inputs" % (L, num, den, where, resident, g["workgroups"], g["n_tiles"], n))
    assert g["kernel"] == TILED and g["workgroups"] == resident and g["n_tiles"] == resident + 3, g
    ref = rig.ref(H[L], L, 2, num, den, first=lead, m_first=where, threads=oracle.max_threads())
    same(rig.call(plan, lead, n, TILED), ref, "resident + 3 tiles from input %d" % where)


@pytest.mark.parametrize("ntaps,L,fmt,kernel", [(128, 4, "CF32", KERNEL_GENERIC), (35, 5, "CF32", KERNEL_AUTO), (96, 3, "CF16", KERNEL_AUTO)])
def test_generic_call_longer_than_the_table(oracle, ntaps, L, fmt, kernel):
    """ONE generic call of den + 300 inputs on den = 65535 with the largest step the ratio allows (s = gcd(L, den): t = 65534 at x4,
    65530 at x5, 65532 at x3).  `mix.phase` carries the absolute part of the index, so interp_mix_generic_kernel sees the call-local
    q alone, and only a call of more than den inputs makes `q % den` wrap; only a large t brings `(q % den) * t` near its stated
    limit of 65535^2.  Without the reduction q * t passes 2^32 from q = 65539 on, and 2^32 = 1 modulo 65535: every later sample would
    take the neighbouring table entry.  den = 65536 would prove nothing: 2^32 = 0 modulo a power of two, the wrapped product has the
    right remainder."""
    den = 65535
    num = rc.mixer_num("one", den, None, L)
    t = back_step(num, den, L)
    n = den + 300
    assert t == den - np.gcd(L, den) and (den - 1) * t < 2 ** 32 <= (n - 1) * t and 2 ** 32 % den == 1 and 2 ** 32 % 65536 == 0
    h = H[4] if (ntaps, L) == (128, 4) else random_taps_cx(ntaps, 9)
    rig = Rig(oracle, streams(1, n, 31), fmt)
    plan = TranslatingInterpolator(h, L, num, den, fmt=fmt)
    plan.set_kernel(kernel)
    jsplit = plan.contract[0]
    assert jsplit == (2 if (ntaps // L) % 2 == 0 else 1)
    same(rig.stream(plan, [n], [GENERIC]), rig.ref(h, L, jsplit, num, den, threads=oracle.max_threads()), "one generic call of den + 300 inputs")


# ---- channels and alignment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 8])
def test_three_channels(oracle, L):
    num, den = 123, 1000
    n = 2 * TILE_IN[L] + 11
    rig = Rig(oracle, streams(3, n, 8))
    ref = rig.ref(H[L], L, 2, num, den)
    same(rig.call(plan_of(L, num, den, KERNEL_TILED, nchan=3), 0, n, TILED, offset=2), ref, "tiled, strides and an offset of one 16-byte unit")
    same(rig.stream(plan_of(L, num, den, KERNEL_GENERIC, nchan=3), [33, n - 33], [GENERIC] * 2), ref, "generic")


@pytest.mark.parametrize("L", [4, 8])
def test_misaligned_output(oracle, L):
    """Output rows an odd number of samples apart, or an output offset by one sample, break the 16-byte stores: the generic kernel
    under AUTO, the same bits; SXFIR_EUNSUPPORTED, plan and output untouched, under a forced TILED."""
    num, den = 3, 7
    n = TILE_IN[L] + 40
    rig = Rig(oracle, streams(3, n, 16))
    ref = rig.ref(H[L], L, 2, num, den)
    same(rig.call(plan_of(L, num, den, nchan=3), 0, n, odd_stride=True), ref, "odd stride under AUTO")
    same(rig.call(plan_of(L, num, den, nchan=3), 0, n, offset=1), ref, "offset output under AUTO")
    plan = plan_of(L, num, den, KERNEL_TILED, nchan=3)
    n1 = 50
    same(rig.call(plan, 0, n1, TILED), ref[:, :2 * L * n1], "first block")
    rig.call(plan, n1, n - n1, TILED, odd_stride=True, expect=EUNSUPPORTED)
    rig.call(plan, n1, n - n1, TILED, offset=1, expect=EUNSUPPORTED)
    # the failed calls left the phase, the history and the position where they were
    same(rig.call(plan, n1, n - n1, TILED), ref[:, 2 * L * n1:], "the call after the refused ones")


# ---- the generic kernel at the shapes and formats without a tiled one -----------------------------------------------------------
@pytest.mark.parametrize("ntaps,L,fmt,jsplit", [(35, 5, "CF32", 1), (96, 3, "CF16", 2), (1536, 48, "CF32", 2), (256, 8, "S32", 2)])
@pytest.mark.parametrize("num,den", [(123, 1000), (3, 7)])
def test_generic_shapes(oracle, ntaps, L, fmt, jsplit, num, den):
    h = random_taps_cx(ntaps, 9) if fmt != "S32" else design_bandpass(ntaps, L, num, den, gain=L)
    n = 300 + 3
    x = streams(2, n, 9)
    if fmt == "S32":
        x = x * np.float32(0.0625)          # (exact; the outputs stay inside the wire words' range)
    rig = Rig(oracle, x, fmt)
    plan = TranslatingInterpolator(h, L, num, den, nchan=2, fmt=fmt)
    assert tuple(plan.contract) == (jsplit, 1) and plan.contract.rot == 0 and plan.complex_taps
    g = plan.geometry(n)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == EUNSUPPORTED
    if fmt == "S32":
        # a threshold that leaves outputs on both sides of the keying rule
        y = mix_tx_ref(oracle, h, L, rig.x[0], jsplit, num, den)
        assert max(np.abs(y.real).max(), np.abs(y.imag).max()) < 1.0
        rig.thr2 = float(np.float32(np.median(y.real.astype(np.float32) ** 2 + y.imag.astype(np.float32) ** 2)))
        plan.set_tx_threshold(rig.thr2)
    ref = rig.ref(h, L, jsplit, num, den)
    if fmt == "S32":
        keyed = (ref[0].view(np.int32).reshape(-1, 2)[:, 0] & 3) == 3
        assert 0 < keyed.sum() < keyed.size
    same(rig.stream(plan, [n], [GENERIC]), ref, "one call")
    again = TranslatingInterpolator(h, L, num, den, nchan=2, fmt=fmt)
    if fmt == "S32":
        again.set_tx_threshold(rig.thr2)
    same(rig.stream(again, [37, 1, n - 38], [GENERIC] * 3), ref, "three calls")


# ---- without the oracle: the complex-tap interpolator plan on the GPU over the host-rotated input ------------------------------
@pytest.mark.parametrize("ntaps,L,kernel,name", [(128, 4, KERNEL_TILED, TILED), (256, 8, KERNEL_TILED, TILED), (128, 4, KERNEL_GENERIC, GENERIC),
                                                 (35, 5, KERNEL_AUTO, GENERIC)])
@pytest.mark.parametrize("num,den", [(12345, 65536), (1, 4)])
def test_equals_the_complex_interpolator_on_rotated_input(oracle, ntaps, L, kernel, name, num, den):
    import torch
    h = random_taps_cx(ntaps, 12)
    n = 2 * 256 + 140
    rig = Rig(oracle, streams(1, n, 10))
    xr = rotate_in_f32(rig.x[0], num, den, L)
    cx = ComplexInterpolator(h, L)
    want = cx.process(torch.from_numpy(xr).cuda())
    torch.cuda.synchronize()
    plan = TranslatingInterpolator(h, L, num, den)
    plan.set_kernel(kernel)
    same(rig.stream(plan, [n], [name]), want.cpu().numpy().view(np.uint32).reshape(1, -1), "x%d x %d against the complex plan" % (L, ntaps))


# ---- keyed ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaps,L,name", [(128, 4, TILED), (256, 8, TILED), (35, 5, GENERIC)])
def test_keyed(oracle, ntaps, L, name):
    """sxfir_interpolate_keyed: the count is taken on the RAW input (sxfir_count_keyed's rule: convert_tx_buffer's keying bit of the
    input samples), whatever the rotation; the outputs are the unkeyed call's."""
    import torch
    num, den = 123, 1000
    n = 3 * 256 + 37
    first, count = 101, n - 101 - 59
    thr2 = 0.49
    h = random_taps_cx(ntaps, 14)
    rig = Rig(oracle, streams(1, n, 11))
    st = torch.cuda.current_stream().cuda_stream
    plan = TranslatingInterpolator(h, L, num, den)
    plan.set_tx_threshold(thr2)
    assert plan.geometry(n)["kernel"] == name
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.empty(n * L, dtype=torch.complex64, device="cuda")
    assert plan.interpolate_keyed_ptr(rig.xg.data_ptr(), n, rig.stride, out.data_ptr(), n * L, first, count, counter.data_ptr(), st) == n * L
    torch.cuda.synchronize()
    want = int(((oracle.convert_tx(rig.x[0, first:first + count], np.float32(thr2)).reshape(-1, 2)[:, 0] & 3) == 3).sum())
    assert 0 < want < count
    assert int(counter.item()) == want
    assert plan.position == (n, n * L)
    same(out.cpu().numpy().view(np.uint32).reshape(1, -1), rig.ref(h, L, plan.contract[0], num, den), "keyed against the reference")


# ---- the frame ------------------------------------------------------------------------------------------------------------------
def test_frame(oracle):
    import torch
    lib = sxxcvr_amd.load_sxfir()
    vp = C.c_void_p
    num, den = 123, 1000
    L, n = 4, TILE_IN[4] + 40
    rig = Rig(oracle, streams(1, n, 12))
    plan = plan_of(L, num, den)
    q, a, b = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.sxfir_taps_are_complex(plan._plan, C.byref(q)) == 0 and q.value == 1
    assert lib.sxfir_plan_translation(plan._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert lib.sxfir_plan_translation_tx(plan._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (num, den)
    assert lib.sxfir_plan_translation_tx(plan._plan, None, C.byref(b)) == EINVAL
    big = TranslatingInterpolator(H[4], 4, 1000 * 7 + 5, 7)
    assert lib.sxfir_plan_translation_tx(big._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (5, 7)
    h4 = sxxcvr_amd.design_lowpass(128, 4)
    cxi = ComplexInterpolator(design_bandpass(128, 4, 1, 4, gain=4), 4)
    rxt = TranslatingDecimator(design_bandpass(128, 4, num, den), 4, num, den)
    others = {"real": Resampler(INTERPOLATE, h4, 4), "complex interpolator": cxi, "translating decimator": rxt,
              "complex decimator": Resampler(DECIMATE, design_bandpass(128, 4, 1, 4), 4)}
    for name, p in others.items():
        assert lib.sxfir_plan_translation_tx(p._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0), name
    assert lib.sxfir_plan_translation(rxt._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (num, den)
    for query in ("sxfir_plan_bands", "sxfir_plan_oversampling", "sxfir_plan_synthesis_bands", "sxfir_plan_synthesis_oversampling"):
        assert getattr(lib, query)(plan._plan, C.byref(q)) == 0 and q.value == 0, query
    assert lib.sxfir_plan_rational(plan._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    # the launch geometry is the complex-tap interpolator's for the same call, but for the kernel's name
    for p, other, names in ((plan, cxi, (TILED, "interp_cx_pass_kernel")),):
        for count in (1, TILE_IN[4], 5 * TILE_IN[4] + 3, 1 << 20):
            g, go = p.geometry(count), other.geometry(count)
            assert (g.pop("kernel"), go.pop("kernel")) == names and g == go, (count, g, go)
    g8, go8 = plan_of(8, num, den).geometry(1 << 20), ComplexInterpolator(H[8], 8).geometry(1 << 20)
    assert g8.pop("kernel") == TILED and go8.pop("kernel") == "interp_cx_pass_kernel" and g8 == go8
    # sxfir_decimate and the band and rational entry points refuse the plan
    pos = plan.position
    out = torch.full((8 * n,), 0.0, dtype=torch.complex64, device="cuda")
    got, ms = C.c_size_t(77), C.c_float()
    io = (plan._plan, vp(rig.xg.data_ptr()), n, rig.stride, vp(out.data_ptr()), 8 * n)
    refused = {
        "sxfir_decimate": lambda: lib.sxfir_decimate(*io, C.byref(got), None),
        "sxfir_time_decimate": lambda: lib.sxfir_time_decimate(*io, 1, None, C.byref(ms)),
        "sxfir_channelize": lambda: lib.sxfir_channelize(*io, 2 * n, C.byref(got), None),
        "sxfir_synthesize": lambda: lib.sxfir_synthesize(*io[:4], 2 * n, *io[4:], C.byref(got), None),
        "sxfir_resample": lambda: lib.sxfir_resample(*io, C.byref(got), None),
    }
    for name, fn in refused.items():
        got.value = 77
        assert fn() == EINVAL, name
        assert plan.position == pos and got.value in (0, 77), name
    torch.cuda.synchronize()
    assert float(out.abs().max().item()) == 0.0
    # sxfir_time_interpolate leaves the position, the history and the phase as they were
    ref = rig.ref(H[4], 4, 2, num, den)
    n1 = 61
    same(rig.call(plan, 0, n1, TILED), ref[:, :2 * 4 * n1], "first block")
    assert plan.time_passes_ptr(rig.xg.data_ptr() + 8 * n1, n - n1, rig.stride, out.data_ptr(), 8 * n, 2) > 0.0
    torch.cuda.synchronize()
    assert plan.position == (n1, 4 * n1)
    same(np.ascontiguousarray(out.cpu().numpy()[:4 * (n - n1)]).view(np.uint32).reshape(1, -1), ref[:, 2 * 4 * n1:], "what the timed passes wrote")
    same(rig.call(plan, n1, n - n1, TILED), ref[:, 2 * 4 * n1:], "the call after the refused and the timed ones")


# ---- anchors --------------------------------------------------------------------------------------------------------------------
ANCHORS = [(128, 4, KERNEL_TILED, TILED), (256, 8, KERNEL_TILED, TILED), (128, 4, KERNEL_GENERIC, GENERIC), (35, 5, KERNEL_GENERIC, GENERIC)]
N_ANCHOR = 2 * 256 + 140


def anchor_taps(ntaps, L, num, den, designed):
    return design_bandpass(ntaps, L, num, den, gain=L) if designed and ntaps == 32 * L else random_taps_cx(ntaps, 9)


@pytest.mark.parametrize("ntaps,L,kernel,name", ANCHORS)
def test_anchor_fp64(oracle, ntaps, L, kernel, name):
    num, den = 123, 1000
    h = anchor_taps(ntaps, L, num, den, True)
    x = streams(1, N_ANCHOR, 13)
    rig = Rig(oracle, x)
    plan = TranslatingInterpolator(h, L, num, den)
    plan.set_kernel(kernel)
    y = rig.stream(plan, [N_ANCHOR], [name]).view(np.complex64)[0].astype(np.complex128)
    want = mix_tx_f64(h, L, num, den, x[0])
    b = bound(h, x[0])
    err = max(np.abs(y.real - want.real).max(), np.abs(y.imag - want.imag).max())
    print("x%d x %d %s: worst error %.3g, bound %.3g" % (L, ntaps, name, err, b))
    assert err <= b


@pytest.mark.parametrize("ntaps,L,kernel,name", ANCHORS)
def test_anchor_non_finite(oracle, ntaps, L, kernel, name):
    """One +Inf and one NaN sample: non-finite outputs exactly where the reference has them (NaNs compared as NaNs, not by
    payload), the same bits everywhere else."""
    num, den = 3, 7
    h = anchor_taps(ntaps, L, num, den, False)
    x = streams(1, N_ANCHOR, 14)
    x[0, 200] = np.complex64(complex(np.inf, 0.25))
    x[0, 500] = np.complex64(complex(-0.5, np.nan))
    rig = Rig(oracle, x)
    plan = TranslatingInterpolator(h, L, num, den)
    plan.set_kernel(kernel)
    got = rig.stream(plan, [N_ANCHOR], [name]).view(np.float32)[0]
    want = rig.ref(h, L, plan.contract[0], num, den).view(np.float32)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    assert np.array_equal(np.isinf(got), np.isinf(want))
    ok = ~np.isnan(want)
    same(got.view(np.uint32)[ok], want.view(np.uint32)[ok], "around the non-finite samples")


@pytest.mark.parametrize("ntaps,L,kernel,name", ANCHORS)
def test_anchor_subnormals(oracle, ntaps, L, kernel, name):
    """A stream scaled into the subnormals: bit-exact, nothing is flushed."""
    num, den = 123, 1000
    h = anchor_taps(ntaps, L, num, den, False)
    x = (streams(1, N_ANCHOR, 15) * np.float32(2.0 ** -130)).astype(np.complex64)
    assert 0 < np.abs(x.view(np.float32)).max() < np.finfo(np.float32).tiny
    rig = Rig(oracle, x)
    plan = TranslatingInterpolator(h, L, num, den)
    plan.set_kernel(kernel)
    want = rig.ref(h, L, plan.contract[0], num, den)
    assert np.count_nonzero(want.view(np.float32)) > want.size // 2
    same(rig.stream(plan, [N_ANCHOR], [name]), want, "subnormal stream")
