"""The tuner bank's references (include/sxfir_bank.h), shared by tests/test_bank_host.py and tests/test_gpu_bank.py.

Band k of a bank is DEFINED as the translating decimator of its taps and centre, so the bank needs nothing new of the oracle: per
band the bit-exact reference is mix_cases.mix_ref and the fp64 definition mix_cases.mix_f64.  The Rig is tests/test_gpu_mix.py's
with an output block of [nchan, K, row] words: every band's row lies between two guards of fill words that must come back
untouched."""
import numpy as np
import pytest

from mix_cases import mix_f64, mix_ref

FILL = 0x7FC07FC0               # a NaN as one fp32 word and as two halves: no output of these streams is this word
GUARD = 8                       # samples of fill words on either side of every band's row (whole 16-byte units in both formats)
TILE = 2048                     # inputs per tile of decim4_bank_kernel
TILED, GENERIC = "decim4_bank_kernel", "decim_bank_generic_kernel"
EINVAL, EUNSUPPORTED = -1, -4
PAIRS = [(3, 7), (123, 1000), (12345, 65536), (1, 4)]         # tests/test_gpu_mix.py's centres


def _i32(word):
    return word - (1 << 32) if word >= 1 << 31 else word


def cdiv(a, b):
    return -(-a // b)


def bank_ref(oracle, hs, ratio, x, contract, centres, m_first=0):
    """complex64 [K, n_out]: band k is mix_ref of taps hs[k] and centre centres[k] over x from zero history."""
    return np.stack([mix_ref(oracle, hs[k], ratio, x, contract, num, den, m_first) for k, (num, den) in enumerate(centres)])


def bank_f64(hs, ratio, x, centres, m_first=0):
    """complex128 [K, n_out]: the definition, band by band."""
    return np.stack([mix_f64(hs[k], ratio, num, den, x, m_first) for k, (num, den) in enumerate(centres)])


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

    def ref(self, hs, ratio, contract, centres, first=0, count=None, m_first=None):
        """[nchan, K, words] of one pass over inputs [0, first + count) from zero history, the outputs of inputs [first, ..) alone;
        the first of THOSE has the absolute index m_first (default: its index in this stream)."""
        count = self.n - first if count is None else count
        skip = cdiv(first, ratio)
        m0 = 0 if m_first is None else m_first - skip
        return np.stack([self.words(bank_ref(self.oracle, hs, ratio, self.x[c, :first + count], contract, centres, m0)[:, skip:])
                         for c in range(self.nchan)])

    def call(self, plan, pos, n, kernel=None, offset=0, expect=None, odd_stride=False, odd_band=False, slack=0, short_band=False):
        """sxfir_decimate_bank over inputs [pos, pos + n) of every row.  Returns [nchan, K, words]; with `expect` (an error code) the
        call must fail with it and leave the plan and the output buffer alone.  `slack`: samples a band's row is longer than it
        must be; odd_band / odd_stride: a band's / a channel's stride one sample more; short_band: a band stride one below the
        outputs per band."""
        import torch
        D, K = plan.ratio, plan.nbands
        c0, p0 = plan.position
        assert p0 == cdiv(c0, D)
        n_out = cdiv(c0 + n, D) - p0
        assert plan.outputs_for(n) == n_out
        if kernel is not None:
            assert plan.geometry(n)["kernel"] == kernel, (plan.geometry(n), kernel)
        row = 2 * GUARD + offset + n_out + (offset + n_out) % 2 + 2 * slack    # an even band stride, larger than the block
        row += 1 if odd_band else 0
        chan = K * row + (K * row) % 2 + (1 if odd_stride else 0)              # samples between two channels' blocks
        buf = torch.full((self.nchan, chan * self.wps), _i32(FILL), dtype=torch.int32, device="cuda")
        args = (self.xg.data_ptr() + self.sb_in * pos, n, self.stride, buf.data_ptr() + self.sb * (GUARD + offset), chan,
                n_out - 1 if short_band else row, torch.cuda.current_stream().cuda_stream)
        if expect is not None:
            import sxxcvr_amd
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
        got = buf.cpu().numpy().view(np.uint32).reshape(self.nchan, chan, self.wps)
        assert np.all(got[:, K * row:] == FILL), "the words behind a channel's last band were written"
        got = got[:, :K * row].reshape(self.nchan, K, row, self.wps)
        lo, hi = GUARD + offset, GUARD + offset + n_out
        assert np.all(got[:, :, :lo] == FILL) and np.all(got[:, :, hi:] == FILL), "the guard around a band's outputs was written"
        return np.ascontiguousarray(got[:, :, lo:hi]).reshape(self.nchan, K, n_out * self.wps)

    def stream(self, plan, blocks, kernels=None, pos=0):
        outs = []
        for i, b in enumerate(blocks):
            outs.append(self.call(plan, pos, b, None if kernels is None else kernels[i]))
            pos += b
        return np.concatenate(outs, axis=2)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.ravel() != want.ravel())[0]
    assert not bad.size, "%s: %d of %d words differ, first at %d: got %08x want %08x" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


# ---- the tiled kernel's per-band index walk, as the code takes it ---------------------------------------------------------------
def bank_reduce_model(x, den):
    """decim4_bank_kernel's bank_reduce: x mod den for x < 64 den through the float32 quotient and two unsigned minimums."""
    x = np.asarray(x, dtype=np.int64)
    assert x.min() >= 0 and x.max() < 64 * den
    rden = np.float32(1.0) / np.float32(den)
    q = np.multiply(x.astype(np.float32), rden).astype(np.int64)              # (float -> unsigned: truncation)
    r = (x - q * den) % (1 << 32)                                             # a 32-bit register wraps
    r = np.minimum(r, (r + den) % (1 << 32))
    r = np.minimum(r, (r - den) % (1 << 32))
    return r


def bank_walk_model(centres, n_waves, w8, n_tiles, m_first=0):
    """decim4_bank_kernel's table indices for every band, every step as the code takes it, all waves of a grid side by side:
    bank_bands' steps (sxfir_launch.hip.h) per band, then per wave and band the first tile's phase -- the kernel's two divisions,
    into the phase word of the band --, and per tile the band loop: the lane's first index (bank_reduce of the band's phase word plus
    lane * lane_step), the add-and-subtract walk over the lane's eight outputs, the phase word advanced by stride_step.  Returns
    the indices [K, n_tiles, 512] and the largest intermediate value met; asserts that every value a 32-bit register holds stays
    below 2^32, every index below den, and that every tile is one wave's."""
    from mix_cases import step
    K = len(centres)
    top = 0

    def u32(v):
        nonlocal top
        v = np.asarray(v)
        assert v.min() >= 0 and v.max() < 2 ** 32, int(v.max())
        top = max(top, int(v.max()))
        return v

    b = np.arange(n_waves, dtype=np.int64)
    tile0 = (b & 7) * w8 + (b >> 3) if w8 else b.copy()          # wide_first_tile: XCD-blocked, or plain strided dealing
    lane = np.arange(64, dtype=np.int64)
    out = np.full((K, n_tiles, 512), -1, dtype=np.int64)
    band = []
    for num, den in centres:
        s = step(num, den, 4)
        tile_step = 512 * s % den
        band.append(dict(den=den, s=s, lane_step=8 * s % den, tile_step=tile_step, stride_step=n_waves % den * tile_step % den,
                         phase=int(m_first) % den * s % den))                  # mixer_of's rule
    # the prologue: every band's phase word at the wave's first tile
    ph = []
    for bd in band:
        den = bd["den"]
        v = u32(bd["phase"] + u32(u32(tile0 % den) * bd["tile_step"]) % den)
        ph.append(v - den * (v >= den))
    tile = tile0.copy()
    while (tile < n_tiles).any():
        live = tile < n_tiles
        for k, bd in enumerate(band):
            den, s = bd["den"], bd["s"]
            assert (out[k, tile[live]] == -1).all(), "two waves own one tile"
            idx = bank_reduce_model(u32(ph[k][:, None] + u32(lane * bd["lane_step"])[None, :]), den)
            for i in range(8):
                assert idx[live].max() < den
                out[k, tile[live][:, None], (8 * lane + i)[None, :]] = idx[live]
                idx = u32(idx + s)
                idx = idx - den * (idx >= den)
            v = u32(ph[k] + bd["stride_step"])
            ph[k] = v - den * (v >= den)
        tile = tile + n_waves
    assert (out >= 0).all(), "a tile is no wave's"
    return out, top
