"""The combiner bank's references (include/sxfir_bank_tx.h), shared by tests/test_bank_tx_host.py and tests/test_gpu_bank_tx.py.

The combiner's output is DEFINED as the float32 sum, in band order, of the translating interpolators of its bands, so it needs
nothing new of the oracle: per band the bit-exact reference is mix_tx_cases.mix_tx_ref, the sum is numpy float32 adds (K = 1 adds
nothing), and the fp64 definition is the sum of mix_tx_cases.mix_tx_f64.  The Rig holds an input block of [nchan, K, row] or
[K, nchan, row] words -- every band's row is followed by NaN words, so a read past n_in shows -- and an output block between two
guards of fill words that must come back untouched."""
import numpy as np
import pytest

from mix_tx_cases import back_step, bound, mix_tx_f64, mix_tx_ref

FILL = 0x7FC07FC0               # a NaN as one fp32 word and as two halves: no output of these streams is this word
GUARD = 8                       # samples of fill words on either side of a channel's outputs (whole 16-byte units in both formats)
TILE_IN = 256                   # inputs per band and tile of interp4_bank_kernel
TILED, GENERIC = "interp4_bank_kernel", "interp_bank_generic_kernel"
EINVAL, EUNSUPPORTED = -1, -4


def _i32(word):
    return word - (1 << 32) if word >= 1 << 31 else word


def sum_in_order(ys, order=None):
    """complex64 [n]: acc = ys[o0]; acc = float32(acc + ys[ok]) for the rest of `order`, re and im each (one numpy float32 add per
    component and band: no pairwise summation, no wider accumulator)."""
    order = range(len(ys)) if order is None else order
    acc = None
    for k in order:
        y = np.ascontiguousarray(ys[k], dtype=np.complex64).view(np.float32)
        acc = y.copy() if acc is None else np.add(acc, y, dtype=np.float32)
    return acc.view(np.complex64)


def band_refs(oracle, hs, ratio, xs, jsplit, centres, m_first=0, threads=None):
    """K complex64 arrays: y_k, the translating interpolator of band k over xs[k] from zero history."""
    return [mix_tx_ref(oracle, hs[k], ratio, xs[k], jsplit, num, den, m_first, threads=threads) for k, (num, den) in enumerate(centres)]


def combiner_ref(oracle, hs, ratio, xs, jsplit, centres, m_first=0, threads=None):
    """complex64 [ratio n]: the definition's bits over xs [K, n] from zero history, input 0 at the absolute index m_first."""
    return sum_in_order(band_refs(oracle, hs, ratio, xs, jsplit, centres, m_first, threads))


def combiner_f64(hs, ratio, xs, centres, m_first=0):
    """complex128 [ratio n]: the fp64 definition -- neither the library's table nor its float reference."""
    return sum(mix_tx_f64(hs[k], ratio, num, den, xs[k], m_first) for k, (num, den) in enumerate(centres))


def combiner_bound(hs, xs, ys):
    """Per component of an output (an array): sum_k bound_k + (K - 1) 2^-24 sum_k (|y_k| + bound_k) -- every band's own bound
    (mix_tx_cases.bound), and for each of the K - 1 adds half an ulp of a partial sum, which is at most sum_k (|y_k| + bound_k)."""
    K = len(hs)
    b = [bound(hs[k], xs[k]) for k in range(K)]
    mag = sum(np.maximum(np.abs(ys[k].real), np.abs(ys[k].imag)) + b[k] for k in range(K))
    return sum(b) + (K - 1) * 2.0 ** -24 * mag


def combiner_walk_model(centres, n_groups, n_tiles, consumed=0):
    """interp4_bank_kernel's table indices, every step as the code takes it, all waves of a grid side by side (int64 arrays, one row
    per wave): bank_tx_bands' steps (sxfir_launch.hip.h), then per wave and band the word of the prologue -- the first tile's phase and
    the lane's offset in one value, the kernel's divisions -- and per step (tile, band) the fetch: the lane's three chunks by
    instr_step, the chunk's second sample by t, the word moved on by stride_step.  Returns the indices [K, n_tiles, 288] of every image
    sample (tile's sample -32 first) and the largest intermediate value met; asserts that every value a 32-bit register holds stays
    below 2^32, every index below den, and that every tile is one wave's."""
    tile_in, chunks, nload = TILE_IN, (TILE_IN + 32) // 2, 3
    top = 0

    def u32(v):
        nonlocal top
        v = np.asarray(v)
        assert v.min() >= 0 and v.max() < 2 ** 32, int(v.max())
        top = max(top, int(v.max()))
        return v

    b = np.arange(n_groups, dtype=np.int64)
    # syn_first_tile: XCD-blocked when the grid is a multiple of 8, else plainly strided
    first_tile = (b & 7) * (n_groups // 8) + (b >> 3) if n_groups % 8 == 0 else b.copy()
    lane = np.arange(64, dtype=np.int64)
    K = len(centres)
    out = np.full((K, n_tiles, tile_in + 32), -1, dtype=np.int64)
    band = []
    for num, den in centres:
        t = back_step(num, den, 4)
        tile_step = tile_in * t % den
        band.append(dict(den=den, t=t, phase=((int(consumed) - 32) % den) * t % den, lane_step=2 * t % den, instr_step=128 * t % den,
                         tile_step=tile_step, stride_step=n_groups % den * tile_step % den))
    # the prologue: band_ph[k][lane] of every wave
    words = []
    for bd in band:
        den = bd["den"]
        wrap = lambda v, den=den: v - den * (v >= den)                  # if (v >= den) v -= den
        ph = wrap(u32(bd["phase"] + u32(u32(first_tile % den) * bd["tile_step"]) % den))
        words.append(wrap(u32(ph[:, None] + (u32(lane * bd["lane_step"]) % den)[None, :])))
    tile = first_tile.copy()
    while (tile < n_tiles).any():
        live = tile < n_tiles
        for k, bd in enumerate(band):                                   # the steps (tile, 0) .. (tile, K - 1)
            den, t = bd["den"], bd["t"]
            wrap = lambda v, den=den: v - den * (v >= den)
            assert (out[k, tile[live]] == -1).all(), "two waves own one tile"
            ph = words[k]
            words[k] = wrap(u32(ph + bd["stride_step"]))
            for i in range(nload):
                i0 = ph
                i1 = wrap(u32(i0 + t))
                assert i0[live].max() < den and i1[live].max() < den
                ok = 64 * i + lane < chunks                             # (the slots past the image's end are read and not written)
                out[k, tile[live][:, None], (2 * (64 * i + lane[ok]))[None, :]] = i0[live][:, ok]
                out[k, tile[live][:, None], (2 * (64 * i + lane[ok]) + 1)[None, :]] = i1[live][:, ok]
                ph = wrap(u32(ph + bd["instr_step"]))
        tile = tile + n_groups
    assert (out >= 0).all(), "a tile is no wave's"
    return out, top


class Rig:
    """K band streams per channel, x [nchan, K, n], on the GPU in one of the two layouts -- "bands": a channel's bands in a row,
    channel after channel; "channels": a band's channels in a row, band after band -- every row `pad` samples longer than the stream
    and filled with NaN words behind it; and their CPU twin as the plan sees them (CF16: quantised to half; S32: CF32 in, wire words
    out)."""

    def __init__(self, oracle, x, fmt="CF32", layout="bands", pad=41, thr2=None):
        import torch
        x = np.ascontiguousarray(x, dtype=np.complex64)
        assert x.ndim == 3
        self.oracle, self.fmt, self.thr2 = oracle, fmt, thr2
        self.nchan, self.K, self.n = x.shape
        self.sb_in, self.wps_in = (4, 1) if fmt == "CF16" else (8, 2)          # input: bytes, 32-bit words per sample
        self.sb, self.wps = self.sb_in, self.wps_in                           # output (S32: wire words, 8 bytes too)
        self.row = self.n + pad
        if layout == "bands":
            self.in_stride, self.band_stride = self.K * self.row, self.row
        else:
            self.in_stride, self.band_stride = self.row, self.nchan * self.row
        if fmt == "CF16":
            h16 = oracle.f32_to_f16(x.view(np.float32).reshape(-1)).reshape(self.nchan, self.K, 2 * self.n)
            self.x = oracle.f16_to_f32(h16.reshape(-1)).view(np.complex64).reshape(x.shape)
            words = np.ascontiguousarray(h16).view(np.int32)
        else:
            self.x = x
            words = x.view(np.int32)
        buf = np.full(self.nchan * self.K * self.row * self.wps_in, _i32(FILL), dtype=np.int32)
        for c in range(self.nchan):
            for k in range(self.K):
                o = (c * self.in_stride + k * self.band_stride) * self.wps_in
                buf[o:o + self.n * self.wps_in] = words[c, k]
        self.xg = torch.from_numpy(buf).cuda()

    def words(self, y):
        """complex64 [n] reference -> the 32-bit words the plan stores"""
        y = np.ascontiguousarray(y, dtype=np.complex64)
        if self.fmt == "CF16":
            return np.ascontiguousarray(self.oracle.f32_to_f16(y.view(np.float32))).view(np.uint32)
        if self.fmt == "S32":
            return self.oracle.convert_tx(y, np.float32(self.thr2)).view(np.uint32)
        return y.view(np.uint32)

    def ref(self, hs, L, jsplit, centres, first=0, count=None, m_first=None, threads=None):
        """[nchan, words] of one pass over inputs [0, first + count) from zero history, the outputs of inputs [first, ..) alone;
        input `first` has the absolute index m_first (default: its index in this stream)."""
        count = self.n - first if count is None else count
        m0 = 0 if m_first is None else m_first - first
        return np.stack([self.words(combiner_ref(self.oracle, hs, L, self.x[c, :, :first + count], jsplit, centres, m0, threads)[L * first:])
                         for c in range(self.nchan)])

    def call(self, plan, pos, n, kernel=None, offset=0, expect=None, odd_stride=False, band_stride=None, out_stride=None):
        """sxfir_interpolate_bank over inputs [pos, pos + n) of every band.  Returns [nchan, words]; with `expect` (an error code) the
        call must fail with it and leave the plan's position and the output buffer alone."""
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
        args = (self.xg.data_ptr() + self.sb_in * pos, n, self.in_stride, self.band_stride if band_stride is None else band_stride,
                buf.data_ptr() + self.sb * (GUARD + offset), row if out_stride is None else out_stride,
                torch.cuda.current_stream().cuda_stream)
        if expect is not None:
            with pytest.raises(Exception) as ei:
                plan.process_ptr(*args)
            torch.cuda.synchronize()
            assert ei.value.code == expect, ei.value
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
