"""The frequency-translating interpolators' references (include/sxfir_translate_tx.h), shared by tests/test_mix_tx_host.py and
tests/test_gpu_mix_tx.py.

The bit-exact reference needs nothing new of the oracle: the input is rotated in float32 by mix_cases.rotate_f32 -- six float32
operations per sample, each a numpy ufunc call of its own -- on the table that sxfir_design_rotator makes, at the index
(den - (m s mod den)) mod den = (m t) mod den with t = (den - s) mod den, and the rotated stream goes through the complex-tap
interpolator's reference (gpu_util.cx_interp_ref).  The fp64 definition uses neither the library's table nor its reference."""
import numpy as np

from gpu_util import cx_interp_ref
from mix_cases import BOUND, rotate_f32

ROT_IN = 8.0                # a rotated component is off by at most ROT_UNITS 2^-24 (|re| + |im|) <= 8 2^-24 |x| (|re| + |im| <= sqrt 2 |x|)


def step(num, den, ratio):
    """s: the turn per input sample, in table entries."""
    return (int(num) % int(den)) * int(ratio) % int(den)


def back_step(num, den, ratio):
    """t = (den - s) mod den: the table index of input m is (m t) mod den."""
    return (int(den) - step(num, den, ratio)) % int(den)


def table_index(m_first, n, s, den):
    """int64 [n]: (den - ((m_first + i) s mod den)) mod den, exact (m_first: a Python int of any size and either sign -- the
    mathematical modulo)."""
    m = (int(m_first) % int(den) + np.arange(n, dtype=np.int64)) % int(den)
    return (int(den) - (m * int(s)) % int(den)) % int(den)


def rotate_in_f32(x, num, den, ratio, m_first=0):
    """complex64 [.., n]: xr[i] = x[i] * w[(den - ((m_first + i) s mod den)) mod den] in float32, six roundings."""
    from sxxcvr_amd import design_rotator
    return rotate_f32(x, design_rotator(den), m_first, back_step(num, den, ratio), den)


def mix_tx_ref(oracle, h, ratio, x, jsplit, num, den, m_first=0, threads=None):
    """complex64: one translating pass over x from zero history, its first input at the absolute index m_first."""
    return cx_interp_ref(oracle, h, ratio, rotate_in_f32(x, num, den, ratio, m_first), jsplit, threads=threads)


def rotor_f64(m_first, n, s, den):
    """complex128 [n]: exp(+2j pi ((m_first + i) s mod den) / den), the index reduced in integers."""
    m = (int(m_first) % int(den) + np.arange(n, dtype=np.int64)) % int(den)
    return np.exp(2j * np.pi * ((m * int(s)) % int(den)).astype(np.float64) / float(den))


def mix_tx_f64(h, ratio, num, den, x, m_first=0):
    """complex128: the definition -- y[n] = sum_j h[j L + n mod L] xr[n / L - j], xr[m] = x[m] exp(+2j pi num L m / den) with m the
    absolute 64-bit input index, x[<0] = 0."""
    x = np.asarray(x, dtype=np.complex128)
    xr = x * rotor_f64(m_first, x.size, step(num, den, ratio), den)
    up = np.zeros(ratio * x.size, dtype=np.complex128)
    up[::ratio] = xr
    return np.convolve(up, np.asarray(h, dtype=np.complex128))[:up.size]


def bound(h, x):
    """Per component of an output: (BOUND (1 + 2^-20) + 8 2^-24) sum|h| max|x| -- mix_cases.BOUND on the chain over xr (whose
    samples are at most (1 + 2^-20) |x|), and the rotation's error of at most 8 2^-24 |x| per sample through sum|h|."""
    sh = float(np.abs(np.asarray(h).astype(np.complex128)).sum())
    return (BOUND * (1.0 + 2.0 ** -20) + ROT_IN * 2.0 ** -24) * sh * float(np.abs(np.asarray(x, dtype=np.complex128)).max())


def tile_walk_model(num, den, ratio, n_groups, n_tiles, consumed=0):
    """interp_mix_pass_kernel's table indices, every step as the code takes it, all waves of a grid side by side (int64 arrays,
    one row per wave): imix_tile_args' steps (sxfir_launch.hip.h), then per wave the first tile's phase and the lane's offsets --
    the kernel's divisions -- and the add-and-subtract walk over (tile, DMA instruction, lane, sample).  Returns the indices
    [n_tiles, TILE_IN + 32] of every image sample (tile's sample -32 first) and the largest intermediate value met; asserts that
    every value a 32-bit register holds stays below 2^32, every index below den, and that every tile is one wave's."""
    tile_in = 256 if ratio == 4 else 128
    chunks = (tile_in + 32) // 2
    nload = (chunks + 63) // 64
    t = back_step(num, den, ratio)
    phase = ((int(consumed) - 32) % den) * t % den               # mixer_of(.., consumed, 32): Python's modulo is the mathematical one
    lane_step = 2 * t % den
    instr_step = 128 * t % den
    tile_step = tile_in * t % den
    stride_step = n_groups % den * tile_step % den
    top = 0

    def u32(v):
        nonlocal top
        v = np.asarray(v)
        assert v.min() >= 0 and v.max() < 2 ** 32, int(v.max())
        top = max(top, int(v.max()))
        return v

    def wrap(v):                                                # if (v >= den) v -= den
        return v - den * (v >= den)

    b = np.arange(n_groups, dtype=np.int64)
    # syn_first_tile: XCD-blocked when the grid is a multiple of 8, else plainly strided
    tile = (b & 7) * (n_groups // 8) + (b >> 3) if n_groups % 8 == 0 else b.copy()
    lane = np.arange(64, dtype=np.int64)
    lane_ph = [u32(lane * lane_step) % den]
    for i in range(1, nload):
        lane_ph.append(wrap(u32(lane_ph[-1] + instr_step)))
    tile_ph = wrap(u32(phase + u32(u32(tile % den) * tile_step) % den))
    out = np.full((n_tiles, tile_in + 32), -1, dtype=np.int64)
    while (tile < n_tiles).any():
        live = tile < n_tiles
        assert (out[tile[live]] == -1).all(), "two waves own one tile"
        for i in range(nload):
            i0 = wrap(u32(tile_ph[:, None] + lane_ph[i][None, :]))
            i1 = wrap(u32(i0 + t))
            assert i0[live].max() < den and i1[live].max() < den
            ok = 64 * i + lane < chunks                         # (the slots past the image's end are read and not written)
            out[tile[live][:, None], (2 * (64 * i + lane[ok]))[None, :]] = i0[live][:, ok]
            out[tile[live][:, None], (2 * (64 * i + lane[ok]) + 1)[None, :]] = i1[live][:, ok]
        tile = tile + n_groups
        tile_ph = wrap(u32(tile_ph + stride_step))
    assert (out >= 0).all(), "a tile is no wave's"
    return out, top
