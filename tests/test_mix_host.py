"""CPU-side checks of the frequency-translating decimators (include/sxfir_translate.h): the extension's symbols and bindings, the
refusals of sxfir_create_translating and sxfir_design_rotator that need no GPU, the rotation table against numpy fp64, the float32
reference of tests/mix_cases.py against the fp64 definition, and the shipped code object of the new kernels."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_bandpass, design_rotator
from gpu_util import cx_decim_ref, random_taps_cx
from mix_cases import ROT_UNITS, bound, mix_f64, mix_ref, rotate_f32, rotor_f64, step, table_index
from rational_cases import gaussian_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    names = _declared("sxfir_translate.h")
    assert names == ["sxfir_create_translating", "sxfir_design_rotator", "sxfir_plan_translation", "sxfir_translate_abi_version"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_translate_abi_version() == 1 and prof.sxfir_translate_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_translate.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_TRANSLATE_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    # the base ABI's number is the header's, untouched by the extension
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    assert lib.sxfir_abi_version() == int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 6
    assert sxxcvr_amd.TranslatingDecimator.__mro__[1] is sxxcvr_amd.Resampler


def test_refusals_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    create = lib.sxfir_create_translating
    taps = np.ones(2 * 128, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    CF32, CF16, S32 = 0, 1, 2
    assert create(None, tp, 128, 4, 3, 7, 1, CF32, -1) == EINVAL
    # (taps, ntaps, ratio, num, den, nchan, fmt) -> code and a word of the message, in the order the creator checks them
    cases = [((None, 128, 4, 3, 7, 1, CF32), EINVAL, b"NULL"),
             ((tp, 0, 4, 3, 7, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 65537, 4, 3, 7, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 128, 0, 3, 7, 1, CF32), EINVAL, b"ratio"),
             ((tp, 128, 4097, 3, 7, 1, CF32), EINVAL, b"ratio"),
             ((tp, 128, 4, 3, 7, 0, CF32), EINVAL, b"nchan"),
             ((tp, 128, 4, 3, 7, 1, 9), EINVAL, b"format"),
             ((tp, 128, 4, 3, 0, 1, CF32), EINVAL, b"den 0 out of range"),
             ((tp, 128, 4, 3, -7, 1, S32), EINVAL, b"den -7 out of range"),
             ((tp, 128, 4, 3, 65537, 1, CF16), EINVAL, b"den 65537 out of range"),
             # two bad arguments at once: the earlier check answers
             ((tp, 0, 0, 3, 0, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 128, 0, 3, 0, 0, CF32), EINVAL, b"ratio"),
             ((tp, 128, 4, 3, 0, 0, 9), EINVAL, b"nchan"),
             ((tp, 128, 4, 3, 0, 1, 9), EINVAL, b"format")]
    for args, code, word in cases:
        plan.value = 0xDEAD if args[0] is not None else None
        assert create(C.byref(plan), *args, -1) == code, args
        assert word in lib.sxfir_last_error(), (args, lib.sxfir_last_error())
        assert not plan.value, args
    w = np.empty(2 * 8, dtype=np.float32)
    wp = w.ctypes.data_as(C.c_void_p)
    assert lib.sxfir_design_rotator(8, None) == EINVAL and b"NULL" in lib.sxfir_last_error()
    for den in (0, -1, 65537):
        assert lib.sxfir_design_rotator(den, wp) == EINVAL and b"out of range" in lib.sxfir_last_error(), den
    n, d = C.c_int(-1), C.c_int(-1)
    assert lib.sxfir_plan_translation(None, C.byref(n), C.byref(d)) == EINVAL
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        design_rotator(0)
    assert ei.value.code == EINVAL
    count = C.c_int(-1)
    lib.sxfir_device_count(C.byref(count))
    if count.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_mix.py)
    # no GPU: refused as the complex-tap create refuses, never computed on the host
    for fmt in (CF32, CF16, S32):
        assert create(C.byref(plan), tp, 128, 4, 3, 7, 1, fmt, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.TranslatingDecimator(design_bandpass(128, 4, 3, 7), 4, 3, 7)
    assert ei.value.code == ENODEVICE


@pytest.mark.parametrize("den", [1, 4, 7, 1000, 65536])
def test_rotator_against_numpy_fp64(den):
    w = design_rotator(den)
    assert w.dtype == np.complex64 and w.shape == (den,)
    want = np.exp(-2j * np.pi * np.arange(den, dtype=np.float64) / den)
    # fp32 rounding is 2^-24 relative; the rest covers libm differences of a few fp64 ulps (test_bandpass_against_fp64_restatement)
    tol = 2.0 ** -22
    err = max(np.abs(w.real.astype(np.float64) - want.real).max(), np.abs(w.imag.astype(np.float64) - want.imag).max())
    print("den %d: max component error %.3g, tolerance %.3g" % (den, err, tol))
    assert err <= tol
    # w[0] = (1, +0.0) bit for bit
    assert w[:1].view(np.uint32).tolist() == [0x3F800000, 0x00000000]


PAIRS = [(7, 3), (1000, 123), (65536, 12345), (4, 1), (65535, 65534)]


@pytest.mark.parametrize("den,num", PAIRS)
def test_rotate_f32_against_fp64(den, num):
    """The float32 rotation at absolute indices near 2^40 against fp64 with the index reduced exactly: per component at most
    4 * 2^-24 * (|z.re| + |z.im|)."""
    s = step(num, den, 5)
    n = 20000
    m_first = (1 << 40) + 12345
    z = gaussian_stream(n, 21 + den)
    idx = table_index(m_first, n, s, den)
    assert idx.tolist()[:3] == [(m_first + i) * s % den for i in range(3)]            # (Python integers: no 64-bit product to overflow)
    got = rotate_f32(z, design_rotator(den), m_first, s, den).astype(np.complex128)
    want = z.astype(np.complex128) * rotor_f64(m_first, n, s, den)
    unit = 2.0 ** -24 * (np.abs(z.real.astype(np.float64)) + np.abs(z.imag.astype(np.float64)))
    worst = max((np.abs(got.real - want.real) / unit).max(), (np.abs(got.imag - want.imag) / unit).max())
    print("den %d num %d: worst error %.2f units of 2^-24 (|z.re| + |z.im|), bound %.0f" % (den, num, worst, ROT_UNITS))
    assert worst <= ROT_UNITS


@pytest.mark.parametrize("ntaps,ratio,num,den", [(128, 4, 3, 7), (128, 4, 12345, 65536), (35, 5, 123, 1000)])
def test_reference_against_fp64(oracle, ntaps, ratio, num, den):
    """mix_ref (the oracle's two real-tap passes, the float32 combine, the float32 rotation) against the fp64 definition, within the
    complex anchors' bound plus the rotation's term, from the stream's start and from an absolute index near 2^40."""
    h = design_bandpass(ntaps, ratio, num, den) if ntaps == 128 else random_taps_cx(35, 9)
    x = gaussian_stream(3000 + 3)
    contract = sxxcvr_amd.resampler.Contract((2, 4) if ntaps == 128 else (1, 5), 0)
    for m_first in (0, (1 << 40) + 77):
        got = mix_ref(oracle, h, ratio, x, contract, num, den, m_first).astype(np.complex128)
        want = mix_f64(h, ratio, num, den, x, m_first)
        assert got.shape == want.shape == (-(-x.size // ratio),)
        b = bound(h, x, want)
        err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
        print("/%d x %d, %d/%d from %d: worst error %.3g, bound there %.3g" % (ratio, ntaps, num, den, m_first, err.max(), b[err.argmax()]))
        assert np.all(err <= b)
    # and the reference is what its name says: the complex plan's reference, rotated
    z = cx_decim_ref(oracle, h, ratio, x, contract)
    assert np.array_equal(mix_ref(oracle, h, ratio, x, contract, num, den).view(np.uint32),
                          rotate_f32(z, design_rotator(den), 0, step(num, den, ratio), den).view(np.uint32))


def tile_walk_model(num, den, n_waves, w8, n_tiles, phase=0):
    """decim4_mix_kernel's table indices, every step as the code takes it, all waves of a grid side by side (int64 arrays, one row
    per wave): mix_tile_args' three steps (sxfir_launch.hip.h), then per wave the first tile's phase -- the kernel's two divisions
    --, the lane's offset, and the add-and-subtract walk over (tile, lane, i).  Returns the indices [n_tiles, 512] and the largest
    intermediate value met; asserts that every value a 32-bit register holds stays below 2^32, every index below den, and that
    every tile is one wave's."""
    s = step(num, den, 4)
    lane_step = 8 * s % den
    tile_step = 512 * s % den
    stride_step = n_waves % den * tile_step % den
    top = 0

    def u32(v):
        nonlocal top
        assert v.min() >= 0 and v.max() < 2 ** 32, int(v.max())
        top = max(top, int(v.max()))
        return v

    def wrap(v):                                                # if (v >= den) v -= den
        return v - den * (v >= den)

    b = np.arange(n_waves, dtype=np.int64)
    tile = (b & 7) * w8 + (b >> 3) if w8 else b.copy()          # wide_first_tile: XCD-blocked, or plain strided dealing
    lane = np.arange(64, dtype=np.int64)
    lane_ph = u32(lane * lane_step) % den
    tile_ph = wrap(u32(phase + u32(u32(tile % den) * tile_step) % den))
    out = np.full((n_tiles, 512), -1, dtype=np.int64)
    while (tile < n_tiles).any():
        live = tile < n_tiles                                   # (a wave past the last tile has left the loop)
        assert (out[tile[live]] == -1).all(), "two waves own one tile"
        idx = wrap(u32(tile_ph[:, None] + lane_ph[None, :]))
        for i in range(8):
            assert idx[live].max() < den
            out[tile[live][:, None], (8 * lane + i)[None, :]] = idx[live]
            idx = wrap(u32(idx + s))
        tile = tile + n_waves
        tile_ph = wrap(u32(tile_ph + stride_step))
    assert (out >= 0).all(), "a tile is no wave's"
    return out, top


def test_the_tile_walk_arithmetic_stays_in_32_bits_and_hits_the_table_index():
    """The three steps mix_tile_args hands decim4_mix_kernel and the kernel's walk, modelled step by step (tile_walk_model), against
    mix_cases.table_index for every mixer of the sweep's menu at /4: grids of 1, 3, 8 and 512 waves, XCD-blocked (w8 = waves / 8)
    and plainly strided (w8 = 0), over 3 waves + 3 tiles, so that every wave walks to a third tile and three to a fourth, from a first
    output at 0, at den - 1 and near 2^40.  What the kernel's comments claim -- "no sum reaches 2^17", "65535^2 < 2^32" -- holds: no
    intermediate value leaves 32 bits, no index reaches den."""
    import rate_cases as rc
    worst = 0
    for cls, den, num in rc.MIXERS + (("tile walk", 7, 3), ("tile walk", 3, 1)):
        num = rc.mixer_num(cls, den, num, 4)
        s = step(num, den, 4)
        for n_waves in (1, 3, 8, 512):
            for w8 in sorted({0, n_waves // 8 if n_waves % 8 == 0 else 0}):
                n_tiles = 3 * n_waves + 3
                for m_first in (0, den - 1, (1 << 40) + 77):
                    phase = m_first % den * s % den                             # mixer_of (sxfir_launch.hip.h)
                    got, top = tile_walk_model(num, den, n_waves, w8, n_tiles, phase)
                    worst = max(worst, top)
                    want = table_index(m_first, 512 * n_tiles, s, den).reshape(n_tiles, 512)
                    bad = np.nonzero((got != want).any(axis=1))[0]
                    assert bad.size == 0, "den %d num %d, %d waves, w8 %d, from %d: tile %d" % (den, num, n_waves, w8, m_first, bad[0])
    print("largest intermediate value: %d (2^32 = %d)" % (worst, 2 ** 32))
    # the one product the grids above keep small, (tile mod den) tile_step of a wave's first tile, at its largest: den - 1 each
    assert worst < 2 ** 32 and 65535 * 65535 < 2 ** 32 and 63 * 65535 < 2 ** 32


def test_shipped_code_object_of_the_mix_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    # the mixer instance of the complex-tap decimators' kernel (the launch geometry's decim4_mix_kernel)
    tiled = [r for r in rows if r["name"] == "decim4_cx_kernel<sxfir::MixTileArgs>"]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    # decim4_cx_kernel's tile: 2 chains x 8 outputs x 128 taps per lane, 18 496 B of LDS and at most 256 VGPRs (8 waves per CU)
    assert t["v_pk_fma_f32"] == 2048, t
    assert t["lds_bytes"] == 18496 and t["vgpr"] <= 256 and t["scratch_bytes"] == 0, t
    assert t["v_mfma"] == 0 and t["s_barrier"] == 0, t
    # ... and of their generic kernel (the launch geometry's decim_mix_generic_kernel)
    generic = sorted(r["name"] for r in rows if r["name"].startswith("decim_cx_generic_kernel<") and r["name"].endswith(", sxfir::MixGenericArgs>"))
    assert generic == ["decim_cx_generic_kernel<sxfir::CF16, sxfir::CF16, sxfir::MixGenericArgs>",
                       "decim_cx_generic_kernel<sxfir::CF32, sxfir::CF32, sxfir::MixGenericArgs>",
                       "decim_cx_generic_kernel<sxfir::S32, sxfir::CF32, sxfir::MixGenericArgs>"], generic
    for r in rows:
        if r["name"] in generic:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r
