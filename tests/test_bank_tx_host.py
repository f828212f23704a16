"""CPU-side checks of the combiner bank (include/sxfir_bank_tx.h): the extension's symbols and bindings, the refusals of
sxfir_create_bank_interpolator and their order, the plan queries on NULL, the reference against an fp64 definition, the shipped code
object of the new kernels, and a numpy model of the tiled kernel's per-band index walk against mix_tx_cases.table_index."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from bank_tx_cases import band_refs, combiner_bound, combiner_f64, combiner_walk_model, sum_in_order
from gpu_util import random_taps_cx
from mix_tx_cases import step, table_index
from rational_cases import gaussian_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    names = _declared("sxfir_bank_tx.h")
    assert names == ["sxfir_bank_tx_abi_version", "sxfir_create_bank_interpolator", "sxfir_interpolate_bank", "sxfir_plan_bank_tx",
                     "sxfir_plan_bank_tx_band", "sxfir_time_interpolate_bank"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_bank_tx_abi_version() == 1 and prof.sxfir_bank_tx_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_bank_tx.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_BANK_TX_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    assert int(re.search(r"^#define\s+SXFIR_BANK_TX_MAX_BANDS\s+(\d+)", text, re.M).group(1)) == 16
    # the base ABI's number is the header's, untouched by the extension; so is the tuner bank's
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    assert lib.sxfir_abi_version() == int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 6
    assert lib.sxfir_bank_abi_version() == 1
    assert sxxcvr_amd.TranslatingCombiner.__mro__[1] is sxxcvr_amd.resampler._Plan and "TranslatingCombiner" in sxxcvr_amd.__all__
    # the header is installed with the others
    assert "include/sxfir_bank_tx.h" in open(os.path.join(ROOT, "CMakeLists.txt")).read()


def test_refusals_and_their_order_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    create = lib.sxfir_create_bank_interpolator
    taps = np.ones(2 * 128 * 16, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    ints = lambda *v: (C.c_int * len(v))(*v)
    num, den = ints(*range(16)), ints(*([7] * 16))
    plan = C.c_void_p()
    CF32, CF16, S32 = 0, 1, 2
    assert create(None, tp, 128, 4, 2, num, den, 1, CF32, -1) == EINVAL and b"NULL" in lib.sxfir_last_error()
    # (taps, ntaps, ratio, nbands, num, den, nchan, fmt) -> code and a word of the message, in the order the header fixes
    cases = [((None, 128, 4, 2, num, den, 1, CF32), EINVAL, b"NULL"),
             ((tp, 128, 4, 2, None, den, 1, CF32), EINVAL, b"NULL"),
             ((tp, 128, 4, 2, num, None, 1, CF32), EINVAL, b"NULL"),
             ((tp, 0, 4, 2, num, den, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 65537, 4, 2, num, den, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 128, 0, 2, num, den, 1, CF32), EINVAL, b"ratio"),
             ((tp, 128, 4097, 2, num, den, 1, CF32), EINVAL, b"ratio"),
             ((tp, 128, 4, 2, num, den, 0, CF32), EINVAL, b"nchan"),
             ((tp, 128, 4, 2, num, den, 1, 9), EINVAL, b"format"),
             ((tp, 130, 4, 2, num, den, 1, CF32), EINVAL, b"ntaps % ratio"),           # as the translating interpolator's creator
             ((tp, 128, 4, 0, num, den, 1, CF32), EINVAL, b"nbands 0 out of range"),
             ((tp, 128, 4, -1, num, den, 1, CF16), EINVAL, b"nbands -1 out of range"),
             ((tp, 128, 4, 17, num, den, 1, S32), EINVAL, b"nbands 17 out of range"),
             ((tp, 128, 4, 3, num, ints(7, 0, 65537), 1, CF32), EINVAL, b"band 1: den 0 out of range"),
             ((tp, 128, 4, 3, num, ints(7, 8, 65537), 1, S32), EINVAL, b"band 2: den 65537 out of range"),
             ((tp, 128, 4, 1, num, ints(-7), 1, CF16), EINVAL, b"band 0: den -7 out of range"),
             ((tp, 128, 4, 2, num, ints(7, 8, 0), 1, CF16), None, b""),          # (a bad den behind the last band is not looked at)
             # two bad arguments at once: the earlier check answers
             ((None, 0, 4, 2, None, den, 1, CF32), EINVAL, b"NULL"),
             ((tp, 0, 0, 0, num, ints(0), 1, CF32), EINVAL, b"ntaps"),
             ((tp, 128, 0, 0, num, ints(0), 0, CF32), EINVAL, b"ratio"),
             ((tp, 128, 4, 0, num, ints(0), 0, 9), EINVAL, b"nchan"),
             ((tp, 130, 4, 0, num, ints(0), 1, 9), EINVAL, b"format"),
             ((tp, 130, 4, 0, num, ints(0), 1, CF32), EINVAL, b"ntaps % ratio"),
             ((tp, 128, 4, 0, num, ints(0), 1, CF32), EINVAL, b"nbands"),
             ((tp, 128, 4, 17, num, ints(0), 1, CF32), EINVAL, b"nbands")]
    count = C.c_int(-1)
    lib.sxfir_device_count(C.byref(count))
    for args, code, word in cases:
        if code is None:
            if count.value > 0:
                continue            # (with a GPU the valid call succeeds: tests/test_gpu_bank_tx.py)
            code, word = ENODEVICE, b"no HIP device"
        plan.value = 0xDEAD
        assert create(C.byref(plan), *args, -1) == code, args
        assert word in lib.sxfir_last_error(), (args, lib.sxfir_last_error())
        assert not plan.value, args
    if count.value > 0:
        return
    # no GPU: refused as the translating create refuses, never computed on the host
    for fmt in (CF32, CF16, S32):
        assert create(C.byref(plan), tp, 128, 4, 16, num, den, 1, fmt, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.TranslatingCombiner(np.stack([random_taps_cx(128, 3), random_taps_cx(128, 4)]), 4, [(3, 7), (1, 4)])
    assert ei.value.code == ENODEVICE
    with pytest.raises(ValueError):
        sxxcvr_amd.TranslatingCombiner(random_taps_cx(128, 3), 4, [(3, 7)])          # taps are [K, ntaps]


def test_queries_and_entry_points_on_null():
    lib = sxxcvr_amd.load_sxfir()
    a, b = C.c_int(-1), C.c_int(-1)
    got, ms = C.c_size_t(77), C.c_float(-1.0)
    assert lib.sxfir_plan_bank_tx(None, C.byref(a)) == EINVAL and b"NULL" in lib.sxfir_last_error()
    assert lib.sxfir_plan_bank_tx_band(None, 0, C.byref(a), C.byref(b)) == EINVAL and b"NULL" in lib.sxfir_last_error()
    assert (a.value, b.value) == (-1, -1)
    assert lib.sxfir_interpolate_bank(None, None, 0, 0, 0, None, 0, C.byref(got), None) == EINVAL and got.value == 0
    assert lib.sxfir_interpolate_bank(None, None, 0, 0, 0, None, 0, None, None) == EINVAL
    assert lib.sxfir_time_interpolate_bank(None, None, 0, 0, 0, None, 0, 1, None, C.byref(ms)) == EINVAL and ms.value == -1.0


# what DESIGN.md 5.16 states of interp4_bank_kernel
DESIGN_VGPR, DESIGN_SGPR, DESIGN_LDS = 204, 106, 15360


def test_shipped_code_object_of_the_combiner_kernels():
    """Counts and metadata of the shipped code object: no scratch memory, the figures DESIGN.md 5.16 states, ONE band's arithmetic
    inside a runtime band loop, eight waves per CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    tiled = [r for r in rows if r["name"].endswith("interp4_bank_kernel")]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0 and t["s_barrier"] == 0, t
    assert (t["vgpr"], t["sgpr"], t["lds_bytes"]) == (DESIGN_VGPR, DESIGN_SGPR, DESIGN_LDS), t
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("**5.16 "):design.index("## 6. Oracle")]
    for word in ("%d VGPRs" % DESIGN_VGPR, "%d SGPRs" % DESIGN_SGPR, "%d B of LDS" % DESIGN_LDS):
        assert word in sec, word
    # two waves per SIMD at up to 256 VGPRs, and LDS for more than those eight waves per CU
    assert t["vgpr"] <= 256 and 8 * t["lds_bytes"] <= 160 * 1024, t
    # 2 tables x 2 row halves x 256 packed FMAs with a scalar tap: the band loop is a runtime loop, not unrolled
    assert t["v_pk_fma_f32"] == 1024, t
    assert 0 < t["global_load_lds_dwordx4_nt"] < t["global_load_lds_dwordx4"]                # the frame's staging policy
    generic = sorted(r["name"] for r in rows if r["name"].startswith("interp_bank_generic_kernel<"))
    assert generic == ["interp_bank_generic_kernel<sxfir::CF16, sxfir::CF16>", "interp_bank_generic_kernel<sxfir::CF32, sxfir::CF32>",
                       "interp_bank_generic_kernel<sxfir::CF32, sxfir::S32>"], generic
    for r in rows:
        if r["name"] in generic:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r


@pytest.mark.parametrize("K,ntaps,L,m_first", [(1, 128, 4, 0), (2, 128, 4, (1 << 40) + 21), (3, 35, 5, (1 << 40) - 3), (16, 128, 4, (1 << 40) + 77)])
def test_reference_against_the_fp64_definition(oracle, K, ntaps, L, m_first):
    """The float reference (K oracle passes, float32 adds in band order) against the fp64 definition, which uses neither the table nor
    the float reference, at positions near 2^40.  Per component: sum_k bound_k + (K - 1) 2^-24 sum_k (|y_k| + bound_k)."""
    dens = [7, 1000, 65536, 4, 1, 65535, 3, 12345, 9, 64, 100, 4093, 17, 255, 1024, 5]
    centres = [((3 + 11 * k) % dens[k], dens[k]) for k in range(K)]
    hs = [random_taps_cx(ntaps, 40 + k) for k in range(K)]
    n = 300
    xs = np.stack([gaussian_stream(n, 50 + k) for k in range(K)])
    jsplit = 2 if (ntaps // L) % 2 == 0 else 1
    ys = band_refs(oracle, hs, L, xs, jsplit, centres, m_first)
    got = sum_in_order(ys).astype(np.complex128)
    want = combiner_f64(hs, L, xs, centres, m_first)
    b = combiner_bound(hs, xs, ys)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    frac = float((err / b).max())
    print("K = %d, x%d x %d from %d: worst error %.3g, worst fraction of the bound %.3g" % (K, L, ntaps, m_first, err.max(), frac))
    assert frac <= 1.0
    if K > 1:       # the far phase matters: the same streams from position 0 give other outputs
        near = sum_in_order(band_refs(oracle, hs, L, xs, jsplit, centres, 0))
        assert np.count_nonzero(near != got.astype(np.complex64)) > got.size // 2


def test_sum_order_is_the_definitions():
    """Three values whose float32 sum depends on the order: the helper adds in band order, from the first band's value."""
    ys = [np.array([2.0 ** 24 + 0j], dtype=np.complex64), np.array([1.0 + 0j], dtype=np.complex64), np.array([-2.0 ** 24 + 0j], dtype=np.complex64)]
    assert sum_in_order(ys)[0] == 0.0 and sum_in_order(ys, [0, 2, 1])[0] == 1.0 and sum_in_order(ys, [1, 2, 0])[0] == 1.0
    # K = 1 adds nothing: a negative zero stays
    z = np.array([complex(-0.0, 0.0)], dtype=np.complex64)
    assert np.array_equal(sum_in_order([z]).view(np.uint32), z.view(np.uint32))


WALK = [[(3, 7), (123, 1000), (12345, 65536), (1, 4)],
        [(0, 1), (5, 7), (999, 1000), (16384, 65535), (49152, 65536)],          # den 1; the largest t on 65535 (s = 1) and 65536 (s = 0 .. )
        [(65534, 65535), (65535, 65536), (1, 3), (16384, 65535), (249, 1000), (2, 7), (0, 1), (1, 65536)]]


@pytest.mark.parametrize("centres", WALK)
def test_the_band_walk_stays_in_32_bits_and_hits_the_table_index(centres):
    """bank_tx_bands' steps and interp4_bank_kernel's per-band walk, modelled step by step (bank_tx_cases.combiner_walk_model), against
    mix_tx_cases.table_index for every band: grids of 1, 3, 8 and 24 waves -- smaller than the tile count --, XCD-blocked and plainly
    strided, over 3 waves + 3 tiles, so that every wave walks to a third tile and three to a fourth, from a first input at 0, at 5
    (the halo's indices reduced from below 0), at den - 1 and near 2^40.  Dens 1, 7, 1000, 65535 and 65536, the largest t among them
    ((16384, 65535): s = 1, t = 65534; (1, 65536): s = 4, t = 65532).  No intermediate value leaves 32 bits, no index reaches den."""
    assert step(16384, 65535, 4) == 1 and step(1, 65536, 4) == 4
    worst = 0
    for n_groups in (1, 3, 8, 24):
        n_tiles = 3 * n_groups + 3
        for consumed in (0, 5, 65535, (1 << 40) + 21):
            got, top = combiner_walk_model(centres, n_groups, n_tiles, consumed)
            worst = max(worst, top)
            for k, (num, den) in enumerate(centres):
                s = step(num, den, 4)
                want = np.stack([table_index(consumed + 256 * tile - 32, 288, s, den) for tile in range(n_tiles)])
                bad = np.nonzero((got[k] != want).any(axis=1))[0]
                assert bad.size == 0, "band %d (%d/%d), %d waves, from %d: tile %d" % (k, num, den, n_groups, consumed, bad[0])
    print("largest intermediate value: %d (2^32 = %d)" % (worst, 2 ** 32))
    assert worst < 2 ** 32 and 65535 * 65535 < 2 ** 32
