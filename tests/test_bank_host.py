"""CPU-side checks of the tuner bank (include/sxfir_bank.h): the extension's symbols and bindings, the refusals of sxfir_create_bank
and their order, the plan queries on NULL, the shipped code object of the two new kernels, and a numpy model of the tiled kernel's
per-band index walk against mix_cases.table_index."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from bank_cases import PAIRS, bank_reduce_model, bank_walk_model
from gpu_util import random_taps_cx
from mix_cases import step, table_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    names = _declared("sxfir_bank.h")
    assert names == ["sxfir_bank_abi_version", "sxfir_create_bank", "sxfir_decimate_bank", "sxfir_plan_bank", "sxfir_plan_bank_band",
                     "sxfir_time_decimate_bank"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_bank_abi_version() == 1 and prof.sxfir_bank_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_bank.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_BANK_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    assert int(re.search(r"^#define\s+SXFIR_BANK_MAX_BANDS\s+(\d+)", text, re.M).group(1)) == 16
    # the base ABI's number is the header's, untouched by the extension
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    assert lib.sxfir_abi_version() == int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 6
    assert sxxcvr_amd.TranslatingBank.__mro__[1] is sxxcvr_amd.resampler._Plan and "TranslatingBank" in sxxcvr_amd.__all__


def test_refusals_and_their_order_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    create = lib.sxfir_create_bank
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
             ((tp, 128, 4, 0, num, ints(0), 1, 9), EINVAL, b"format"),
             ((tp, 128, 4, 0, num, ints(0), 1, CF32), EINVAL, b"nbands"),
             ((tp, 128, 4, 17, num, ints(0), 1, CF32), EINVAL, b"nbands")]
    count = C.c_int(-1)
    lib.sxfir_device_count(C.byref(count))
    for args, code, word in cases:
        if code is None:
            if count.value > 0:
                continue            # (with a GPU the valid call succeeds: tests/test_gpu_bank.py)
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
        sxxcvr_amd.TranslatingBank(np.stack([random_taps_cx(128, 3), random_taps_cx(128, 4)]), 4, [(3, 7), (1, 4)])
    assert ei.value.code == ENODEVICE
    with pytest.raises(ValueError):
        sxxcvr_amd.TranslatingBank(random_taps_cx(128, 3), 4, [(3, 7)])          # taps are [K, ntaps]


def test_queries_and_entry_points_on_null():
    lib = sxxcvr_amd.load_sxfir()
    a, b = C.c_int(-1), C.c_int(-1)
    got, ms = C.c_size_t(77), C.c_float(-1.0)
    assert lib.sxfir_plan_bank(None, C.byref(a)) == EINVAL and b"NULL" in lib.sxfir_last_error()
    assert lib.sxfir_plan_bank_band(None, 0, C.byref(a), C.byref(b)) == EINVAL and b"NULL" in lib.sxfir_last_error()
    assert (a.value, b.value) == (-1, -1)
    assert lib.sxfir_decimate_bank(None, None, 0, 0, None, 0, 0, C.byref(got), None) == EINVAL and got.value == 0
    assert lib.sxfir_decimate_bank(None, None, 0, 0, None, 0, 0, None, None) == EINVAL
    assert lib.sxfir_time_decimate_bank(None, None, 0, 0, None, 0, 0, 1, None, C.byref(ms)) == EINVAL and ms.value == -1.0


def test_shipped_code_object_of_the_bank_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    tiled = [r for r in rows if r["name"].endswith("decim4_bank_kernel")]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    # the band loop is a runtime loop around ONE complex-tap tile's arithmetic: 2 chains x 8 outputs x 128 taps per lane, no more;
    # the image, the 1 KiB transposition scratch and sixteen phase words: 8 waves per CU, two per SIMD at up to 256 VGPRs
    assert t["v_pk_fma_f32"] == 2048, t
    assert t["lds_bytes"] == 18496 + 1024 + 64 and 8 * t["lds_bytes"] <= 160 * 1024 and t["vgpr"] <= 256, t
    assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0 and t["s_barrier"] == 0, t
    assert 0 < t["global_load_lds_dwordx4_nt"] < t["global_load_lds_dwordx4"]                # the wide kernel's staging policy, once per tile
    generic = sorted(r["name"] for r in rows if r["name"].startswith("decim_bank_generic_kernel<"))
    assert generic == ["decim_bank_generic_kernel<sxfir::CF16, sxfir::CF16>", "decim_bank_generic_kernel<sxfir::CF32, sxfir::CF32>",
                       "decim_bank_generic_kernel<sxfir::S32, sxfir::CF32>"], generic
    for r in rows:
        if r["name"] in generic:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r


@pytest.mark.parametrize("den", [1, 2, 3, 7, 1000, 4093, 65535, 65536])
def test_bank_reduce_is_the_modulo(den):
    """The kernel's division-free reduction over its whole domain's edges: every x < 64 den near a multiple of den, and a sweep."""
    edges = np.concatenate([np.arange(64, dtype=np.int64) * den + d for d in (0, 1, den - 1, den // 2)])
    edges = edges[(edges >= 0) & (edges < 64 * den)]
    sweep = np.arange(0, 64 * den, max(1, den // 97), dtype=np.int64)
    for x in (edges, sweep):
        assert np.array_equal(bank_reduce_model(x, den), x % den)


WALK = [PAIRS, [(3, 7), (65535, 65536), (1, 3)], [(65534, 65535), (123, 1000), (12345, 65536), (1, 4), (0, 1), (3, 7)]]


@pytest.mark.parametrize("centres", WALK)
def test_the_band_walk_stays_in_32_bits_and_hits_the_table_index(centres):
    """bank_bands' steps and decim4_bank_kernel's per-band walk, modelled step by step (bank_cases.bank_walk_model), against
    mix_cases.table_index for every band: grids of 1, 3, 8 and 24 waves -- smaller than the tile count --, XCD-blocked (w8 = waves / 8)
    and plainly strided, over 3 waves + 3 tiles, so that every wave walks to a third tile and three to a fourth, from a first output
    at 0, at den - 1 and near 2^40.  No intermediate value leaves 32 bits, no index reaches den."""
    worst = 0
    for n_waves in (1, 3, 8, 24):
        for w8 in sorted({0, n_waves // 8 if n_waves % 8 == 0 else 0}):
            n_tiles = 3 * n_waves + 3
            for m_first in (0, 65535, (1 << 40) + 77):
                got, top = bank_walk_model(centres, n_waves, w8, n_tiles, m_first)
                worst = max(worst, top)
                for k, (num, den) in enumerate(centres):
                    want = table_index(m_first, 512 * n_tiles, step(num, den, 4), den).reshape(n_tiles, 512)
                    bad = np.nonzero((got[k] != want).any(axis=1))[0]
                    assert bad.size == 0, "band %d (%d/%d), %d waves, w8 %d, from %d: tile %d" % (k, num, den, n_waves, w8, m_first, bad[0])
    print("largest intermediate value: %d (2^32 = %d)" % (worst, 2 ** 32))
    assert worst < 2 ** 32 and 65535 * 65535 < 2 ** 32 and 64 * 65536 <= 2 ** 22
