"""CPU-side checks of the frequency-translating interpolators (include/sxfir_translate_tx.h): the extension's symbols and bindings,
the refusals of sxfir_create_translating_interpolator that need no GPU, the float32 reference of tests/mix_tx_cases.py against the
fp64 definition, where a designed filter places the band, the tiled kernel's index walk, and the shipped code object of the new
kernels."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_bandpass
from gpu_util import random_taps_cx
from mix_tx_cases import back_step, bound, mix_tx_f64, mix_tx_ref, step, table_index, tile_walk_model
from rational_cases import gaussian_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5
NAMES = ["sxfir_create_translating_interpolator", "sxfir_plan_translation_tx", "sxfir_translate_tx_abi_version"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    assert _declared("sxfir_translate_tx.h") == NAMES
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in NAMES:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_translate_tx_abi_version() == 1 and prof.sxfir_translate_tx_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_translate_tx.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_TRANSLATE_TX_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    # the base ABI's number is the header's, the extensions this one stands on keep theirs
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    assert lib.sxfir_abi_version() == int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 6
    assert lib.sxfir_translate_abi_version() == 1 and lib.sxfir_complex_tx_abi_version() == 1
    assert sxxcvr_amd.TranslatingInterpolator.__mro__[1] is sxxcvr_amd.Resampler
    assert "TranslatingInterpolator" in sxxcvr_amd.__all__


def test_refusals_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    create = lib.sxfir_create_translating_interpolator
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
             ((tp, 127, 4, 3, 7, 1, CF32), EINVAL, b"ntaps % ratio"),          # as sxfir_create_complex_interpolator refuses it
             ((tp, 128, 4, 3, 0, 1, CF32), EINVAL, b"den 0 out of range"),
             ((tp, 128, 4, 3, -7, 1, S32), EINVAL, b"den -7 out of range"),
             ((tp, 128, 4, 3, 65537, 1, CF16), EINVAL, b"den 65537 out of range"),
             # two bad arguments at once: the earlier check answers
             ((tp, 0, 0, 3, 0, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 128, 0, 3, 0, 0, CF32), EINVAL, b"ratio"),
             ((tp, 128, 4, 3, 0, 0, 9), EINVAL, b"nchan"),
             ((tp, 128, 4, 3, 0, 1, 9), EINVAL, b"format"),
             ((tp, 127, 4, 3, 0, 1, CF32), EINVAL, b"ntaps % ratio")]
    for args, code, word in cases:
        plan.value = 0xDEAD if args[0] is not None else None
        assert create(C.byref(plan), *args, -1) == code, args
        assert word in lib.sxfir_last_error(), (args, lib.sxfir_last_error())
        assert not plan.value, args
    n, d = C.c_int(-1), C.c_int(-1)
    assert lib.sxfir_plan_translation_tx(None, C.byref(n), C.byref(d)) == EINVAL
    count = C.c_int(-1)
    lib.sxfir_device_count(C.byref(count))
    if count.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_mix_tx.py)
    # no GPU: refused as the complex-tap create refuses, never computed on the host
    for fmt in (CF32, CF16, S32):
        assert create(C.byref(plan), tp, 128, 4, 3, 7, 1, fmt, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.TranslatingInterpolator(design_bandpass(128, 4, 3, 7, gain=4), 4, 3, 7)
    assert ei.value.code == ENODEVICE


PAIRS = [(7, 3), (1000, 123), (65536, 12345), (4, 1), (65535, 65534)]          # tests/test_mix_host.py's


@pytest.mark.parametrize("den,num", PAIRS)
def test_reference_against_fp64(oracle, den, num):
    """mix_tx_ref (the float32 rotation of the input, the oracle's two real-tap passes, the float32 combine) against the fp64
    definition from an absolute input index near 2^40, at x4 x 128 and at (35 taps, x5): per component within
    (BOUND (1 + 2^-20) + 8 2^-24) sum|h| max|x|."""
    worst = 0.0
    for ntaps, L, jsplit in ((128, 4, 2), (35, 5, 1)):
        h = random_taps_cx(ntaps, 9)
        x = gaussian_stream(2000 + 3, 31 + den)
        m_first = (1 << 40) + 12345
        idx = table_index(m_first, x.size, step(num, den, L), den)
        assert idx.tolist()[:3] == [(den - (m_first + i) * step(num, den, L) % den) % den for i in range(3)]    # (Python integers)
        assert idx.tolist()[:3] == [(m_first + i) * back_step(num, den, L) % den for i in range(3)]
        got = mix_tx_ref(oracle, h, L, x, jsplit, num, den, m_first).astype(np.complex128)
        want = mix_tx_f64(h, L, num, den, x, m_first)
        assert got.shape == want.shape == (L * x.size,)
        err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
        b = bound(h, x)
        worst = max(worst, err / b)
        assert err <= b, (ntaps, L, err, b)
    print("den %d num %d: worst error / bound %.4f" % (den, num, worst))


@pytest.mark.parametrize("L,num,den", [(4, 123, 1000), (8, 3, 7)])
def test_places_the_band(L, num, den):
    """In fp64 on the designed (fp32-rounded) taps: a base-band tone 0.1 cycles per input sample above 0 Hz comes out at
    num / den + 0.1 / L cycles per output sample at 0 dB within 0.01 dB, every other bin at least 90 dB down -- the criterion of
    tests/test_gpu_complex_interp.py::test_places_the_band."""
    ntaps = 32 * L
    h = design_bandpass(ntaps, L, num, den, gain=L)
    q = np.arange(1 << 14, dtype=np.int64)
    x = np.exp(2j * np.pi * (q % 10) / 10.0)
    y = mix_tx_f64(h, L, num, den, x)[ntaps:]
    period = 10 * L * den                                       # the tone's frequency is (10 L num + den) / (10 L den)
    m = y.size // period * period
    assert m > 0
    Y = np.abs(np.fft.fft(y[:m])) / m
    tone = (10 * L * num + den) * (m // period) % m
    wanted = 20 * np.log10(Y[tone])
    Y[tone] = 0.0
    other = 20 * np.log10(max(Y.max(), 1e-300))
    print("x%d centre %d/%d: wanted tone %.5f dB, worst other bin %.1f dB" % (L, num, den, wanted, other))
    assert abs(wanted) <= 0.01
    assert other <= -90.0


def test_the_tile_walk_arithmetic_stays_in_32_bits_and_hits_the_table_index():
    """The steps imix_tile_args hands interp_mix_pass_kernel and the kernel's walk, modelled step by step (tile_walk_model), against
    mix_tx_cases.table_index for every mixer of the sweep's menu at x4 and x8: grids of 1, 3, 8 and 512 waves over 3 waves + 3 tiles,
    so that every wave walks to a third tile and three to a fourth, from a stream position of 0 (the halo's negative indices), 5,
    den + 31 and near 2^40.  No intermediate value leaves 32 bits, no index reaches den."""
    import rate_cases as rc
    worst = 0
    for L, tile_in in ((4, 256), (8, 128)):
        for cls, den, num in rc.MIXERS + (("tile walk", 7, 3), ("tile walk", 3, 1)):
            num = rc.mixer_num(cls, den, num, L)
            s = step(num, den, L)
            for n_groups in (1, 3, 8, 512):
                n_tiles = 3 * n_groups + 3
                for consumed in (0, 5, den + 31, (1 << 40) + 77):
                    got, top = tile_walk_model(num, den, L, n_groups, n_tiles, consumed)
                    worst = max(worst, top)
                    # tile k's image: samples consumed + k tile_in - 32 .. consumed + (k + 1) tile_in - 1
                    want = np.stack([table_index(consumed + k * tile_in - 32, tile_in + 32, s, den) for k in range(n_tiles)])
                    bad = np.nonzero((got != want).any(axis=1))[0]
                    assert bad.size == 0, "x%d den %d num %d, %d waves, from %d: tile %d" % (L, den, num, n_groups, consumed, bad[0])
    print("largest intermediate value: %d (2^32 = %d)" % (worst, 2 ** 32))
    # the one product the grids above keep small, (tile mod den) tile_step of a wave's first tile, at its largest: den - 1 each
    assert worst < 2 ** 32 and 65535 * 65535 < 2 ** 32 and 63 * 65535 < 2 ** 32


RESIDENT = {4: 2048, 8: 3072}       # workgroups an MI355X holds of interp_mix_pass_kernel's two instances, as tests/test_gpu_mix_tx.py prints them
# (what, n_groups per channel, n_tiles per channel, (class or num, den), consumed) by the resident figure R: the grids of the
# tile-walk tests of tests/test_gpu_mix_tx.py -- 2 R + 3 tiles on one channel, groups + 4 tiles on each of three channels (x4: 682
# groups, no multiple of 8, plainly strided; x8: 1024, XCD-blocked), R + 3 tiles from a placed position
GPU_GRIDS = [("third tile", lambda R: (R, 2 * R + 3), mixer, 0) for mixer in ((3, 7), (1, 3), (65535, 65536), (65534, 65535))]
GPU_GRIDS += [("three channels", lambda R: (R // 3, R // 3 + 4), (123, 1000), 0)]
GPU_GRIDS += [("placed", lambda R: (R, R + 3), ("max", 65535), (1 << 40) + 21), ("placed", lambda R: (R, R + 3), ("one", 7), (1 << 40) + 21),
              ("placed below 0", lambda R: (R, R + 3), ("one", 65535), 5)]


@pytest.mark.parametrize("what,grid,mixer,consumed", GPU_GRIDS, ids=["%s-%s-%s" % (g[0], g[2][0], g[2][1]) for g in GPU_GRIDS])
@pytest.mark.parametrize("L", [4, 8])
def test_the_tile_walk_on_the_grids_the_gpu_tests_run(L, what, grid, mixer, consumed):
    """A second model of what the GPU tests compare with the oracle: tile_walk_model at their own grids, mixers and positions, EVERY
    index it returns against mix_tx_cases.table_index.  Every wave of the first grid takes a second tile and three a third
    (stride_step twice); from the placed positions the first tile's phase is (consumed - 32) t reduced in 64 bits, from position 5
    from below 0."""
    import rate_cases as rc
    tile_in = 256 if L == 4 else 128
    n_groups, n_tiles = grid(RESIDENT[L])
    num, den = mixer if isinstance(mixer[0], int) else (rc.mixer_num(mixer[0], mixer[1], None, L), mixer[1])
    assert n_groups < n_tiles and (what != "third tile" or n_tiles > 2 * n_groups)
    assert what != "three channels" or (n_groups, n_tiles, n_groups % 8) == {4: (682, 686, 2), 8: (1024, 1028, 0)}[L]
    got, top = tile_walk_model(num, den, L, n_groups, n_tiles, consumed)
    want = np.stack([table_index(consumed + k * tile_in - 32, tile_in + 32, step(num, den, L), den) for k in range(n_tiles)])
    assert got.shape == want.shape == (n_tiles, tile_in + 32)
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, "x%d %d/%d, %d waves, from %d: tile %d sample %d" % (L, num, den, n_groups, consumed, bad[0][0], bad[1][0] - 32)
    assert top < 2 ** 32 and 0 <= got.min() and got.max() < den
    if consumed == 5:
        assert table_index(5 - 32, 1, step(num, den, L), den)[0] == (-27 * back_step(num, den, L)) % den     # (Python's modulo: the mathematical one)


def test_shipped_code_object_of_the_translating_interpolators():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    # the mixer instances of the complex-tap interpolators' kernel (the launch geometry's interp_mix_pass_kernel)
    tiled = {r["name"]: r for r in rows if "interp_cx_pass_kernel" in r["name"] and r["name"].endswith(", sxfir::InterpMixTileArgs>")}
    assert sorted(tiled) == ["interp_cx_pass_kernel<2, 8, sxfir::InterpMixTileArgs>", "interp_cx_pass_kernel<4, 4, sxfir::InterpMixTileArgs>"], sorted(tiled)
    real = {r["name"]: r for r in rows if r["name"].startswith("interp8_pass_kernel<")}
    cx = {r["name"]: r for r in rows if r["name"].startswith("interp_cx_pass_kernel<")}
    for name, t in tiled.items():
        qi, ll = [int(v) for v in name.split("<")[1].split(",")[:2]]
        base = real["interp8_pass_kernel<%d, false, false, true, %d, %d, false>" % (qi, ll, ll)]
        print(t)
        assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0 and t["s_barrier"] == 0 and t["vgpr"] <= 256, t
        assert t["lds_bytes"] == cx["interp_cx_pass_kernel<%d, %d, sxfir::InterpTileArgs>" % (qi, ll)]["lds_bytes"], t
        # two chains per window read: twice the real pass instance's packed FMAs, every one with a scalar tap
        assert t["v_pk_fma_f32"] == 2 * base["v_pk_fma_f32"] and t["scalar_tap_fmas"] == t["v_pk_fma_f32"], t
        # the counted wait's premises, read off the disassembly as for interp_cx_pass_kernel: the hand-written wait is the first
        # vmcnt(N > 0) of the kernel and waits for 8; behind the loop's last DMA the code holds stores alone (the table reads sit in
        # front of the DMAs), exactly eight in the block that loops back; no atomic
        cw = t["counted_wait"]
        assert cw["n"] == 8 and cw["dma_loads"] >= 2 and cw["atomics_after_first_dma"] == 0, t
        assert cw["last_block_vmem"] == ["global_store_dwordx4"] * 8 and cw["non_store_vmem_after_last_dma"] == [], t
    generic = sorted(r["name"] for r in rows if r["name"].startswith("interp_mix_generic_kernel<"))
    assert generic == ["interp_mix_generic_kernel<sxfir::CF16, sxfir::CF16>", "interp_mix_generic_kernel<sxfir::CF32, sxfir::CF32>",
                       "interp_mix_generic_kernel<sxfir::CF32, sxfir::S32>"], generic
    for r in rows:
        if "interp_mix_generic_kernel" in r["name"]:
            assert r["scratch_bytes"] == 0, r
