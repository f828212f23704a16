"""CPU-side checks of the 2x oversampled 4-band synthesizer (include/sxfir_synthesizer_os.h): the extension's symbols and
bindings, the argument checks of sxfir_create_synthesizer_os that need no GPU, the shipped code object of the two new kernel
families, the definition in fp64 numpy against the direct sum over the bands and against the two-pass route it replaces, and the
fp64 figures the property tests of tests/test_gpu_synthesizer_os.py lean on."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_lowpass
import test_channelizer_host as chan_host                  # channelize_fp64
import test_channelizer_os_host as chan_os_host            # channelize_os_fp64, edge_tone, _declared, _version
import test_synthesizer_host as syn_host                   # synth_fp64, butterflies_fp64, band_tone, tone_and_rest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5

OUTPUTS_PER_LANE = 16                                       # synthesis4x2_kernel, the 512-input tile: a lane's 8 inputs x 2

# The fp64 figures of the GPU property tests (dB re the tone's amplitude), as test_fp64_figures_of_the_gpu_property_tests
# below derives them with the library's own designer.
BAND_TONE_N, BAND_TONE_DROP, BAND_TONE_KEEP, BAND_TONE_BIN, BAND_TONE_DB = 1 << 15, 256, 65000, 19500, 0.00024
LOOP_DROP, LOOP_KEEP, LOOP_BIN, LOOP_TONE_DB = 536, 64000, 7200, -0.58733
CRIT_IMAGE_BIN, CRIT_IMAGE_DB = 55200, -29.9               # the critically sampled pair's image: 0.8625 cycles per sample


def test_extension_symbols_are_exported_and_bound():
    names = chan_os_host._declared("sxfir_synthesizer_os.h")
    assert names == ["sxfir_create_synthesizer_os", "sxfir_plan_synthesis_oversampling", "sxfir_synthesizer_os_abi_version"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_synthesizer_os_abi_version() == 1 and prof.sxfir_synthesizer_os_abi_version() == 1
    assert chan_os_host._version("sxfir_synthesizer_os.h", "SXFIR_SYNTHESIZER_OS_ABI_VERSION") == 1
    # the ABIs it stands on are untouched
    assert chan_os_host._version("sxfir.h", "SXFIR_ABI_VERSION") == 6 and lib.sxfir_abi_version() == 6
    assert chan_os_host._version("sxfir_synthesizer.h", "SXFIR_SYNTHESIZER_ABI_VERSION") == 1 and lib.sxfir_synthesizer_abi_version() == 1
    assert chan_os_host._version("sxfir_channelizer.h", "SXFIR_CHANNELIZER_ABI_VERSION") == 1 and lib.sxfir_channelizer_abi_version() == 1
    assert chan_os_host._version("sxfir_channelizer_os.h", "SXFIR_CHANNELIZER_OS_ABI_VERSION") == 1 and lib.sxfir_channelizer_os_abi_version() == 1
    assert chan_os_host._declared("sxfir_synthesizer.h") == ["sxfir_create_synthesizer", "sxfir_plan_synthesis_bands", "sxfir_synthesize",
                                                             "sxfir_synthesizer_abi_version"]
    assert chan_os_host._declared("sxfir_channelizer.h") == ["sxfir_channelize", "sxfir_channelizer_abi_version", "sxfir_create_channelizer",
                                                             "sxfir_plan_bands"]
    assert chan_os_host._declared("sxfir_channelizer_os.h") == ["sxfir_channelizer_os_abi_version", "sxfir_create_channelizer_os",
                                                                "sxfir_plan_oversampling"]
    assert chan_os_host._declared("sxfir_complex.h") == ["sxfir_complex_abi_version", "sxfir_create_complex", "sxfir_design_bandpass",
                                                         "sxfir_taps_are_complex"]
    assert list(inspect.signature(sxxcvr_amd.Synthesizer.__init__).parameters)[-1] == "oversample"
    assert isinstance(sxxcvr_amd.Synthesizer.oversampling, property)


def test_create_argument_errors_need_no_gpu():
    """Every row of the header's table, with device = -1: arguments are checked before the device is looked at."""
    lib = sxxcvr_amd.load_sxfir()
    taps = np.ones(256, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    create = lib.sxfir_create_synthesizer_os
    err = lambda: lib.sxfir_last_error().decode()
    # any other positive nbands / oversample: unsupported, with a message
    for nbands in (8, 2, 1, 16):
        assert create(C.byref(plan), tp, 128, nbands, 2, 1, 0, -1) == EUNSUPPORTED, nbands
        assert "4 bands only" in err()
    for oversample in (3, 4, 8):
        assert create(C.byref(plan), tp, 128, 4, oversample, 1, 0, -1) == EUNSUPPORTED, oversample
        assert "oversample 2 only" in err()
    assert create(C.byref(plan), tp, 128, 4, 1, 1, 0, -1) == EUNSUPPORTED
    assert "sxfir_create_synthesizer" in err() and "sxfir_create_synthesizer_os" not in err()
    # invalid
    assert create(None, tp, 128, 4, 2, 1, 0, -1) == EINVAL
    assert create(C.byref(plan), None, 128, 4, 2, 1, 0, -1) == EINVAL              # NULL taps
    assert create(C.byref(plan), tp, 128, 0, 2, 1, 0, -1) == EINVAL
    assert create(C.byref(plan), tp, 128, -4, 2, 1, 0, -1) == EINVAL
    assert create(C.byref(plan), tp, 128, 4, 0, 1, 0, -1) == EINVAL
    assert create(C.byref(plan), tp, 128, 4, -2, 1, 0, -1) == EINVAL
    assert create(C.byref(plan), tp, 0, 4, 2, 1, 0, -1) == EINVAL
    assert create(C.byref(plan), tp, -128, 4, 2, 1, 0, -1) == EINVAL
    assert create(C.byref(plan), tp, 128, 4, 2, 0, 0, -1) == EINVAL
    assert create(C.byref(plan), tp, 130, 4, 2, 1, 0, -1) == EINVAL                # ntaps % nbands
    assert create(C.byref(plan), tp, 128, 4, 2, 1, 9, -1) == EINVAL                # unknown format
    assert not plan.value
    n = C.c_int(-1)
    assert lib.sxfir_plan_synthesis_oversampling(None, C.byref(n)) == EINVAL
    lib.sxfir_device_count(C.byref(n))
    if n.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_synthesizer_os.py)
    # no GPU: arguments first, the device afterwards -- refused, never computed on the host
    for fmt in (0, 1, 2):
        plan = C.c_void_p()
        assert create(C.byref(plan), tp, 128, 4, 2, 1, fmt, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Synthesizer(design_lowpass(128, 4, 8.0, 2.0), oversample=2)
    assert ei.value.code == ENODEVICE
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Synthesizer(design_lowpass(128, 4, 8.0, 2.0), oversample=3)
    assert ei.value.code == EUNSUPPORTED
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Synthesizer(design_lowpass(128, 4, 8.0, 2.0), nbands=8, oversample=2)
    assert ei.value.code == EUNSUPPORTED


def test_shipped_code_object_of_the_oversampled_synthesizer_kernels():
    """The targets of sxfir_synthesis4x2.hip.h, read off the code object inside libsxfir.so (DESIGN.md 5.9 quotes the same rows)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    tiled = [r for r in rows if r["name"].endswith("synthesis4x2_kernel")]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    # one real-tap x2 pass of arithmetic: 16 outputs per lane x 64 taps, every FMA with a scalar tap operand
    assert t["v_pk_fma_f32"] == t["scalar_tap_fmas"] == OUTPUTS_PER_LANE * 64 == 1024
    assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0 and t["s_barrier"] == 0
    assert t["vgpr"] <= 256 and t["lds_bytes"] == 4 * 288 * 16 + 8192                        # two waves per SIMD; 26 624 B: 6 waves per CU
    assert 0 < t["global_load_lds_dwordx4_nt"] < t["global_load_lds_dwordx4"]                # the interior instructions alone
    generic = sorted(r["name"] for r in rows if r["name"].startswith("synthesis_os_generic_kernel<"))
    assert generic == ["synthesis_os_generic_kernel<sxfir::CF16, sxfir::CF16>", "synthesis_os_generic_kernel<sxfir::CF32, sxfir::CF32>",
                       "synthesis_os_generic_kernel<sxfir::CF32, sxfir::S32>"], generic
    for r in rows:
        if "synthesis_os_generic_kernel" in r["name"]:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r
    # the critically sampled synthesizer's rows are still there
    assert len([r for r in rows if r["name"].endswith("synthesis4_kernel")]) == 1
    assert len([r for r in rows if r["name"].startswith("synthesis_generic_kernel<")]) == 3


def synth_os_fp64(h, x, m0=0):
    """The header's formula in fp64: w[n] = sum_i h[2i + (n & 1)] v_(n & 3)[(n >> 1) - i] (x[<0] = 0), n the absolute output index
    of a stream whose first input has the per-band index m0.  x: [4, n_in]; returns [2 n_in]."""
    h = np.asarray(h, dtype=np.float64)
    v = syn_host.butterflies_fp64(x)
    n_in = v.shape[1]
    n = np.arange(2 * n_in)
    w = np.empty(2 * n_in, dtype=np.complex128)
    for r in range(4):
        y = np.empty(2 * n_in, dtype=np.complex128)          # the x2 interpolation of v_r
        y[0::2] = np.convolve(v[r], h[0::2])[:n_in]
        y[1::2] = np.convolve(v[r], h[1::2])[:n_in]
        pick = ((n + 2 * m0) & 3) == r
        w[pick] = y[pick]
    return w


def test_definition_against_the_direct_sum_and_the_two_pass_route():
    h = design_lowpass(128, 4, 8.0, 2.0).astype(np.float64)
    rng = np.random.default_rng(12)
    n_in = 300
    x = rng.standard_normal((4, n_in)) + 1j * rng.standard_normal((4, n_in))
    w = synth_os_fp64(h, x)
    # (1) every band zero-stuffed by 2, convolved with h, turned by exact quarter turns j^(k n): band k lands at k/4
    n = np.arange(2 * n_in)
    quarter = np.array([1, 1j, -1, -1j])
    want = np.zeros(2 * n_in, dtype=np.complex128)
    for k in range(4):
        z = np.zeros(2 * n_in, dtype=np.complex128)
        z[::2] = x[k]
        want += quarter[(k * n) % 4] * np.convolve(z, h)[:2 * n_in]
    err = np.abs(w - want).max()
    print("direct sum: max error %.3g" % err)
    assert err <= 1e-12
    # (2) the route it replaces: even and odd times apart, bands 1 and 3 of the odd half negated, two critically sampled passes
    # with the same taps, the odd half's result two samples late
    xe, xo = x[:, 0::2], x[:, 1::2] * np.array([1.0, -1.0, 1.0, -1.0])[:, None]
    a, b = syn_host.synth_fp64(h, xe), syn_host.synth_fp64(h, xo)
    two_pass = a + np.concatenate([np.zeros(2), b[:-2]])
    err = np.abs(w - two_pass).max()
    print("two-pass route: max error %.3g" % err)
    assert err <= 1e-12
    # a stream that starts at an odd per-band index reads the other pair of images
    wo = synth_os_fp64(h, x, m0=1)
    full = synth_os_fp64(h, np.concatenate([np.zeros((4, 1)), x], axis=1))
    assert np.abs(wo - full[2:]).max() <= 1e-12


def place_band_fp64(h2):
    """Property (a): band 1 alone, a tone 1/10 cycle per band sample."""
    return synth_os_fp64(h2, syn_host.band_tone(BAND_TONE_N))[BAND_TONE_DROP:BAND_TONE_DROP + BAND_TONE_KEEP]


def test_fp64_figures_of_the_gpu_property_tests():
    """The fp64 figures tests/test_gpu_synthesizer_os.py::test_places_the_band and ::test_band_edge_loopback lean on, with the
    library's own designer (measured with the oracle's design formula: (a) tone +0.00024 dB, rest -119.6 dB; (b) tone -0.58733 dB,
    rest -112.7 dB, the critically sampled pair's image -29.9 dB at 0.8625).  Margins: the tones to 0.001 dB, a tenth of what the
    GPU tests allow fp32; the rests 20 dB under the GPU tests' -80 dB; the image to the figure's last quoted digit."""
    h1 = design_lowpass(128, 4).astype(np.float64)
    h2 = design_lowpass(128, 4, 8.0, 2.0).astype(np.float64)
    h4 = design_lowpass(128, 4, 8.0, 4.0).astype(np.float64)
    # (a) band 1 alone: the tone lands at 1/4 + 0.1/2 = 0.3 cycles per output sample
    w = place_band_fp64(h2)
    assert w.size == BAND_TONE_KEEP and BAND_TONE_BIN == round(0.3 * BAND_TONE_KEEP)
    tone, rest, at = syn_host.tone_and_rest(w, BAND_TONE_BIN)
    print("(a) tone %.5f dB, rest %.1f dB at %.4f" % (tone, rest, at / w.size))
    assert abs(tone - BAND_TONE_DB) <= 0.001 and rest <= -100.0
    # (b) the band-edge tone through the oversampled pair: it comes back, and nothing else does
    x = chan_os_host.edge_tone()
    w = synth_os_fp64(h2, chan_os_host.channelize_os_fp64(h1, x))[LOOP_DROP:LOOP_DROP + LOOP_KEEP]
    assert w.size == LOOP_KEEP and LOOP_BIN == round(9 / 80 * LOOP_KEEP)
    tone, rest, at = syn_host.tone_and_rest(w, LOOP_BIN)
    print("(b) oversampled pair: tone %.5f dB, rest %.1f dB at %.4f" % (tone, rest, at / w.size))
    assert abs(tone - LOOP_TONE_DB) <= 0.001 and rest <= -100.0
    # ... and through the critically sampled pair: the same tone, and an image the neighbouring band's alias leaves
    wc = syn_host.synth_fp64(h4, chan_host.channelize_fp64(h1, x))[LOOP_DROP:LOOP_DROP + LOOP_KEEP]
    tone_c, rest_c, at_c = syn_host.tone_and_rest(wc, LOOP_BIN)
    image = syn_host.spectrum_db(wc)[CRIT_IMAGE_BIN]
    print("(b) critically sampled pair: tone %.5f dB, image at 0.8625 %.2f dB, largest other bin %.2f dB at %.4f" % (
        tone_c, image, rest_c, at_c / wc.size))
    assert abs(tone_c - LOOP_TONE_DB) <= 0.001
    # (band 0's image at 0.1125 - 1/4 and band 1's alias, put back at 1/4 + 0.1125, pass the same two transition bands: the two
    # bins are level to the last digit, and which of them is the larger is rounding's choice)
    assert CRIT_IMAGE_BIN == round(0.8625 * LOOP_KEEP) and at_c in (CRIT_IMAGE_BIN, round(0.3625 * LOOP_KEEP))
    assert abs(image - CRIT_IMAGE_DB) <= 0.05 and abs(rest_c - CRIT_IMAGE_DB) <= 0.05
