"""CPU-side checks of the 4-band synthesizer (include/sxfir_synthesizer.h): the extension's symbols and bindings, the argument
checks of sxfir_create_synthesizer that need no GPU, the shipped code object of the two new kernel families, the convention (which
band lands where) in fp64 numpy, and the fp64 figures the two property tests of tests/test_gpu_synthesizer.py lean on."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_lowpass
import test_channelizer_host as chan_host          # channelize_fp64, the channelizer header's symbol list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5


def test_extension_symbols_are_exported_and_bound():
    names = chan_host._declared("sxfir_synthesizer.h")
    assert names == ["sxfir_create_synthesizer", "sxfir_plan_synthesis_bands", "sxfir_synthesize", "sxfir_synthesizer_abi_version"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_synthesizer_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_synthesizer.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_SYNTHESIZER_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    # the base ABI's number and the channelizer's extension are untouched by this one
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    want = int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1))
    assert want == 6 and lib.sxfir_abi_version() == want
    assert chan_host._declared("sxfir_channelizer.h") == ["sxfir_channelize", "sxfir_channelizer_abi_version", "sxfir_create_channelizer",
                                                          "sxfir_plan_bands"]
    assert lib.sxfir_channelizer_abi_version() == 1
    assert sxxcvr_amd.Synthesizer is not None and "Synthesizer" in sxxcvr_amd.__all__


def test_create_synthesizer_argument_errors_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    taps = np.ones(256, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    assert lib.sxfir_create_synthesizer(None, tp, 128, 4, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_synthesizer(C.byref(plan), None, 128, 4, 1, 0, -1) == EINVAL           # NULL taps
    assert lib.sxfir_create_synthesizer(C.byref(plan), tp, 128, 8, 1, 0, -1) == EUNSUPPORTED        # 8 bands
    assert b"4 bands only" in lib.sxfir_last_error()
    assert lib.sxfir_create_synthesizer(C.byref(plan), tp, 128, 2, 1, 0, -1) == EUNSUPPORTED
    assert b"4 bands only" in lib.sxfir_last_error()
    assert lib.sxfir_create_synthesizer(C.byref(plan), tp, 130, 4, 1, 0, -1) == EINVAL              # ntaps % nbands
    assert lib.sxfir_create_synthesizer(C.byref(plan), tp, 0, 4, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_synthesizer(C.byref(plan), tp, 128, 0, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_synthesizer(C.byref(plan), tp, 128, 4, 0, 0, -1) == EINVAL
    assert lib.sxfir_create_synthesizer(C.byref(plan), tp, 128, 4, 1, 9, -1) == EINVAL
    assert not plan.value
    n = C.c_int(-1)
    assert lib.sxfir_plan_synthesis_bands(None, C.byref(n)) == EINVAL
    assert lib.sxfir_synthesize(None, None, 0, 0, 0, None, 0, None, None) == EINVAL
    lib.sxfir_device_count(C.byref(n))
    if n.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_synthesizer.py)
    # no GPU: arguments first, the device afterwards -- refused, never computed on the host
    plan = C.c_void_p()
    assert lib.sxfir_create_synthesizer(C.byref(plan), tp, 128, 4, 1, 0, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Synthesizer(design_lowpass(128, 4, 8.0, 4.0))
    assert ei.value.code == ENODEVICE
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Synthesizer(design_lowpass(128, 4, 8.0, 4.0), nbands=8)
    assert ei.value.code == EUNSUPPORTED


def test_shipped_code_object_of_the_synthesizer_kernels():
    """The targets of sxfir_synthesis4.hip.h, read off the code object inside libsxfir.so (DESIGN.md 5.7 quotes the same rows)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    tiled = [r for r in rows if r["name"].endswith("synthesis4_kernel")]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    # one real-tap x4 pass of arithmetic: 16 outputs per lane x 32 taps, every FMA with a scalar tap operand
    assert t["v_pk_fma_f32"] == 512 and t["scalar_tap_fmas"] == 512
    assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0 and t["s_barrier"] == 0
    generic = sorted(r["name"] for r in rows if r["name"].startswith("synthesis_generic_kernel<"))
    assert generic == ["synthesis_generic_kernel<sxfir::CF16, sxfir::CF16>", "synthesis_generic_kernel<sxfir::CF32, sxfir::CF32>",
                       "synthesis_generic_kernel<sxfir::CF32, sxfir::S32>"], generic
    for r in rows:
        if "synthesis_generic_kernel" in r["name"]:
            assert r["scratch_bytes"] == 0, r


def butterflies_fp64(x):
    """v_r = sum_k (j)^(k r) x_k by the header's radix-2 steps; x: [4, n]."""
    x = np.asarray(x, dtype=np.complex128)
    a0, a1, b0, b1 = x[0] + x[2], x[0] - x[2], x[1] + x[3], x[1] - x[3]
    v1 = (a1.real - b1.imag) + 1j * (a1.imag + b1.real)
    v3 = (a1.real + b1.imag) + 1j * (a1.imag - b1.real)
    return np.stack([a0 + b0, v1, a0 - b0, v3])


def synth_fp64(h, x):
    """The header's formula in fp64: w[4m + r] = sum_j h[4j + r] v_r[m - j] (x[<0] = 0).  x: [4, n]; returns [4 n]."""
    h = np.asarray(h, dtype=np.float64)
    v = butterflies_fp64(x)
    n = v.shape[1]
    w = np.empty(4 * n, dtype=np.complex128)
    for r in range(4):
        w[r::4] = np.convolve(v[r], h[r::4])[:n]
    return w


def spectrum_db(w):
    return 20 * np.log10(np.maximum(np.abs(np.fft.fft(w)) / w.size, 1e-300))


def tone_and_rest(w, tone_bin):
    """dB of the tone's bin and of the largest other bin."""
    W = spectrum_db(w)
    rest = np.delete(W, tone_bin)
    return W[tone_bin], rest.max(), int(np.argmax(np.where(np.arange(W.size) == tone_bin, -1e9, W)))


def band_tone(n=1 << 14):
    """Property (a)'s input: band 1 holds a tone 1/10 cycle per band sample (phases reduced in integers), the others nothing."""
    m = np.arange(n, dtype=np.int64)
    x = np.zeros((4, n), dtype=np.complex128)
    x[1] = np.exp(2j * np.pi * (m % 10) / 10.0)
    return x


def wideband_tone(n=1 << 16):
    """Property (b)'s input: 11/40 cycles per wideband sample."""
    k = np.arange(n, dtype=np.int64)
    return np.exp(2j * np.pi * ((k * 11) % 40) / 40.0)


def test_convention():
    """The butterflies and the phase-wise polyphase sum are the direct sum over k of the zero-stuffed band k convolved with
    h[n] (j)^(k n): band k lands at k/4 cycles per output sample."""
    h = design_lowpass(128, 4, 8.0, 4.0).astype(np.float64)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((4, 300)) + 1j * rng.standard_normal((4, 300))
    w = synth_fp64(h, x)
    n = np.arange(128)
    quarter = np.array([1, 1j, -1, -1j])                       # exact quarter turns
    want = np.zeros(4 * 300, dtype=np.complex128)
    for k in range(4):
        z = np.zeros(4 * 300, dtype=np.complex128)
        z[::4] = x[k]
        want += np.convolve(z, h * quarter[(n * k) % 4])[:4 * 300]
    err = np.abs(w - want).max()
    print("max error %.3g" % err)
    assert err <= 1e-12


def test_fp64_figures_of_the_gpu_property_tests():
    """The fp64 figures tests/test_gpu_synthesizer.py::test_places_the_band and ::test_loopback lean on, with the library's own designer
    (measured with the oracle's design formula: (a) tone +0.00024 dB, rest -104.8 dB, the image at 0.525; (b) +0.00047 dB, rest
    -103.5 dB)."""
    h1 = design_lowpass(128, 4).astype(np.float64)
    h4 = design_lowpass(128, 4, 8.0, 4.0).astype(np.float64)
    # (a) band 1 alone: the tone lands at 1/4 + 0.1/4 = 11/40 cycles per output sample
    w = synth_fp64(h4, band_tone())[256:]
    assert w.size == 65280
    tone, rest, at = tone_and_rest(w, 17952)
    print("(a) tone %.5f dB, rest %.1f dB at %.4f" % (tone, rest, at / w.size))
    assert abs(tone) <= 0.001 and rest <= -90.0
    # (b) channelizer, then synthesizer: the wideband tone comes back
    y = chan_host.channelize_fp64(h1, wideband_tone())
    w = synth_fp64(h4, y)[536:]
    assert w.size == 65000
    tone, rest, at = tone_and_rest(w, 17875)
    print("(b) tone %.5f dB, rest %.1f dB at %.4f" % (tone, rest, at / w.size))
    assert abs(tone) <= 0.002 and rest <= -90.0
