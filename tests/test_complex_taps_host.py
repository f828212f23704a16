"""CPU-side checks of the complex-tap (band-pass) decimators (include/sxfir_complex.h): the extension's symbols and bindings,
the band-pass designer against an fp64 restatement and its frequency response, the shipped code object of the two new kernel
families, and the argument checks of sxfir_create_complex that need no GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_bandpass, design_lowpass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    names = _declared("sxfir_complex.h")
    assert names == ["sxfir_complex_abi_version", "sxfir_create_complex", "sxfir_design_bandpass", "sxfir_taps_are_complex"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_complex_abi_version() == 1
    # the base ABI's number is the header's, untouched by the extension
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    assert lib.sxfir_abi_version() == int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1))


@pytest.mark.parametrize("n,d", [(128, 4), (256, 8), (1024, 32), (35, 5)])
def test_bandpass_at_zero_is_the_lowpass(n, d):
    h = design_bandpass(n, d, 0, 1)
    assert h.dtype == np.complex64 and h.shape == (n,)
    lp = design_lowpass(n, d)
    assert np.array_equal(h.real.view(np.uint32), lp.view(np.uint32))
    assert np.array_equal(h.imag.view(np.uint32), np.zeros(n, dtype=np.uint32))          # +0.0, never -0.0


def _restated(n, d, num, den, beta=8.0, gain=1.0):
    """fp64: sinc(2 (0.5/D)(k - (N-1)/2)) x kaiser(N, beta), normalised to the gain, times the integer-reduced phasor."""
    k = np.arange(n, dtype=np.float64)
    proto = np.sinc(2.0 * (0.5 / d) * (k - (n - 1) / 2.0)) * np.kaiser(n, beta)
    proto *= gain / proto.sum()
    r = (np.arange(n, dtype=np.int64) * num) % den
    return proto * np.exp(2j * np.pi * r.astype(np.float64) / den)


CASES = [(128, 4, 1, 4), (256, 8, 7, 8)]


@pytest.mark.parametrize("n,d,num,den", CASES)
def test_bandpass_against_fp64_restatement(n, d, num, den):
    h = design_bandpass(n, d, num, den).astype(np.complex128)
    want = _restated(n, d, num, den)
    # fp32 rounding is 2^-24 relative; the rest covers libm / i0 differences of a few fp64 ulps
    tol = 2.0 ** -22 * np.abs(want).max()
    err = max(np.abs(h.real - want.real).max(), np.abs(h.imag - want.imag).max())
    print("max component error %.3g, tolerance %.3g" % (err, tol))
    assert err <= tol


def _response_db(h, freqs):
    k = np.arange(h.size, dtype=np.float64)
    H = np.exp(-2j * np.pi * np.outer(freqs, k)) @ h.astype(np.complex128)
    return 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))


@pytest.mark.parametrize("n,d,num,den", CASES)
def test_bandpass_frequency_response(n, d, num, den):
    h = design_bandpass(n, d, num, den)
    centre = num / den
    off = np.linspace(-0.2 / d, 0.2 / d, 401)
    passband = _response_db(h, centre + off)
    ripple = np.abs(passband).max()                                # gain 1 = 0 dB
    worst = -np.inf
    for j in range(d):
        c = j / d
        if abs(((c - centre + 0.5) % 1.0) - 0.5) < 1e-12:
            continue
        worst = max(worst, _response_db(h, c + off).max())
    print("ripple %.3g dB, rejection %.1f dB" % (ripple, -worst))
    assert ripple <= 0.001
    assert -worst >= 90.0


def test_shipped_code_object_of_the_complex_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    # (the kernel's other instance, <sxfir::MixTileArgs>, is the translating decimators': tests/test_mix_host.py)
    tiled = [r for r in rows if r["name"] == "decim4_cx_kernel<sxfir::DecimTileArgs>"]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0
    # lane map (sxfir_decim_cx.hip.h): 8 outputs per lane x 128 taps x 2 chains (A = a (*) x, B = b (*) x) = 2048 packed FMAs per
    # tile of 512 outputs -- twice the 1024 of a real-tap tile of 512 outputs (decim4_wide_kernel)
    assert t["v_pk_fma_f32"] == 2 * 1024
    assert t.get("scalar_tap_fmas", 0) > 0 and t["global_load_lds_dwordx4_nt"] > 0
    assert t["s_barrier"] == 0 and t["lds_bytes"] == 18496 and t["vgpr"] <= 256            # 8 waves per CU, two per SIMD
    generic = sorted(r["name"] for r in rows if r["name"].startswith("decim_cx_generic_kernel<") and r["name"].endswith(", sxfir::GenericArgs>"))
    assert generic == ["decim_cx_generic_kernel<sxfir::CF16, sxfir::CF16, sxfir::GenericArgs>",
                       "decim_cx_generic_kernel<sxfir::CF32, sxfir::CF32, sxfir::GenericArgs>",
                       "decim_cx_generic_kernel<sxfir::S32, sxfir::CF32, sxfir::GenericArgs>"], generic
    for r in rows:
        if r["name"] in generic:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r


def test_create_complex_argument_errors_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    taps = np.ones(2 * 128, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5
    assert lib.sxfir_create_complex(None, 0, tp, 128, 4, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_complex(C.byref(plan), 0, None, 128, 4, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_complex(C.byref(plan), 7, tp, 128, 4, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_complex(C.byref(plan), 0, tp, 0, 4, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_complex(C.byref(plan), 0, tp, 128, 0, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_complex(C.byref(plan), 0, tp, 128, 4, 0, 1, -1) == EINVAL
    assert lib.sxfir_create_complex(C.byref(plan), 0, tp, 128, 4, 1, 9, -1) == EINVAL
    assert lib.sxfir_create_complex(C.byref(plan), 1, tp, 128, 4, 1, 0, -1) == EUNSUPPORTED
    assert b"decimators only" in lib.sxfir_last_error()
    assert not plan.value
    f = C.c_int(-1)
    assert lib.sxfir_taps_are_complex(None, C.byref(f)) == EINVAL
    assert lib.sxfir_design_bandpass(128, 4, 8.0, 1.0, 1, 0, tp) == EINVAL            # den >= 1
    n = C.c_int(-1)
    lib.sxfir_device_count(C.byref(n))
    if n.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_complex_taps.py)
    # no GPU: refused as the real-tap create refuses, never computed on the host
    assert lib.sxfir_create_complex(C.byref(plan), 0, tp, 128, 4, 1, 0, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Resampler(0, design_bandpass(128, 4, 1, 4), 4)
    assert ei.value.code == ENODEVICE
