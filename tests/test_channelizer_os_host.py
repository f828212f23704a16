"""CPU-side checks of the 2x oversampled 4-band channelizer (include/sxfir_channelizer_os.h): the extension's symbols and
bindings, the argument checks of sxfir_create_channelizer_os that need no GPU, the shipped code object of the two new kernel
families, the convention (which band comes out where, and what the odd times' rotated operands mean) in fp64 numpy, and the fp64
figures of the GPU test that shows the band-edge alias gone."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_lowpass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5

# the band-edge tone of tests/test_gpu_channelizer_os.py::test_it_removes_the_alias, in fp64 (dB re the tone's amplitude)
EDGE_TONE_BAND0_DB, EDGE_TONE_BAND1_DB = -0.29367, -29.56216
EDGE_TONE_BIN0, EDGE_TONE_BIN1, EDGE_TONE_M = 7344, 23664, 32640


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def _version(header, macro):
    text = open(os.path.join(ROOT, "include", header)).read()
    return int(re.search(r"^#define\s+%s\s+(\d+)" % macro, text, re.M).group(1))


def test_extension_symbols_are_exported_and_bound():
    names = _declared("sxfir_channelizer_os.h")
    assert names == ["sxfir_channelizer_os_abi_version", "sxfir_create_channelizer_os", "sxfir_plan_oversampling"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_channelizer_os_abi_version() == 1 and prof.sxfir_channelizer_os_abi_version() == 1
    assert _version("sxfir_channelizer_os.h", "SXFIR_CHANNELIZER_OS_ABI_VERSION") == 1
    # the ABIs it stands on are untouched
    assert _version("sxfir.h", "SXFIR_ABI_VERSION") == 6 and lib.sxfir_abi_version() == 6
    assert _version("sxfir_channelizer.h", "SXFIR_CHANNELIZER_ABI_VERSION") == 1 and lib.sxfir_channelizer_abi_version() == 1
    assert _version("sxfir_synthesizer.h", "SXFIR_SYNTHESIZER_ABI_VERSION") == 1 and lib.sxfir_synthesizer_abi_version() == 1
    assert _declared("sxfir_channelizer.h") == ["sxfir_channelize", "sxfir_channelizer_abi_version", "sxfir_create_channelizer",
                                                "sxfir_plan_bands"]
    assert _declared("sxfir_synthesizer.h") == ["sxfir_create_synthesizer", "sxfir_plan_synthesis_bands", "sxfir_synthesize",
                                                "sxfir_synthesizer_abi_version"]
    import inspect
    assert list(inspect.signature(sxxcvr_amd.Channelizer.__init__).parameters)[-1] == "oversample"
    assert isinstance(sxxcvr_amd.Channelizer.oversampling, property)


def test_create_argument_errors_need_no_gpu():
    """Every row of the header's table, with device = -1: arguments are checked before the device is looked at."""
    lib = sxxcvr_amd.load_sxfir()
    taps = np.ones(256, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    create = lib.sxfir_create_channelizer_os
    err = lambda: lib.sxfir_last_error().decode()
    # any other positive nbands / oversample: unsupported, with a message
    for nbands in (8, 2, 1, 16):
        assert create(C.byref(plan), tp, 128, nbands, 2, 1, 0, -1) == EUNSUPPORTED, nbands
        assert "4 bands only" in err()
    for oversample in (3, 4, 8):
        assert create(C.byref(plan), tp, 128, 4, oversample, 1, 0, -1) == EUNSUPPORTED, oversample
        assert "oversample 2 only" in err()
    assert create(C.byref(plan), tp, 128, 4, 1, 1, 0, -1) == EUNSUPPORTED
    assert "sxfir_create_channelizer" in err() and "sxfir_create_channelizer_os" not in err()
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
    assert lib.sxfir_plan_oversampling(None, C.byref(n)) == EINVAL
    lib.sxfir_device_count(C.byref(n))
    if n.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_channelizer_os.py)
    # no GPU: arguments first, the device afterwards -- refused, never computed on the host
    for fmt in (0, 1, 2):
        plan = C.c_void_p()
        assert create(C.byref(plan), tp, 128, 4, 2, 1, fmt, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Channelizer(design_lowpass(128, 4), oversample=2)
    assert ei.value.code == ENODEVICE
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Channelizer(design_lowpass(128, 4), oversample=3)
    assert ei.value.code == EUNSUPPORTED
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Channelizer(design_lowpass(128, 4), nbands=8, oversample=2)
    assert ei.value.code == EUNSUPPORTED


def test_shipped_code_object_of_the_oversampled_channelizer_kernels():
    """The targets of sxfir_chan4x2.hip.h, read off the code object inside libsxfir.so (DESIGN.md 5.8 quotes the same rows)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    tiled = [r for r in rows if r["name"].endswith("chan4x2_kernel")]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    # two real-tap passes of arithmetic: 16 outputs per lane x 128 taps, every FMA with a scalar tap operand
    assert t["v_pk_fma_f32"] == 2048 and t["scalar_tap_fmas"] == 2048
    assert t["scratch_bytes"] == 0 and t["s_barrier"] == 0 and t["v_mfma"] == 0
    assert 0 < t["global_load_lds_dwordx4_nt"] < t["global_load_lds_dwordx4"]                # the wide kernel's staging policy
    assert t["vgpr"] <= 256 and t["lds_bytes"] == 18496                                       # 8 waves per CU, two per SIMD
    generic = sorted(r["name"] for r in rows if "chan4x2_generic_kernel" in r["name"])
    assert generic == ["chan4x2_generic_kernel<sxfir::CF16, sxfir::CF16>", "chan4x2_generic_kernel<sxfir::CF32, sxfir::CF32>",
                       "chan4x2_generic_kernel<sxfir::S32, sxfir::CF32>"], generic
    for r in rows:
        if "chan4x2_generic_kernel" in r["name"]:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r


def channelize_os_fp64(h, x):
    """The header's formula in fp64: the four branch sums u_r[m] = sum_j h[4j + r] x[2m - 4j - r] (x[<0] = 0), then the radix-2
    butterflies of sxfir_channelizer.h on (u0, u1, u2, u3) for even m and on (u2, u3, u0, u1) for odd m.  Returns [4, ceil(len(x) / 2)]."""
    h = np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.complex128)
    n_out = (x.size + 1) // 2
    u = []
    for r in range(4):
        hr = np.zeros_like(h)
        hr[r::4] = h[r::4]
        u.append(np.convolve(x, hr)[:2 * n_out:2])
    odd = (np.arange(n_out) & 1) == 1
    a = [np.where(odd, u[(r + 2) % 4], u[r]) for r in range(4)]
    s0, s1, t0, t1 = a[0] + a[2], a[0] - a[2], a[1] + a[3], a[1] - a[3]
    y1 = (s1.real - t1.imag) + 1j * (s1.imag + t1.real)
    y3 = (s1.real + t1.imag) + 1j * (s1.imag - t1.real)
    return np.stack([s0 + t0, y1, s0 - t0, y3])


def test_convention_of_the_rotated_butterflies():
    """Band k of the butterflies with the odd times' operands shifted by two is (-1)^(k m) sum_n h[n] j^(k n) x[2m - n]: direct
    convolution with the band-pass that design_bandpass(128, 4, k, 4) centres, every second output, turned back to 0 Hz."""
    h = design_lowpass(128, 4).astype(np.float64)
    rng = np.random.default_rng(12)
    x = rng.standard_normal(2 * 601 + 1) + 1j * rng.standard_normal(2 * 601 + 1)
    y = channelize_os_fp64(h, x)
    assert y.shape == (4, 602)
    n = np.arange(128)
    m = np.arange(y.shape[1])
    quarter = np.array([1, 1j, -1, -1j])                       # exact quarter turns
    for k in range(4):
        hk = h * quarter[(n * k) % 4]
        want = np.convolve(x, hk)[:2 * y.shape[1]:2] * np.where((k * m) % 2 == 1, -1.0, 1.0)
        err = np.abs(y[k] - want).max()
        print("band %d: max error %.3g" % (k, err))
        assert err <= 1e-9
    # ... and the even times are the critically sampled channelizer's
    import test_channelizer_host as crit
    assert np.array_equal(y[:, 0::2][:, :x.size // 4], crit.channelize_fp64(h, x))


def edge_tone_spectra(y):
    """[4, m] dB spectra of the four bands after the first 128 outputs."""
    y = np.asarray(y)[:, 128:].astype(np.complex128)
    m = y.shape[1]
    assert m == EDGE_TONE_M
    return 20 * np.log10(np.maximum(np.abs(np.fft.fft(y, axis=1)) / m, 1e-300))


def edge_tone(n=1 << 16):
    """9/80 cycles per input sample, 0.0125 under the edge between bands 0 and 1 (phases reduced in integers)."""
    t = np.arange(n, dtype=np.int64)
    return np.exp(2j * np.pi * ((9 * t) % 80) / 80.0)


def test_fp64_figures_of_the_band_edge_tone():
    """The fp64 figures tests/test_gpu_channelizer_os.py::test_it_removes_the_alias leans on, with the library's own designer.  The
    tone leaves band 0 at -0.29 dB at +0.225 cycles per output sample and band 1 at -29.56 dB at -0.275: two different places, and
    nothing else anywhere -- where the critically sampled plan puts both at +0.45, an alias in band 1."""
    h = design_lowpass(128, 4).astype(np.float64)
    x = edge_tone()
    Y = edge_tone_spectra(channelize_os_fp64(h, x))
    assert EDGE_TONE_BIN0 == round(0.225 * EDGE_TONE_M) and EDGE_TONE_BIN1 == round((1 - 0.275) * EDGE_TONE_M)
    rest0, rest1 = np.delete(Y[0], EDGE_TONE_BIN0).max(), np.delete(Y[1], EDGE_TONE_BIN1).max()
    print("band 0 tone %.5f dB, band 1 tone %.5f dB; bands 2, 3 peak %.1f, %.1f dB; other bins of bands 0, 1 peak %.1f, %.1f dB" % (
        Y[0, EDGE_TONE_BIN0], Y[1, EDGE_TONE_BIN1], Y[2].max(), Y[3].max(), rest0, rest1))
    assert abs(Y[0, EDGE_TONE_BIN0] - EDGE_TONE_BAND0_DB) <= 0.001
    assert abs(Y[1, EDGE_TONE_BIN1] - EDGE_TONE_BAND1_DB) <= 0.001
    assert abs(Y[2].max() - -118.4) <= 0.1 and abs(Y[3].max() - -112.2) <= 0.1
    assert max(Y[2].max(), Y[3].max()) <= -100.0
    assert max(rest0, rest1) <= -200.0
    # the critically sampled plan on the same tone: both bands hold it in the SAME bin (+0.45 cycles per output sample)
    import test_channelizer_host as crit
    yc = crit.channelize_fp64(h, x)[:, 64:]
    Yc = 20 * np.log10(np.maximum(np.abs(np.fft.fft(yc, axis=1)) / yc.shape[1], 1e-300))
    b = round(0.45 * yc.shape[1])
    print("critically sampled: band 0 %.2f dB and band 1 %.2f dB, both in bin %d of %d" % (Yc[0, b], Yc[1, b], b, yc.shape[1]))
    assert int(np.argmax(Yc[0])) == b and int(np.argmax(Yc[1])) == b
