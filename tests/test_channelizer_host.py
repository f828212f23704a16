"""CPU-side checks of the 4-band channelizer (include/sxfir_channelizer.h): the extension's symbols and bindings, the argument
checks of sxfir_create_channelizer that need no GPU, the shipped code object of the two new kernel families, and the butterfly
convention (which band comes out where) in fp64 numpy."""
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


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    names = _declared("sxfir_channelizer.h")
    assert names == ["sxfir_channelize", "sxfir_channelizer_abi_version", "sxfir_create_channelizer", "sxfir_plan_bands"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_channelizer_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_channelizer.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_CHANNELIZER_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    # the base ABI's number is the header's, untouched by the extension
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    want = int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1))
    assert want == 6 and lib.sxfir_abi_version() == want
    assert sxxcvr_amd.Channelizer is not None and "Channelizer" in sxxcvr_amd.__all__


def test_create_channelizer_argument_errors_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    taps = np.ones(256, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    assert lib.sxfir_create_channelizer(None, tp, 128, 4, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_channelizer(C.byref(plan), None, 128, 4, 1, 0, -1) == EINVAL           # NULL taps
    assert lib.sxfir_create_channelizer(C.byref(plan), tp, 128, 8, 1, 0, -1) == EUNSUPPORTED        # 8 bands
    assert b"4 bands only" in lib.sxfir_last_error()
    assert lib.sxfir_create_channelizer(C.byref(plan), tp, 128, 2, 1, 0, -1) == EUNSUPPORTED
    assert lib.sxfir_create_channelizer(C.byref(plan), tp, 130, 4, 1, 0, -1) == EINVAL              # ntaps % nbands
    assert lib.sxfir_create_channelizer(C.byref(plan), tp, 0, 4, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_channelizer(C.byref(plan), tp, 128, 0, 1, 0, -1) == EINVAL
    assert lib.sxfir_create_channelizer(C.byref(plan), tp, 128, 4, 0, 0, -1) == EINVAL
    assert lib.sxfir_create_channelizer(C.byref(plan), tp, 128, 4, 1, 9, -1) == EINVAL
    assert not plan.value
    n = C.c_int(-1)
    assert lib.sxfir_plan_bands(None, C.byref(n)) == EINVAL
    assert lib.sxfir_channelize(None, None, 0, 0, None, 0, 0, None, None) == EINVAL
    lib.sxfir_device_count(C.byref(n))
    if n.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_channelizer.py)
    # no GPU: arguments first, the device afterwards -- refused, never computed on the host
    plan = C.c_void_p()
    assert lib.sxfir_create_channelizer(C.byref(plan), tp, 128, 4, 1, 0, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Channelizer(design_lowpass(128, 4))
    assert ei.value.code == ENODEVICE
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Channelizer(design_lowpass(128, 4), nbands=8)
    assert ei.value.code == EUNSUPPORTED


def test_shipped_code_object_of_the_channelizer_kernels():
    """The targets of sxfir_chan4.hip.h, read off the code object inside libsxfir.so (DESIGN.md 5.6 quotes the same rows)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    tiled = [r for r in rows if r["name"].endswith("chan4_kernel")]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    # one real-tap pass of arithmetic: 8 outputs per lane x 128 taps, every FMA with a scalar tap operand
    assert t["v_pk_fma_f32"] == 1024 and t["scalar_tap_fmas"] == 1024
    assert t["vgpr"] <= 256 and t["lds_bytes"] == 18496 and t["scratch_bytes"] == 0          # 8 waves per CU, two per SIMD
    assert t["s_barrier"] == 0 and t["v_mfma"] == 0
    assert 0 < t["global_load_lds_dwordx4_nt"] < t["global_load_lds_dwordx4"]                # the wide kernel's staging policy
    generic = sorted(r["name"] for r in rows if r["name"].startswith("chan_generic_kernel<"))
    assert generic == ["chan_generic_kernel<sxfir::CF16, sxfir::CF16>", "chan_generic_kernel<sxfir::CF32, sxfir::CF32>",
                       "chan_generic_kernel<sxfir::S32, sxfir::CF32>"], generic
    for r in rows:
        if "chan_generic_kernel" in r["name"]:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r


def channelize_fp64(h, x):
    """The header's formula in fp64: the four branch sums u_r[m] = sum_j h[4j + r] x[4m - 4j - r] (x[<0] = 0), then the radix-2
    butterflies as sxfir_channelizer.h writes them.  Returns [4, len(x) // 4]."""
    h = np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.complex128)
    n_out = x.size // 4
    u = []
    for r in range(4):
        hr = np.zeros_like(h)
        hr[r::4] = h[r::4]
        u.append(np.convolve(x, hr)[:4 * n_out:4])
    s0, s1, t0, t1 = u[0] + u[2], u[0] - u[2], u[1] + u[3], u[1] - u[3]
    y1 = (s1.real - t1.imag) + 1j * (s1.imag + t1.real)
    y3 = (s1.real + t1.imag) + 1j * (s1.imag - t1.real)
    return np.stack([s0 + t0, y1, s0 - t0, y3])


def test_butterfly_convention():
    """Band k of the radix-2 steps is direct convolution with h[n] exp(j 2 pi ((n k) mod 4) / 4), decimated by 4: the band that
    design_bandpass(128, 4, k, 4) centres."""
    h = design_lowpass(128, 4).astype(np.float64)
    rng = np.random.default_rng(11)
    x = rng.standard_normal(4 * 300) + 1j * rng.standard_normal(4 * 300)
    y = channelize_fp64(h, x)
    n = np.arange(128)
    quarter = np.array([1, 1j, -1, -1j])                       # exact quarter turns
    for k in range(4):
        hk = h * quarter[(n * k) % 4]
        want = np.convolve(x, hk)[:x.size:4]
        err = np.abs(y[k] - want).max()
        print("band %d: max error %.3g" % (k, err))
        assert err <= 1e-12


def test_fp64_band_separation_of_the_gpu_test():
    """The fp64 figures tests/test_gpu_channelizer.py::test_takes_the_bands_apart leans on, with the library's own designer: the tone
    11/40 cycles per sample (band 1's centre + 0.1/4) is at 0 dB in band 1 and nowhere above -80 dB in bands 0, 2, 3."""
    h = design_lowpass(128, 4).astype(np.float64)
    k = np.arange(1 << 16, dtype=np.int64)
    x = np.exp(2j * np.pi * ((k * 11) % 40) / 40.0)
    y = channelize_fp64(h, x)[:, 64:]
    m = y.shape[1]
    assert m == 16320
    Y = 20 * np.log10(np.maximum(np.abs(np.fft.fft(y, axis=1)) / m, 1e-300))
    print("band 1 tone %.5f dB; bands 0, 2, 3 peak %.1f, %.1f, %.1f dB" % (Y[1, 1632], Y[0].max(), Y[2].max(), Y[3].max()))
    assert abs(Y[1, 1632]) <= 0.001
    assert max(Y[0].max(), Y[2].max(), Y[3].max()) <= -90.0
