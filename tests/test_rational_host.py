"""CPU-side checks of the rational resamplers (include/sxfir_rational.h): the extension's symbols and bindings, the refusals of
sxfir_create_rational that need no GPU, the reference of tests/rational_cases.py against the fp64 definition, and the shipped code
object of the new kernels."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_lowpass, design_rational
from rational_cases import SHAPES, bound, gaussian_stream, n_out_for, rational_f64, rational_ref, rational_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    names = _declared("sxfir_rational.h")
    assert names == ["sxfir_create_rational", "sxfir_plan_rational", "sxfir_rational_abi_version", "sxfir_resample",
                     "sxfir_time_resample"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_rational_abi_version() == 1 and prof.sxfir_rational_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_rational.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_RATIONAL_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    # the base ABI's number is the header's, untouched by the extension
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    assert lib.sxfir_abi_version() == int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1))
    assert sxxcvr_amd.RationalResampler.__mro__[1] is sxxcvr_amd.Resampler


def test_create_refusals_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    create = lib.sxfir_create_rational
    taps = np.ones(128, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    CF32, CF16, S32 = 0, 1, 2
    assert create(None, tp, 128, 4, 5, 1, CF32, -1) == EINVAL
    # (taps, ntaps, up, down, nchan, fmt) -> code and a word of the message, in the order the creator checks them
    cases = [((None, 128, 4, 5, 1, CF32), EINVAL, b"NULL"),
             ((tp, 0, 4, 5, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 128, 1, 5, 1, CF32), EINVAL, b"integer decimator or interpolator"),
             ((tp, 128, 4, 1, 1, CF32), EINVAL, b"integer decimator or interpolator"),
             ((tp, 128, 0, 5, 1, CF32), EINVAL, b"out of range"),
             ((tp, 128, 4, 4097, 1, CF32), EINVAL, b"out of range"),
             ((tp, 128, 4097, 5, 1, CF32), EINVAL, b"out of range"),
             ((tp, 128, 4, 6, 1, CF32), EINVAL, b"2/3"),
             ((tp, 126, 4, 5, 1, CF32), EINVAL, b"ntaps % up"),
             ((tp, 128, 4, 5, 0, CF32), EINVAL, b"nchan"),
             ((tp, 128, 4, 5, 1, 9), EINVAL, b"format"),
             ((tp, 128, 4, 5, 1, S32), EUNSUPPORTED, b"neither wire side"),
             # two bad arguments at once: the earlier check answers
             ((tp, 0, 4, 6, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 128, 1, 5, 0, CF32), EINVAL, b"integer decimator or interpolator"),
             ((tp, 126, 4, 6, 1, CF32), EINVAL, b"2/3"),
             ((tp, 126, 4, 5, 0, CF32), EINVAL, b"ntaps % up"),
             ((tp, 128, 4, 5, 0, 9), EINVAL, b"nchan"),
             ((tp, 126, 4, 5, 1, S32), EINVAL, b"ntaps % up"),
             ((tp, 128, 4, 6, 1, S32), EINVAL, b"2/3")]
    for args, code, word in cases:
        plan.value = 0xDEAD if args[0] is not None else None
        assert create(C.byref(plan), *args, -1) == code, args
        assert word in lib.sxfir_last_error(), (args, lib.sxfir_last_error())
        assert not plan.value, args
    n = C.c_int(-1)
    lib.sxfir_device_count(C.byref(n))
    if n.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_rational.py)
    # no GPU: refused as the real-tap create refuses, never computed on the host
    for fmt in (CF32, CF16):
        assert create(C.byref(plan), tp, 128, 4, 5, 1, fmt, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.RationalResampler(design_rational(4, 5), 4, 5)
    assert ei.value.code == ENODEVICE


@pytest.mark.parametrize("up,down,T", SHAPES)
def test_reference_against_fp64(oracle, up, down, T):
    """The float32 reference (the oracle's interpolator pass, every down-th sample) against np.convolve of the zero-stuffed stream in
    fp64, within 2e-6 sum|h| max|x|, under jsplit 1 and, where T is even, 2."""
    h = rational_taps(up, T)
    x = gaussian_stream(3000)
    want = rational_f64(h, up, down, x)
    assert want.size == n_out_for(x.size, up, down) == -(-x.size * up // down)
    for jsplit in (1, 2) if T % 2 == 0 else (1,):
        got = rational_ref(oracle, h, up, down, x, jsplit)
        assert got.dtype == np.complex64 and got.shape == want.shape
        err = float(np.abs(got.astype(np.complex128) - want).max())
        print("%d/%d x %d jsplit %d: error %.3g, bound %.3g (%.0f times inside)" % (up, down, T, jsplit, err, bound(h, x), bound(h, x) / err))
        assert err <= bound(h, x)


@pytest.mark.parametrize("up,down,T", SHAPES)
def test_output_count_formula(up, down, T):
    """ceil((c + n) up / down) - ceil(c up / down) counts the outputs m with c <= floor(m down / up) < c + n."""
    for c in range(3 * down + 1):
        for n in range(3 * down + 1):
            brute = sum(1 for m in range((c + n) * up + 2) if c <= (m * down) // up < c + n)
            assert n_out_for(n, up, down, c) == brute, (c, n)


def test_design_rational_is_the_lowpass_it_stands_for():
    for up, down, tpp, beta in [(4, 5, 32, 8.0), (5, 4, 32, 8.0), (2, 3, 32, 8.0), (3, 4, 8, 6.5), (16, 25, 32, 8.0)]:
        a = design_rational(up, down, tpp, beta)
        b = design_lowpass(up * tpp, max(up, down), beta, float(up))
        assert a.dtype == np.float32 and a.size == up * tpp
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (up, down)
    assert design_rational(4, 5).size == 128


def test_shipped_code_object_of_the_rational_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    tiled = [r for r in rows if "resample45_kernel" in r["name"]]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0 and t["vgpr"] <= 256, t
    assert t["scalar_tap_fmas"] == t["v_pk_fma_f32"] > 0, t
    # the rows no other tile reads are staged non-temporally, the halo plainly
    assert 0 < t["global_load_lds_dwordx4_nt"] < t["global_load_lds_dwordx4"], t
    generic = sorted(r["name"] for r in rows if "resample_generic_kernel<" in r["name"])
    assert generic == ["resample_generic_kernel<sxfir::CF16, sxfir::CF16>", "resample_generic_kernel<sxfir::CF32, sxfir::CF32>"], generic
    for r in rows:
        if "resample_generic_kernel" in r["name"]:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r
