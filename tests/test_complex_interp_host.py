"""CPU-side checks of the complex-tap (band-pass) interpolators (include/sxfir_complex_tx.h): the extension's symbols and bindings,
the argument checks of sxfir_create_complex_interpolator that need no GPU, and the shipped code object of the two new kernel
families."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_bandpass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    names = _declared("sxfir_complex_tx.h")
    assert names == ["sxfir_complex_tx_abi_version", "sxfir_create_complex_interpolator"], names
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in names:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_complex_tx_abi_version() == 1 and prof.sxfir_complex_tx_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_complex_tx.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_COMPLEX_TX_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    # the base ABI's number is the header's, untouched by the extension; so is the decimators' extension
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    assert lib.sxfir_abi_version() == int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1))
    assert lib.sxfir_complex_abi_version() == 1
    assert sxxcvr_amd.ComplexInterpolator.__mro__[1] is sxxcvr_amd.Resampler


def test_create_argument_errors_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    create = lib.sxfir_create_complex_interpolator
    taps = np.ones(2 * 128, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    EINVAL, ENODEVICE = -1, -5
    assert create(None, tp, 128, 4, 1, 0, -1) == EINVAL
    for args in [(None, 128, 4, 1, 0), (tp, 0, 4, 1, 0), (tp, 128, 0, 1, 0), (tp, 128, 4, 0, 0), (tp, 128, 4, 1, 9)]:
        assert create(C.byref(plan), *args, -1) == EINVAL, args
        assert not plan.value, args
    # an interpolator's own shape rule, as sxfir_create states it: before the device is looked at too
    assert create(C.byref(plan), tp, 127, 4, 1, 0, -1) == EINVAL and not plan.value
    # the decimators' creator keeps its answer
    assert lib.sxfir_create_complex(C.byref(plan), 1, tp, 128, 4, 1, 0, -1) == -4
    assert b"decimators only" in lib.sxfir_last_error()
    n = C.c_int(-1)
    lib.sxfir_device_count(C.byref(n))
    if n.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_complex_interp.py)
    # no GPU: refused as the real-tap create refuses, never computed on the host
    assert create(C.byref(plan), tp, 128, 4, 1, 0, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.ComplexInterpolator(design_bandpass(128, 4, 1, 4, gain=4), 4)
    assert ei.value.code == ENODEVICE


def test_shipped_code_object_of_the_complex_interpolators():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    # (the kernel's other instances, <.., sxfir::InterpMixTileArgs>, are the translating interpolators': tests/test_mix_tx_host.py)
    tiled = {r["name"]: r for r in rows if "interp_cx_pass_kernel" in r["name"] and r["name"].endswith(", sxfir::InterpTileArgs>")}
    assert sorted(tiled) == ["interp_cx_pass_kernel<2, 8, sxfir::InterpTileArgs>", "interp_cx_pass_kernel<4, 4, sxfir::InterpTileArgs>"], sorted(tiled)
    # the real-tap pass instance of the same ratio in the same code object: unkeyed, CF32, <QI, false, false, true, L, L, false>
    real = {r["name"]: r for r in rows if r["name"].startswith("interp8_pass_kernel<")}
    for name, t in tiled.items():
        qi, ll = [int(v) for v in name.split("<")[1].split(",")[:2]]
        base = real["interp8_pass_kernel<%d, false, false, true, %d, %d, false>" % (qi, ll, ll)]
        print(t)
        assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0 and t["s_barrier"] == 0, t
        assert t["lds_bytes"] == base["lds_bytes"] and t["vgpr"] <= 256, t
        # two chains per window read: twice the real instance's packed FMAs, every one with a scalar tap, on the real
        # instance's window reads (the ds_read_b128 count also holds the transposition's, as the real instance's does)
        assert t["v_pk_fma_f32"] == 2 * base["v_pk_fma_f32"] and t["scalar_tap_fmas"] == t["v_pk_fma_f32"], t
        assert t["ds_read_b128"] == base["ds_read_b128"], t
        # the rows no other tile reads are staged non-temporally, the shared ones plainly
        assert 0 < t["global_load_lds_dwordx4_nt"] < t["global_load_lds_dwordx4"], t
        # the counted wait's premises, read off the disassembly as for the real instances (tests/test_abi.py): the next tile's
        # DMAs, then exactly eight stores and nothing else that counts as VMEM; no atomic (there is no keyed instance)
        cw = t["counted_wait"]
        assert cw["n"] == 8 and cw["waits"] == 1 and cw["dma_loads"] >= 2 and cw["atomics_after_first_dma"] == 0, t
        assert cw["last_block_vmem"] == ["global_store_dwordx4"] * 8 and cw["non_store_vmem_after_last_dma"] == [], t
    generic = sorted(r["name"] for r in rows if r["name"].startswith("interp_cx_generic_kernel<"))
    assert generic == ["interp_cx_generic_kernel<sxfir::CF16, sxfir::CF16>", "interp_cx_generic_kernel<sxfir::CF32, sxfir::CF32>",
                       "interp_cx_generic_kernel<sxfir::CF32, sxfir::S32>"], generic
    for r in rows:
        if "interp_cx_generic_kernel" in r["name"]:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r
