"""ctypes loader for the in-tree native libraries.  Fails loudly when a
library is missing: the product has no fallback path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(_HERE, "lib")

_sxfir = None
_sxfir_prof = None


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sxfir error %d: %s" % (code, msg))
        self.code = code


def _share_hip_runtime_with_torch():
    # torch ships its own libamdhip64.so.7; importing it first makes our
    # library resolve the same runtime instance instead of a second copy.
    if os.environ.get("SXFIR_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load_sxfir(profiling=False):
    """Load sxxcvr_amd/lib/libsxfir.so and declare its prototypes.

    profiling=True loads libsxfir_prof.so instead: the same C ABI plus include/sxfir_prof.h, with the kernel
    A/B variants and environment knobs (tools/ and tests/test_gpu_variants.py; an explicit argument, never
    an environment switch: the product's arithmetic does not depend on the environment)."""
    global _sxfir, _sxfir_prof
    if profiling:
        if _sxfir_prof is not None:
            return _sxfir_prof
    elif _sxfir is not None:
        return _sxfir
    path = os.path.join(LIBDIR, "libsxfir_prof.so" if profiling else "libsxfir.so")
    if profiling and os.environ.get("SXFIR_PROF_LIB"):
        # tools only (tools/prev_lib.sh): the PROFILING library of another commit, built into sxxcvr_amd/lib/prev/, for
        # before / after timings on the same box.  Only a library in that directory is accepted, and only by the profiling
        # loader: the product library's path is never taken from the environment.
        cand = os.path.realpath(os.environ["SXFIR_PROF_LIB"])
        prev = os.path.realpath(os.path.join(LIBDIR, "prev"))
        if os.path.dirname(cand) != prev:
            raise ImportError("SXFIR_PROF_LIB must name a library under %s (tools/prev_lib.sh builds it there), got %s" % (prev, cand))
        path = cand
    if not os.path.exists(path):
        raise ImportError(
            "%s is missing: build the HIP extension first (python -m sxxcvr_amd.build). "
            "There is no CPU fallback." % path)
    _share_hip_runtime_with_torch()
    lib = C.CDLL(path, mode=C.RTLD_LOCAL if profiling else C.RTLD_GLOBAL)
    vp, sz, i64, u64, ll, dbl, ci = C.c_void_p, C.c_size_t, C.c_int64, C.c_uint64, C.c_longlong, C.c_double, C.c_int
    P = C.POINTER
    sig = {
        "sxfir_abi_version": (ci, []),
        "sxfir_last_error": (C.c_char_p, []),
        "sxfir_device_count": (ci, [P(ci)]),
        "sxfir_device_info": (ci, [ci, C.c_char_p, C.c_char_p, P(ci), P(sz)]),
        "sxfir_device_pci_bus_id": (ci, [ci, C.c_char_p, sz]),
        "sxfir_create": (ci, [P(vp), ci, vp, ci, ci, ci, ci, ci]),
        "sxfir_destroy": (ci, [vp]),
        "sxfir_reset": (ci, [vp, vp]),
        "sxfir_set_history": (ci, [vp, vp, sz, sz, vp]),
        "sxfir_set_position": (ci, [vp, i64]),
        "sxfir_set_kernel": (ci, [vp, ci]),
        "sxfir_set_tx_threshold": (ci, [vp, C.c_float]),
        "sxfir_contract": (ci, [vp, P(ci), P(ci)]),
        "sxfir_contract_rotation": (ci, [vp, P(ci)]),
        "sxfir_position": (ci, [vp, P(i64), P(i64)]),
        "sxfir_outputs_for": (ci, [vp, sz, P(sz)]),
        "sxfir_launch_geometry": (ci, [vp, sz, vp]),
        "sxfir_decimate": (ci, [vp, vp, sz, sz, vp, sz, P(sz), vp]),
        "sxfir_interpolate": (ci, [vp, vp, sz, sz, vp, sz, P(sz), vp]),
        "sxfir_comm_unique_id": (ci, [vp]),
        "sxfir_comm_init_rank": (ci, [P(vp), vp, ci, ci, ci]),
        "sxfir_comm_init_all": (ci, [P(vp), ci, P(ci)]),
        "sxfir_comm_destroy": (ci, [vp]),
        "sxfir_comm_rank": (ci, [vp, P(ci), P(ci), P(ci)]),
        "sxfir_comm_query": (ci, [vp, P(ci), P(ci), P(ci)]),
        "sxfir_comm_gather": (ci, [vp, vp, vp, sz, sz, ci, sz, vp]),
        "sxfir_comm_gather_all": (ci, [P(vp), ci, P(vp), vp, sz, sz, ci, sz, P(vp)]),
        "sxfir_interpolate_keyed": (ci, [vp, vp, sz, sz, vp, sz, P(sz), sz, sz, vp, vp]),
        "sxfir_time_decimate": (ci, [vp, vp, sz, sz, vp, sz, ci, vp, P(C.c_float)]),
        "sxfir_time_interpolate": (ci, [vp, vp, sz, sz, vp, sz, ci, vp, P(C.c_float)]),
        "sxfir_clock_probe_start": (ci, [P(vp), ci, ci]),
        "sxfir_clock_probe_read": (ci, [vp, P(dbl)]),
        "sxfir_synth_fill": (ci, [vp, sz, sz, ci, u64, C.c_uint32, i64, ci, vp]),
        "sxfir_convert_rx_s32": (ci, [vp, vp, sz, vp]),
        "sxfir_convert_tx_s32": (ci, [vp, vp, sz, C.c_float, vp]),
        "sxfir_count_keyed": (ci, [vp, sz, C.c_float, vp, vp]),
        "sxfir_cf32_to_cf16": (ci, [vp, vp, sz, vp]),
        "sxfir_cf16_to_cf32": (ci, [vp, vp, sz, vp]),
        "sxfir_ticks_to_time_ns": (ll, [ll, dbl]),
        "sxfir_time_ns_to_ticks": (ll, [ll, dbl]),
        "sxfir_design_lowpass": (ci, [ci, ci, dbl, dbl, vp]),
        "sxfir_malloc": (ci, [P(vp), sz]),
        "sxfir_free": (ci, [vp]),
        "sxfir_set_device": (ci, [ci]),
        "sxfir_host_alloc": (ci, [P(vp), sz]),
        "sxfir_host_free": (ci, [vp]),
        "sxfir_host_register": (ci, [vp, sz]),
        "sxfir_host_unregister": (ci, [vp]),
        "sxfir_host_device_pointer": (ci, [vp, sz, P(vp)]),
        "sxfir_stream_create": (ci, [P(vp)]),
        "sxfir_stream_destroy": (ci, [vp]),
        "sxfir_event_create": (ci, [P(vp)]),
        "sxfir_event_destroy": (ci, [vp]),
        "sxfir_event_create_timing": (ci, [P(vp)]),
        "sxfir_event_elapsed_ms": (ci, [vp, vp, P(C.c_float)]),
        "sxfir_event_record": (ci, [vp, vp]),
        "sxfir_event_sync": (ci, [vp]),
        "sxfir_stream_wait_event": (ci, [vp, vp]),
        "sxfir_memcpy_h2d": (ci, [vp, vp, sz, vp]),
        "sxfir_memcpy_d2h": (ci, [vp, vp, sz, vp]),
        "sxfir_stream_sync": (ci, [vp]),
        # include/sxfir_complex.h: complex-tap (band-pass) decimators
        "sxfir_complex_abi_version": (ci, []),
        "sxfir_create_complex": (ci, [P(vp), ci, vp, ci, ci, ci, ci, ci]),
        "sxfir_taps_are_complex": (ci, [vp, P(ci)]),
        "sxfir_design_bandpass": (ci, [ci, ci, dbl, dbl, ci, ci, vp]),
        # include/sxfir_complex_tx.h: complex-tap (band-pass) interpolators
        "sxfir_complex_tx_abi_version": (ci, []),
        "sxfir_create_complex_interpolator": (ci, [P(vp), vp, ci, ci, ci, ci, ci]),
        # include/sxfir_channelizer.h: the 4-band channelizer
        "sxfir_channelizer_abi_version": (ci, []),
        "sxfir_create_channelizer": (ci, [P(vp), vp, ci, ci, ci, ci, ci]),
        "sxfir_channelize": (ci, [vp, vp, sz, sz, vp, sz, sz, P(sz), vp]),
        "sxfir_plan_bands": (ci, [vp, P(ci)]),
        # include/sxfir_channelizer_os.h: the 2x oversampled 4-band channelizer
        "sxfir_channelizer_os_abi_version": (ci, []),
        "sxfir_create_channelizer_os": (ci, [P(vp), vp, ci, ci, ci, ci, ci, ci]),
        "sxfir_plan_oversampling": (ci, [vp, P(ci)]),
        # include/sxfir_synthesizer.h: the 4-band synthesizer
        "sxfir_synthesizer_abi_version": (ci, []),
        "sxfir_create_synthesizer": (ci, [P(vp), vp, ci, ci, ci, ci, ci]),
        "sxfir_synthesize": (ci, [vp, vp, sz, sz, sz, vp, sz, P(sz), vp]),
        "sxfir_plan_synthesis_bands": (ci, [vp, P(ci)]),
        # include/sxfir_synthesizer_os.h: the 2x oversampled 4-band synthesizer
        "sxfir_synthesizer_os_abi_version": (ci, []),
        "sxfir_create_synthesizer_os": (ci, [P(vp), vp, ci, ci, ci, ci, ci, ci]),
        "sxfir_plan_synthesis_oversampling": (ci, [vp, P(ci)]),
        # include/sxfir_rational.h: rational up / down resamplers
        "sxfir_rational_abi_version": (ci, []),
        "sxfir_create_rational": (ci, [P(vp), vp, ci, ci, ci, ci, ci, ci]),
        "sxfir_resample": (ci, [vp, vp, sz, sz, vp, sz, P(sz), vp]),
        "sxfir_time_resample": (ci, [vp, vp, sz, sz, vp, sz, ci, vp, P(C.c_float)]),
        "sxfir_plan_rational": (ci, [vp, P(ci), P(ci)]),
        # include/sxfir_translate.h: frequency-translating decimators
        "sxfir_translate_abi_version": (ci, []),
        "sxfir_design_rotator": (ci, [ci, vp]),
        "sxfir_create_translating": (ci, [P(vp), vp, ci, ci, ci, ci, ci, ci, ci]),
        "sxfir_plan_translation": (ci, [vp, P(ci), P(ci)]),
        # include/sxfir_translate_tx.h: frequency-translating interpolators
        "sxfir_translate_tx_abi_version": (ci, []),
        "sxfir_create_translating_interpolator": (ci, [P(vp), vp, ci, ci, ci, ci, ci, ci, ci]),
        "sxfir_plan_translation_tx": (ci, [vp, P(ci), P(ci)]),
        # include/sxfir_bank.h: the tuner bank, K translating decimators in one pass
        "sxfir_bank_abi_version": (ci, []),
        "sxfir_create_bank": (ci, [P(vp), vp, ci, ci, ci, vp, vp, ci, ci, ci]),
        "sxfir_decimate_bank": (ci, [vp, vp, sz, sz, vp, sz, sz, P(sz), vp]),
        "sxfir_time_decimate_bank": (ci, [vp, vp, sz, sz, vp, sz, sz, ci, vp, P(C.c_float)]),
        "sxfir_plan_bank": (ci, [vp, P(ci)]),
        "sxfir_plan_bank_band": (ci, [vp, ci, P(ci), P(ci)]),
        # include/sxfir_bank_tx.h: the combiner bank, K translating interpolators summed in one pass
        "sxfir_bank_tx_abi_version": (ci, []),
        "sxfir_create_bank_interpolator": (ci, [P(vp), vp, ci, ci, ci, vp, vp, ci, ci, ci]),
        "sxfir_interpolate_bank": (ci, [vp, vp, sz, sz, sz, vp, sz, P(sz), vp]),
        "sxfir_time_interpolate_bank": (ci, [vp, vp, sz, sz, sz, vp, sz, ci, vp, P(C.c_float)]),
        "sxfir_plan_bank_tx": (ci, [vp, P(ci)]),
        "sxfir_plan_bank_tx_band": (ci, [vp, ci, P(ci), P(ci)]),
        # include/sxfir_arbitrary.h: arbitrary-rate resamplers
        "sxfir_arbitrary_abi_version": (ci, []),
        "sxfir_create_arbitrary": (ci, [P(vp), vp, ci, ci, u64, ci, ci, ci]),
        "sxfir_set_rate": (ci, [vp, u64]),
        "sxfir_set_time": (ci, [vp, i64, i64, C.c_uint32]),
        "sxfir_plan_arbitrary": (ci, [vp, P(ci), P(u64), P(i64), P(C.c_uint32)]),
        "sxfir_resample_arbitrary": (ci, [vp, vp, sz, sz, vp, sz, P(sz), vp]),
        "sxfir_time_resample_arbitrary": (ci, [vp, vp, sz, sz, vp, sz, ci, vp, P(C.c_float)]),
        "sxfir_arbitrary_outputs": (ci, [i64, C.c_uint32, u64, i64, u64, P(u64), P(i64), P(C.c_uint32)]),
        "sxfir_arbitrary_locate": (ci, [u64, u64, u64, ci, P(i64), P(ci), P(C.c_float)]),
    }
    if profiling:
        sig["sxfir_debug_clock"] = (ci, [vp, P(dbl)])
        sig["sxfir_debug_stamps"] = (ci, [vp, P(C.c_ulonglong), sz, P(sz)])
        sig["sxfir_debug_join_poison"] = (ci, [vp, C.c_uint32, vp])
        sig["sxfir_debug_join_counters"] = (ci, [vp, P(ll), vp])
        sig["sxfir_debug_join_set_counter"] = (ci, [vp, ll, C.c_uint, vp])
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    lib._sx_signatures = sig
    if profiling:
        _sxfir_prof = lib
    else:
        _sxfir = lib
    return lib


def check(rc, lib=None):
    if rc != 0:
        raise NativeError(rc, (lib or load_sxfir()).sxfir_last_error().decode("utf-8", "replace"))
