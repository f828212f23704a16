"""Python face of the C ABI in include/sxfir.h, include/sxfir_complex.h, include/sxfir_complex_tx.h, include/sxfir_channelizer.h, include/sxfir_synthesizer.h, include/sxfir_rational.h, include/sxfir_translate.h, include/sxfir_translate_tx.h and include/sxfir_arbitrary.h.

Device memory comes either from torch (complex64 / int32 CUDA tensors, the
current torch stream is used) or from the library's own sxfir_malloc for
numpy-only callers (``*_host`` helpers).  No arithmetic happens in Python.
"""
import ctypes as C

import numpy as np

from ._native import check as _check, load_sxfir

DECIMATE, INTERPOLATE = 0, 1
CF32, CF16, S32 = 0, 1, 2
KERNEL_AUTO, KERNEL_TILED, KERNEL_GENERIC = 0, 1, 2
_FMT = {"CF32": CF32, "CF16": CF16, "S32": S32, CF32: CF32, CF16: CF16, S32: S32}


class Contract(tuple):
    """(jsplit, cw) with the rotation beside it: unpacks and compares as the pair it always was.  Under a rotation
    (rot != 0: the decimators by 48 and 96) the pair ALONE does not state the summation order -- unpacking it without ever
    having read .rot warns once (a caller written before ABI 5 would feed (2, 4) to its own check and get other bits)."""
    def __new__(cls, pair, rot=0):
        self = super().__new__(cls, pair)
        self._rot = rot
        self._rot_seen = rot == 0
        return self

    @property
    def rot(self):
        self._rot_seen = True
        return self._rot

    def __iter__(self):
        if not self._rot_seen:
            import warnings
            self._rot_seen = True
            warnings.warn("this plan's contract (%d, %d) holds under rotation %d (sxfir_contract_rotation): read Contract.rot too"
                          % (self[0], self[1], self._rot), stacklevel=2)
        return super().__iter__()


def check(rc, lib=None):
    _check(rc, lib)


def design_lowpass(ntaps, ratio, beta=8.0, gain=1.0):
    lib = load_sxfir()
    taps = np.empty(ntaps, dtype=np.float32)
    check(lib.sxfir_design_lowpass(ntaps, ratio, beta, gain, taps.ctypes.data_as(C.c_void_p)))
    return taps


def design_bandpass(ntaps, ratio, num, den, beta=8.0, gain=1.0):
    """Complex band-pass taps (complex64): the design_lowpass prototype turned to the band centre num/den cycles per INPUT
    sample (sxfir_design_bandpass); k/ratio is sub-band k of the output raster.  Resampler(DECIMATE, these taps, ratio) takes
    that band out in one pass and leaves its centre at 0 Hz of the output.

    The TX reading: for ComplexInterpolator(these taps, ratio) the phasors are on the OUTPUT side -- num/den is the band centre in
    cycles per OUTPUT sample, and gain=ratio keeps the stream's level through the zero stuffing: design_bandpass(ntaps, ratio, k,
    ratio, gain=ratio) places the input at sub-band k of the x ratio raster."""
    lib = load_sxfir()
    taps = np.empty(ntaps, dtype=np.complex64)
    check(lib.sxfir_design_bandpass(ntaps, ratio, beta, gain, int(num), int(den), taps.ctypes.data_as(C.c_void_p)))
    return taps


def design_rotator(den):
    """The rotation table of TranslatingDecimator (sxfir_design_rotator): complex64 [den], w[i] = exp(-2j pi i / den), each component
    computed in fp64 from the integer i and rounded to float32 once."""
    lib = load_sxfir()
    w = np.empty(max(int(den), 0), dtype=np.complex64)
    check(lib.sxfir_design_rotator(int(den), w.ctypes.data_as(C.c_void_p)), lib)
    return w


def design_rational(up, down, taps_per_phase=32, beta=8.0):
    """Unit-gain taps of RationalResampler(taps, up, down): the low-pass of the narrower side at the x up raster,
    design_lowpass(up * taps_per_phase, max(up, down), beta, up)."""
    return design_lowpass(int(up) * int(taps_per_phase), max(int(up), int(down)), beta, float(up))


def _torch_stream(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def synth_fill(out, seed, first_channel=0, start=0, fmt="CF32"):
    """Fill a CUDA tensor [nchan, n] (complex64 for CF32, int32 words for CF16)
    with the synthetic IQ source."""
    lib = load_sxfir()
    t = out if out.dim() == 2 else out.unsqueeze(0)
    nchan, n = t.shape
    check(lib.sxfir_synth_fill(C.c_void_p(t.data_ptr()), n, t.stride(0), nchan, seed, first_channel, start,
                               _FMT[fmt], _torch_stream(t)))
    return out


def pin_array(a):
    """Page-lock a numpy array's memory (sxfir_host_register) so that the GPU can store into it directly: large
    readStream calls into such a buffer skip the staging copy.  Undo with unpin_array before the array is freed."""
    lib = load_sxfir()
    check(lib.sxfir_host_register(C.c_void_p(a.ctypes.data), a.nbytes))
    return a


def unpin_array(a):
    check(load_sxfir().sxfir_host_unregister(C.c_void_p(a.ctypes.data)))


class StreamTimer:
    """GPU time of whatever is launched on `stream` between start() and stop(): HIP events recorded on that
    stream through the C ABI (torch.cuda.Event would only see torch's current stream)."""

    def __init__(self, stream=0):
        self._lib = load_sxfir()
        self._stream = C.c_void_p(stream)
        self._e0, self._e1 = C.c_void_p(), C.c_void_p()
        check(self._lib.sxfir_event_create_timing(C.byref(self._e0)))
        check(self._lib.sxfir_event_create_timing(C.byref(self._e1)))

    def start(self):
        check(self._lib.sxfir_event_record(self._e0, self._stream))

    def stop(self):
        check(self._lib.sxfir_event_record(self._e1, self._stream))

    def elapsed_ms(self):
        ms = C.c_float()
        check(self._lib.sxfir_event_elapsed_ms(self._e0, self._e1, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            self._lib.sxfir_event_destroy(self._e0)
            self._lib.sxfir_event_destroy(self._e1)
        except Exception:
            pass


class ClockProbe:
    """In-kernel shader clock while other work runs (sxfir_clock_probe_*): start, run the work, read()."""

    def __init__(self, device=-1, duration_us=20000):
        self._lib = load_sxfir()
        self._h = C.c_void_p()
        check(self._lib.sxfir_clock_probe_start(C.byref(self._h), int(device), int(duration_us)))

    def read(self):
        mhz = C.c_double()
        h, self._h = self._h, C.c_void_p()
        check(self._lib.sxfir_clock_probe_read(h, C.byref(mhz)))
        return mhz.value


class Geometry(C.Structure):
    """sxfir_geometry of include/sxfir.h: what a call would launch."""
    _fields_ = [("kernel", C.c_char * 64), ("tiled", C.c_int), ("split", C.c_int), ("tile_samples", C.c_longlong),
                ("n_tiles", C.c_longlong), ("workgroups", C.c_longlong), ("resident", C.c_longlong)]


class _Plan:
    """What every sxfir_plan answers, whichever entry point created it: the stream state, the numeric contract, the launch
    geometry and the kernel choice.  Resampler and the band plans (Channelizer, Synthesizer) create the plan (self._plan in self._lib) and add their passes."""

    _plan = None

    def _ck(self, rc):
        _check(rc, self._lib)      # error text from the library this plan lives in

    def close(self):
        if self._plan:
            self._lib.sxfir_destroy(self._plan)
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- introspection --------------------------------------------------------
    @property
    def contract(self):
        """(jsplit, cw) of the plan's numeric contract; the tuple's attribute `rot` is the contract's rotation
        (sxfir_contract_rotation: 1 for the decimators by 48 and 96, else 0)."""
        a, b, r = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._lib.sxfir_contract(self._plan, C.byref(a), C.byref(b)))
        self._ck(self._lib.sxfir_contract_rotation(self._plan, C.byref(r)))
        return Contract((a.value, b.value), r.value)

    @property
    def position(self):
        a, b = C.c_int64(), C.c_int64()
        self._ck(self._lib.sxfir_position(self._plan, C.byref(a), C.byref(b)))
        return a.value, b.value

    def geometry(self, n_in):
        """What a call with n_in new input samples would launch now (sxfir_launch_geometry): kernel family, whether an
        LDS-tiled kernel runs it, tiles, work items per tile, workgroups, and the workgroup slots of the chip."""
        g = Geometry()
        self._ck(self._lib.sxfir_launch_geometry(self._plan, n_in, C.byref(g)))
        return {"kernel": g.kernel.decode(), "tiled": bool(g.tiled), "split": g.split, "tile_samples": g.tile_samples,
                "n_tiles": g.n_tiles, "workgroups": g.workgroups, "resident": g.resident}

    def outputs_for(self, n_in):
        n = C.c_size_t()
        self._ck(self._lib.sxfir_outputs_for(self._plan, n_in, C.byref(n)))
        return n.value

    def set_kernel(self, kernel):
        self._ck(self._lib.sxfir_set_kernel(self._plan, kernel))

    def reset(self, stream=None):
        self._ck(self._lib.sxfir_reset(self._plan, C.c_void_p(stream or 0)))

    def set_history_ptr(self, src_ptr, n, stride, stream=0):
        """The filter state becomes the last samples of the device block [src_ptr, src_ptr + n) of every channel
        (sxfir_set_history): as if that block had just been processed."""
        self._ck(self._lib.sxfir_set_history(self._plan, C.c_void_p(src_ptr), n, stride, C.c_void_p(stream)))

    def set_position(self, consumed):
        """Place the plan at input sample `consumed` of its stream (sxfir_set_position): a decimator's output phase
        and output count of the next call follow from it."""
        self._ck(self._lib.sxfir_set_position(self._plan, int(consumed)))


class Resampler(_Plan):
    """One sxfir plan: `nchan` independent channels of one GPU."""

    def __init__(self, mode, taps, ratio, nchan=1, fmt="CF32", device=-1, profiling=False):
        self._lib = load_sxfir(profiling)
        self.profiling = bool(profiling)
        self._plan = C.c_void_p()
        # complex-dtype taps: a complex-tap (band-pass) decimator, sxfir_create_complex; real arrays take sxfir_create as ever
        cx = np.iscomplexobj(taps)
        taps = np.ascontiguousarray(taps, dtype=np.complex64 if cx else np.float32)
        self.mode, self.ratio, self.nchan, self.fmt, self.ntaps = mode, int(ratio), int(nchan), _FMT[fmt], taps.size
        create = self._lib.sxfir_create_complex if cx else self._lib.sxfir_create
        self._ck(create(C.byref(self._plan), mode, taps.ctypes.data_as(C.c_void_p), taps.size,
                        int(ratio), int(nchan), self.fmt, int(device)))

    def _create_complex(self, create, mode, taps, ratio, extra, nchan, fmt, device, profiling):
        """The creators of the one-direction complex-tap plans: create(&plan, taps, ntaps, ratio, *extra, nchan, fmt, device)."""
        self._lib = load_sxfir(profiling)
        self.profiling = bool(profiling)
        self._plan = C.c_void_p()
        taps = np.ascontiguousarray(taps, dtype=np.complex64)
        self.mode, self.ratio, self.nchan, self.fmt, self.ntaps = mode, int(ratio), int(nchan), _FMT[fmt], taps.size
        self._ck(getattr(self._lib, create)(C.byref(self._plan), taps.ctypes.data_as(C.c_void_p), taps.size, int(ratio),
                                            *[int(e) for e in extra], int(nchan), self.fmt, int(device)))

    @property
    def complex_taps(self):
        """True for a plan with complex taps (sxfir_taps_are_complex)."""
        f = C.c_int()
        self._ck(self._lib.sxfir_taps_are_complex(self._plan, C.byref(f)))
        return bool(f.value)

    def set_tx_threshold(self, threshold2):
        self._ck(self._lib.sxfir_set_tx_threshold(self._plan, float(threshold2)))

    # -- test hooks of the (tile, block) join of the decimators by 48 and 96 (include/sxfir_prof.h) ----------
    def _hook(self, name):
        if not self.profiling:
            raise RuntimeError("%s exists in the profiling build only: Resampler(..., profiling=True)" % name)
        return getattr(self._lib, name)

    def join_poison(self, word=0x7FC00000, stream=0):
        """Fill the plan's block-value scratch with `word` (a quiet NaN in every lane), asynchronously on `stream`."""
        self._ck(self._hook("sxfir_debug_join_poison")(self._plan, int(word), C.c_void_p(stream or 0)))

    def join_counters(self, stream=0):
        """Wait for `stream`; how many of the plan's arrival counters are not zero (between launches: none)."""
        n = C.c_longlong()
        self._ck(self._hook("sxfir_debug_join_counters")(self._plan, C.byref(n), C.c_void_p(stream or 0)))
        return n.value

    def join_set_counter(self, tile_index, value, stream=0):
        """Write one arrival counter (index: channel * tiles of the call + tile); only reset() puts the plan right again."""
        self._ck(self._hook("sxfir_debug_join_set_counter")(self._plan, int(tile_index), int(value), C.c_void_p(stream or 0)))

    # -- raw pointers ---------------------------------------------------------
    def process_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, stream=0):
        n_out = C.c_size_t()
        fn = self._lib.sxfir_decimate if self.mode == DECIMATE else self._lib.sxfir_interpolate
        self._ck(fn(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride, C.byref(n_out),
                 C.c_void_p(stream)))
        return n_out.value

    def interpolate_keyed_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, key_first, key_count, counter_ptr,
                              stream=0):
        """sxfir_interpolate_keyed: the interpolation pass that also adds to the 8-byte device word at counter_ptr how
        many of channel 0's input samples [key_first, key_first + key_count) reach the keying threshold
        (convert_tx_buffer, SoapySX.cpp:132-133)."""
        n_out = C.c_size_t()
        self._ck(self._lib.sxfir_interpolate_keyed(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr),
                                                   out_stride, C.byref(n_out), key_first, key_count,
                                                   C.c_void_p(counter_ptr), C.c_void_p(stream)))
        return n_out.value

    def time_decimate_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, iters, stream=0):
        return self.time_passes_ptr(in_ptr, n_in, in_stride, out_ptr, out_stride, iters, stream)

    def time_passes_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, iters, stream=0):
        """Mean milliseconds of `iters` back-to-back launches of the resampling kernel (HIP events on `stream`);
        the filter state is left alone."""
        ms = C.c_float()
        fn = self._lib.sxfir_time_decimate if self.mode == DECIMATE else self._lib.sxfir_time_interpolate
        self._ck(fn(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride, iters,
                    C.c_void_p(stream), C.byref(ms)))
        return ms.value

    # -- torch tensors --------------------------------------------------------
    def process(self, x, out=None):
        """x: CUDA tensor [nchan, n] or [n]; complex64 (CF32) or int32 words (CF16).
        S32 plans: a decimator takes int32 wire words [.., n, 2] (I, Q) and returns complex64; an
        interpolator takes complex64 and returns int32 wire words [.., n_out, 2]."""
        import torch
        if self.fmt == S32:
            if self.mode == DECIMATE:
                xc = torch.view_as_complex(x.view(torch.float32))          # same 8 bytes per sample
                return self._process(xc, out, torch.complex64)
            y = self._process(x, None if out is None else torch.view_as_complex(out.view(torch.float32)),
                              torch.complex64)
            return torch.view_as_real(y).view(torch.int32)
        return self._process(x, out, x.dtype)

    def _process(self, x, out, out_dtype):
        import torch
        squeeze = x.dim() == 1
        x2 = x.unsqueeze(0) if squeeze else x
        if x2.shape[0] != self.nchan or x2.stride(1) != 1:
            raise ValueError("expected a [nchan=%d, n] tensor with unit sample stride" % self.nchan)
        n_in = x2.shape[1]
        n_out = self.outputs_for(n_in)
        if out is None:
            out = torch.empty((self.nchan, n_out), dtype=out_dtype, device=x2.device)
        o2 = out.unsqueeze(0) if out.dim() == 1 else out
        # the kernel writes through a raw pointer: a caller-supplied `out` must really hold the result
        if (o2.dim() != 2 or o2.shape[0] != self.nchan or o2.shape[1] < n_out or (o2.shape[1] > 1 and o2.stride(1) != 1)
                or o2.dtype != out_dtype or o2.device != x2.device):
            raise ValueError("out must be a [nchan=%d, >=%d] %s tensor with unit sample stride on %s" % (
                self.nchan, n_out, out_dtype, x2.device))
        got = self.process_ptr(x2.data_ptr(), n_in, x2.stride(0) if self.nchan > 1 else n_in, o2.data_ptr(),
                               o2.stride(0) if self.nchan > 1 else max(n_out, 1),
                               torch.cuda.current_stream(x2.device).cuda_stream)
        assert got == n_out
        res = o2[:, :n_out]
        return res[0] if squeeze else res

    # -- numpy host arrays (library-owned device memory) ----------------------
    def process_host(self, x):
        """x: complex64 numpy [nchan, n] or [n] (CF32 plans only).  Copies to the
        GPU, runs the HIP path, copies back."""
        if self.fmt != CF32:
            raise ValueError("process_host handles CF32 plans")
        lib = self._lib
        x = np.ascontiguousarray(x, dtype=np.complex64)
        squeeze = x.ndim == 1
        x2 = x.reshape(1, -1) if squeeze else x
        nchan, n_in = x2.shape
        n_out = self.outputs_for(n_in)
        y = np.empty((nchan, n_out), dtype=np.complex64)
        din, dout = C.c_void_p(), C.c_void_p()
        check(lib.sxfir_malloc(C.byref(din), max(x2.nbytes, 16)))
        check(lib.sxfir_malloc(C.byref(dout), max(y.nbytes, 16)))
        try:
            if x2.nbytes:
                check(lib.sxfir_memcpy_h2d(din, x2.ctypes.data_as(C.c_void_p), x2.nbytes, None))
            self.process_ptr(din.value, n_in, n_in, dout.value, max(n_out, 1))
            if y.nbytes:
                check(lib.sxfir_memcpy_d2h(y.ctypes.data_as(C.c_void_p), dout, y.nbytes, None))
            check(lib.sxfir_stream_sync(None))
        finally:
            lib.sxfir_free(din)
            lib.sxfir_free(dout)
        return y[0] if squeeze else y


class ComplexInterpolator(Resampler):
    """A complex-tap (band-pass) interpolator (include/sxfir_complex_tx.h): one narrowband stream onto a band of the x ratio raster
    in one pass -- the way back from Resampler(DECIMATE, complex taps, ratio).  `taps`: complex, ntaps a multiple of ratio;
    design_bandpass(ntaps, ratio, k, ratio, gain=ratio) places the input at sub-band k, k / ratio cycles per output sample.  The plan
    is an interpolator plan (mode INTERPOLATE) in everything else: the same methods as Resampler."""

    def __init__(self, taps, ratio, nchan=1, fmt="CF32", device=-1, profiling=False):
        self._create_complex("sxfir_create_complex_interpolator", INTERPOLATE, taps, ratio, (), nchan, fmt, device, profiling)


class _Translating:
    """What the two translating plans answer alike; `_query` names the plan query of the class's header."""

    def _translation(self):
        n, d = C.c_int(), C.c_int()
        self._ck(getattr(self._lib, self._query)(self._plan, C.byref(n), C.byref(d)))
        return n.value, d.value

    @property
    def num(self):
        """The band centre's numerator, reduced into [0, den)."""
        return self._translation()[0]

    @property
    def den(self):
        return self._translation()[1]


class TranslatingDecimator(Resampler, _Translating):
    """A frequency-translating decimator (include/sxfir_translate.h): the complex-tap decimator Resampler(DECIMATE, taps, ratio) with
    output m turned by exp(-2j pi (m * s mod den) / den), s = num * ratio mod den, m the absolute output index -- the band centred at
    num / den cycles per input sample (taps = design_bandpass(ntaps, ratio, num, den)) lands at 0 Hz of the output in one pass, on or
    off the output raster.  The plan is a decimator plan with complex taps in everything else: the same methods as Resampler."""

    _query = "sxfir_plan_translation"

    def __init__(self, taps, ratio, num, den, nchan=1, fmt="CF32", device=-1, profiling=False):
        self._create_complex("sxfir_create_translating", DECIMATE, taps, ratio, (num, den), nchan, fmt, device, profiling)


class TranslatingInterpolator(Resampler, _Translating):
    """A frequency-translating interpolator (include/sxfir_translate_tx.h), the way back from TranslatingDecimator: the complex-tap
    interpolator ComplexInterpolator(taps, ratio) with input m turned by exp(+2j pi (m * s mod den) / den), s = num * ratio mod den, m
    the absolute input index, where it is read -- a base-band stream lands centred at num / den cycles per output sample
    (taps = design_bandpass(ntaps, ratio, num, den, gain=ratio)) in one pass, on or off the x ratio raster.  History is raw samples.
    The plan is an interpolator plan with complex taps in everything else: the same methods as Resampler."""

    _query = "sxfir_plan_translation_tx"

    def __init__(self, taps, ratio, num, den, nchan=1, fmt="CF32", device=-1, profiling=False):
        self._create_complex("sxfir_create_translating_interpolator", INTERPOLATE, taps, ratio, (num, den), nchan, fmt, device,
                             profiling)


class RationalResampler(Resampler):
    """A rational up / down resampler (include/sxfir_rational.h): up outputs for every down inputs in one pass -- sample m * down
    of the x up interpolator's output, bit for bit.  `taps`: real, ntaps a multiple of up (design_rational(up, down)); up and down
    coprime, 2..4096 each; CF32 or CF16.  The plan is an interpolator plan of ratio `up` in its history and contract; call,
    outputs_for, position, contract, geometry, set_kernel, set_history_ptr, set_position and close are Resampler's."""

    def __init__(self, taps, up, down, nchan=1, fmt="CF32", device=0, profiling=False):
        self._lib = load_sxfir(profiling)
        self.profiling = bool(profiling)
        self._plan = C.c_void_p()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.mode, self.ratio, self.nchan, self.fmt, self.ntaps = INTERPOLATE, int(up), int(nchan), _FMT[fmt], taps.size
        self._ck(self._lib.sxfir_create_rational(C.byref(self._plan), taps.ctypes.data_as(C.c_void_p), taps.size, int(up), int(down),
                                                 int(nchan), self.fmt, int(device)))

    def _ratio(self):
        u, d = C.c_int(), C.c_int()
        self._ck(self._lib.sxfir_plan_rational(self._plan, C.byref(u), C.byref(d)))
        return u.value, d.value

    @property
    def up(self):
        return self._ratio()[0]

    @property
    def down(self):
        return self._ratio()[1]

    def process_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, stream=0):
        n_out = C.c_size_t()
        self._ck(self._lib.sxfir_resample(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride,
                                          C.byref(n_out), C.c_void_p(stream)))
        return n_out.value

    def time_resample_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, iters, stream=0):
        """Mean milliseconds of `iters` back-to-back launches of the resampling kernel (sxfir_time_resample); position and
        history are left alone."""
        ms = C.c_float()
        self._ck(self._lib.sxfir_time_resample(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride, iters,
                                               C.c_void_p(stream), C.byref(ms)))
        return ms.value

    time_passes_ptr = time_resample_ptr


def design_arbitrary(nphases, taps_per_phase=32, rate=1.0, beta=8.0):
    """Unit-gain taps of ArbitraryResampler(taps, nphases, rate=rate): the low-pass of the narrower side at the x nphases raster,
    design_lowpass(nphases * taps_per_phase, ceil(nphases * max(1, 1 / rate)), beta, nphases).  `rate` is out / in."""
    import math
    P = int(nphases)
    return design_lowpass(P * int(taps_per_phase), int(math.ceil(P * max(1.0, 1.0 / float(rate)))), beta, float(P))


class ArbitraryResampler(Resampler):
    """An arbitrary-rate resampler (include/sxfir_arbitrary.h): a polyphase bank of `nphases` phases with linear interpolation between
    adjacent phases, at a 64.32 fixed-point time that advances by `step` input samples (unsigned Q32.32, 2^28 .. 2^36) per output.
    Give `rate` (out / in: step = round(2^32 / rate)) or `step`.  `taps`: real, ntaps a multiple of nphases
    (design_arbitrary(nphases, rate=rate)); CF32 or CF16.  set_rate() changes the step in mid-stream, the time of the next output stays.
    The plan is an interpolator plan of ratio `nphases` in its history and contract; outputs_for, position, contract, geometry,
    set_kernel, set_history_ptr, set_position, reset and close are Resampler's."""

    def __init__(self, taps, nphases, rate=None, step=None, nchan=1, fmt="CF32", device=0, profiling=False):
        if (rate is None) == (step is None):
            raise ValueError("give rate (out / in) or step (input samples per output, Q32.32), not both")
        self._lib = load_sxfir(profiling)
        self.profiling = bool(profiling)
        self._plan = C.c_void_p()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.mode, self.ratio, self.nchan, self.fmt, self.ntaps = INTERPOLATE, int(nphases), int(nchan), _FMT[fmt], taps.size
        self._ck(self._lib.sxfir_create_arbitrary(C.byref(self._plan), taps.ctypes.data_as(C.c_void_p), taps.size, int(nphases),
                                                  self._step_of(rate, step), int(nchan), self.fmt, int(device)))

    @staticmethod
    def _step_of(rate, step):
        from fractions import Fraction
        if step is not None:
            return int(step)
        if not rate > 0:
            raise ValueError("rate must be positive")
        return int(round(Fraction(1 << 32) / Fraction(rate)))

    def _state(self):
        n, s, ti, tf = C.c_int(), C.c_uint64(), C.c_int64(), C.c_uint32()
        self._ck(self._lib.sxfir_plan_arbitrary(self._plan, C.byref(n), C.byref(s), C.byref(ti), C.byref(tf)))
        return n.value, s.value, ti.value, tf.value

    @property
    def nphases(self):
        return self._state()[0]

    @property
    def step(self):
        """Input samples per output sample, unsigned Q32.32."""
        return self._state()[1]

    @property
    def time(self):
        """(t_index, t_frac): the time of the next output, whole input samples and the fraction in units of 2^-32."""
        return self._state()[2:]

    def set_rate(self, rate=None, step=None):
        """The rate (out / in) or step of the outputs from now on (sxfir_set_rate); the time of the next output stays."""
        if (rate is None) == (step is None):
            raise ValueError("give rate or step, not both")
        self._ck(self._lib.sxfir_set_rate(self._plan, self._step_of(rate, step)))

    def set_time(self, consumed, t_index, t_frac=0):
        """Place the stream exactly (sxfir_set_time): `consumed` inputs taken, the next output at t_index + t_frac * 2^-32."""
        self._ck(self._lib.sxfir_set_time(self._plan, int(consumed), int(t_index), int(t_frac)))

    def process_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, stream=0):
        n_out = C.c_size_t()
        self._ck(self._lib.sxfir_resample_arbitrary(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride,
                                                    C.byref(n_out), C.c_void_p(stream)))
        return n_out.value

    def time_resample_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, iters, stream=0):
        """Mean milliseconds of `iters` back-to-back launches of the resampling kernel (sxfir_time_resample_arbitrary); position,
        time and history are left alone."""
        ms = C.c_float()
        self._ck(self._lib.sxfir_time_resample_arbitrary(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr),
                                                         out_stride, iters, C.c_void_p(stream), C.byref(ms)))
        return ms.value

    time_passes_ptr = time_resample_ptr


class _BandPlan(_Plan):
    """What Channelizer and Synthesizer share: the constructor (a critically sampled plan through the first creator, an oversampled
    one through the second) and the plan's own band count and oversampling factor."""

    _mode = None
    _create = (None, None)      # sxfir_create_<what>, sxfir_create_<what>_os
    _query = (None, None)       # the queries behind `bands` and `oversampling`

    def __init__(self, taps, nbands=4, nchan=1, fmt="CF32", device=-1, oversample=1):
        self._lib = load_sxfir()
        self._plan = C.c_void_p()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        nbands, oversample = int(nbands), int(oversample)
        self.mode, self.nbands, self.nchan, self.fmt, self.ntaps = self._mode, nbands, int(nchan), _FMT[fmt], taps.size
        head = (C.byref(self._plan), taps.ctypes.data_as(C.c_void_p), taps.size, nbands)
        if oversample == 1:
            self.ratio = nbands
            self._ck(getattr(self._lib, self._create[0])(*head, int(nchan), self.fmt, int(device)))
        else:
            self.ratio = nbands // oversample if oversample > 0 else 0
            self._ck(getattr(self._lib, self._create[1])(*head, oversample, int(nchan), self.fmt, int(device)))

    def _answer(self, query):
        n = C.c_int()
        self._ck(getattr(self._lib, query)(self._plan, C.byref(n)))
        return n.value

    @property
    def bands(self):
        """The plan's own band count (sxfir_plan_bands / sxfir_plan_synthesis_bands)."""
        return self._answer(self._query[0])

    @property
    def oversampling(self):
        """1 for the critically sampled plan, 2 for the oversampled one (sxfir_plan_oversampling / sxfir_plan_synthesis_oversampling)."""
        return self._answer(self._query[1])


class Channelizer(_BandPlan):
    """The 4-band channelizer (include/sxfir_channelizer.h): all `nbands` sub-bands of the /nbands raster out of one wideband
    stream in one pass.  `taps`: the REAL prototype low-pass (design_lowpass(ntaps, nbands)); band k is the band that
    design_bandpass(ntaps, nbands, k, nbands) centres, at 0 Hz of its output.  Stream state, contract, geometry and kernel
    choice are a /nbands decimator's: the same methods as Resampler.

    `oversample=2` (include/sxfir_channelizer_os.h): the same bands and centres, each leaving at fs/2 instead of fs/4 -- alias-free
    across its whole width.  Even-time outputs have the bits of the critically sampled plan's; the plan is a /(nbands // oversample)
    decimator in everything about the stream."""

    _mode = DECIMATE
    _create = ("sxfir_create_channelizer", "sxfir_create_channelizer_os")
    _query = ("sxfir_plan_bands", "sxfir_plan_oversampling")

    def process_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, band_stride, stream=0):
        """sxfir_channelize: band k of channel c starts at out_ptr + c * out_stride + k * band_stride (samples of the output
        format); returns the outputs PER BAND."""
        n_out = C.c_size_t()
        self._ck(self._lib.sxfir_channelize(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride,
                                            band_stride, C.byref(n_out), C.c_void_p(stream)))
        return n_out.value

    def process(self, x, out=None):
        """x: CUDA tensor [nchan, n] or [n]; complex64 (CF32), int32 words (CF16: half pairs) or int32 wire words [.., n, 2]
        (S32, complex64 out).  Returns [nbands, n_out], or [nchan, nbands, n_out] for a 2-D x.  A caller-given `out` of that
        shape (or longer rows) supplies its own channel and band strides."""
        import torch
        if self.fmt == S32:
            x = torch.view_as_complex(x.view(torch.float32))               # same 8 bytes per sample
        out_dtype = torch.complex64 if self.fmt == S32 else x.dtype
        squeeze = x.dim() == 1
        x2 = x.unsqueeze(0) if squeeze else x
        if x2.dim() != 2 or x2.shape[0] != self.nchan or (x2.shape[1] > 1 and x2.stride(1) != 1):
            raise ValueError("expected a [nchan=%d, n] tensor with unit sample stride" % self.nchan)
        n_in = x2.shape[1]
        n_out = self.outputs_for(n_in)
        if out is None:
            # rows of whole 16-byte units: an odd band stride would break the tiled kernel's store alignment
            q = 4 if self.fmt == CF16 else 2
            out = torch.empty((self.nchan, self.nbands, -(-n_out // q) * q), dtype=out_dtype, device=x2.device)
        o3 = out.unsqueeze(0) if out.dim() == 2 else out
        # the kernel writes through a raw pointer: a caller-supplied `out` must really hold the result
        if (o3.dim() != 3 or o3.shape[0] != self.nchan or o3.shape[1] != self.nbands or o3.shape[2] < n_out
                or (o3.shape[2] > 1 and o3.stride(2) != 1) or o3.dtype != out_dtype or o3.device != x2.device):
            raise ValueError("out must be a [nchan=%d, nbands=%d, >=%d] %s tensor with unit sample stride on %s" % (
                self.nchan, self.nbands, n_out, out_dtype, x2.device))
        got = self.process_ptr(x2.data_ptr(), n_in, x2.stride(0) if self.nchan > 1 else n_in, o3.data_ptr(),
                               o3.stride(0) if self.nchan > 1 else 0, max(o3.stride(1), n_out),
                               torch.cuda.current_stream(x2.device).cuda_stream)
        assert got == n_out
        res = o3[:, :, :n_out]
        return res[0] if squeeze else res


class TranslatingBank(_Plan):
    """A bank of frequency-translating decimators (include/sxfir_bank.h): K bands at any centres out of one wideband stream in one
    pass.  `taps`: complex [K, ntaps], band k's own (design_bandpass(ntaps, ratio, num_k, den_k), or anything else); `centres`: K
    (num, den) pairs.  Band k has the bits of TranslatingDecimator(taps[k], ratio, num_k, den_k) over the same stream.  One history
    and one position whatever K is: stream state, contract, geometry and kernel choice are a /ratio decimator's, the same methods
    as Resampler."""

    def __init__(self, taps, ratio, centres, nchan=1, fmt="CF32", device=-1):
        self._lib = load_sxfir()
        self._plan = C.c_void_p()
        taps = np.ascontiguousarray(taps, dtype=np.complex64)
        centres = [(int(n), int(d)) for n, d in centres]
        if taps.ndim != 2 or taps.shape[0] != len(centres):
            raise ValueError("taps must be [K, ntaps] complex, one row per centre (%d centres)" % len(centres))
        self.mode, self.ratio, self.nchan, self.fmt, self.ntaps = DECIMATE, int(ratio), int(nchan), _FMT[fmt], taps.shape[1]
        num = (C.c_int * max(len(centres), 1))(*[n for n, _ in centres])
        den = (C.c_int * max(len(centres), 1))(*[d for _, d in centres])
        self._ck(self._lib.sxfir_create_bank(C.byref(self._plan), taps.ctypes.data_as(C.c_void_p), taps.shape[1], int(ratio),
                                             len(centres), num, den, int(nchan), self.fmt, int(device)))

    @property
    def nbands(self):
        """The band count K (sxfir_plan_bank)."""
        n = C.c_int()
        self._ck(self._lib.sxfir_plan_bank(self._plan, C.byref(n)))
        return n.value

    @property
    def centres(self):
        """The K (num mod den, den) pairs (sxfir_plan_bank_band)."""
        out = []
        for k in range(self.nbands):
            n, d = C.c_int(), C.c_int()
            self._ck(self._lib.sxfir_plan_bank_band(self._plan, k, C.byref(n), C.byref(d)))
            out.append((n.value, d.value))
        return out

    @property
    def complex_taps(self):
        f = C.c_int()
        self._ck(self._lib.sxfir_taps_are_complex(self._plan, C.byref(f)))
        return bool(f.value)

    def process_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, band_stride, stream=0):
        """sxfir_decimate_bank: band k of channel c starts at out_ptr + c * out_stride + k * band_stride (samples of the output
        format); returns the outputs PER BAND."""
        n_out = C.c_size_t()
        self._ck(self._lib.sxfir_decimate_bank(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride,
                                               band_stride, C.byref(n_out), C.c_void_p(stream)))
        return n_out.value

    def time_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride, band_stride, iters, stream=0):
        """Mean milliseconds of `iters` back-to-back launches of the call's kernel (sxfir_time_decimate_bank); the state is left alone."""
        ms = C.c_float()
        self._ck(self._lib.sxfir_time_decimate_bank(self._plan, C.c_void_p(in_ptr), n_in, in_stride, C.c_void_p(out_ptr), out_stride,
                                                    band_stride, iters, C.c_void_p(stream), C.byref(ms)))
        return ms.value

    def process(self, x, out=None):
        """x: CUDA tensor [nchan, n] or [n]; complex64 (CF32), int32 words (CF16: half pairs) or int32 wire words [.., n, 2]
        (S32, complex64 out).  Returns [K, n_out], or [nchan, K, n_out] for a 2-D x.  A caller-given `out` of that shape (or
        longer rows) supplies its own channel and band strides."""
        import torch
        if self.fmt == S32:
            x = torch.view_as_complex(x.view(torch.float32))               # same 8 bytes per sample
        out_dtype = torch.complex64 if self.fmt == S32 else x.dtype
        squeeze = x.dim() == 1
        x2 = x.unsqueeze(0) if squeeze else x
        if x2.dim() != 2 or x2.shape[0] != self.nchan or (x2.shape[1] > 1 and x2.stride(1) != 1):
            raise ValueError("expected a [nchan=%d, n] tensor with unit sample stride" % self.nchan)
        K = self.nbands
        n_in = x2.shape[1]
        n_out = self.outputs_for(n_in)
        if out is None:
            # rows of whole 16-byte units: an odd band stride would break the tiled kernel's store alignment
            q = 4 if self.fmt == CF16 else 2
            out = torch.empty((self.nchan, K, -(-n_out // q) * q), dtype=out_dtype, device=x2.device)
        o3 = out.unsqueeze(0) if out.dim() == 2 else out
        # the kernel writes through a raw pointer: a caller-supplied `out` must really hold the result
        if (o3.dim() != 3 or o3.shape[0] != self.nchan or o3.shape[1] != K or o3.shape[2] < n_out
                or (o3.shape[2] > 1 and o3.stride(2) != 1) or o3.dtype != out_dtype or o3.device != x2.device):
            raise ValueError("out must be a [nchan=%d, K=%d, >=%d] %s tensor with unit sample stride on %s" % (
                self.nchan, K, n_out, out_dtype, x2.device))
        got = self.process_ptr(x2.data_ptr(), n_in, x2.stride(0) if self.nchan > 1 else n_in, o3.data_ptr(),
                               o3.stride(0) if self.nchan > 1 else 0, max(o3.stride(1), n_out),
                               torch.cuda.current_stream(x2.device).cuda_stream)
        assert got == n_out
        res = o3[:, :, :n_out]
        return res[0] if squeeze else res


class TranslatingCombiner(_Plan):
    """A bank of frequency-translating interpolators (include/sxfir_bank_tx.h), TranslatingBank's way back: K base-band streams, each
    turned to its own centre and interpolated x ratio with its own complex taps, summed into one wideband stream in one pass.
    `taps`: complex [K, ntaps], band k's own; `centres`: K (num, den) pairs.  The output is the float32 sum, in band order, of
    TranslatingInterpolator(taps[k], ratio, num_k, den_k) over band k's stream; with K = 1 it has that plan's bits.  One position and
    a history per band inside the plan: stream state, contract, geometry and kernel choice are a x ratio interpolator's, the same
    methods as Resampler (set_history_ptr is refused)."""

    def __init__(self, taps, ratio, centres, nchan=1, fmt="CF32", device=0):
        self._lib = load_sxfir()
        self._plan = C.c_void_p()
        taps = np.ascontiguousarray(taps, dtype=np.complex64)
        centres = [(int(n), int(d)) for n, d in centres]
        if taps.ndim != 2 or taps.shape[0] != len(centres):
            raise ValueError("taps must be [K, ntaps] complex, one row per centre (%d centres)" % len(centres))
        self.mode, self.ratio, self.nchan, self.fmt, self.ntaps = INTERPOLATE, int(ratio), int(nchan), _FMT[fmt], taps.shape[1]
        num = (C.c_int * max(len(centres), 1))(*[n for n, _ in centres])
        den = (C.c_int * max(len(centres), 1))(*[d for _, d in centres])
        self._ck(self._lib.sxfir_create_bank_interpolator(C.byref(self._plan), taps.ctypes.data_as(C.c_void_p), taps.shape[1],
                                                          int(ratio), len(centres), num, den, int(nchan), self.fmt, int(device)))

    @property
    def nbands(self):
        """The band count K (sxfir_plan_bank_tx)."""
        n = C.c_int()
        self._ck(self._lib.sxfir_plan_bank_tx(self._plan, C.byref(n)))
        return n.value

    @property
    def centres(self):
        """The K (num mod den, den) pairs (sxfir_plan_bank_tx_band)."""
        out = []
        for k in range(self.nbands):
            n, d = C.c_int(), C.c_int()
            self._ck(self._lib.sxfir_plan_bank_tx_band(self._plan, k, C.byref(n), C.byref(d)))
            out.append((n.value, d.value))
        return out

    @property
    def complex_taps(self):
        f = C.c_int()
        self._ck(self._lib.sxfir_taps_are_complex(self._plan, C.byref(f)))
        return bool(f.value)

    def set_tx_threshold(self, threshold2):
        self._ck(self._lib.sxfir_set_tx_threshold(self._plan, float(threshold2)))

    def process_ptr(self, in_ptr, n_in, in_stride, band_stride, out_ptr, out_stride, stream=0):
        """sxfir_interpolate_bank: band k of channel c is read at in_ptr + c * in_stride + k * band_stride (samples of the input
        format), n_in inputs PER BAND; returns the wideband outputs per channel (ratio x n_in)."""
        n_out = C.c_size_t()
        self._ck(self._lib.sxfir_interpolate_bank(self._plan, C.c_void_p(in_ptr), n_in, in_stride, band_stride, C.c_void_p(out_ptr),
                                                  out_stride, C.byref(n_out), C.c_void_p(stream)))
        return n_out.value

    def time_ptr(self, in_ptr, n_in, in_stride, band_stride, out_ptr, out_stride, iters, stream=0):
        """Mean milliseconds of `iters` back-to-back launches of the call's kernel (sxfir_time_interpolate_bank); the state is left alone."""
        ms = C.c_float()
        self._ck(self._lib.sxfir_time_interpolate_bank(self._plan, C.c_void_p(in_ptr), n_in, in_stride, band_stride, C.c_void_p(out_ptr),
                                                       out_stride, iters, C.c_void_p(stream), C.byref(ms)))
        return ms.value

    def process(self, x, out=None):
        """x: CUDA tensor [K, n] or [nchan, K, n], possibly strided between bands and channels; complex64 (CF32 and S32 plans) or
        int32 words (CF16: half pairs).  Returns [ratio * n], or [nchan, ratio * n] for a 3-D x: complex64, int32 words (CF16) or
        int32 wire words [.., ratio * n, 2] (S32).  A caller-given `out` of that shape (or longer rows) supplies its own channel
        stride."""
        import torch
        K = self.nbands
        squeeze = x.dim() == 2
        x3 = x.unsqueeze(0) if squeeze else x
        if x3.dim() != 3 or x3.shape[0] != self.nchan or x3.shape[1] != K or (x3.shape[2] > 1 and x3.stride(2) != 1):
            raise ValueError("expected a [nchan=%d, K=%d, n] tensor with unit sample stride" % (self.nchan, K))
        n_in = x3.shape[2]
        n_out = self.outputs_for(n_in)
        if self.fmt == S32 and out is not None:
            out = torch.view_as_complex(out.view(torch.float32))          # same 8 bytes per sample
        if out is None:
            out = torch.empty((self.nchan, n_out), dtype=x3.dtype, device=x3.device)
        o2 = out.unsqueeze(0) if out.dim() == 1 else out
        # the kernel writes through a raw pointer: a caller-supplied `out` must really hold the result
        if (o2.dim() != 2 or o2.shape[0] != self.nchan or o2.shape[1] < n_out or (o2.shape[1] > 1 and o2.stride(1) != 1)
                or o2.dtype != x3.dtype or o2.device != x3.device):
            raise ValueError("out must be a [nchan=%d, >=%d] %s tensor with unit sample stride on %s" % (self.nchan, n_out, x3.dtype, x3.device))
        got = self.process_ptr(x3.data_ptr(), n_in, x3.stride(0) if self.nchan > 1 else 0, max(x3.stride(1), n_in) if K > 1 else n_in,
                               o2.data_ptr(), o2.stride(0) if self.nchan > 1 else max(n_out, 1),
                               torch.cuda.current_stream(x3.device).cuda_stream)
        assert got == n_out
        res = o2[:, :n_out]
        if self.fmt == S32:
            res = torch.view_as_real(res).view(torch.int32)
        return res[0] if squeeze else res


class Synthesizer(_BandPlan):
    """The 4-band synthesizer (include/sxfir_synthesizer.h): `nbands` sub-bands of the x nbands raster into one wideband stream in one
    pass -- what Channelizer takes apart, put together.  `taps`: the REAL prototype low-pass of a x nbands interpolator
    (design_lowpass(ntaps, nbands, gain=nbands)); band k lands at k / nbands cycles per output sample.  Stream state, contract,
    geometry and kernel choice are a x nbands interpolator's: the same methods as Resampler (set_history_ptr is refused).

    `oversample=2` (include/sxfir_synthesizer_os.h): the bands arrive at fs/2 each instead of fs/4 -- what
    Channelizer(..., oversample=2) hands out -- and the prototype is a x2 interpolator's with the /4 band edge
    (design_lowpass(ntaps, nbands, gain=2)); the plan is a x(nbands // oversample) interpolator in everything about the stream."""

    _mode = INTERPOLATE
    _create = ("sxfir_create_synthesizer", "sxfir_create_synthesizer_os")
    _query = ("sxfir_plan_synthesis_bands", "sxfir_plan_synthesis_oversampling")

    def set_tx_threshold(self, threshold2):
        self._ck(self._lib.sxfir_set_tx_threshold(self._plan, float(threshold2)))

    def process_ptr(self, in_ptr, n_in, in_stride, band_stride, out_ptr, out_stride, stream=0):
        """sxfir_synthesize: band k of channel c is read at in_ptr + c * in_stride + k * band_stride (samples of the input format),
        n_in inputs PER BAND; returns the wideband outputs per channel (ratio x n_in)."""
        n_out = C.c_size_t()
        self._ck(self._lib.sxfir_synthesize(self._plan, C.c_void_p(in_ptr), n_in, in_stride, band_stride, C.c_void_p(out_ptr), out_stride,
                                            C.byref(n_out), C.c_void_p(stream)))
        return n_out.value

    def process(self, x, out=None):
        """x: CUDA tensor [nbands, n] or [nchan, nbands, n], possibly strided between bands and channels; complex64 (CF32 and S32
        plans) or int32 words (CF16: half pairs).  Returns [ratio * n], or [nchan, ratio * n] for a 3-D x: complex64, int32 words
        (CF16) or int32 wire words [.., ratio * n, 2] (S32).  A caller-given `out` of that shape (or longer rows) supplies its own
        channel stride."""
        import torch
        squeeze = x.dim() == 2
        x3 = x.unsqueeze(0) if squeeze else x
        if x3.dim() != 3 or x3.shape[0] != self.nchan or x3.shape[1] != self.nbands or (x3.shape[2] > 1 and x3.stride(2) != 1):
            raise ValueError("expected a [nchan=%d, nbands=%d, n] tensor with unit sample stride" % (self.nchan, self.nbands))
        n_in = x3.shape[2]
        n_out = self.outputs_for(n_in)
        if self.fmt == S32 and out is not None:
            out = torch.view_as_complex(out.view(torch.float32))          # same 8 bytes per sample
        if out is None:
            out = torch.empty((self.nchan, n_out), dtype=x3.dtype, device=x3.device)
        o2 = out.unsqueeze(0) if out.dim() == 1 else out
        # the kernel writes through a raw pointer: a caller-supplied `out` must really hold the result
        if (o2.dim() != 2 or o2.shape[0] != self.nchan or o2.shape[1] < n_out or (o2.shape[1] > 1 and o2.stride(1) != 1)
                or o2.dtype != x3.dtype or o2.device != x3.device):
            raise ValueError("out must be a [nchan=%d, >=%d] %s tensor with unit sample stride on %s" % (self.nchan, n_out, x3.dtype, x3.device))
        got = self.process_ptr(x3.data_ptr(), n_in, x3.stride(0) if self.nchan > 1 else 0, max(x3.stride(1), n_in), o2.data_ptr(),
                               o2.stride(0) if self.nchan > 1 else max(n_out, 1), torch.cuda.current_stream(x3.device).cuda_stream)
        assert got == n_out
        res = o2[:, :n_out]
        if self.fmt == S32:
            res = torch.view_as_real(res).view(torch.int32)
        return res[0] if squeeze else res


class PipelinedResampler:
    """Consecutive blocks of ONE stream on `depth` plans and `depth` HIP streams in turn, so that their passes
    overlap on the GPU.  Block k+1 needs nothing of block k but the tail of its INPUT, which is in device memory
    before either pass runs: each plan's filter state is seeded from there (sxfir_set_history) and the passes are
    independent launches.  Each plan is also told where in the stream its block starts (sxfir_set_position), so
    blocks need not be multiples of the ratio: the outputs, their count and their positions are those of one plan
    fed block by block.  (On one GPU this buys nothing once every block is new data -- LABBOOK.md 7 -- it is the way
    to split one stream over plans or GPUs.)

    Ordering: every pass waits (on the GPU) for the work the CALLER's current torch stream had queued when
    process_ptr was called -- the kernels that produced the block -- and nothing else.  The caller keeps every input
    block unchanged until the pass over the NEXT block has run (join() waits for all)."""

    def __init__(self, mode, taps, ratio, nchan=1, fmt="CF32", device=-1, depth=4):
        import torch
        self.depth = int(depth)
        self.plans = [Resampler(mode, taps, ratio, nchan=nchan, fmt=fmt, device=device) for _ in range(self.depth)]
        self.streams = [torch.cuda.Stream(device=None if device < 0 else device) for _ in range(self.depth)]
        self._k = 0
        self._prev = None                                   # (ptr, n, stride) of the previous input block
        self._consumed = 0                                  # input samples of the stream before the next block

    @property
    def contract(self):
        return self.plans[0].contract

    def restart(self):
        """The next block is the first of a new stream (zero history, position 0)."""
        self._prev = None
        self._consumed = 0

    def process_ptr(self, in_ptr, n_in, in_stride, out_ptr, out_stride):
        """Queue the pass over one block; returns its output count.  Asynchronous: join() before using outputs."""
        import torch
        k = self._k % self.depth
        plan, st = self.plans[k], self.streams[k].cuda_stream
        # the block (and the previous one, whose tail is the history) was produced on the caller's stream
        self.streams[k].wait_stream(torch.cuda.current_stream(self.streams[k].device))
        if self._prev is None:
            plan.reset(st)
        else:
            # (a previous block shorter than the filter history is refused by sxfir_set_history: SXFIR_EINVAL)
            plan.set_history_ptr(self._prev[0], self._prev[1], self._prev[2], st)
        plan.set_position(self._consumed)
        n_out = plan.process_ptr(in_ptr, n_in, in_stride, out_ptr, out_stride, st)
        self._prev = (in_ptr, n_in, in_stride)
        self._consumed += n_in
        self._k += 1
        return n_out

    def join(self):
        for s in self.streams:
            s.synchronize()
