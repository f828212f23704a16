"""The 4-band synthesizer on the GPU (include/sxfir_synthesizer.h), bit for bit against the oracle as it stands.

The reference value is always built the same way: v_r by the header's radix-2 butterflies in float32 numpy, one rounding
per operation; then output phase r of oracle.interp_f32(h, 4, v_r, jsplit) -- the real-tap interpolator under the contract the plan
reports, applied to the stream v_r -- for r = 0..3, interleaved."""
import ctypes as C
import functools

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_lowpass
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE, KERNEL_GENERIC, KERNEL_TILED
from gpu_util import OUT_FILL, assert_bit_exact, band_proto, four_band_source, random_taps, run, syn_ref, to_cpu, to_gpu
from test_synthesizer_host import band_tone, tone_and_rest, wideband_tone

pytestmark = pytest.mark.gpu

SEED = 0x5E7A11
T = 256                                                     # inputs per band of a tile
TILED, GENERIC = "synthesis4_kernel", "synthesis_generic_kernel"
source = functools.partial(four_band_source, seed=SEED)


@pytest.fixture(scope="module")
def proto():
    return band_proto(gain=4.0)


@pytest.mark.parametrize("which", ["lowpass", "random"])
def test_tiled_4x128(oracle, proto, which):
    """1. One call of 3 tiles plus a ragged tail through synthesis4_kernel."""
    h = proto if which == "lowpass" else random_taps(128)
    assert which == "lowpass" or not np.array_equal(h, h[::-1])
    n = 3 * T + 37
    xg, xs = source(oracle, 0, n)
    plan = sxxcvr_amd.Synthesizer(h)
    assert plan.bands == 4 and tuple(plan.contract) == (2, 1) and plan.contract.rot == 0
    plan.set_kernel(KERNEL_TILED)
    g = plan.geometry(n)
    assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == 4 and g["tile_samples"] == 1024, g
    y = run(plan, xg)
    assert y.shape == (4 * n,)
    assert_bit_exact(y, syn_ref(oracle, h, xs, plan.contract[0]), "tiled 4 x 128 (%s)" % which)
    assert plan.position == (n, 4 * n)


def test_streaming_and_history(oracle, proto):
    """2. Five calls on one plan (the second shorter than the 32-sample history, one of a single input) give the bits of one pass."""
    import torch
    blocks = [2 * T, 31, T + 5, 1, T]
    n = sum(blocks)
    xg, xs = source(oracle, 4, n)
    plan = sxxcvr_amd.Synthesizer(proto)
    ref = syn_ref(oracle, proto, xs, plan.contract[0])
    outs, pos = [], 0
    for b in blocks:
        assert plan.geometry(b)["kernel"] == TILED
        outs.append(plan.process(xg[:, pos:pos + b]))       # (a view: the band stride is the whole buffer's)
        pos += b
    torch.cuda.synchronize()
    assert_bit_exact(np.concatenate([to_cpu(o) for o in outs]), ref, "streaming %r" % blocks)
    assert plan.position == (n, 4 * n)
    plan.reset()
    assert plan.position == (0, 0)
    assert_bit_exact(run(plan, xg[:, :blocks[0]]), to_cpu(outs[0]), "after reset")


@pytest.mark.parametrize("nesting", ["bands inside channels", "channels inside bands"])
def test_channels_and_strides(oracle, proto, nesting):
    """3. Three channels, every stride larger than needed (and odd on the input, which the tiled loads do not mind), a distinct source
    per band and channel; nothing between or behind the channels of the output is written."""
    import torch
    nchan, n = 3, 2 * T + 11
    if nesting == "bands inside channels":
        sband = n + 25
        sin = 3 * sband + n + 40
        total = nchan * sin
    else:
        sin = n + 25
        sband = (nchan - 1) * sin + n + 40
        total = 4 * sband
    xbuf = torch.zeros(total, dtype=torch.complex64, device="cuda")
    x = torch.as_strided(xbuf, (nchan, 4, n), (sin, sband, 1))
    for c in range(nchan):
        sxxcvr_amd.synth_fill(x[c], SEED, 10 + 4 * c, 0)
    sout = 4 * n + 34                           # (an even stride: the tiled kernel's 16-byte stores)
    assert sout % 2 == 0 and OUT_FILL < 1 << 31
    ybuf = torch.full((nchan + 1, 2 * sout), OUT_FILL, dtype=torch.int32, device="cuda")
    yc = torch.view_as_complex(ybuf.view(torch.float32).view(nchan + 1, sout, 2))
    plan = sxxcvr_amd.Synthesizer(proto, nchan=nchan)
    plan.set_kernel(KERNEL_TILED)
    assert plan.geometry(n)["kernel"] == TILED
    y = plan.process(x, out=yc[:nchan])
    torch.cuda.synchronize()
    assert y.shape == (nchan, 4 * n)
    words = to_cpu(ybuf).view(np.uint32).reshape(nchan + 1, sout, 2)
    for c in range(nchan):
        xs = np.stack([oracle.synth_iq(SEED, 10 + 4 * c + k, 0, n) for k in range(4)])
        got = words[c, :4 * n].copy().view(np.complex64).ravel()
        assert_bit_exact(got, syn_ref(oracle, proto, xs, 2), "channel %d (%s)" % (c, nesting))
    assert np.all(words[:nchan, 4 * n:] == OUT_FILL), "the padding between the channels was written"
    assert np.all(words[nchan] == OUT_FILL), "something was written behind the last channel"


def test_alignment(oracle, proto):
    """4. The tiled kernel stores 16 bytes at a time: an output pointer offset by one sample runs the generic kernel under AUTO (same
    bits, nothing outside written) and answers -4 under a forced TILED.  Its LOADS are indifferent to 8-byte alignment -- LDS-DMA
    sources need no 16-byte alignment on gfx950 (the other tiled kernels of this library rely on it: sxfir_launch.hip.h), and the
    edge tiles load 8 bytes at a time -- so an input pointer offset by one sample and an odd band stride stay with the tiled kernel:
    they run under a forced TILED, with the reference's bits."""
    import torch
    n = 2 * T + 9
    xg, xs = source(oracle, 30, n)
    plan = sxxcvr_amd.Synthesizer(proto)
    ref = syn_ref(oracle, proto, xs, plan.contract[0])
    # (a) output offset by one sample (8 bytes: not 16-byte aligned)
    buf = torch.zeros(4 * n + 3, dtype=torch.complex64, device="cuda")
    out = buf[1:1 + 4 * n + 1]
    assert out.data_ptr() % 16 == 8
    assert plan.geometry(n)["kernel"] == TILED          # (the geometry query assumes an aligned output: the call decides)
    plan.process(xg, out=out)
    torch.cuda.synchronize()
    assert_bit_exact(to_cpu(out)[:4 * n], ref, "misaligned output")
    assert to_cpu(buf[:1]).view(np.uint64)[0] == 0, "something was written in front of the output"
    assert np.all(to_cpu(buf[1 + 4 * n:]).view(np.uint64) == 0), "something was written behind the output"
    plan.set_kernel(KERNEL_TILED)
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.process(xg, out=out)
    assert ei.value.code == -4 and plan.position == (n, 4 * n)
    # (b) input offset by one sample, (c) an odd band stride: the tiled kernel, forced
    for what, sband in (("input offset by one sample", n + 1), ("odd band stride", n + 2 if n % 2 else n + 1)):
        xbuf = torch.zeros(4 * sband + 2, dtype=torch.complex64, device="cuda")
        off = 1 if what.startswith("input") else 0
        if off == 0:
            assert sband % 2 == 1 and xbuf.data_ptr() % 16 == 0
        x = torch.as_strided(xbuf, (4, n), (sband, 1), off)
        assert off == 0 or x.data_ptr() % 16 == 8
        x.copy_(xg)
        fresh = sxxcvr_amd.Synthesizer(proto)
        fresh.set_kernel(KERNEL_TILED)
        assert_bit_exact(run(fresh, x), ref, what)


def test_more_tiles_than_resident_workgroups(oracle, proto):
    """5. resident + 3 tiles: a call this small is dealt as ONE generation of waves, so the grid is the chip's resident waves, a
    multiple of 8 -- the XCD-blocked dealing -- and three waves walk on to a second tile."""
    plan = sxxcvr_amd.Synthesizer(proto)
    plan.set_kernel(KERNEL_TILED)
    resident = plan.geometry(T)["resident"]
    n = (resident + 3) * T
    g = plan.geometry(n)
    assert g["kernel"] == TILED and g["n_tiles"] == resident + 3 and g["workgroups"] == resident and resident % 8 == 0, g
    xg, xs = source(oracle, 40, n)
    y = run(plan, xg)
    assert_bit_exact(y, syn_ref(oracle, proto, xs, plan.contract[0], threads=oracle.max_threads()), "resident + 3 tiles")


@pytest.mark.parametrize("ntaps", [64, 40])
def test_generic_tap_counts(oracle, ntaps):
    """6. Other tap counts on CF32: the generic kernel (40 taps: 10 per phase, jsplit 2)."""
    h = design_lowpass(64, 4, 8.0, 4.0) if ntaps == 64 else random_taps(40, 9)
    n = 4 * 175 + 3
    xg, xs = source(oracle, 50, n)
    plan = sxxcvr_amd.Synthesizer(h)
    assert tuple(plan.contract) == (2, 1) and plan.contract.rot == 0
    g = plan.geometry(n)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    assert_bit_exact(run(plan, xg), syn_ref(oracle, h, xs, 2), "generic 4 x %d" % ntaps)
    assert plan.position == (n, 4 * n)


def test_generic_cf16(oracle, proto):
    """6. CF16 in and out: inputs quantised to half, the result rounded to half once after the last sum."""
    import torch
    n = 4 * 175 + 3
    xs = np.stack([oracle.synth_iq(SEED, 60 + k, 0, n) for k in range(4)])
    x16 = torch.empty((4, n), dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(x16, SEED, 60, 0, fmt="CF16")
    plan = sxxcvr_amd.Synthesizer(proto, fmt="CF16")
    assert plan.geometry(n)["kernel"] == GENERIC
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    y16 = run(plan, x16)
    assert y16.shape == (4 * n,) and y16.dtype == np.int32
    h16 = oracle.f32_to_f16(xs.view(np.float32))
    assert np.array_equal(to_cpu(x16).view(np.uint16), h16), "CF16 synthetic source"
    xq = oracle.f16_to_f32(h16).view(np.complex64)
    ref = syn_ref(oracle, proto, xq, plan.contract[0])
    want = oracle.f32_to_f16(ref.view(np.float32))
    assert np.array_equal(np.ascontiguousarray(y16).view(np.uint16), want.ravel()), "CF16 output"


def test_generic_s32_words(oracle, proto):
    """6. S32 wire words out: convert_tx of the CF32 result, word for word.  The inputs are scaled by 2^-3 on both sides (exact), so
    that no output reaches convert_tx's saturating corner: asserted on the reference first."""
    import torch
    n = 4 * 175 + 3
    xg, xs = source(oracle, 70, n)
    torch.view_as_real(xg).mul_(0.125)
    xs = (xs.view(np.float32) * np.float32(0.125)).view(np.complex64)
    assert_bit_exact(to_cpu(xg).ravel(), xs.ravel(), "scaled source")
    plan = sxxcvr_amd.Synthesizer(proto, fmt="S32")
    plan.set_tx_threshold(1e-6)
    assert plan.geometry(n)["kernel"] == GENERIC
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    ref = syn_ref(oracle, proto, xs, plan.contract[0])
    assert max(np.abs(ref.real).max(), np.abs(ref.imag).max()) < 1.0
    y = run(plan, xg)
    assert y.shape == (4 * n, 2) and y.dtype == np.int32
    assert np.array_equal(y.ravel(), oracle.convert_tx(ref, 1e-6)), "S32 words out"


def test_tiled_equals_generic(oracle):
    """7. The same plan shape under KERNEL_TILED and KERNEL_GENERIC on 4 tiles."""
    h = random_taps(128, 21)
    xg, _ = source(oracle, 80, 4 * T)
    a = sxxcvr_amd.Synthesizer(h)
    a.set_kernel(KERNEL_TILED)
    b = sxxcvr_amd.Synthesizer(h)
    b.set_kernel(KERNEL_GENERIC)
    assert a.geometry(4 * T)["kernel"] == TILED and b.geometry(4 * T)["kernel"] == GENERIC
    assert_bit_exact(run(a, xg), run(b, xg), "tiled vs generic")


def test_places_the_band(proto):
    """8. Band 1 alone holds a tone 0.1 cycles per band sample: it lands at 1/4 + 0.1/4 = 11/40 cycles per output sample at 0 dB +-
    0.01 dB, and nothing else is above -80 dB anywhere -- the thresholds and margins test_takes_the_bands_apart
    (tests/test_gpu_channelizer.py) uses for this prototype.  The same pass in fp64 with the library's own designer
    (tests/test_synthesizer_host.py::test_fp64_figures_of_the_gpu_property_tests): +0.00024 dB, everything else below -104.8 dB (the
    image at 0.525).  The margin is for fp32 accumulation; the first 256 outputs (twice the filter's length) are dropped and the tone
    is on a bin of the remaining 65 280, so neither a transient nor leakage uses it."""
    x = band_tone()
    plan = sxxcvr_amd.Synthesizer(proto)
    assert plan.geometry(x.shape[1])["kernel"] == TILED
    w = run(plan, to_gpu(x.astype(np.complex64)))[256:].astype(np.complex128)
    assert w.size == 65280
    tone, rest, at = tone_and_rest(w, 17952)
    print("tone %.5f dB, rest %.1f dB at %.4f" % (tone, rest, at / w.size))
    assert abs(tone) <= 0.01
    assert rest <= -80.0


def test_loopback(proto):
    """9. Channelizer (gain-1 prototype), then Synthesizer (the same prototype with gain 4), on a tone 11/40 cycles per wideband
    sample: the tone comes back at 0 dB +- 0.01 dB and nothing else is above -80 dB.  In fp64: +0.00047 dB, rest -103.5 dB.  536
    outputs (both filters' transients) are dropped; the tone is on bin 17 875 of the remaining 65 000."""
    x = wideband_tone()
    chan = sxxcvr_amd.Channelizer(design_lowpass(128, 4))
    syn = sxxcvr_amd.Synthesizer(proto)
    assert chan.geometry(x.size)["kernel"] == "chan4_kernel" and syn.geometry(x.size // 4)["kernel"] == TILED
    w = run(syn, chan.process(to_gpu(x.astype(np.complex64))))[536:].astype(np.complex128)
    assert w.size == 65000
    tone, rest, at = tone_and_rest(w, 17875)
    print("tone %.5f dB, rest %.1f dB at %.4f" % (tone, rest, at / w.size))
    assert abs(tone) <= 0.01
    assert rest <= -80.0


def test_errors(oracle, proto):
    """10. The plan refuses every other pass's entry point (the message names sxfir_synthesize) and sxfir_set_history, is left
    untouched by that and goes on working; stride errors; the other plans report 0 synthesis bands and are refused."""
    import torch
    lib = sxxcvr_amd.load_sxfir()
    n = T
    xg, xs = source(oracle, 90, n)
    plan = sxxcvr_amd.Synthesizer(proto)
    y = torch.zeros(4 * n, dtype=torch.complex64, device="cuda")
    xp, yp, null = C.c_void_p(xg.data_ptr()), C.c_void_p(y.data_ptr()), None
    n_out = C.c_size_t(77)
    ms = C.c_float()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    refusals = [
        lambda: lib.sxfir_decimate(plan._plan, xp, n, n, yp, 4 * n, C.byref(n_out), null),
        lambda: lib.sxfir_interpolate(plan._plan, xp, n, n, yp, 4 * n, C.byref(n_out), null),
        lambda: lib.sxfir_interpolate_keyed(plan._plan, xp, n, n, yp, 4 * n, C.byref(n_out), 0, n, C.c_void_p(counter.data_ptr()), null),
        lambda: lib.sxfir_channelize(plan._plan, xp, n, n, yp, 0, n, C.byref(n_out), null),
        lambda: lib.sxfir_time_decimate(plan._plan, xp, n, n, yp, 4 * n, 1, null, C.byref(ms)),
        lambda: lib.sxfir_time_interpolate(plan._plan, xp, n, n, yp, 4 * n, 1, null, C.byref(ms)),
    ]
    for i, call in enumerate(refusals):
        n_out.value = 77
        assert call() == -1, i
        assert b"sxfir_synthesize" in lib.sxfir_last_error(), (i, lib.sxfir_last_error())
        assert i >= 4 or n_out.value == 0, i
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_history_ptr(xg.data_ptr(), n, n)
    assert ei.value.code == -4 and b"stride" in lib.sxfir_last_error()
    torch.cuda.synchronize()
    assert plan.position == (0, 0) and int(torch.count_nonzero(torch.view_as_real(y))) == 0 and int(counter[0]) == 0
    bad = [
        (xg.data_ptr(), n, 0, n - 1, y.data_ptr(), 0),          # band stride smaller than the inputs per band
        (0, n, 0, n, y.data_ptr(), 0),                          # NULL buffers
        (xg.data_ptr(), n, 0, n, 0, 0),
        (xg.data_ptr() + 4, n, 0, n, y.data_ptr(), 0),          # not aligned to one sample
        (xg.data_ptr(), n, 0, n, y.data_ptr() + 4, 0),
    ]
    for args in bad:
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            plan.process_ptr(*args)
        assert ei.value.code == -1 and plan.position == (0, 0), args
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(torch.view_as_real(y))) == 0
    assert_bit_exact(run(plan, xg, out=y), syn_ref(oracle, proto, xs, plan.contract[0]), "after the refused calls")
    # two channels: bands and channels that would overlap, an output stride smaller than the block
    two = sxxcvr_amd.Synthesizer(proto, nchan=2)
    x2 = torch.zeros((2, 4, n), dtype=torch.complex64, device="cuda")
    y2 = torch.zeros((2, 4 * n), dtype=torch.complex64, device="cuda")
    for in_stride, band_stride, out_stride in ((n, n, 4 * n), (2 * n, n, 4 * n), (n, 2 * n - 1, 4 * n), (4 * n, n, 4 * n - 1)):
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            two.process_ptr(x2.data_ptr(), n, in_stride, band_stride, y2.data_ptr(), out_stride)
        assert ei.value.code == -1 and two.position == (0, 0), (in_stride, band_stride, out_stride)
    assert two.process_ptr(x2.data_ptr(), n, 4 * n, n, y2.data_ptr(), 4 * n) == 4 * n          # bands inside channels
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Synthesizer(proto, nbands=2)
    assert ei.value.code == -4
    # what the plan is, and what the others are not
    assert plan.bands == 4
    nb, f = C.c_int(-1), C.c_int(-1)
    assert lib.sxfir_plan_bands(plan._plan, C.byref(nb)) == 0 and nb.value == 0          # (its documented meaning: channelizer bands)
    assert lib.sxfir_taps_are_complex(plan._plan, C.byref(f)) == 0 and f.value == 0
    real = sxxcvr_amd.Resampler(INTERPOLATE, proto, 4)
    chan = sxxcvr_amd.Channelizer(design_lowpass(128, 4))
    for other in (real, chan):
        nb.value = -1
        assert lib.sxfir_plan_synthesis_bands(other._plan, C.byref(nb)) == 0 and nb.value == 0
        n_out.value = 77
        assert lib.sxfir_synthesize(other._plan, xp, n, 0, n, yp, 0, C.byref(n_out), null) == -1 and n_out.value == 0
        assert other.position == (0, 0)
    torch.cuda.synchronize()
