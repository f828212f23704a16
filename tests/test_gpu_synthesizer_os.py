"""The 2x oversampled 4-band synthesizer on the GPU (include/sxfir_synthesizer_os.h), bit for bit against the oracle as it stands.

The reference value is always built the same way: v_r by the header's radix-2 butterflies in float32 numpy
(gpu_util.butterflies_f32), one rounding per operation; then oracle.interp_f32(h, 2, v_r, jsplit) -- the real-tap x2 interpolator
under the contract the plan reports, applied to the stream v_r -- for r = 0..3, and output n taken from run n & 3, n the ABSOLUTE
output index."""
import ctypes as C
import functools

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_lowpass
from sxxcvr_amd.resampler import INTERPOLATE, KERNEL_GENERIC, KERNEL_TILED
from gpu_util import OUT_FILL, assert_bit_exact, band_proto, four_band_source, random_taps, run, syn_os_ref, to_cpu, to_gpu
from test_channelizer_os_host import edge_tone
from test_synthesizer_host import band_tone, spectrum_db, tone_and_rest
from test_synthesizer_os_host import (BAND_TONE_BIN, BAND_TONE_DB, BAND_TONE_DROP, BAND_TONE_KEEP, BAND_TONE_N, CRIT_IMAGE_BIN,
                                      CRIT_IMAGE_DB, LOOP_BIN, LOOP_DROP, LOOP_KEEP, LOOP_TONE_DB)

pytestmark = pytest.mark.gpu

SEED = 0x5E7A12
T = 512                                                     # inputs per band of a tile (outputs: 2 T)
HIST = 64                                                   # a band's history: ntaps / 2
TILED, GENERIC = "synthesis4x2_kernel", "synthesis_os_generic_kernel"
source = functools.partial(four_band_source, seed=SEED)


def os_plan(h, **kw):
    return sxxcvr_amd.Synthesizer(h, oversample=2, **kw)


@pytest.fixture(scope="module")
def proto():
    return band_proto(gain=2.0)


@pytest.mark.parametrize("which", ["lowpass", "random"])
def test_tiled_4x128(oracle, proto, which):
    """1. One call of 3 tiles plus a ragged 37 through synthesis4x2_kernel, forced."""
    h = proto if which == "lowpass" else random_taps(128)
    assert which == "lowpass" or not np.array_equal(h, h[::-1])
    n = 3 * T + 37
    xg, xs = source(oracle, 0, n)
    plan = os_plan(h)
    assert plan.bands == 4 and plan.oversampling == 2 and plan.ratio == 2
    assert tuple(plan.contract) == (2, 1) and plan.contract.rot == 0
    assert plan.outputs_for(n) == 2 * n
    plan.set_kernel(KERNEL_TILED)
    g = plan.geometry(n)
    assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == 4 and g["tile_samples"] == 2 * T, g
    y = run(plan, xg)
    assert y.shape == (2 * n,)
    assert_bit_exact(y, syn_os_ref(oracle, h, xs, plan.contract[0]), "tiled 4 x 128 (%s)" % which)
    assert plan.position == (n, 2 * n)


def test_streaming_and_history(oracle, proto):
    """2. Five calls on one plan -- one shorter than the 64-sample history, one of a single input, two that start at an odd
    per-band index -- all through the tiled kernel, give the bits of one pass; reset then reproduces the first block."""
    import torch
    blocks = [2 * T, 63, T + 5, 1, T]
    starts = np.cumsum([0] + blocks[:-1])
    assert blocks[1] < HIST and sum(int(s) & 1 for s in starts) == 2
    n = sum(blocks)
    xg, xs = source(oracle, 4, n)
    plan = os_plan(proto)
    plan.set_kernel(KERNEL_TILED)
    ref = syn_os_ref(oracle, proto, xs, plan.contract[0])
    outs, pos = [], 0
    for b in blocks:
        g = plan.geometry(b)
        assert g["tiled"] and g["kernel"] == TILED, (pos, g)
        outs.append(plan.process(xg[:, pos:pos + b]))       # (a view: the band stride is the whole buffer's)
        pos += b
        assert plan.position == (pos, 2 * pos)
    torch.cuda.synchronize()
    assert_bit_exact(np.concatenate([to_cpu(o) for o in outs]), ref, "streaming %r" % blocks)
    plan.reset()
    assert plan.position == (0, 0)
    assert_bit_exact(run(plan, xg[:, :blocks[0]]), to_cpu(outs[0]), "after reset")


@pytest.mark.parametrize("m0", [1, 2 * T + 3])
def test_parity_of_the_start(oracle, proto, m0):
    """3. A fresh plan told that its stream stands at an odd per-band index, zero history: the tiled kernel, forced, reads the other
    pair of images -- the reference with the residues counted from that index."""
    n = 2 * T + 21
    xg, xs = source(oracle, 8, n)
    plan = os_plan(random_taps(128, 7))
    plan.set_kernel(KERNEL_TILED)
    plan.set_position(m0)
    assert plan.position == (m0, 2 * m0) and plan.geometry(n)["kernel"] == TILED
    y = run(plan, xg)
    assert_bit_exact(y, syn_os_ref(oracle, random_taps(128, 7), xs, 2, m0=m0), "start at %d" % m0)
    assert plan.position == (m0 + n, 2 * (m0 + n))
    even = syn_os_ref(oracle, random_taps(128, 7), xs, 2, m0=0)
    assert not np.array_equal(y.view(np.uint64), even.view(np.uint64)), "the parity changes the result"


@pytest.mark.parametrize("nesting", ["bands inside channels", "channels inside bands"])
def test_channels_and_strides(oracle, proto, nesting):
    """4. Three channels, every stride larger than needed (and odd on the input, which the tiled loads do not mind), a distinct source
    per band and channel; nothing between or behind the channels of the output is written."""
    import torch
    nchan, n = 3, 2 * T + 11
    if nesting == "bands inside channels":
        sband = n + 26
        sin = 3 * sband + n + 41
        total = nchan * sin
    else:
        sin = n + 26
        sband = (nchan - 1) * sin + n + 40
        total = 4 * sband
    assert sband % 2 == 1 and sin % 2 == 1
    xbuf = torch.zeros(total, dtype=torch.complex64, device="cuda")
    x = torch.as_strided(xbuf, (nchan, 4, n), (sin, sband, 1))
    for c in range(nchan):
        sxxcvr_amd.synth_fill(x[c], SEED, 10 + 4 * c, 0)
    sout = 2 * n + 34                           # (an even stride: the tiled kernel's 16-byte stores)
    assert sout % 2 == 0 and OUT_FILL < 1 << 31
    ybuf = torch.full((nchan + 1, 2 * sout), OUT_FILL, dtype=torch.int32, device="cuda")
    yc = torch.view_as_complex(ybuf.view(torch.float32).view(nchan + 1, sout, 2))
    plan = os_plan(proto, nchan=nchan)
    plan.set_kernel(KERNEL_TILED)
    assert plan.geometry(n)["kernel"] == TILED
    y = plan.process(x, out=yc[:nchan])
    torch.cuda.synchronize()
    assert y.shape == (nchan, 2 * n)
    words = to_cpu(ybuf).view(np.uint32).reshape(nchan + 1, sout, 2)
    for c in range(nchan):
        xs = np.stack([oracle.synth_iq(SEED, 10 + 4 * c + k, 0, n) for k in range(4)])
        got = words[c, :2 * n].copy().view(np.complex64).ravel()
        assert_bit_exact(got, syn_os_ref(oracle, proto, xs, 2), "channel %d (%s)" % (c, nesting))
    assert np.all(words[:nchan, 2 * n:] == OUT_FILL), "the padding between the channels was written"
    assert np.all(words[nchan] == OUT_FILL), "something was written behind the last channel"


def test_alignment(oracle, proto):
    """5. The tiled kernel stores 16 bytes at a time: an output pointer offset by one sample runs the generic kernel under AUTO (same
    bits, nothing outside written) and answers -4 under a forced TILED, the position unchanged."""
    import torch
    n = 2 * T + 9
    xg, xs = source(oracle, 30, n)
    plan = os_plan(proto)
    ref = syn_os_ref(oracle, proto, xs, plan.contract[0])
    buf = torch.zeros(2 * n + 3, dtype=torch.complex64, device="cuda")
    out = buf[1:1 + 2 * n + 1]
    assert out.data_ptr() % 16 == 8
    assert plan.geometry(n)["kernel"] == TILED          # (the geometry query assumes an aligned output: the call decides)
    plan.process(xg, out=out)
    torch.cuda.synchronize()
    assert_bit_exact(to_cpu(out)[:2 * n], ref, "misaligned output")
    assert to_cpu(buf[:1]).view(np.uint64)[0] == 0, "something was written in front of the output"
    assert np.all(to_cpu(buf[1 + 2 * n:]).view(np.uint64) == 0), "something was written behind the output"
    assert plan.position == (n, 2 * n)
    plan.set_kernel(KERNEL_TILED)
    buf.zero_()
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.process(xg, out=out)
    assert ei.value.code == -4 and plan.position == (n, 2 * n)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(torch.view_as_real(buf))) == 0, "a refused call wrote something"


def test_more_tiles_than_resident_workgroups(oracle, proto):
    """6. resident + 3 tiles: a call this small is dealt as ONE generation of waves, so the grid is the chip's resident waves, a
    multiple of 8 -- the XCD-blocked dealing -- and three waves walk on to a second tile, an interior one whose DMAs they await
    with the counted wait."""
    plan = os_plan(proto)
    plan.set_kernel(KERNEL_TILED)
    resident = plan.geometry(T)["resident"]
    n = (resident + 3) * T
    g = plan.geometry(n)
    assert g["kernel"] == TILED and g["n_tiles"] == resident + 3 and g["workgroups"] == resident and resident % 8 == 0, g
    xg, xs = source(oracle, 40, n)
    y = run(plan, xg)
    assert_bit_exact(y, syn_os_ref(oracle, proto, xs, plan.contract[0], threads=oracle.max_threads()), "resident + 3 tiles")


@pytest.mark.parametrize("ntaps", [64, 40])
def test_generic_tap_counts(oracle, ntaps):
    """7. Other tap counts on CF32: the generic kernel (40 taps: 20 per parity, jsplit 2), two calls, the second from an odd index."""
    import torch
    h = design_lowpass(64, 4, 8.0, 2.0) if ntaps == 64 else random_taps(40, 9)
    n = 4 * 175 + 3
    xg, xs = source(oracle, 50, n)
    plan = os_plan(h)
    assert tuple(plan.contract) == (2, 1) and plan.contract.rot == 0
    g = plan.geometry(n)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    a, b = plan.process(xg[:, :301]), plan.process(xg[:, 301:])
    torch.cuda.synchronize()
    assert_bit_exact(np.concatenate([to_cpu(a), to_cpu(b)]), syn_os_ref(oracle, h, xs, 2), "generic 4 x %d" % ntaps)
    assert plan.position == (n, 2 * n)


def test_generic_cf16(oracle, proto):
    """7. CF16 in and out: inputs quantised to half, the result rounded to half once after the last sum."""
    import torch
    n = 4 * 175 + 3
    xs = np.stack([oracle.synth_iq(SEED, 60 + k, 0, n) for k in range(4)])
    x16 = torch.empty((4, n), dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(x16, SEED, 60, 0, fmt="CF16")
    plan = os_plan(proto, fmt="CF16")
    assert plan.geometry(n)["kernel"] == GENERIC
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    y16 = run(plan, x16)
    assert y16.shape == (2 * n,) and y16.dtype == np.int32
    h16 = oracle.f32_to_f16(xs.view(np.float32))
    assert np.array_equal(to_cpu(x16).view(np.uint16), h16), "CF16 synthetic source"
    xq = oracle.f16_to_f32(h16).view(np.complex64)
    ref = syn_os_ref(oracle, proto, xq, plan.contract[0])
    want = oracle.f32_to_f16(ref.view(np.float32))
    assert np.array_equal(np.ascontiguousarray(y16).view(np.uint16), want.ravel()), "CF16 output"


def test_generic_s32_words(oracle, proto):
    """7. S32 wire words out: convert_tx of the CF32 result, word for word, with a tx_threshold set.  The inputs are scaled by 2^-3
    on both sides (exact), so that no output reaches convert_tx's saturating corner: asserted on the reference first."""
    import torch
    n = 4 * 175 + 3
    xg, xs = source(oracle, 70, n)
    torch.view_as_real(xg).mul_(0.125)
    xs = (xs.view(np.float32) * np.float32(0.125)).view(np.complex64)
    assert_bit_exact(to_cpu(xg).ravel(), xs.ravel(), "scaled source")
    plan = os_plan(proto, fmt="S32")
    plan.set_tx_threshold(1e-6)
    assert plan.geometry(n)["kernel"] == GENERIC
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    ref = syn_os_ref(oracle, proto, xs, plan.contract[0])
    assert max(np.abs(ref.real).max(), np.abs(ref.imag).max()) < 1.0
    y = run(plan, xg)
    assert y.shape == (2 * n, 2) and y.dtype == np.int32
    assert np.array_equal(y.ravel(), oracle.convert_tx(ref, 1e-6)), "S32 words out"


def test_tiled_equals_generic(oracle):
    """8. The same plan shape under KERNEL_TILED and KERNEL_GENERIC on 4 tiles."""
    h = random_taps(128, 21)
    xg, _ = source(oracle, 80, 4 * T)
    a = os_plan(h)
    a.set_kernel(KERNEL_TILED)
    b = os_plan(h)
    b.set_kernel(KERNEL_GENERIC)
    assert a.geometry(4 * T)["kernel"] == TILED and b.geometry(4 * T)["kernel"] == GENERIC
    assert_bit_exact(run(a, xg), run(b, xg), "tiled vs generic")


def test_places_the_band(proto):
    """9a. Band 1 alone holds a tone 0.1 cycles per band sample: it lands at 1/4 + 0.1/2 = 0.3 cycles per output sample within
    0.01 dB of the fp64 figure (tests/test_synthesizer_os_host.py::test_fp64_figures_of_the_gpu_property_tests: +0.00024 dB, every
    other bin below -119 dB), and nothing else is above -80 dB -- the fp32 margins test_takes_the_bands_apart
    (tests/test_gpu_channelizer.py) uses for this prototype.  The first 256 outputs are dropped and the tone is on a bin of the
    65 000 kept, so neither a transient nor leakage uses the margins."""
    x = band_tone(BAND_TONE_N)
    plan = os_plan(proto)
    assert plan.geometry(x.shape[1])["kernel"] == TILED
    w = run(plan, to_gpu(x.astype(np.complex64)))[BAND_TONE_DROP:BAND_TONE_DROP + BAND_TONE_KEEP].astype(np.complex128)
    assert w.size == BAND_TONE_KEEP
    tone, rest, at = tone_and_rest(w, BAND_TONE_BIN)
    print("tone %.5f dB, rest %.1f dB at %.4f" % (tone, rest, at / w.size))
    assert abs(tone - BAND_TONE_DB) <= 0.01
    assert rest <= -80.0


def test_band_edge_loopback(proto):
    """9b. Channelizer(oversample=2) (gain-1 prototype), then Synthesizer(oversample=2) (gain 2), on the tone 0.0125 cycles per
    sample under the edge between bands 0 and 1: it comes back within 0.01 dB of the fp64 figure (-0.58733 dB: the two prototypes'
    transition bands) and every other bin is <= -80 dB (fp64: -112.7 dB).  The critically sampled pair on the same input returns
    the tone with an image at 0.8625 cycles per sample, within 0.1 dB of the fp64 figure (-29.9 dB), and band 1's alias of it at
    0.3625, as large."""
    x = edge_tone()
    xg = to_gpu(x.astype(np.complex64))
    h1 = design_lowpass(128, 4)
    chan, syn = sxxcvr_amd.Channelizer(h1, oversample=2), os_plan(proto)
    assert chan.geometry(x.size)["kernel"] == "chan4x2_kernel" and syn.geometry(x.size // 2)["kernel"] == TILED
    w = run(syn, chan.process(xg))[LOOP_DROP:LOOP_DROP + LOOP_KEEP].astype(np.complex128)
    assert w.size == LOOP_KEEP
    tone, rest, at = tone_and_rest(w, LOOP_BIN)
    print("oversampled pair: tone %.5f dB, rest %.1f dB at %.4f" % (tone, rest, at / w.size))
    assert abs(tone - LOOP_TONE_DB) <= 0.01
    assert rest <= -80.0
    chan1, syn1 = sxxcvr_amd.Channelizer(h1), sxxcvr_amd.Synthesizer(design_lowpass(128, 4, 8.0, 4.0))
    wc = run(syn1, chan1.process(xg))[LOOP_DROP:LOOP_DROP + LOOP_KEEP].astype(np.complex128)
    tone_c, rest_c, at_c = tone_and_rest(wc, LOOP_BIN)
    image = spectrum_db(wc)[CRIT_IMAGE_BIN]
    print("critically sampled pair: tone %.5f dB, image at 0.8625 %.2f dB, largest other bin %.2f dB at %.4f" % (tone_c, image, rest_c, at_c / wc.size))
    # (the alias at 0.3625 is level with the image to the last digit: the largest other bin is one of the two)
    assert abs(image - CRIT_IMAGE_DB) <= 0.1 and abs(rest_c - CRIT_IMAGE_DB) <= 0.1


def test_errors(oracle, proto):
    """10. The plan refuses every other pass's entry point (the message names sxfir_synthesize) and sxfir_set_history, is left
    untouched by that and goes on working; stride errors; what the plan kinds answer to the two oversampling queries."""
    import torch
    lib = sxxcvr_amd.load_sxfir()
    n = T
    xg, xs = source(oracle, 90, n)
    plan = os_plan(proto)
    y = torch.zeros(2 * n, dtype=torch.complex64, device="cuda")
    xp, yp, null = C.c_void_p(xg.data_ptr()), C.c_void_p(y.data_ptr()), None
    n_out = C.c_size_t(77)
    ms = C.c_float()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    refusals = [
        lambda: lib.sxfir_decimate(plan._plan, xp, n, n, yp, 2 * n, C.byref(n_out), null),
        lambda: lib.sxfir_interpolate(plan._plan, xp, n, n, yp, 2 * n, C.byref(n_out), null),
        lambda: lib.sxfir_interpolate_keyed(plan._plan, xp, n, n, yp, 2 * n, C.byref(n_out), 0, n, C.c_void_p(counter.data_ptr()), null),
        lambda: lib.sxfir_channelize(plan._plan, xp, n, n, yp, 0, n, C.byref(n_out), null),
        lambda: lib.sxfir_time_decimate(plan._plan, xp, n, n, yp, 2 * n, 1, null, C.byref(ms)),
        lambda: lib.sxfir_time_interpolate(plan._plan, xp, n, n, yp, 2 * n, 1, null, C.byref(ms)),
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
    assert_bit_exact(run(plan, xg, out=y), syn_os_ref(oracle, proto, xs, plan.contract[0]), "after the refused calls")
    # two channels: bands and channels that would overlap, an output stride smaller than the block
    two = os_plan(proto, nchan=2)
    x2 = torch.zeros((2, 4, n), dtype=torch.complex64, device="cuda")
    y2 = torch.zeros((2, 2 * n), dtype=torch.complex64, device="cuda")
    for in_stride, band_stride, out_stride in ((n, n, 2 * n), (2 * n, n, 2 * n), (n, 2 * n - 1, 2 * n), (4 * n, n, 2 * n - 1)):
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            two.process_ptr(x2.data_ptr(), n, in_stride, band_stride, y2.data_ptr(), out_stride)
        assert ei.value.code == -1 and two.position == (0, 0), (in_stride, band_stride, out_stride)
    assert two.process_ptr(x2.data_ptr(), n, 4 * n, n, y2.data_ptr(), 2 * n) == 2 * n          # bands inside channels
    for kw in (dict(oversample=3), dict(nbands=8, oversample=2)):
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            sxxcvr_amd.Synthesizer(proto, **kw)
        assert ei.value.code == -4, kw
    # what the plan is, and what the others are not
    crit = sxxcvr_amd.Synthesizer(design_lowpass(128, 4, 8.0, 4.0))
    real = sxxcvr_amd.Resampler(INTERPOLATE, proto, 2)
    chan = sxxcvr_amd.Channelizer(design_lowpass(128, 4), oversample=2)
    assert plan.bands == 4 and plan.oversampling == 2 and crit.oversampling == 1 and crit.ratio == 4
    v = C.c_int(-1)
    for other, want in ((plan, 2), (crit, 1), (real, 0), (chan, 0)):
        v.value = -1
        assert lib.sxfir_plan_synthesis_oversampling(other._plan, C.byref(v)) == 0 and v.value == want
    for syn in (plan, crit):                                    # sxfir_plan_oversampling speaks of channelizers
        v.value = -1
        assert lib.sxfir_plan_oversampling(syn._plan, C.byref(v)) == 0 and v.value == 0
        assert lib.sxfir_plan_bands(syn._plan, C.byref(v)) == 0 and v.value == 0
    assert lib.sxfir_plan_oversampling(chan._plan, C.byref(v)) == 0 and v.value == 2
    torch.cuda.synchronize()
