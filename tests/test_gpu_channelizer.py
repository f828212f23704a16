"""The 4-band channelizer on the GPU (include/sxfir_channelizer.h), bit for bit against the oracle as it stands.

The reference value is always built the same way: u_r = oracle.decim_f32(h_r, 4, x, 1, 1), where h_r is h with
every tap of phase != r set to +0.0 -- the oracle's (1, 1) tree then adds three +0.0 columns to the one chain, which is exact, and
a chain from +0.0 never yields -0.0 -- then the radix-2 butterflies of the header in float32 numpy, one rounding per operation."""
import ctypes as C
import functools

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_lowpass
from sxxcvr_amd.resampler import DECIMATE, KERNEL_GENERIC, KERNEL_TILED
from gpu_util import OUT_FILL, assert_bands, assert_bit_exact, band_proto, chan_os_ref, chan_ref, random_taps, run, to_cpu, to_gpu, wideband_source

pytestmark = pytest.mark.gpu

SEED = 0xC4A77E1
TILE_IN = 2048
TILED, GENERIC = "chan4_kernel", "chan_generic_kernel"
source = functools.partial(wideband_source, seed=SEED)


@pytest.fixture(scope="module")
def proto():
    return band_proto()


@pytest.mark.parametrize("which", ["lowpass", "random"])
def test_tiled_4x128(oracle, proto, which):
    """1. One call of 3 tiles plus a ragged tail through chan4_kernel."""
    h = proto if which == "lowpass" else random_taps(128)
    assert which == "lowpass" or not np.array_equal(h, h[::-1])
    n_in = 3 * TILE_IN + 4 * 37
    xg, xs = source(oracle, 0, n_in)
    plan = sxxcvr_amd.Channelizer(h)
    assert plan.bands == 4 and tuple(plan.contract) == (1, 1) and plan.contract.rot == 0
    plan.set_kernel(KERNEL_TILED)
    g = plan.geometry(n_in)
    assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == 4 and g["tile_samples"] == TILE_IN, g
    y = run(plan, xg)
    assert_bands(y, chan_ref(oracle, h, xs), "tiled 4 x 128 (%s)" % which)
    assert plan.position == (n_in, n_in // 4)


def test_streaming_and_history(oracle, proto):
    """2. Five calls on one plan (one shorter than the 128-sample history, one of a single output) give the bits of one pass."""
    import torch
    blocks = [TILE_IN * 2, 4 * 31, TILE_IN + 4 * 5, 4 * 1, TILE_IN]
    n = sum(blocks)
    xg, xs = source(oracle, 1, n)
    plan = sxxcvr_amd.Channelizer(proto)
    ref = chan_ref(oracle, proto, xs)
    outs, pos = [], 0
    for b in blocks:
        assert plan.geometry(b)["kernel"] == TILED
        outs.append(plan.process(xg[pos:pos + b].clone()))
        pos += b
    torch.cuda.synchronize()
    assert_bands(np.concatenate([to_cpu(o) for o in outs], axis=1), ref, "streaming %r" % blocks)
    assert plan.position == (n, n // 4)
    plan.reset()
    assert plan.position == (0, 0)
    assert_bands(run(plan, xg[:blocks[0]].clone()), to_cpu(outs[0]), "after reset")


def test_off_boundary_and_misaligned(oracle, proto):
    """3. A call that starts off an output boundary, and an output pointer offset by one sample: chan_generic_kernel."""
    import torch
    n1, n2 = 4 * 100 + 3, TILE_IN
    xg, xs = source(oracle, 2, n1 + n2)
    plan = sxxcvr_amd.Channelizer(proto)
    ref = chan_ref(oracle, proto, xs)
    y1 = plan.process(xg[:n1].clone())
    g = plan.geometry(n2)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    y2 = plan.process(xg[n1:].clone())
    torch.cuda.synchronize()
    assert y1.shape == (4, 101) and y2.shape == (4, (n1 + n2 + 3) // 4 - 101)
    assert_bands(np.concatenate([to_cpu(y1), to_cpu(y2)], axis=1), ref, "off-boundary second call")
    assert plan.position == (n1 + n2, (n1 + n2 + 3) // 4)
    # set_position: a fresh plan placed where the second call started, its history seeded from the first block
    other = sxxcvr_amd.Channelizer(proto)
    other.set_history_ptr(xg.data_ptr(), n1, n1)
    other.set_position(n1)
    assert_bands(run(other, xg[n1:].clone()), to_cpu(y2), "set_position + set_history")
    # output offset by one sample (8 bytes: not 16-byte aligned), an even band stride
    plan.reset()
    n3 = TILE_IN + 4 * 9
    n_out, row = n3 // 4, n3 // 4 + 1
    assert row % 2 == 0
    buf = torch.zeros(4 * row + 1, dtype=torch.complex64, device="cuda")
    out = buf[1:].view(4, row)
    assert out.data_ptr() % 16 == 8
    assert plan.geometry(n3)["kernel"] == TILED          # (the geometry query assumes an aligned output: the call decides)
    plan.process(xg[:n3].clone(), out=out)
    torch.cuda.synchronize()
    assert_bands(to_cpu(out)[:, :n_out], ref[:, :n_out], "misaligned output")
    assert to_cpu(buf[:1]).view(np.uint64)[0] == 0, "something was written in front of the output"
    assert np.all(to_cpu(out)[:, n_out:].view(np.uint64) == 0), "something was written behind a band"
    plan.set_kernel(KERNEL_TILED)
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.process(xg[:n3].clone(), out=out)
    assert ei.value.code == -4


def test_channels_and_strides(oracle, proto):
    """4. Three channels, every stride larger than needed, a distinct source per channel; the padding between bands and between
    channels is untouched."""
    import torch
    nchan, n_in = 3, 2 * TILE_IN + 4 * 11
    n_out = n_in // 4
    sin, sband = n_in + 40, n_out + 25
    sout = 4 * sband + 34                       # (even strides: the tiled kernel's 16-byte stores)
    assert sband % 2 == 0 and sout % 2 == 0
    xbuf = torch.zeros((nchan, sin), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(xbuf[:, :n_in], SEED, 7, 0)
    assert OUT_FILL < 1 << 31                   # (fits an int32 as it is)
    ybuf = torch.full((nchan, 2 * sout), OUT_FILL, dtype=torch.int32, device="cuda")
    yc = torch.view_as_complex(ybuf.view(torch.float32).view(nchan, sout, 2))
    out = torch.as_strided(yc, (nchan, 4, sband), (sout, sband, 1))
    plan = sxxcvr_amd.Channelizer(proto, nchan=nchan)
    plan.set_kernel(KERNEL_TILED)
    assert plan.geometry(n_in)["kernel"] == TILED
    y = plan.process(xbuf[:, :n_in], out=out)
    torch.cuda.synchronize()
    assert y.shape == (nchan, 4, n_out)
    words = to_cpu(ybuf).view(np.uint32).reshape(nchan, sout, 2)
    written = np.zeros((nchan, sout), dtype=bool)
    for c in range(nchan):
        ref = chan_ref(oracle, proto, oracle.synth_iq(SEED, 7 + c, 0, n_in))
        for k in range(4):
            got = words[c, k * sband:k * sband + n_out].copy().view(np.complex64).ravel()
            assert_bit_exact(got, ref[k], "channel %d band %d" % (c, k))
            written[c, k * sband:k * sband + n_out] = True
    assert np.all(words[~written] == OUT_FILL), "the padding between bands or channels was written"


def test_more_tiles_than_resident_workgroups(oracle, proto):
    """5. resident + 3 tiles: a call this small is dealt as ONE generation of waves, so the grid is the chip's resident waves, a
    multiple of 8 -- the XCD-blocked dealing -- and three waves walk on to a second tile."""
    plan = sxxcvr_amd.Channelizer(proto)
    plan.set_kernel(KERNEL_TILED)
    resident = plan.geometry(TILE_IN)["resident"]
    n_in = (resident + 3) * TILE_IN
    g = plan.geometry(n_in)
    assert g["kernel"] == TILED and g["n_tiles"] == resident + 3 and g["workgroups"] == resident and resident % 8 == 0, g
    xg, xs = source(oracle, 3, n_in)
    y = run(plan, xg)
    assert_bands(y, chan_ref(oracle, proto, xs, threads=oracle.max_threads()), "resident + 3 tiles")


@pytest.mark.parametrize("ntaps", [64, 40])
def test_generic_tap_counts(oracle, ntaps):
    """6. Other tap counts on CF32: the generic kernel."""
    h = design_lowpass(64, 4) if ntaps == 64 else random_taps(40, 9)
    n_in = 4 * 700 + 3
    xg, xs = source(oracle, 4, n_in)
    plan = sxxcvr_amd.Channelizer(h)
    assert tuple(plan.contract) == (1, 1) and plan.contract.rot == 0
    g = plan.geometry(n_in)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    assert_bands(run(plan, xg), chan_ref(oracle, h, xs), "generic 4 x %d" % ntaps)


@pytest.mark.parametrize("oversample", [1, 2])
def test_generic_start_parity(oracle, oversample):
    """6. Calls that start at an odd absolute output index, on both generic channelizer kernels: 32 taps (no tiled form), three
    calls of 5, 6 and 3 outputs per band -- the second starts at output 5, the third at output 11.  The oversampled plan shifts
    the butterflies' operands by the parity of the ABSOLUTE output index; the critically sampled plan never does."""
    import torch
    h = random_taps(32)
    ratio = 4 // oversample
    blocks = [ratio * m for m in (5, 6, 3)]
    xg, xs = source(oracle, 10, sum(blocks))
    plan = sxxcvr_amd.Channelizer(h, oversample=oversample)
    name = GENERIC if oversample == 1 else "chan4x2_generic_kernel"
    outs, pos = [], 0
    for b in blocks:
        g = plan.geometry(b)
        assert not g["tiled"] and g["kernel"] == name, g
        outs.append(plan.process(xg[pos:pos + b].clone()))
        pos += b
    torch.cuda.synchronize()
    assert [o.shape[1] for o in outs] == [5, 6, 3]
    ref = chan_ref(oracle, h, xs) if oversample == 1 else chan_os_ref(oracle, h, xs)
    assert_bands(np.concatenate([to_cpu(o) for o in outs], axis=1), ref, "generic, oversample %d, calls of 5, 6, 3 outputs" % oversample)
    assert plan.position == (sum(blocks), 14)


def test_generic_cf16(oracle, proto):
    """6. CF16 in and out: inputs quantised to half, outputs rounded to half once after the butterflies."""
    import torch
    n_in = TILE_IN + 4 * 13
    xs = oracle.synth_iq(SEED, 5, 0, n_in)
    x16 = torch.empty(n_in, dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(x16, SEED, 5, 0, fmt="CF16")
    plan = sxxcvr_amd.Channelizer(proto, fmt="CF16")
    assert plan.geometry(n_in)["kernel"] == GENERIC
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    y16 = run(plan, x16)
    assert y16.shape == (4, n_in // 4) and y16.dtype == np.int32
    h16 = oracle.f32_to_f16(xs.view(np.float32))
    assert np.array_equal(to_cpu(x16).view(np.uint16), h16), "CF16 synthetic source"
    xq = oracle.f16_to_f32(h16).view(np.complex64)
    ref = chan_ref(oracle, proto, xq)
    for k in range(4):
        want = oracle.f32_to_f16(np.ascontiguousarray(ref[k]).view(np.float32))
        assert np.array_equal(np.ascontiguousarray(y16[k]).view(np.uint16), want.ravel()), "CF16 band %d" % k


def test_generic_s32_words(oracle, proto):
    """6. S32 wire words in: convert_rx on the way in, CF32 out."""
    import torch
    n_in = TILE_IN + 4 * 13
    s32 = torch.empty((n_in, 2), dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(torch.view_as_complex(s32.view(torch.float32)), SEED, 6, 0, fmt="S32")
    plan = sxxcvr_amd.Channelizer(proto, fmt="S32")
    assert plan.geometry(n_in)["kernel"] == GENERIC
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    y = run(plan, s32)
    x = oracle.convert_rx(to_cpu(s32).ravel())
    assert_bit_exact(x, oracle.synth_iq(SEED, 6, 0, n_in), "S32 synthetic source")
    assert y.dtype == np.complex64
    assert_bands(y, chan_ref(oracle, proto, x), "S32 words in")


def test_tiled_equals_generic(oracle):
    """7. The same plan shape under KERNEL_TILED and KERNEL_GENERIC on 4 tiles."""
    h = random_taps(128, 21)
    xg, _ = source(oracle, 8, 4 * TILE_IN)
    a = sxxcvr_amd.Channelizer(h)
    a.set_kernel(KERNEL_TILED)
    b = sxxcvr_amd.Channelizer(h)
    b.set_kernel(KERNEL_GENERIC)
    assert a.geometry(4 * TILE_IN)["kernel"] == TILED and b.geometry(4 * TILE_IN)["kernel"] == GENERIC
    assert_bands(run(a, xg), run(b, xg), "tiled vs generic")


def test_takes_the_bands_apart(proto):
    """8. A tone 0.1/4 above band 1's centre (11/40 cycles per input sample, phases reduced in integers) lands in band 1 at +0.1
    cycles per output sample at 0 dB +- 0.01 dB, and bands 0, 2 and 3 hold nothing above -80 dB anywhere: the thresholds
    test_takes_the_band_out (tests/test_gpu_complex_taps.py) uses for this prototype.  The same pass in fp64 with the library's own
    designer (tests/test_channelizer_host.py::test_fp64_band_separation_of_the_gpu_test): +0.00024 dB in band 1; peaks of -104.8,
    -109.6 and -126.4 dB in bands 0, 2 and 3.  The margin is for fp32 accumulation; the first 64 outputs (twice the filter's
    length) are dropped and the tone is on a bin of the remaining 16 320, so neither a transient nor leakage uses it."""
    n = 1 << 16
    k = np.arange(n, dtype=np.int64)
    x = np.exp(2j * np.pi * ((k * 11) % 40) / 40.0)
    plan = sxxcvr_amd.Channelizer(proto)
    assert plan.geometry(n)["kernel"] == TILED
    y = run(plan, to_gpu(x.astype(np.complex64)))[:, 64:].astype(np.complex128)
    m = y.shape[1]
    assert m == 16320
    Y = 20 * np.log10(np.maximum(np.abs(np.fft.fft(y, axis=1)) / m, 1e-300))
    peaks = [Y[b].max() for b in (0, 2, 3)]
    print("band 1 tone %.5f dB; bands 0, 2, 3 peak %.1f, %.1f, %.1f dB" % (Y[1, 1632], peaks[0], peaks[1], peaks[2]))
    assert abs(Y[1, 1632]) <= 0.01
    assert max(peaks) <= -80.0


def test_errors(oracle, proto):
    """9. The plan refuses the decimator's entry point and goes on working; stride and band-count errors; sxfir_plan_bands."""
    import torch
    lib = sxxcvr_amd.load_sxfir()
    n_in = TILE_IN
    xg, xs = source(oracle, 9, n_in)
    plan = sxxcvr_amd.Channelizer(proto)
    y = torch.zeros((4, n_in // 4), dtype=torch.complex64, device="cuda")
    n_out = C.c_size_t(77)
    rc = lib.sxfir_decimate(plan._plan, C.c_void_p(xg.data_ptr()), n_in, n_in, C.c_void_p(y.data_ptr()), n_in // 4, C.byref(n_out), None)
    assert rc == -1 and n_out.value == 0 and b"channelizer" in lib.sxfir_last_error()
    ms = C.c_float()
    assert lib.sxfir_time_decimate(plan._plan, C.c_void_p(xg.data_ptr()), n_in, n_in, C.c_void_p(y.data_ptr()), n_in // 4, 1, None, C.byref(ms)) == -1
    assert lib.sxfir_interpolate(plan._plan, C.c_void_p(xg.data_ptr()), n_in, n_in, C.c_void_p(y.data_ptr()), n_in // 4, C.byref(n_out), None) == -1
    torch.cuda.synchronize()
    assert plan.position == (0, 0) and int(torch.count_nonzero(torch.view_as_real(y))) == 0
    with pytest.raises(sxxcvr_amd.NativeError) as ei:          # band stride smaller than the outputs per band
        plan.process_ptr(xg.data_ptr(), n_in, n_in, y.data_ptr(), 0, n_in // 4 - 1)
    assert ei.value.code == -1 and plan.position == (0, 0)
    assert_bands(run(plan, xg, out=y), chan_ref(oracle, proto, xs), "after the refused calls")
    # channels that would overlap the bands
    two = sxxcvr_amd.Channelizer(proto, nchan=2)
    x2 = torch.zeros((2, n_in), dtype=torch.complex64, device="cuda")
    y2 = torch.zeros((2, 4, n_in // 4), dtype=torch.complex64, device="cuda")
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        two.process_ptr(x2.data_ptr(), n_in, n_in, y2.data_ptr(), 2 * (n_in // 4), n_in // 4)
    assert ei.value.code == -1
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Channelizer(proto, nbands=2)
    assert ei.value.code == -4
    assert plan.bands == 4
    real = sxxcvr_amd.Resampler(DECIMATE, proto, 4)
    nb = C.c_int(-1)
    assert lib.sxfir_plan_bands(real._plan, C.byref(nb)) == 0 and nb.value == 0
    assert not real.complex_taps
    f = C.c_int(-1)
    assert lib.sxfir_taps_are_complex(plan._plan, C.byref(f)) == 0 and f.value == 0
