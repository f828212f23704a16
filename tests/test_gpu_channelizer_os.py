"""The 2x oversampled 4-band channelizer on the GPU (include/sxfir_channelizer_os.h), bit for bit against the oracle as it stands.

The reference value is always built the same way: u_r = oracle.decim_f32(h_r, 2, x, 1, 1), where h_r is h with every tap of phase
!= r set to +0.0 -- under (1, 1) the oracle's one chain over all taps then meets three +0.0 taps in four, which leave a chain that
started from +0.0 as it is -- then the radix-2 butterflies of the header in float32 numpy, one rounding per operation, on
(u0, u1, u2, u3) in the even columns and on (u2, u3, u0, u1) in the odd ones."""
import ctypes as C
import functools

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_lowpass
from sxxcvr_amd.resampler import DECIMATE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED
from gpu_util import (OUT_FILL, assert_bands, assert_bit_exact, band_proto, chan_os_ref, random_taps, run, to_cpu, to_gpu,
                      wideband_source)
from test_channelizer_os_host import (EDGE_TONE_BAND0_DB, EDGE_TONE_BAND1_DB, EDGE_TONE_BIN0, EDGE_TONE_BIN1, edge_tone,
                                      edge_tone_spectra)

pytestmark = pytest.mark.gpu

SEED = 0xC4A77E2
TILE_IN = 2048
TILED, GENERIC = "chan4x2_kernel", "chan4x2_generic_kernel"
source = functools.partial(wideband_source, seed=SEED)


def os_plan(h, **kw):
    return sxxcvr_amd.Channelizer(h, oversample=2, **kw)


@pytest.fixture(scope="module")
def proto():
    return band_proto()


@pytest.mark.parametrize("which", ["lowpass", "random"])
def test_tiled_4x128(oracle, proto, which):
    """1. One call of 3 tiles plus a ragged tail that ends between an even and an odd output, through chan4x2_kernel."""
    h = proto if which == "lowpass" else random_taps(128)
    assert which == "lowpass" or not np.array_equal(h, h[::-1])
    n_in = 3 * TILE_IN + 2 * 37
    assert n_in % 4 == 2
    xg, xs = source(oracle, 0, n_in)
    plan = os_plan(h)
    assert plan.bands == 4 and plan.oversampling == 2 and plan.ratio == 2
    assert tuple(plan.contract) == (1, 1) and plan.contract.rot == 0
    assert plan.outputs_for(n_in) == (n_in + 1) // 2
    plan.set_kernel(KERNEL_TILED)
    g = plan.geometry(n_in)
    assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == 4 and g["tile_samples"] == TILE_IN, g
    y = run(plan, xg)
    assert y.shape == (4, (n_in + 1) // 2)
    assert_bands(y, chan_os_ref(oracle, h, xs), "tiled 4 x 128 oversampled (%s)" % which)
    assert plan.position == (n_in, (n_in + 1) // 2)


def test_even_columns_are_the_channelizers(oracle):
    """2. y_k[2m'] has the bits of sxfir_channelize on the same stream at output m': both tiled, 2 tiles plus a tail."""
    h = random_taps(128, 31)
    n_in = 2 * TILE_IN + 4 * 21
    xg, _ = source(oracle, 10, n_in)
    a, b = os_plan(h), sxxcvr_amd.Channelizer(h)
    assert b.oversampling == 1
    assert a.geometry(n_in)["kernel"] == TILED and b.geometry(n_in)["kernel"] == "chan4_kernel"
    ya, yb = run(a, xg), run(b, xg)
    assert ya.shape == (4, n_in // 2) and yb.shape == (4, n_in // 4)
    assert_bands(np.ascontiguousarray(ya[:, 0::2]), yb, "even columns against the critically sampled plan")


def test_streaming_and_history(oracle, proto):
    """3. Six calls on one plan (one shorter than the 128-sample history, one of a single output, two that start at a position
    = 2 mod 4, i.e. at an odd output index) give the bits of one pass."""
    import torch
    blocks = [2 * TILE_IN, 4 * 31, TILE_IN + 4 * 5 + 2, 2, TILE_IN + 2, TILE_IN]
    n = sum(blocks)
    xg, xs = source(oracle, 1, n)
    plan = os_plan(proto)
    ref = chan_os_ref(oracle, proto, xs)
    outs, pos, kernels = [], 0, []
    for b in blocks:
        g = plan.geometry(b)
        kernels.append(g["kernel"])
        assert g["kernel"] == (TILED if pos % 4 == 0 else GENERIC) and g["tiled"] == (pos % 4 == 0), (pos, g)
        outs.append(plan.process(xg[pos:pos + b].clone()))
        pos += b
        assert plan.position == (pos, (pos + 1) // 2)
    assert kernels == [TILED, TILED, TILED, GENERIC, TILED, GENERIC]
    torch.cuda.synchronize()
    assert outs[3].shape == (4, 1)
    assert_bands(np.concatenate([to_cpu(o) for o in outs], axis=1), ref, "streaming %r" % blocks)
    plan.reset()
    assert plan.position == (0, 0)
    assert_bands(run(plan, xg[:blocks[0]].clone()), to_cpu(outs[0]), "after reset")


def test_off_position_and_misaligned(oracle, proto):
    """4. A call that starts off an output boundary, a fresh plan placed there, and an output pointer offset by one sample:
    chan4x2_generic_kernel, the same bits."""
    import torch
    n1, n2 = 2 * 100 + 1, TILE_IN
    xg, xs = source(oracle, 2, n1 + n2)
    plan = os_plan(proto)
    ref = chan_os_ref(oracle, proto, xs)
    y1 = plan.process(xg[:n1].clone())
    g = plan.geometry(n2)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    y2 = plan.process(xg[n1:].clone())
    torch.cuda.synchronize()
    assert y1.shape == (4, 101) and y2.shape == (4, (n1 + n2 + 1) // 2 - 101)
    assert_bands(np.concatenate([to_cpu(y1), to_cpu(y2)], axis=1), ref, "off-boundary second call")
    assert plan.position == (n1 + n2, (n1 + n2 + 1) // 2)
    # set_position: a fresh plan placed where the second call started, its history seeded from the first block
    other = os_plan(proto)
    other.set_history_ptr(xg.data_ptr(), n1, n1)
    other.set_position(n1)
    assert other.position == (n1, 101)
    assert_bands(run(other, xg[n1:].clone()), to_cpu(y2), "set_position + set_history")
    # output offset by one sample (8 bytes: not 16-byte aligned), an even band stride
    plan.reset()
    n3 = TILE_IN + 2 * 9
    n_out, row = n3 // 2, n3 // 2 + 1
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
    plan.reset()
    plan.set_kernel(KERNEL_TILED)
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.process(xg[:n3].clone(), out=out)
    assert ei.value.code == -4 and plan.position == (0, 0)
    # ... and a forced TILED at a position = 2 mod 4, aligned output: refused too, nothing written
    plan.set_kernel(KERNEL_AUTO)
    plan.process(xg[:2].clone())
    plan.set_kernel(KERNEL_TILED)
    ok = torch.zeros((4, TILE_IN // 2), dtype=torch.complex64, device="cuda")
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.process(xg[2:2 + TILE_IN].clone(), out=ok)
    torch.cuda.synchronize()
    assert ei.value.code == -4 and plan.position == (2, 1) and int(torch.count_nonzero(torch.view_as_real(ok))) == 0


def test_channels_and_strides(oracle, proto):
    """5. Three channels, every stride larger than needed, a distinct source per channel; the padding between bands and between
    channels is untouched."""
    import torch
    nchan, n_in = 3, 2 * TILE_IN + 2 * 11
    n_out = n_in // 2
    sin, sband = n_in + 40, n_out + 25
    sout = 4 * sband + 34                       # (even strides: the tiled kernel's 16-byte stores)
    assert sband % 2 == 0 and sout % 2 == 0
    xbuf = torch.zeros((nchan, sin), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(xbuf[:, :n_in], SEED, 7, 0)
    assert OUT_FILL < 1 << 31                   # (fits an int32 as it is)
    ybuf = torch.full((nchan, 2 * sout), OUT_FILL, dtype=torch.int32, device="cuda")
    yc = torch.view_as_complex(ybuf.view(torch.float32).view(nchan, sout, 2))
    out = torch.as_strided(yc, (nchan, 4, sband), (sout, sband, 1))
    plan = os_plan(proto, nchan=nchan)
    plan.set_kernel(KERNEL_TILED)
    assert plan.geometry(n_in)["kernel"] == TILED
    y = plan.process(xbuf[:, :n_in], out=out)
    torch.cuda.synchronize()
    assert y.shape == (nchan, 4, n_out)
    words = to_cpu(ybuf).view(np.uint32).reshape(nchan, sout, 2)
    written = np.zeros((nchan, sout), dtype=bool)
    for c in range(nchan):
        ref = chan_os_ref(oracle, proto, oracle.synth_iq(SEED, 7 + c, 0, n_in))
        for k in range(4):
            got = words[c, k * sband:k * sband + n_out].copy().view(np.complex64).ravel()
            assert_bit_exact(got, ref[k], "channel %d band %d" % (c, k))
            written[c, k * sband:k * sband + n_out] = True
    assert np.all(words[~written] == OUT_FILL), "the padding between bands or channels was written"


def test_more_tiles_than_resident_workgroups(oracle, proto):
    """6. resident + 3 tiles: a call this small is dealt as ONE generation of waves, so the grid is the chip's resident waves, a
    multiple of 8 -- the XCD-blocked dealing -- and three waves walk on to a second tile."""
    plan = os_plan(proto)
    plan.set_kernel(KERNEL_TILED)
    resident = plan.geometry(TILE_IN)["resident"]
    n_in = (resident + 3) * TILE_IN
    g = plan.geometry(n_in)
    assert g["kernel"] == TILED and g["n_tiles"] == resident + 3 and g["workgroups"] == resident and resident % 8 == 0, g
    xg, xs = source(oracle, 3, n_in)
    y = run(plan, xg)
    assert_bands(y, chan_os_ref(oracle, proto, xs, threads=oracle.max_threads()), "resident + 3 tiles")


@pytest.mark.parametrize("ntaps", [64, 40])
def test_generic_tap_counts(oracle, ntaps):
    """7. Other tap counts on CF32: the generic kernel."""
    h = design_lowpass(64, 4) if ntaps == 64 else random_taps(40, 9)
    n_in = 2 * 700 + 1
    xg, xs = source(oracle, 4, n_in)
    plan = os_plan(h)
    assert tuple(plan.contract) == (1, 1) and plan.contract.rot == 0 and plan.oversampling == 2
    g = plan.geometry(n_in)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    assert_bands(run(plan, xg), chan_os_ref(oracle, h, xs), "generic 4 x %d oversampled" % ntaps)


def test_generic_cf16(oracle, proto):
    """7. CF16 in and out: inputs quantised to half, outputs rounded to half once after the butterflies."""
    import torch
    n_in = TILE_IN + 2 * 13
    xs = oracle.synth_iq(SEED, 5, 0, n_in)
    x16 = torch.empty(n_in, dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(x16, SEED, 5, 0, fmt="CF16")
    plan = os_plan(proto, fmt="CF16")
    assert plan.geometry(n_in)["kernel"] == GENERIC
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    y16 = run(plan, x16)
    assert y16.shape == (4, n_in // 2) and y16.dtype == np.int32
    h16 = oracle.f32_to_f16(xs.view(np.float32))
    assert np.array_equal(to_cpu(x16).view(np.uint16), h16), "CF16 synthetic source"
    xq = oracle.f16_to_f32(h16).view(np.complex64)
    ref = chan_os_ref(oracle, proto, xq)
    for k in range(4):
        want = oracle.f32_to_f16(np.ascontiguousarray(ref[k]).view(np.float32))
        assert np.array_equal(np.ascontiguousarray(y16[k]).view(np.uint16), want.ravel()), "CF16 band %d" % k


def test_generic_s32_words(oracle, proto):
    """7. S32 wire words in: convert_rx on the way in, CF32 out."""
    import torch
    n_in = TILE_IN + 2 * 13
    s32 = torch.empty((n_in, 2), dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(torch.view_as_complex(s32.view(torch.float32)), SEED, 6, 0, fmt="S32")
    plan = os_plan(proto, fmt="S32")
    assert plan.geometry(n_in)["kernel"] == GENERIC
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    y = run(plan, s32)
    x = oracle.convert_rx(to_cpu(s32).ravel())
    assert_bit_exact(x, oracle.synth_iq(SEED, 6, 0, n_in), "S32 synthetic source")
    assert y.dtype == np.complex64
    assert_bands(y, chan_os_ref(oracle, proto, x), "S32 words in")


def test_tiled_equals_generic(oracle):
    """8. The same plan shape under KERNEL_TILED and KERNEL_GENERIC on 4 tiles."""
    h = random_taps(128, 21)
    xg, _ = source(oracle, 8, 4 * TILE_IN)
    a = os_plan(h)
    a.set_kernel(KERNEL_TILED)
    b = os_plan(h)
    b.set_kernel(KERNEL_GENERIC)
    assert a.geometry(4 * TILE_IN)["kernel"] == TILED and b.geometry(4 * TILE_IN)["kernel"] == GENERIC
    assert_bands(run(a, xg), run(b, xg), "tiled vs generic")


def test_it_removes_the_alias(proto):
    """9. A tone 0.0125 cycles per input sample under the edge between bands 0 and 1 (9/80, phases reduced in integers).  The
    critically sampled plan puts it into both bands at +0.45 cycles per output sample (-0.29 dB and -29.56 dB): in band 1 an alias.
    Here band 0 holds it at +0.225 (bin 7344 of 32 640) and band 1 at -0.275 (bin 23 664): two different places, each within
    0.01 dB of the fp64 figure (tests/test_channelizer_os_host.py::test_fp64_figures_of_the_band_edge_tone: -0.29367 and -29.56216 dB,
    bands 2 and 3 peaking at -118.4 and -112.2 dB, nothing else above -300 dB), and every other bin of bands 0 and 1 and all of
    bands 2 and 3 are <= -80 dB.  The 0.01 dB and -80 dB margins for fp32 accumulation are the ones test_takes_the_bands_apart
    (tests/test_gpu_channelizer.py) uses for this prototype; the first 128 outputs (twice the filter's length at fs/2) are dropped
    and the tone is on a bin of the rest, so neither a transient nor leakage uses them."""
    x = edge_tone()
    plan = os_plan(proto)
    assert plan.geometry(x.size)["kernel"] == TILED
    Y = edge_tone_spectra(run(plan, to_gpu(x.astype(np.complex64))))
    rest0, rest1 = np.delete(Y[0], EDGE_TONE_BIN0).max(), np.delete(Y[1], EDGE_TONE_BIN1).max()
    print("band 0 tone %.5f dB, band 1 tone %.5f dB; bands 2, 3 peak %.1f, %.1f dB; other bins of bands 0, 1 peak %.1f, %.1f dB" % (
        Y[0, EDGE_TONE_BIN0], Y[1, EDGE_TONE_BIN1], Y[2].max(), Y[3].max(), rest0, rest1))
    assert abs(Y[0, EDGE_TONE_BIN0] - EDGE_TONE_BAND0_DB) <= 0.01
    assert abs(Y[1, EDGE_TONE_BIN1] - EDGE_TONE_BAND1_DB) <= 0.01
    assert max(rest0, rest1, Y[2].max(), Y[3].max()) <= -80.0


def test_errors(oracle, proto):
    """10. The plan refuses the decimator's and the interpolator's entry points and goes on working; stride and argument errors;
    sxfir_plan_oversampling of the other plan kinds."""
    import torch
    lib = sxxcvr_amd.load_sxfir()
    n_in = TILE_IN
    n_band = n_in // 2
    xg, xs = source(oracle, 9, n_in)
    plan = os_plan(proto)
    y = torch.zeros((4, n_band), dtype=torch.complex64, device="cuda")
    n_out = C.c_size_t(77)
    rc = lib.sxfir_decimate(plan._plan, C.c_void_p(xg.data_ptr()), n_in, n_in, C.c_void_p(y.data_ptr()), n_band, C.byref(n_out), None)
    assert rc == -1 and n_out.value == 0 and b"channelizer" in lib.sxfir_last_error()
    ms = C.c_float()
    assert lib.sxfir_time_decimate(plan._plan, C.c_void_p(xg.data_ptr()), n_in, n_in, C.c_void_p(y.data_ptr()), n_band, 1, None, C.byref(ms)) == -1
    n_out = C.c_size_t(77)
    assert lib.sxfir_interpolate(plan._plan, C.c_void_p(xg.data_ptr()), n_in, n_in, C.c_void_p(y.data_ptr()), n_band, C.byref(n_out), None) == -1
    assert n_out.value == 0
    torch.cuda.synchronize()
    assert plan.position == (0, 0) and int(torch.count_nonzero(torch.view_as_real(y))) == 0
    with pytest.raises(sxxcvr_amd.NativeError) as ei:          # band stride smaller than the outputs per band
        plan.process_ptr(xg.data_ptr(), n_in, n_in, y.data_ptr(), 0, n_band - 1)
    assert ei.value.code == -1 and plan.position == (0, 0)
    assert_bands(run(plan, xg, out=y), chan_os_ref(oracle, proto, xs), "after the refused calls")
    # channels that would overlap the bands
    two = os_plan(proto, nchan=2)
    x2 = torch.zeros((2, n_in), dtype=torch.complex64, device="cuda")
    y2 = torch.zeros((2, 4, n_band), dtype=torch.complex64, device="cuda")
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        two.process_ptr(x2.data_ptr(), n_in, n_in, y2.data_ptr(), 2 * n_band, n_band)
    assert ei.value.code == -1
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Channelizer(proto, oversample=3)
    assert ei.value.code == -4
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Channelizer(proto, nbands=8, oversample=2)
    assert ei.value.code == -4
    assert plan.bands == 4 and plan.oversampling == 2
    crit = sxxcvr_amd.Channelizer(proto)
    assert crit.oversampling == 1 and crit.bands == 4 and crit.ratio == 4
    real = sxxcvr_amd.Resampler(DECIMATE, proto, 4)
    ov = C.c_int(-1)
    assert lib.sxfir_plan_oversampling(real._plan, C.byref(ov)) == 0 and ov.value == 0
    syn = sxxcvr_amd.Synthesizer(design_lowpass(128, 4, gain=4.0))
    ov = C.c_int(-1)
    assert lib.sxfir_plan_oversampling(syn._plan, C.byref(ov)) == 0 and ov.value == 0
