"""Complex-tap (band-pass) decimators on the GPU (include/sxfir_complex.h), bit for bit against the oracle as it stands.

The reference value is always built the same way: A = a (*) x and B = b (*) x are two real-tap oracle passes
under the contract the plan reports, then y = (A.re - B.im) + j (A.im + B.re) in float32."""
import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_bandpass, design_lowpass
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE, KERNEL_GENERIC, KERNEL_TILED
from gpu_util import assert_bit_exact, cx_decim_ref as cx_ref, random_taps_cx as random_taps, to_cpu, to_gpu

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
TILE_IN = 2048
CX_TILED, CX_GENERIC = "decim4_cx_kernel", "decim_cx_generic_kernel"


def source(oracle, channel, n, start=0):
    """The synthetic source on the GPU and its CPU twin."""
    import torch
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, SEED, channel, start)
    return x, oracle.synth_iq(SEED, channel, start, n)


def run(plan, xg):
    import torch
    y = plan.process(xg)
    torch.cuda.synchronize()
    return to_cpu(y)


@pytest.fixture(scope="module")
def band4():
    return design_bandpass(128, 4, 1, 4)


@pytest.mark.parametrize("which", ["bandpass", "random"])
def test_tiled_d4_n128(oracle, band4, which):
    """1. One call of 3 tiles plus a ragged tail through decim4_cx_kernel."""
    h = band4 if which == "bandpass" else random_taps(128)
    n_in = 3 * TILE_IN + 4 * 37
    xg, xs = source(oracle, 0, n_in)
    plan = sxxcvr_amd.Resampler(DECIMATE, h, 4)
    assert plan.complex_taps and tuple(plan.contract) == (2, 4) and plan.contract.rot == 0
    plan.set_kernel(KERNEL_TILED)
    g = plan.geometry(n_in)
    assert g["tiled"] and g["kernel"] == CX_TILED and g["n_tiles"] == 4 and g["tile_samples"] == TILE_IN, g
    y = run(plan, xg)
    assert_bit_exact(y, cx_ref(oracle, h, 4, xs, plan.contract), "tiled /4 x 128 (%s)" % which)
    assert plan.position == (n_in, n_in // 4)


def test_streaming_and_history(oracle, band4):
    """2. Five calls on one plan (one shorter than the 128-sample history, one of a single output) give the bits of one pass."""
    import torch
    blocks = [TILE_IN * 2, 4 * 31, TILE_IN + 4 * 5, 4 * 1, TILE_IN]
    n = sum(blocks)
    xg, xs = source(oracle, 1, n)
    plan = sxxcvr_amd.Resampler(DECIMATE, band4, 4)
    ref = cx_ref(oracle, band4, 4, xs, plan.contract)
    outs, pos = [], 0
    for b in blocks:
        assert plan.geometry(b)["kernel"] == CX_TILED
        outs.append(plan.process(xg[pos:pos + b].clone()))
        pos += b
    torch.cuda.synchronize()
    assert_bit_exact(np.concatenate([to_cpu(o) for o in outs]), ref, "streaming %r" % blocks)
    assert plan.position == (n, n // 4)
    plan.reset()
    assert plan.position == (0, 0)
    assert_bit_exact(run(plan, xg[:blocks[0]].clone()), to_cpu(outs[0]), "after reset")


def test_off_boundary_and_misaligned(oracle, band4):
    """3. A call that starts off an output boundary, and an output pointer offset by one sample: the generic complex kernel."""
    import torch
    n1, n2 = 4 * 100 + 3, TILE_IN
    xg, xs = source(oracle, 2, n1 + n2)
    plan = sxxcvr_amd.Resampler(DECIMATE, band4, 4)
    ref = cx_ref(oracle, band4, 4, xs, plan.contract)
    y1 = plan.process(xg[:n1].clone())
    g = plan.geometry(n2)
    assert not g["tiled"] and g["kernel"] == CX_GENERIC, g
    y2 = plan.process(xg[n1:].clone())
    torch.cuda.synchronize()
    assert y1.numel() == 101 and y2.numel() == (n1 + n2 + 3) // 4 - 101
    assert_bit_exact(np.concatenate([to_cpu(y1), to_cpu(y2)]), ref, "off-boundary second call")
    assert plan.position == (n1 + n2, (n1 + n2 + 3) // 4)
    # set_position: a fresh plan placed where the second call started, its history seeded from the first block
    other = sxxcvr_amd.Resampler(DECIMATE, band4, 4)
    other.set_history_ptr(xg.data_ptr(), n1, n1)
    other.set_position(n1)
    assert_bit_exact(run(other, xg[n1:].clone()), to_cpu(y2), "set_position + set_history")
    # output offset by one sample (8 bytes: not 16-byte aligned)
    plan.reset()
    n3 = TILE_IN + 4 * 9
    buf = torch.zeros(n3 // 4 + 1, dtype=torch.complex64, device="cuda")
    plan.process(xg[:n3].clone(), out=buf[1:])
    torch.cuda.synchronize()
    assert_bit_exact(to_cpu(buf[1:]), ref[:n3 // 4], "misaligned output")
    assert to_cpu(buf[:1]).view(np.uint64)[0] == 0
    plan.set_kernel(KERNEL_TILED)
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.process(xg[:n3].clone(), out=buf[1:])
    assert ei.value.code == -4


def test_channels(oracle, band4):
    """4. Three channels, strides larger than the block, a distinct source per row; the padding between rows is untouched."""
    import torch
    nchan, n_in = 3, 2 * TILE_IN + 4 * 11
    n_out = n_in // 4
    sin, sout = n_in + 40, n_out + 25          # (an even output stride: the tiled kernel's 16-byte stores)
    xbuf = torch.zeros((nchan, sin), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(xbuf[:, :n_in], SEED, 7, 0)
    FILL = 0x7FC07FC0
    ybuf = torch.full((nchan, 2 * sout), FILL - (1 << 32) if FILL >= 1 << 31 else FILL, dtype=torch.int32, device="cuda")
    yc = torch.view_as_complex(ybuf.view(torch.float32).view(nchan, sout, 2))
    plan = sxxcvr_amd.Resampler(DECIMATE, band4, 4, nchan=nchan)
    plan.set_kernel(KERNEL_TILED)
    plan.process(xbuf[:, :n_in], out=yc)
    torch.cuda.synchronize()
    got = to_cpu(yc)
    for c in range(nchan):
        xs = oracle.synth_iq(SEED, 7 + c, 0, n_in)
        assert_bit_exact(got[c, :n_out], cx_ref(oracle, band4, 4, xs, plan.contract), "channel %d" % c)
    pad = to_cpu(ybuf).view(np.uint32).reshape(nchan, sout, 2)[:, n_out:, :]
    assert np.all(pad == FILL), "the padding between the rows was written"


def test_more_tiles_than_resident_workgroups(oracle, band4):
    """5. resident + 3 tiles: a call this small is dealt as ONE generation of waves (four tiles per wave would need more), so the
    grid is the chip's resident waves, a multiple of 8 -- the XCD-blocked dealing -- and three waves walk on to a second tile."""
    plan = sxxcvr_amd.Resampler(DECIMATE, band4, 4)
    plan.set_kernel(KERNEL_TILED)
    resident = plan.geometry(TILE_IN)["resident"]
    n_in = (resident + 3) * TILE_IN
    g = plan.geometry(n_in)
    assert g["kernel"] == CX_TILED and g["n_tiles"] == resident + 3 and g["workgroups"] == resident and resident % 8 == 0, g
    xg, xs = source(oracle, 3, n_in)
    y = run(plan, xg)
    assert_bit_exact(y, cx_ref(oracle, band4, 4, xs, plan.contract, threads=oracle.max_threads()), "resident + 3 tiles")


@pytest.mark.parametrize("ntaps,D,contract", [(256, 8, (2, 4, 0)), (1024, 32, (2, 4, 0)), (1536, 48, (2, 4, 1)), (35, 5, (1, 5, 0))])
def test_generic_shapes(oracle, ntaps, D, contract):
    """6. The generic complex kernel at the shapes without a tiled one."""
    h = design_bandpass(ntaps, D, 1, D) if ntaps != 35 else random_taps(35, 9)
    n_in = D * 700 + 3
    xg, xs = source(oracle, 4, n_in)
    plan = sxxcvr_amd.Resampler(DECIMATE, h, D)
    c = plan.contract
    assert c.rot == contract[2] and tuple(c) == contract[:2], (tuple(c), c.rot)
    g = plan.geometry(n_in)
    assert not g["tiled"] and g["kernel"] == CX_GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    y = run(plan, xg)
    assert_bit_exact(y, cx_ref(oracle, h, D, xs, plan.contract), "generic /%d x %d" % (D, ntaps))


def test_generic_cf16(oracle, band4):
    """6. CF16 in and out at /4: inputs quantised to half, outputs rounded to half once after the combine."""
    import torch
    n_in = TILE_IN + 4 * 13
    xs = oracle.synth_iq(SEED, 5, 0, n_in)
    x16 = torch.empty(n_in, dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(x16, SEED, 5, 0, fmt="CF16")
    plan = sxxcvr_amd.Resampler(DECIMATE, band4, 4, fmt="CF16")
    assert plan.geometry(n_in)["kernel"] == CX_GENERIC
    y16 = run(plan, x16).view(np.uint16)
    h16 = oracle.f32_to_f16(xs.view(np.float32))
    assert np.array_equal(to_cpu(x16).view(np.uint16), h16), "CF16 synthetic source"
    xq = oracle.f16_to_f32(h16).view(np.complex64)
    ref16 = oracle.f32_to_f16(cx_ref(oracle, band4, 4, xq, plan.contract).view(np.float32))
    assert y16.size == ref16.size and np.array_equal(y16, ref16.ravel())


def test_generic_s32_words(oracle, band4):
    """6. S32 wire words in at /4: convert_rx on the way in, CF32 out."""
    import torch
    n_in = TILE_IN + 4 * 13
    s32 = torch.empty((n_in, 2), dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(torch.view_as_complex(s32.view(torch.float32)), SEED, 6, 0, fmt="S32")
    plan = sxxcvr_amd.Resampler(DECIMATE, band4, 4, fmt="S32")
    assert plan.geometry(n_in)["kernel"] == CX_GENERIC
    y = run(plan, s32)
    x = oracle.convert_rx(to_cpu(s32).ravel())
    assert_bit_exact(x, oracle.synth_iq(SEED, 6, 0, n_in), "S32 synthetic source")
    assert_bit_exact(y, cx_ref(oracle, band4, 4, x, plan.contract), "S32 words in")


def test_tiled_equals_generic(oracle):
    """7. The same plan shape under KERNEL_TILED and KERNEL_GENERIC on 4 tiles."""
    h = random_taps(128, 21)
    xg, _ = source(oracle, 8, 4 * TILE_IN)
    a = sxxcvr_amd.Resampler(DECIMATE, h, 4)
    a.set_kernel(KERNEL_TILED)
    b = sxxcvr_amd.Resampler(DECIMATE, h, 4)
    b.set_kernel(KERNEL_GENERIC)
    assert a.geometry(4 * TILE_IN)["kernel"] == CX_TILED and b.geometry(4 * TILE_IN)["kernel"] == CX_GENERIC
    assert_bit_exact(run(a, xg), run(b, xg), "tiled vs generic")


@pytest.mark.parametrize("kernel", [KERNEL_TILED, KERNEL_GENERIC])
def test_degenerate_taps(oracle, kernel):
    """8. b = 0: the real-tap plan's bits.  a = 0, b = h: j times the real-tap plan's output, bit for bit."""
    h = design_lowpass(128, 4)
    xg, _ = source(oracle, 9, 3 * TILE_IN)
    real = sxxcvr_amd.Resampler(DECIMATE, h, 4)
    assert not real.complex_taps
    real.set_kernel(kernel)
    r = run(real, xg)
    p1 = sxxcvr_amd.Resampler(DECIMATE, h.astype(np.complex64), 4)
    p1.set_kernel(kernel)
    assert p1.complex_taps and tuple(p1.contract) == tuple(real.contract)
    assert_bit_exact(run(p1, xg), r, "b = 0")
    p2 = sxxcvr_amd.Resampler(DECIMATE, (1j * h).astype(np.complex64), 4)
    p2.set_kernel(kernel)
    want = np.empty(r.shape, dtype=np.complex64)
    want.real = np.float32(0.0) - r.imag
    want.imag = np.float32(0.0) + r.real
    assert_bit_exact(run(p2, xg), want, "a = 0")


def test_takes_the_band_out(band4):
    """9. Sub-band 1 of the /4 raster: a tone 0.1/4 above the band centre lands at +0.1 cycles per output sample at 0 dB, a tone
    in the neighbouring band (2/4 - 0.15/4) is at least 80 dB down (the fp64 response gives 95.2 dB; the margin is for fp32
    accumulation and the truncated transient)."""
    n = 1 << 16
    k = np.arange(n, dtype=np.int64)
    # 1/4 + 0.1/4 = 11/40 and 2/4 - 0.15/4 = 37/80 cycles per sample, phases reduced in integers
    x = np.exp(2j * np.pi * ((k * 11) % 40) / 40.0) + np.exp(2j * np.pi * ((k * 37) % 80) / 80.0)
    plan = sxxcvr_amd.Resampler(DECIMATE, band4, 4)
    assert plan.geometry(n)["kernel"] == CX_TILED
    y = run(plan, to_gpu(x.astype(np.complex64)))[64:].astype(np.complex128)
    m = y.size
    assert m == 16320
    Y = np.abs(np.fft.fft(y)) / m
    wanted = 20 * np.log10(Y[1632])                      # +0.1 cycles per output sample
    other = 20 * np.log10(max(Y[m - 2448], 1e-300))      # 4 (37/80 - 1/4) = 0.85 = -0.15 cycles per output sample
    print("wanted tone %.5f dB, neighbour %.1f dB" % (wanted, other))
    assert abs(wanted) <= 0.01
    assert other <= -80.0


def test_errors(band4):
    """10."""
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.Resampler(INTERPOLATE, band4, 4)
    assert ei.value.code == -4
    p32 = sxxcvr_amd.Resampler(DECIMATE, design_bandpass(1024, 32, 3, 32), 32)
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        p32.set_kernel(KERNEL_TILED)
    assert ei.value.code == -4
    assert p32.complex_taps is True
    assert sxxcvr_amd.Resampler(DECIMATE, design_lowpass(1024, 32), 32).complex_taps is False


def test_pipelined_resampler_passes_complex_taps_through(oracle, band4):
    import torch
    blocks = [TILE_IN, TILE_IN + 4 * 7, 4 * 64 + 2, TILE_IN]
    n = sum(blocks)
    xg, xs = source(oracle, 10, n)
    pr = sxxcvr_amd.PipelinedResampler(DECIMATE, band4, 4, depth=2)
    assert all(p.complex_taps for p in pr.plans)
    y = torch.zeros((n + 3) // 4, dtype=torch.complex64, device="cuda")
    pos = done = 0
    for b in blocks:
        done += pr.process_ptr(xg.data_ptr() + 8 * pos, b, b, y.data_ptr() + 8 * done, (n + 3) // 4)
        pos += b
    pr.join()
    torch.cuda.synchronize()
    assert done == (n + 3) // 4
    assert_bit_exact(to_cpu(y), cx_ref(oracle, band4, 4, xs, pr.contract), "pipelined")
