"""Complex-tap (band-pass) interpolators on the GPU (include/sxfir_complex_tx.h), bit for bit against the oracle as it stands.

The reference value is always built the same way: A = a (*) x and B = b (*) x are two real-tap oracle interpolator
passes under the contract the plan reports, then y = (A.re - B.im) + j (A.im + B.re) in float32."""
import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import ComplexInterpolator, design_bandpass, design_lowpass
from sxxcvr_amd.resampler import INTERPOLATE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED
from gpu_util import assert_bit_exact, cx_interp_ref as cx_ref, random_taps_cx as random_taps, to_cpu, to_gpu

pytestmark = pytest.mark.gpu

SEED = 0x7C0FFEE
TILE_IN = {4: 256, 8: 128}                  # inputs per tile of interp_cx_pass_kernel
CX_TILED, CX_GENERIC = "interp_cx_pass_kernel", "interp_cx_generic_kernel"


def band_taps(L, k=1):
    return design_bandpass(32 * L, L, k, L, gain=L)


def source(oracle, channel, n, start=0):
    """The synthetic source on the GPU and its CPU twin."""
    import torch
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, SEED, channel, start)
    return x, oracle.synth_iq(SEED, channel, start, n)


def run(plan, xg, **kw):
    import torch
    y = plan.process(xg, **kw)
    torch.cuda.synchronize()
    return to_cpu(y)


@pytest.mark.parametrize("which", ["bandpass", "random"])
@pytest.mark.parametrize("L", [4, 8])
def test_tiled(oracle, L, which):
    """1. One call of 3 tiles plus 37 inputs through interp_cx_pass_kernel."""
    h = band_taps(L) if which == "bandpass" else random_taps(32 * L)
    n = 3 * TILE_IN[L] + 37
    xg, xs = source(oracle, 0, n)
    plan = ComplexInterpolator(h, L)
    assert plan.mode == INTERPOLATE and plan.complex_taps and tuple(plan.contract) == (2, 1) and plan.contract.rot == 0
    plan.set_kernel(KERNEL_TILED)
    g = plan.geometry(n)
    assert g["tiled"] and g["kernel"] == CX_TILED and g["n_tiles"] == 4 and g["tile_samples"] == L * TILE_IN[L], g
    y = run(plan, xg)
    assert_bit_exact(y, cx_ref(oracle, h, L, xs, plan.contract[0]), "tiled x%d (%s)" % (L, which))
    assert plan.position == (n, L * n)


@pytest.mark.parametrize("L", [4, 8])
def test_streaming_and_history(oracle, L):
    """2. Five calls on one plan (one shorter than the 32-sample history, one of a single input) give the bits of one pass."""
    import torch
    T = TILE_IN[L]
    blocks = [2 * T, 31, T + 5, 1, T]
    n = sum(blocks)
    h = band_taps(L)
    xg, xs = source(oracle, 1, n)
    plan = ComplexInterpolator(h, L)
    ref = cx_ref(oracle, h, L, xs, plan.contract[0])
    outs, pos = [], 0
    for b in blocks:
        assert plan.geometry(b)["kernel"] == CX_TILED
        outs.append(plan.process(xg[pos:pos + b].clone()))
        pos += b
    torch.cuda.synchronize()
    assert_bit_exact(np.concatenate([to_cpu(o) for o in outs]), ref, "streaming %r" % blocks)
    assert plan.position == (n, L * n)
    plan.reset()
    assert plan.position == (0, 0)
    assert_bit_exact(run(plan, xg[:blocks[0]].clone()), to_cpu(outs[0]), "after reset")


@pytest.mark.parametrize("L", [4, 8])
def test_misaligned_output_and_a_failed_call(oracle, L):
    """3. An output pointer offset by one sample: the generic complex kernel, the same bits, the sample in front untouched; with
    KERNEL_TILED forced the same call is refused.  11. The refused call changed nothing: the position and the next call's bits
    (the stream goes on from the first block's history) are what they were."""
    import torch
    T = TILE_IN[L]
    n1, n2 = T + 9, T + 3
    h = band_taps(L)
    xg, xs = source(oracle, 2, n1 + n2)
    plan = ComplexInterpolator(h, L)
    ref = cx_ref(oracle, h, L, xs, plan.contract[0])
    FILL = 0x7FC07FC0
    buf = torch.full((2 * (L * n1 + 1),), FILL, dtype=torch.int32, device="cuda")
    bc = torch.view_as_complex(buf.view(torch.float32).view(-1, 2))
    y1 = run(plan, xg[:n1].clone(), out=bc[1:])
    assert_bit_exact(y1, ref[:L * n1], "misaligned output")
    assert np.all(to_cpu(buf[:2]).view(np.uint32) == FILL), "the sample in front of the output was written"
    assert plan.position == (n1, L * n1)
    plan.set_kernel(KERNEL_TILED)
    buf2 = torch.zeros(L * n2 + 1, dtype=torch.complex64, device="cuda")
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.process(xg[n1:].clone(), out=buf2[1:])
    assert ei.value.code == -4
    assert plan.position == (n1, L * n1)
    for kernel, name in ((KERNEL_AUTO, CX_TILED), (KERNEL_GENERIC, CX_GENERIC)):
        p = plan if kernel == KERNEL_AUTO else None
        if p is None:
            # the same stream on a second plan through the generic kernel: first block, the refused call, second block
            p = ComplexInterpolator(h, L)
            run(p, xg[:n1].clone())
            p.set_kernel(KERNEL_TILED)
            with pytest.raises(sxxcvr_amd.NativeError):
                p.process(xg[n1:].clone(), out=buf2[1:])
        p.set_kernel(kernel)
        assert p.geometry(n2)["kernel"] == name
        assert_bit_exact(run(p, xg[n1:].clone()), ref[L * n1:], "the call after the refused one (%s)" % name)
        assert p.position == (n1 + n2, L * (n1 + n2))


@pytest.mark.parametrize("L", [4, 8])
def test_channels(oracle, L):
    """4. Three channels, strides larger than the block, a distinct source per row; the padding between rows is untouched."""
    import torch
    nchan, n = 3, 2 * TILE_IN[L] + 11
    n_out = L * n
    sin, sout = n + 41, n_out + 26             # (an even output stride: the tiled kernel's 16-byte stores)
    xbuf = torch.zeros((nchan, sin), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(xbuf[:, :n], SEED, 7, 0)
    FILL = 0x7FC07FC0
    ybuf = torch.full((nchan, 2 * sout), FILL, dtype=torch.int32, device="cuda")
    yc = torch.view_as_complex(ybuf.view(torch.float32).view(nchan, sout, 2))
    h = band_taps(L)
    plan = ComplexInterpolator(h, L, nchan=nchan)
    plan.set_kernel(KERNEL_TILED)
    plan.process(xbuf[:, :n], out=yc)
    torch.cuda.synchronize()
    got = to_cpu(yc)
    for c in range(nchan):
        xs = oracle.synth_iq(SEED, 7 + c, 0, n)
        assert_bit_exact(got[c, :n_out], cx_ref(oracle, h, L, xs, plan.contract[0]), "channel %d" % c)
    pad = to_cpu(ybuf).view(np.uint32).reshape(nchan, sout, 2)[:, n_out:, :]
    assert np.all(pad == FILL), "the padding between the rows was written"


@pytest.mark.parametrize("L", [4, 8])
def test_more_tiles_than_resident_workgroups(oracle, L):
    """5. resident + 3 tiles: a call this small is dealt as ONE generation of waves, so the grid is the chip's resident waves and
    three waves walk on to a second tile (the counted wait behind a tile's own stores)."""
    h = band_taps(L)
    plan = ComplexInterpolator(h, L)
    plan.set_kernel(KERNEL_TILED)
    resident = plan.geometry(TILE_IN[L])["resident"]
    n = (resident + 3) * TILE_IN[L]
    g = plan.geometry(n)
    assert g["kernel"] == CX_TILED and g["n_tiles"] == resident + 3 and g["workgroups"] == resident, g
    xg, xs = source(oracle, 3, n)
    y = run(plan, xg)
    assert_bit_exact(y, cx_ref(oracle, h, L, xs, plan.contract[0], threads=oracle.max_threads()), "resident + 3 tiles")


@pytest.mark.parametrize("ntaps,L,forced", [(512, 16, False), (1536, 48, False), (40, 5, False), (128, 4, True)])
def test_generic_shapes(oracle, ntaps, L, forced):
    """6. The generic complex kernel at the shapes without a tiled one, and at x4 x 128 when asked for."""
    h = design_bandpass(ntaps, L, 1, L, gain=L) if ntaps != 40 else random_taps(40, 9)
    n = 700 + 3
    xg, xs = source(oracle, 4, n)
    plan = ComplexInterpolator(h, L)
    real = sxxcvr_amd.Resampler(INTERPOLATE, np.ascontiguousarray(h.real), L)
    assert tuple(plan.contract) == tuple(real.contract) and plan.contract.rot == 0
    if forced:
        plan.set_kernel(KERNEL_GENERIC)
    else:
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            plan.set_kernel(KERNEL_TILED)
        assert ei.value.code == -4
    g = plan.geometry(n)
    assert not g["tiled"] and g["kernel"] == CX_GENERIC, g
    y = run(plan, xg)
    assert_bit_exact(y, cx_ref(oracle, h, L, xs, plan.contract[0]), "generic x%d x %d" % (L, ntaps))
    assert plan.position == (n, L * n)


def test_generic_cf16(oracle):
    """7. CF16 in and out at x4: inputs quantised to half, outputs rounded to half once after the combine."""
    import torch
    n = TILE_IN[4] + 13
    h = band_taps(4)
    xs = oracle.synth_iq(SEED, 5, 0, n)
    x16 = torch.empty(n, dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(x16, SEED, 5, 0, fmt="CF16")
    plan = ComplexInterpolator(h, 4, fmt="CF16")
    assert plan.geometry(n)["kernel"] == CX_GENERIC
    y16 = run(plan, x16).view(np.uint16)
    h16 = oracle.f32_to_f16(xs.view(np.float32))
    assert np.array_equal(to_cpu(x16).view(np.uint16), h16), "CF16 synthetic source"
    xq = oracle.f16_to_f32(h16).view(np.complex64)
    ref16 = oracle.f32_to_f16(cx_ref(oracle, h, 4, xq, plan.contract[0]).view(np.float32))
    assert y16.size == ref16.size and np.array_equal(y16, ref16.ravel())


def test_generic_s32_words(oracle):
    """7. An S32 plan at x4: CF32 in, convert_tx of the combined CF32 result out, under the plan's keying threshold."""
    n = TILE_IN[4] + 13
    h = band_taps(4)
    xg, xs = source(oracle, 6, n)
    xg, xs = xg * 0.5, xs * np.float32(0.5)         # (exact; the x4 gain then keeps the outputs inside the wire words' range)
    plan = ComplexInterpolator(h, 4, fmt="S32")
    assert plan.geometry(n)["kernel"] == CX_GENERIC
    ref = cx_ref(oracle, h, 4, xs, plan.contract[0])
    assert max(np.abs(ref.real).max(), np.abs(ref.imag).max()) < 1.0
    # a threshold that leaves outputs on both sides of the keying rule
    mag2 = ref.real.astype(np.float32) ** 2 + ref.imag.astype(np.float32) ** 2
    thr2 = np.float32(np.median(mag2))
    plan.set_tx_threshold(float(thr2))
    want = oracle.convert_tx(ref, thr2)
    keyed = (want.reshape(-1, 2)[:, 0] & 3) == 3
    assert 0 < keyed.sum() < keyed.size
    y = run(plan, xg)
    assert y.shape == (4 * n, 2) and y.dtype == np.int32
    assert np.array_equal(y.ravel(), want), "S32 words out"


@pytest.mark.parametrize("L", [4, 8])
def test_tiled_equals_generic(oracle, L):
    """8. The same plan shape under KERNEL_TILED and KERNEL_GENERIC on 4 tiles."""
    h = random_taps(32 * L, 21)
    n = 4 * TILE_IN[L]
    xg, _ = source(oracle, 8, n)
    a = ComplexInterpolator(h, L)
    a.set_kernel(KERNEL_TILED)
    b = ComplexInterpolator(h, L)
    b.set_kernel(KERNEL_GENERIC)
    assert a.geometry(n)["kernel"] == CX_TILED and b.geometry(n)["kernel"] == CX_GENERIC
    assert_bit_exact(run(a, xg), run(b, xg), "tiled vs generic")


@pytest.mark.parametrize("kernel", [KERNEL_TILED, KERNEL_GENERIC])
@pytest.mark.parametrize("L", [4, 8])
def test_degenerate_taps(oracle, L, kernel):
    """9. b = 0: the real-tap plan's bits.  a = 0, b = h: j times the real-tap plan's output, bit for bit."""
    h = design_lowpass(32 * L, L, 8.0, float(L))
    xg, _ = source(oracle, 9, 3 * TILE_IN[L])
    real = sxxcvr_amd.Resampler(INTERPOLATE, h, L)
    assert not real.complex_taps
    real.set_kernel(kernel)
    r = run(real, xg)
    p1 = ComplexInterpolator(h.astype(np.complex64), L)
    p1.set_kernel(kernel)
    assert p1.complex_taps and tuple(p1.contract) == tuple(real.contract)
    assert p1.geometry(3 * TILE_IN[L])["kernel"] == (CX_TILED if kernel == KERNEL_TILED else CX_GENERIC)
    assert_bit_exact(run(p1, xg), r, "b = 0")
    p2 = ComplexInterpolator((1j * h).astype(np.complex64), L)
    p2.set_kernel(kernel)
    want = np.empty(r.shape, dtype=np.complex64)
    want.real = np.float32(0.0) - r.imag
    want.imag = np.float32(0.0) + r.real
    assert_bit_exact(run(p2, xg), want, "a = 0")


@pytest.mark.parametrize("ntaps,L,name", [(128, 4, CX_TILED), (256, 8, CX_TILED), (512, 16, CX_GENERIC)])
def test_keyed(oracle, ntaps, L, name):
    """10. sxfir_interpolate_keyed over a range strictly inside the block: the counter a real-tap plan reports for the same
    input, range and threshold, and the unkeyed bits."""
    import torch
    n = 3 * 256 + 37
    first, count = 101, n - 101 - 59
    thr2 = 0.49
    h = design_bandpass(ntaps, L, 1, L, gain=L)
    xg, xs = source(oracle, 11, n)
    st = torch.cuda.current_stream().cuda_stream
    counts = []
    real = sxxcvr_amd.Resampler(INTERPOLATE, np.ascontiguousarray(h.real), L)
    keyed, plain = ComplexInterpolator(h, L), ComplexInterpolator(h, L)
    assert keyed.geometry(n)["kernel"] == name
    outs = []
    for p in (real, keyed):
        p.set_tx_threshold(thr2)
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        out = torch.empty(n * L, dtype=torch.complex64, device="cuda")
        assert p.interpolate_keyed_ptr(xg.data_ptr(), n, n, out.data_ptr(), n * L, first, count, counter.data_ptr(), st) == n * L
        torch.cuda.synchronize()
        counts.append(int(counter.item()))
        outs.append(to_cpu(out))
    want = int(((oracle.convert_tx(xs[first:first + count], np.float32(thr2)).reshape(-1, 2)[:, 0] & 3) == 3).sum())
    assert 0 < want < count
    assert counts == [want, want], counts
    assert_bit_exact(outs[1], run(plain, xg), "keyed against unkeyed")
    assert keyed.position == (n, n * L)


@pytest.mark.parametrize("L,k", [(4, 1), (8, 3)])
def test_places_the_band(L, k):
    """12. A tone 0.1 cycles per input sample above 0 Hz lands at (10 k + 1) / (10 L) cycles per output sample at 0 dB; every other
    bin is at least 90 dB down.  (fp64 on the fp32-rounded taps: 0.0002-0.0003 dB, worst other bin -104.8 dB at x4 band 1 and
    -103.1 dB at x8 band 3; the margin is for fp32 accumulation, as test_takes_the_band_out of the decimators takes it.)"""
    ntaps = 32 * L
    q = np.arange(1 << 14, dtype=np.int64)
    x = np.exp(2j * np.pi * (q % 10) / 10.0).astype(np.complex64)
    plan = ComplexInterpolator(design_bandpass(ntaps, L, k, L, gain=L), L)
    assert plan.geometry(x.size)["kernel"] == CX_TILED
    y = run(plan, to_gpu(x))[ntaps:].astype(np.complex128)
    m = y.size // (10 * L) * (10 * L)
    Y = np.abs(np.fft.fft(y[:m])) / m
    tone = (10 * k + 1) * m // (10 * L)
    wanted = 20 * np.log10(Y[tone])
    Y[tone] = 0.0
    other = 20 * np.log10(max(Y.max(), 1e-300))
    print("x%d band %d: wanted tone %.5f dB, worst other bin %.1f dB" % (L, k, wanted, other))
    assert abs(wanted) <= 0.01
    assert other <= -90.0
