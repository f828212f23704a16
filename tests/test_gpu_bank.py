"""The tuner bank on the GPU (include/sxfir_bank.h), bit for bit against tests/bank_cases.py: per band the translating decimator's
reference (mix_cases.mix_ref), and on the GPU the TranslatingDecimator of the same band under the same kernel request.

Every call goes through `Rig.call`: each band's row lands between two guards of fill words that must come back untouched, and the
plan's position, outputs_for and geometry(...)["kernel"] are checked around it.  The two layout tests (`_laid_out`) name both
strides themselves: bands and channels that overlap, and channels inside bands.  The seeded sweep is tests/test_gpu_bank_sweep.py."""
import ctypes as C

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import TranslatingBank, TranslatingDecimator, design_bandpass
from sxxcvr_amd.resampler import DECIMATE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED
from bank_cases import (EINVAL, EUNSUPPORTED, FILL, GENERIC, GUARD, PAIRS, TILE, TILED, Rig, _i32, bank_f64,
                        cdiv, same)
from gpu_util import random_taps_cx
from mix_cases import bound, mix_ref
from rational_cases import gaussian_stream

pytestmark = pytest.mark.gpu

TOTALS = [TILE - 4, TILE, 2 * TILE + 140, 3 * TILE + 28]
HS = np.stack([random_taps_cx(128, 31 + k) for k in range(16)])           # sixteen different tap sets
# sixteen different centres: bands 0 and 4 share den 7, bands 2 and 6 den 65536
SIXTEEN = PAIRS + [(5, 7), (1, 3), (65535, 65536), (65534, 65535), (2, 9), (7, 11), (12, 13), (100, 1001), (0, 1), (1, 2), (4093, 4096), (9, 31)]


def streams(nchan, n, seed=3):
    return np.stack([gaussian_stream(n, seed + 17 * c) for c in range(nchan)])


def bank4(hs, centres, kernel=KERNEL_AUTO, nchan=1):
    plan = TranslatingBank(hs, 4, centres, nchan=nchan)
    assert plan.complex_taps and plan.mode == DECIMATE and tuple(plan.contract) == (2, 4) and plan.contract.rot == 0
    assert plan.nbands == len(centres) and plan.centres == [(n % d, d) for n, d in centres]
    plan.set_kernel(kernel)
    return plan


def single_plans(rig, hs, centres, kernel, D=4, fmt="CF32"):
    """[nchan, K, words]: every band through the TranslatingDecimator of its taps and centre, under `kernel`, over the rig's stream"""
    import torch
    out = []
    x = rig.xg[:, :rig.n * rig.wps_in]
    if fmt == "CF32":
        x = torch.view_as_complex(x.view(torch.float32).reshape(rig.nchan, rig.n, 2))
    for k, (num, den) in enumerate(centres):
        plan = TranslatingDecimator(hs[k], D, num, den, nchan=rig.nchan, fmt=fmt)
        plan.set_kernel(kernel)
        y = plan.process(x.contiguous())
        torch.cuda.synchronize()
        out.append(y.cpu().numpy().view(np.uint32).reshape(rig.nchan, -1))
    return np.stack(out, axis=1)


# ---- the tiled kernel, /4 x 128 on CF32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("n", TOTALS)
def test_tiled_auto_tiled_generic(oracle, n, K):
    hs, centres = HS[:K], PAIRS[:K]
    rig = Rig(oracle, streams(1, n, 5))
    g = bank4(hs, centres).geometry(n)
    assert g["tiled"] and g["kernel"] == TILED and g["n_tiles"] == cdiv(n, TILE) and g["tile_samples"] == TILE, g
    ref = rig.ref(hs, 4, bank4(hs, centres).contract, centres)
    assert ref.shape == (1, K, 2 * (n // 4))
    for what, request, name in (("auto", KERNEL_AUTO, TILED), ("tiled", KERNEL_TILED, TILED), ("generic", KERNEL_GENERIC, GENERIC)):
        got = rig.stream(bank4(hs, centres, request), [n], [name])
        same(got, ref, what)
        same(got, single_plans(rig, hs, centres, request), what + " against the single-band plans on the GPU")


def test_sixteen_bands(oracle):
    """The argument array's last slot: sixteen different taps and centres, two pairs of bands sharing a table."""
    n = 2 * TILE + 140
    rig = Rig(oracle, streams(1, n, 4))
    assert len(set(SIXTEEN)) == 16 and len({d for _, d in SIXTEEN}) == 14
    ref = rig.ref(HS, 4, bank4(HS, SIXTEEN).contract, SIXTEEN)
    same(rig.stream(bank4(HS, SIXTEEN), [n], [TILED]), ref, "tiled")
    same(rig.stream(bank4(HS, SIXTEEN, KERNEL_GENERIC), [n], [GENERIC]), ref, "generic")


def test_negative_num_is_reduced(oracle):
    n = TILE + 140
    rig = Rig(oracle, streams(1, n, 4))
    plan = TranslatingBank(HS[:2], 4, [(-4 - 7 * 1000, 7), (1000 + 123, 1000)])
    assert plan.centres == [(3, 7), (123, 1000)]
    same(rig.stream(plan, [n], [TILED]), rig.ref(HS[:2], 4, plan.contract, [(3, 7), (123, 1000)]), "reduced centres")


@pytest.mark.parametrize("n", [TOTALS[0], TOTALS[3]])
def test_splits(oracle, n):
    """A stream cut at multiples of 4 stays tiled; a cut elsewhere runs the generic kernel for the call that starts off the output
    boundary (under a forced TILED: refused, plan and output untouched) and the stream comes back; a first call shorter than the
    128-sample history; five calls through both kernels give the bits of one call, on every band."""
    hs, centres = HS[:3], [(123, 1000), (3, 7), (12345, 65536)]
    rig = Rig(oracle, streams(1, n, 6))
    ref = rig.ref(hs, 4, bank4(hs, centres).contract, centres)
    a, b = 4 * 77, 4 * 131
    same(rig.stream(bank4(hs, centres), [a, b, n - a - b], [TILED] * 3), ref, "cut at multiples of 4")
    same(rig.stream(bank4(hs, centres), [a + 2, b, n - a - b - 2], [TILED, GENERIC, GENERIC]), ref, "cut off the boundary")
    same(rig.stream(bank4(hs, centres), [a + 2, 2, n - a - 4], [TILED, GENERIC, TILED]), ref, "back on the boundary")
    same(rig.stream(bank4(hs, centres), [100, n - 100], [TILED, TILED]), ref, "100 samples, then the rest")
    same(rig.stream(bank4(hs, centres), [a + 2, 2, 100, 3, n - a - 107], [TILED, GENERIC, TILED, TILED, GENERIC]), ref, "five calls")
    # a cut at 4 * 50 + 1: the next call is the generic kernel's under AUTO, refused under TILED
    plan = bank4(hs, centres)
    c1 = 4 * 50 + 1
    k1 = 2 * cdiv(c1, 4)
    same(rig.call(plan, 0, c1, TILED), ref[:, :, :k1], "first block")
    plan.set_kernel(KERNEL_TILED)
    rig.call(plan, c1, n - c1, GENERIC, expect=EUNSUPPORTED)
    plan.set_kernel(KERNEL_AUTO)
    same(rig.call(plan, c1, n - c1, GENERIC), ref[:, :, k1:], "the call after the refused one")


def test_three_channels(oracle):
    n = TOTALS[2]
    hs, centres = HS[:3], PAIRS[:3]
    rig = Rig(oracle, streams(3, n, 8), pad=41)
    ref = rig.ref(hs, 4, bank4(hs, centres).contract, centres)
    same(rig.stream(bank4(hs, centres, KERNEL_TILED, nchan=3), [n], [TILED]), ref, "tiled")
    same(rig.stream(bank4(hs, centres, KERNEL_GENERIC, nchan=3), [4 * 33 + 1, n - 4 * 33 - 1], [GENERIC] * 2), ref, "generic")
    same(rig.call(bank4(hs, centres, KERNEL_TILED, nchan=3), 0, n, TILED, slack=5), ref, "a band stride larger than the outputs, tiled")
    same(rig.call(bank4(hs, centres, KERNEL_GENERIC, nchan=3), 0, n, GENERIC, slack=5), ref, "a band stride larger than the outputs, generic")


def test_strides(oracle):
    """An odd out_stride, an odd band_stride or an output offset by one sample break the 16-byte stores: the generic kernel under
    AUTO, the same bits; SXFIR_EUNSUPPORTED, plan and output untouched, under a forced TILED.  A band_stride below the outputs per
    band: SXFIR_EINVAL whatever the kernel."""
    hs, centres = HS[:3], [(3, 7), (123, 1000), (1, 4)]
    n = TILE + 140
    rig = Rig(oracle, streams(3, n, 16))
    ref = rig.ref(hs, 4, bank4(hs, centres).contract, centres)
    breaks = [dict(odd_stride=True), dict(odd_band=True), dict(offset=1)]
    for kw in breaks:
        same(rig.call(bank4(hs, centres, nchan=3), 0, n, **kw), ref, "%r under AUTO" % kw)
    plan = bank4(hs, centres, KERNEL_TILED, nchan=3)
    for kw in breaks:
        rig.call(plan, 0, n, TILED, expect=EUNSUPPORTED, **kw)
    same(rig.call(plan, 0, n, TILED), ref, "the call after the refused ones")
    for request in (KERNEL_AUTO, KERNEL_TILED, KERNEL_GENERIC):
        plan = bank4(hs, centres, request, nchan=3)
        rig.call(plan, 0, n, expect=EINVAL, short_band=True)
        same(rig.call(plan, 0, n), ref, "the call after the short band stride")
    # one channel: an odd band stride alone breaks the alignment of every second band
    one = Rig(oracle, streams(1, n, 16))
    same(one.call(bank4(hs, centres), 0, n, odd_band=True), ref[:1], "one channel, odd band stride under AUTO")
    one.call(bank4(hs, centres, KERNEL_TILED), 0, n, TILED, expect=EUNSUPPORTED, odd_band=True)


def _laid_out(rig, plan, n, out_stride, band_stride, expect=None, timed=False):
    """sxfir_decimate_bank (timed: sxfir_time_decimate_bank, one pass) over inputs [0, n) with the two strides as given, the first
    output GUARD samples into a buffer of fill that holds either nesting.  Returns [nchan, K, words], everything else still fill; with
    `expect` the call must fail with that code and leave the plan and the whole buffer alone."""
    import torch
    K, nchan = plan.nbands, rig.nchan
    n_out = plan.outputs_for(n)
    pos = plan.position
    at = [[GUARD + c * out_stride + k * band_stride for k in range(K)] for c in range(nchan)]
    total = max(max(r) for r in at) + n_out + GUARD
    buf = torch.full((total, rig.wps), _i32(FILL), dtype=torch.int32, device="cuda")
    args = (rig.xg.data_ptr(), n, rig.stride, buf.data_ptr() + rig.sb * GUARD, out_stride, band_stride)
    stream = torch.cuda.current_stream().cuda_stream
    if expect is not None:
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            plan.time_ptr(*args, 1, stream) if timed else plan.process_ptr(*args, stream)
        torch.cuda.synchronize()
        assert ei.value.code == expect and plan.position == pos
        assert np.all(buf.cpu().numpy().view(np.uint32) == FILL), "a refused call wrote to the output"
        return None
    if timed:
        assert plan.time_ptr(*args, 1, stream) > 0.0 and plan.position == pos
    else:
        assert plan.process_ptr(*args, stream) == n_out and plan.position == (pos[0] + n, pos[1] + n_out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    rows = np.zeros(total, dtype=bool)
    for r in at:
        for a in r:
            assert not rows[a:a + n_out].any(), "two rows overlap"
            rows[a:a + n_out] = True
    assert np.all(got[~rows] == FILL), "something outside the %d x %d rows was written" % (K, nchan)
    return np.stack([np.stack([got[a:a + n_out].reshape(-1) for a in r]) for r in at])


def test_overlapping_bands_and_channels(oracle):
    """Three channels, three bands, strides under which neither nesting holds: out_stride one short of a channel's three rows, and
    band_stride far below three channels' rows.  SXFIR_EINVAL whatever the kernel request (check_band_layout comes in front of the
    kernel choice), plan and output untouched, through sxfir_decimate_bank and sxfir_time_decimate_bank; the next call gives the
    reference's bits."""
    hs, centres, K = HS[:3], [(3, 7), (123, 1000), (12345, 65536)], 3
    n = TILE + 144
    rig = Rig(oracle, streams(3, n, 18))
    ref = rig.ref(hs, 4, bank4(hs, centres).contract, centres)
    n_out = n // 4
    band = n_out + 12                                           # an even band stride, and an even out_stride once it holds the rows
    short = (K - 1) * band + n_out - 1
    assert band % 2 == 0 and (short + 1) % 2 == 0 and n_out <= band < 2 * short + n_out and short >= n_out
    for request, name in ((KERNEL_AUTO, TILED), (KERNEL_TILED, TILED), (KERNEL_GENERIC, GENERIC)):
        plan = bank4(hs, centres, request, nchan=3)
        assert plan.geometry(n)["kernel"] == name
        _laid_out(rig, plan, n, short, band, expect=EINVAL)
        assert b"overlap" in plan._lib.sxfir_last_error()
        _laid_out(rig, plan, n, short, band, expect=EINVAL, timed=True)
        assert b"overlap" in plan._lib.sxfir_last_error()
        same(_laid_out(rig, plan, n, short + 1, band), ref, "one sample more: bands inside channels, request %d" % request)
        plan.reset()
        same(rig.call(plan, 0, n, name), ref, "the call after the refused ones, request %d" % request)


def test_channels_inside_bands(oracle):
    """The output's other nesting: a band's three channels in a row, band after band (band_stride >= (nchan - 1) * out_stride +
    n_out).  One tiled call of a tile and 140 samples, the same call on the generic kernel, and a timed pass of each: the
    reference's bits in every row, nothing written between them."""
    hs, centres = HS[:3], [(123, 1000), (65535, 65536), (1, 3)]
    n = TILE + 140
    rig = Rig(oracle, streams(3, n, 19))
    ref = rig.ref(hs, 4, bank4(hs, centres).contract, centres)
    n_out = n // 4
    chan = n_out + 7                                            # even, larger than the block
    band = 2 * chan + n_out + 9                                 # even, larger than three channels' rows
    assert chan % 2 == 0 and band % 2 == 0 and chan < 2 * band + n_out
    for request, name in ((KERNEL_TILED, TILED), (KERNEL_AUTO, TILED), (KERNEL_GENERIC, GENERIC)):
        plan = bank4(hs, centres, request, nchan=3)
        g = plan.geometry(n)
        assert g["kernel"] == name and g["tiled"] == (name == TILED), g
        same(_laid_out(rig, plan, n, chan, band, timed=True), ref, "%s, a timed pass" % name)
        same(_laid_out(rig, plan, n, chan, band), ref, name)
    # an odd stride between the channels of a band: the generic kernel under AUTO, refused under a forced TILED
    same(_laid_out(rig, bank4(hs, centres, nchan=3), n, chan + 1, band + 2), ref, "odd out_stride under AUTO")
    _laid_out(rig, bank4(hs, centres, KERNEL_TILED, nchan=3), n, chan + 1, band + 2, expect=EUNSUPPORTED)


# ---- more tiles than waves: the tile loop's second iteration ----------------------------------------------------------------------
WALK_SEED = 0x3A1C
WALK_CENTRES = [(3, 7), (65535, 65536), (1, 3)]


def _walk(oracle, nchan=1, where=0):
    """tests/test_gpu_mix.py's _walk for a bank of three bands: one tiled call of 3 tiles and 140 samples more than the grid has waves
    (per channel), so that four waves walk on to a second tile -- every band's phase word advanced and wrapped, the next tile's
    staging over an image the last band has just read -- and the wave that carries the history over owns two tiles.  The whole call
    is compared on the GPU with the bank's generic kernel over the same input; five windows of 200 outputs of every band and the
    whole of a second tiled call of TILE + 8 samples are compared with the oracle's reference, from inputs regenerated for each
    window alone.  Returns the first call's geometry and size."""
    import torch
    hs, centres, K = HS[:3], WALK_CENTRES, 3
    lead = 256 if where else 0                                  # (a placed plan: the samples in front are its history)
    assert where % 4 == 0 and lead % 4 == 0
    plans = [bank4(hs, centres, k, nchan) for k in (KERNEL_TILED, KERNEL_GENERIC)]
    contract = plans[0].contract
    per = plans[0].geometry(TILE)["resident"] // nchan
    n, n2 = (per + 3) * TILE + 140, TILE + 8
    x = torch.empty((nchan, lead + n + n2), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, WALK_SEED, 40, 0)
    stream = torch.cuda.current_stream().cuda_stream
    for plan in plans:
        if where:
            plan.set_history_ptr(x.data_ptr(), lead, x.stride(0), stream)
            plan.set_position(where)
        assert plan.position == (where, where // 4)
    g = plans[0].geometry(n)
    G = g["workgroups"] // nchan                                # waves per channel: the first tile a wave reaches in its second iteration
    assert g["kernel"] == TILED and g["tiled"] and g["tile_samples"] == TILE and g["n_tiles"] == per + 4, g
    assert G < g["n_tiles"] and G == per, "no wave walks to a second tile: %r" % (g,)
    assert plans[1].geometry(n)["kernel"] == GENERIC

    def call(plan, pos, count):
        """sxfir_decimate_bank over inputs [pos, pos + count) of the stream, every band's row between guards of fill: int32 [nchan, K, row, 2]"""
        n_out = count // 4
        row = 2 * GUARD + n_out + n_out % 2
        buf = torch.full((nchan, K, row, 2), _i32(FILL), dtype=torch.int32, device="cuda")
        c0, p0 = plan.position
        assert plan.outputs_for(count) == n_out
        assert plan.process_ptr(x.data_ptr() + 8 * (lead + pos), count, x.stride(0), buf.data_ptr() + 8 * GUARD, K * row, row, stream) == n_out
        assert plan.position == (c0 + count, p0 + n_out)
        assert bool((buf[:, :, :GUARD] == _i32(FILL)).all()) and bool((buf[:, :, GUARD + n_out:] == _i32(FILL)).all()), "the guard around a band's outputs was written"
        return buf, n_out

    def window(c, k, m0, cnt):
        """[cnt, 2] words of outputs [m0, m0 + cnt) of band k (the stream's first output: the absolute where / 4), channel c"""
        pre = min(128, lead + 4 * m0)                           # samples in front of the window: the filter's reach, or all there are
        assert pre == 128 or (pre == 4 * m0 and lead == 0)
        xw = oracle.synth_iq(WALK_SEED, 40 + c, lead + 4 * m0 - pre, pre + 4 * cnt)
        num, den = centres[k]
        return mix_ref(oracle, hs[k], 4, xw, contract, num, den, where // 4 + m0 - pre // 4)[pre // 4:].view(np.uint32).reshape(cnt, 2)

    got, n_out = call(plans[0], 0, n)
    other, _ = call(plans[1], 0, n)
    torch.cuda.synchronize()
    assert torch.equal(got, other), "the tiled and the generic kernel differ: first at (channel, band, output) %r" % (
        (got != other).any(dim=3).nonzero()[0].tolist(),)
    starts = {"the stream's start": 0, "the first tile of a second iteration": G * 512, "the seam in front of it": G * 512 - 100,
              "the middle": n_out // 2 + 3, "the last, ragged tile": n_out - 200}
    assert n_out % 512 == 35
    for what, m0 in starts.items():
        for c in range(nchan):
            for k in range(K):
                same(got[c, k, GUARD + m0:GUARD + m0 + 200].cpu().numpy().view(np.uint32), window(c, k, m0, 200), "%s, channel %d, band %d" % (what, c, k))
    # the history was carried over by a wave that owned more than one tile
    assert (g["n_tiles"] - 1) % G < g["n_tiles"] - G
    assert plans[0].geometry(n2)["kernel"] == TILED
    second, n_out2 = call(plans[0], n, n2)
    torch.cuda.synchronize()
    for c in range(nchan):
        for k in range(K):
            same(second[c, k, GUARD:GUARD + n_out2].cpu().numpy().view(np.uint32), window(c, k, n_out, n_out2), "the call after it, channel %d, band %d" % (c, k))
    print("%d ch from %d: resident %d, grid %d per channel, %d tiles, %d samples" % (nchan, where, g["resident"], G, g["n_tiles"], n))
    return g, n


def test_more_tiles_than_resident_workgroups(oracle):
    """One channel: the grid is the chip's resident waves, a multiple of 8 -- the XCD-blocked dealing (w8 != 0).  (3, 7) and (1, 3):
    more tiles than table entries; (65535, 65536): s at the top of the table."""
    g, n = _walk(oracle)
    assert g["workgroups"] == g["resident"] and g["resident"] % 8 == 0, g


def test_more_tiles_than_workgroups_channels_off_the_multiple_of_8(oracle):
    """Three channels (or the count in 2..5 that does it): the grid per channel is no multiple of 8, so the tiles are dealt plainly
    strided (w8 = 0)."""
    resident = bank4(HS[:3], WALK_CENTRES).geometry(TILE)["resident"]
    nchan = next(c for c in (3, 2, 4, 5) if (resident // c) % 8 and (resident // c * c) % 8)
    g, n = _walk(oracle, nchan=nchan)
    assert (g["workgroups"] // nchan) % 8 != 0 and g["workgroups"] % 8 != 0, g


def test_more_tiles_than_resident_workgroups_far(oracle):
    """The same many-tile call on a plan placed at input 2^40 + 20: every band's phase comes from a 64-bit position."""
    _walk(oracle, where=(1 << 40) + 20)


# ---- the generic kernel at the shapes and formats without a tiled one ----------------------------------------------------------
@pytest.mark.parametrize("ntaps,D,fmt,contract", [(256, 8, "CF32", (2, 4, 0)), (35, 5, "CF32", (1, 5, 0)), (128, 4, "CF16", (2, 4, 0)),
                                                  (128, 4, "S32", (2, 4, 0)), (1536, 48, "CF32", (2, 4, 1))])
def test_generic_shapes(oracle, ntaps, D, fmt, contract):
    hs = np.stack([random_taps_cx(ntaps, 9), random_taps_cx(ntaps, 10)])
    centres = [(123, 1000), (3, 7)]
    n = D * 600 + 3
    rig = Rig(oracle, streams(2, n, 9), fmt)
    plan = TranslatingBank(hs, D, centres, nchan=2, fmt=fmt)
    c = plan.contract
    assert c.rot == contract[2] and tuple(c) == contract[:2], (tuple(c), c.rot)
    assert plan.complex_taps and plan.nbands == 2
    g = plan.geometry(n)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == EUNSUPPORTED
    ref = rig.ref(hs, D, plan.contract, centres)
    assert ref.shape[2] == 601 * rig.wps
    same(rig.stream(plan, [n], [GENERIC]), ref, "one call")
    again = TranslatingBank(hs, D, centres, nchan=2, fmt=fmt)
    same(rig.stream(again, [D * 7 + 1, 1, n - D * 7 - 2], [GENERIC] * 3), ref, "three calls")
    if fmt != "S32":
        same(ref, single_plans(rig, hs, centres, KERNEL_AUTO, D, fmt), "the single-band plans on the GPU")


# ---- the frame -----------------------------------------------------------------------------------------------------------------
def test_frame(oracle):
    import torch
    lib = sxxcvr_amd.load_sxfir()
    vp = C.c_void_p
    hs, centres, K = HS[:3], PAIRS[:3], 3
    n = TILE + 140
    rig = Rig(oracle, streams(3, n, 12))
    plan = bank4(hs, centres, nchan=3)
    ref = rig.ref(hs, 4, plan.contract, centres)
    n1 = 4 * 61
    k1 = 2 * (n1 // 4)
    assert plan.outputs_for(n1) == n1 // 4 and plan.outputs_for(3) == 1
    same(rig.call(plan, 0, n1, TILED), ref[:, :, :k1], "first block")
    pos = plan.position
    assert plan.outputs_for(4) == 1 and plan.outputs_for(5) == 2        # (output m is complete with input 4 m)
    out = torch.full((3, 8 * n), 0.0, dtype=torch.complex64, device="cuda")
    got, ms, counter = C.c_size_t(77), C.c_float(), torch.zeros(1, dtype=torch.int64, device="cuda")
    io = (plan._plan, vp(rig.xg.data_ptr() + 8 * n1), n - n1, rig.stride, vp(out.data_ptr()), 8 * n)
    refused = {
        "sxfir_decimate": lambda: lib.sxfir_decimate(*io, C.byref(got), None),
        "sxfir_time_decimate": lambda: lib.sxfir_time_decimate(*io, 1, None, C.byref(ms)),
        "sxfir_interpolate": lambda: lib.sxfir_interpolate(*io, C.byref(got), None),
        "sxfir_interpolate_keyed": lambda: lib.sxfir_interpolate_keyed(*io, C.byref(got), 0, 8, vp(counter.data_ptr()), None),
        "sxfir_time_interpolate": lambda: lib.sxfir_time_interpolate(*io, 1, None, C.byref(ms)),
        "sxfir_channelize": lambda: lib.sxfir_channelize(*io, 2 * n, C.byref(got), None),
        "sxfir_synthesize": lambda: lib.sxfir_synthesize(*io[:4], 2 * n, *io[4:], C.byref(got), None),
        "sxfir_resample": lambda: lib.sxfir_resample(*io, C.byref(got), None),
        "sxfir_time_resample": lambda: lib.sxfir_time_resample(*io, 1, None, C.byref(ms)),
        "sxfir_resample_arbitrary": lambda: lib.sxfir_resample_arbitrary(*io, C.byref(got), None),
    }
    for name, fn in refused.items():
        got.value = 77
        assert fn() == EINVAL, name
        assert plan.position == pos, name
        assert got.value in (0, 77), name
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and float(out.abs().max().item()) == 0.0
    # sxfir_decimate_bank refuses every other plan the same way
    single = TranslatingDecimator(hs[0], 4, 3, 7, nchan=3)
    got.value = 77
    assert lib.sxfir_decimate_bank(single._plan, *io[1:], 2 * n, C.byref(got), None) == EINVAL and got.value == 0
    assert lib.sxfir_time_decimate_bank(single._plan, *io[1:], 2 * n, 1, None, C.byref(ms)) == EINVAL
    assert single.position == (0, 0)
    torch.cuda.synchronize()
    assert float(out.abs().max().item()) == 0.0
    # sxfir_time_decimate_bank leaves the position, the history and every band's phase as they were
    assert plan.time_ptr(io[1].value, n - n1, rig.stride, out.data_ptr(), 8 * n, 2 * n, 2) > 0.0
    torch.cuda.synchronize()
    assert plan.position == pos
    timed = out.cpu().numpy().reshape(3, 4, 2 * n)[:, :K, :(n - n1) // 4]
    same(np.ascontiguousarray(timed).view(np.uint32), ref[:, :, k1:], "what the timed passes wrote")
    same(rig.call(plan, n1, n - n1, TILED), ref[:, :, k1:], "the call after the refused and the timed ones")
    # reset: position and every band's phase back to 0
    plan.reset()
    assert plan.position == (0, 0)
    same(rig.call(plan, 0, n, TILED), ref, "after reset")
    # set_history + set_position: the plan placed in mid-stream
    lead = 4 * 64
    plan.set_history_ptr(rig.xg.data_ptr(), lead, rig.stride, torch.cuda.current_stream().cuda_stream)
    plan.set_position(lead)
    assert plan.position == (lead, lead // 4)
    same(rig.call(plan, lead, n - lead, TILED), ref[:, :, 2 * (lead // 4):], "placed at input 256")
    # the queries tell the kinds apart
    a, b, q = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.sxfir_plan_bank(plan._plan, C.byref(q)) == 0 and q.value == K
    assert lib.sxfir_plan_bank_band(plan._plan, 2, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == centres[2]
    for band in (-1, K):
        assert lib.sxfir_plan_bank_band(plan._plan, band, C.byref(a), C.byref(b)) == EINVAL
    assert lib.sxfir_plan_bank_band(plan._plan, 0, None, C.byref(b)) == EINVAL
    h4 = sxxcvr_amd.design_lowpass(128, 4)
    others = {"real": sxxcvr_amd.Resampler(DECIMATE, h4, 4), "complex": sxxcvr_amd.Resampler(DECIMATE, design_bandpass(128, 4, 1, 4), 4),
              "translating": single, "channelizer": sxxcvr_amd.Channelizer(h4),
              "rational": sxxcvr_amd.RationalResampler(sxxcvr_amd.design_rational(4, 5), 4, 5)}
    for name, p in others.items():
        assert lib.sxfir_plan_bank(p._plan, C.byref(q)) == 0 and q.value == 0, name
        assert lib.sxfir_plan_bank_band(p._plan, 0, C.byref(a), C.byref(b)) == EINVAL, name
    assert lib.sxfir_plan_translation(plan._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert lib.sxfir_plan_rational(plan._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    for query in ("sxfir_plan_bands", "sxfir_plan_oversampling", "sxfir_plan_synthesis_bands", "sxfir_plan_synthesis_oversampling"):
        assert getattr(lib, query)(plan._plan, C.byref(q)) == 0 and q.value == 0, query
    step, nph, ti, tf = C.c_uint64(7), C.c_int(-1), C.c_int64(7), C.c_uint32(7)
    assert lib.sxfir_plan_arbitrary(plan._plan, C.byref(nph), C.byref(step), C.byref(ti), C.byref(tf)) == 0
    assert (nph.value, step.value, ti.value, tf.value) == (0, 0, 0, 0)
    assert lib.sxfir_taps_are_complex(plan._plan, C.byref(q)) == 0 and q.value == 1
    # the torch form: [nchan, K, n_out]
    x = torch.view_as_complex(rig.xg[:, :2 * n].view(torch.float32).reshape(3, n, 2)).contiguous()
    y = bank4(hs, centres, nchan=3).process(x)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (3, K, n // 4)
    same(np.ascontiguousarray(y.cpu().numpy()).view(np.uint32).reshape(3, K, -1), ref, "process()")


# ---- anchors, per band -----------------------------------------------------------------------------------------------------------
ANCHORS = [(128, 4, KERNEL_TILED, TILED), (128, 4, KERNEL_GENERIC, GENERIC), (35, 5, KERNEL_GENERIC, GENERIC)]
ANCHOR_CENTRES = [(123, 1000), (3, 7)]


def anchor_taps(ntaps, D, designed):
    return np.stack([design_bandpass(ntaps, D, num, den) if designed and ntaps == 128 else random_taps_cx(ntaps, 9 + k)
                     for k, (num, den) in enumerate(ANCHOR_CENTRES)])


@pytest.mark.parametrize("ntaps,D,kernel,name", ANCHORS)
def test_anchor_fp64(oracle, ntaps, D, kernel, name):
    hs = anchor_taps(ntaps, D, True)
    n = 2 * TILE + 140
    x = streams(1, n, 13)
    rig = Rig(oracle, x)
    plan = TranslatingBank(hs, D, ANCHOR_CENTRES)
    plan.set_kernel(kernel)
    y = rig.stream(plan, [n], [name]).view(np.complex64)[0].astype(np.complex128)
    want = bank_f64(hs, D, x[0], ANCHOR_CENTRES)
    for k in range(2):
        b = bound(hs[k], x[0], want[k])
        err = np.maximum(np.abs(y[k].real - want[k].real), np.abs(y[k].imag - want[k].imag))
        print("/%d x %d %s band %d: worst error %.3g, bound there %.3g" % (D, ntaps, name, k, err.max(), b[err.argmax()]))
        assert np.all(err <= b)


@pytest.mark.parametrize("ntaps,D,kernel,name", ANCHORS)
def test_anchor_non_finite(oracle, ntaps, D, kernel, name):
    """One +Inf sample: in every band, non-finite outputs at exactly the outputs whose window holds it (NaNs where the reference has
    NaNs), the same bits everywhere else."""
    hs = anchor_taps(ntaps, D, False)
    n = 2 * TILE + 140
    at = 2900
    x = streams(1, n, 14)
    x[0, at] = np.complex64(complex(np.inf, 0.25))
    rig = Rig(oracle, x)
    plan = TranslatingBank(hs, D, ANCHOR_CENTRES)
    plan.set_kernel(kernel)
    got = rig.stream(plan, [n], [name])[0].view(np.float32)
    want = rig.ref(hs, D, plan.contract, ANCHOR_CENTRES)[0].view(np.float32)
    hit = np.zeros(cdiv(n, D), dtype=bool)
    hit[cdiv(at, D):(at + ntaps - 1) // D + 1] = True             # output m reads inputs [m D - ntaps + 1, m D]
    for k in range(2):
        bad = ~np.isfinite(got[k]).reshape(-1, 2).all(axis=1)
        assert np.array_equal(bad, hit), "band %d: non-finite outputs %r" % (k, np.nonzero(bad != hit)[0][:8])
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])) and np.array_equal(np.isinf(got[k]), np.isinf(want[k]))
        ok = ~np.isnan(want[k])
        same(got[k].view(np.uint32)[ok], want[k].view(np.uint32)[ok], "band %d around the non-finite sample" % k)


@pytest.mark.parametrize("ntaps,D,kernel,name", ANCHORS)
def test_anchor_subnormals(oracle, ntaps, D, kernel, name):
    """A stream scaled into the subnormals: bit-exact, nothing is flushed, on every band."""
    hs = anchor_taps(ntaps, D, False)
    n = 2 * TILE + 140
    x = (streams(1, n, 15) * np.float32(2.0 ** -130)).astype(np.complex64)
    assert 0 < np.abs(x.view(np.float32)).max() < np.finfo(np.float32).tiny
    rig = Rig(oracle, x)
    plan = TranslatingBank(hs, D, ANCHOR_CENTRES)
    plan.set_kernel(kernel)
    want = rig.ref(hs, D, plan.contract, ANCHOR_CENTRES)
    for k in range(2):
        assert np.count_nonzero(want[0, k].view(np.float32)) > want[0, k].size // 2
    same(rig.stream(plan, [n], [name]), want, "subnormal stream")
