"""The combiner bank on the GPU (include/sxfir_bank_tx.h), bit for bit against tests/bank_tx_cases.py: per band the translating
interpolator's reference, then float32 adds in band order.

Every call goes through `Rig.call`: the output lands between two guards of fill words that must come back untouched, every band's
input row is followed by NaN words, and the plan's position, outputs_for and geometry(...)["kernel"] are checked around it."""
import ctypes as C

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import Resampler, Synthesizer, TranslatingBank, TranslatingCombiner, TranslatingInterpolator, design_bandpass, design_lowpass
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED
from bank_tx_cases import EINVAL, EUNSUPPORTED, FILL, GENERIC, TILE_IN, TILED, Rig, band_refs, combiner_ref, same, sum_in_order
from gpu_util import random_taps_cx
import rate_cases as rc
from mix_tx_cases import back_step, step
from rational_cases import gaussian_stream

pytestmark = pytest.mark.gpu

T = TILE_IN
HS = [random_taps_cx(128, 60 + k) for k in range(16)]
DENS16 = [7, 1000, 65536, 4, 1, 65535, 3, 12345, 9, 64, 1000, 4093, 7, 255, 1024, 65536]
CENTRES16 = [((3 + 11 * k) % d, d) for k, d in enumerate(DENS16)]


def streams(nchan, K, n, seed=3):
    return np.stack([np.stack([gaussian_stream(n, seed + 17 * c + 101 * k) for k in range(K)]) for c in range(nchan)])


def plan_of(centres, kernel=KERNEL_AUTO, nchan=1, hs=None, L=4, fmt="CF32"):
    hs = HS[:len(centres)] if hs is None else hs
    plan = TranslatingCombiner(np.stack(hs), L, centres, nchan=nchan, fmt=fmt)
    assert plan.complex_taps and plan.mode == INTERPOLATE and plan.nbands == len(centres)
    assert plan.centres == [(n % d, d) for n, d in centres]
    plan.set_kernel(kernel)
    return plan


# ---- 1. K = 1: the translating interpolator, word for word ------------------------------------------------------------------------
@pytest.mark.parametrize("num,den", [(3, 7), (123, 1000), (12345, 65536), (1, 4), (16384, 65536)])
@pytest.mark.parametrize("kernel,name,single", [(KERNEL_TILED, TILED, "interp_mix_pass_kernel"), (KERNEL_GENERIC, GENERIC, "interp_mix_generic_kernel")])
def test_one_band_is_the_translating_interpolator(oracle, num, den, kernel, name, single):
    """K = 1 against TranslatingInterpolator on the GPU, the same kernel family, the stream cut into calls of 1, 31, 255, 256, 257 and
    700 inputs: a call below the history depth, below a tile, an exact tile, an edge tile.  (16384, 65536): s = 0, nothing turns."""
    import torch
    if den == 65536 and num == 16384:
        assert step(num, den, 4) == 0
    blocks = [1, 31, 255, 256, 257, 700]
    n = sum(blocks)
    rig = Rig(oracle, streams(1, 1, n, 5))
    one = TranslatingInterpolator(HS[0], 4, num, den)
    one.set_kernel(kernel)
    plan = plan_of([(num, den)], kernel)
    assert tuple(plan.contract) == tuple(one.contract)
    xg = torch.from_numpy(rig.x[0, 0].copy()).cuda()
    pos, outs, wants = 0, [], []
    for b in blocks:
        assert one.geometry(b)["kernel"] == single
        wants.append(one.process(xg[pos:pos + b]).cpu().numpy().view(np.uint32).reshape(1, -1))
        outs.append(rig.call(plan, pos, b, name))
        pos += b
    same(np.concatenate(outs, axis=1), np.concatenate(wants, axis=1), "K = 1 against the single plan")
    same(np.concatenate(outs, axis=1), rig.ref(HS[:1], 4, 2, [(num, den)]), "K = 1 against the reference")


@pytest.mark.parametrize("kernel,name", [(KERNEL_TILED, TILED), (KERNEL_GENERIC, GENERIC)])
def test_one_band_keeps_its_signed_zeros(oracle, kernel, name):
    """K = 1 adds nothing: a stream at the bottom of the subnormals, whose chains underflow to zeros of either sign, comes out with
    the translating interpolator's words -- the negative zeros among them, which a sum started from +0.0 would turn positive."""
    n = T + 40
    x = (streams(1, 1, n, 21) * np.float32(2.0 ** -147)).astype(np.complex64)
    assert 0 < np.abs(x.view(np.float32)).max() < 2.0 ** -140
    rig = Rig(oracle, x)
    want = rig.ref(HS[:1], 4, 2, [(3, 7)])
    neg, pos = np.count_nonzero(want == 0x80000000), np.count_nonzero(want == 0)
    print("%d negative and %d positive zeros among %d words" % (neg, pos, want.size))
    assert neg > want.size // 16 and pos > want.size // 16
    same(rig.call(plan_of([(3, 7)], kernel), 0, n, name), want, "K = 1 at the bottom of the subnormals")


# ---- 2. K = 2, 3, 16 against the reference ---------------------------------------------------------------------------------------------
CASES = [([(3, 7), (5, 7)], 1, "bands"),                                    # a shared den: one table
         ([(3, 7), (123, 1000), (12345, 65536)], 1, "bands"),               # distinct dens
         ([(0, 1), (65535, 65536)], 3, "bands"),                            # den 1 and 65536, three channels
         ([(3, 7), (123, 1000), (1, 4)], 3, "channels"),                    # channels inside bands
         (CENTRES16, 1, "channels")]


@pytest.mark.parametrize("centres,nchan,layout", CASES)
def test_bands_against_the_reference(oracle, centres, nchan, layout):
    """Tiled, generic, and one stream through both in turn, call by call; odd in_stride and band_stride stay with the tiled kernel."""
    K = len(centres)
    blocks = [T + 3, 1, 31, T - 1, 2 * T + 10] if K < 16 else [T + 3, 31, 40]
    n = sum(blocks)
    rig = Rig(oracle, streams(nchan, K, n, 6), layout=layout, pad=41 - n % 2)
    assert rig.row % 2 == 1 and (rig.band_stride % 2 == 1 or rig.in_stride % 2 == 1)
    ref = rig.ref(HS[:K], 4, 2, centres)
    same(rig.stream(plan_of(centres, nchan=nchan), [n], [TILED]), ref, "one call under AUTO")
    same(rig.stream(plan_of(centres, KERNEL_TILED, nchan), blocks, [TILED] * len(blocks)), ref, "tiled, call by call")
    same(rig.stream(plan_of(centres, KERNEL_GENERIC, nchan), blocks, [GENERIC] * len(blocks)), ref, "generic, call by call")
    plan = plan_of(centres, nchan=nchan)
    outs, pos = [], 0
    for i, b in enumerate(blocks):
        plan.set_kernel(KERNEL_GENERIC if i % 2 else KERNEL_TILED)
        outs.append(rig.call(plan, pos, b, GENERIC if i % 2 else TILED))
        pos += b
    same(np.concatenate(outs, axis=1), ref, "the kernels in turn")


def test_process_takes_tensors(oracle):
    import torch
    centres = [(3, 7), (123, 1000)]
    n = T + 9
    x = streams(3, 2, n, 8)
    plan = plan_of(centres, nchan=3)
    y = plan.process(torch.from_numpy(x).cuda())
    assert tuple(y.shape) == (3, 4 * n)
    want = np.stack([combiner_ref(oracle, HS[:2], 4, x[c], 2, centres) for c in range(3)])
    same(y.cpu().numpy().view(np.uint32), want.view(np.uint32), "[nchan, K, n] -> [nchan, 4 n]")
    one = plan_of(centres)
    y1 = one.process(torch.from_numpy(x[1]).cuda())
    assert tuple(y1.shape) == (4 * n,)
    same(y1.cpu().numpy().view(np.uint32), want[1].view(np.uint32), "[K, n] -> [4 n]")


# ---- 3. the order of the sum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales,differ", [((2.0 ** 24, 1.0, -2.0 ** 24), [(0, 2, 1), (2, 0, 1)]),
                                           ((2.0 ** 24, 1.0, -2.0 ** 23), [(0, 2, 1), (2, 0, 1), (1, 2, 0), (2, 1, 0)])])
@pytest.mark.parametrize("kernel,name", [(KERNEL_TILED, TILED), (KERNEL_GENERIC, GENERIC)])
def test_order_of_the_sum(oracle, kernel, name, scales, differ):
    """Three bands of equal taps and centres whose inputs are one stream times 2^24, 1 and -2^24 (exact scalings): y_0 + y_1 loses y_1's
    low bits.  Checked on the CPU before the GPU is asked: the reference's words differ from those of the other orders.  What no
    triple can tell apart is (1, 0, 2): a float add commutes, it IS the definition's sum.  With -2^24 the orders that start y_1 + y_2
    round y_1 onto y_0's grid exactly as y_0 + y_1 does and give the reference's words too (asserted, so that the case says what it
    proves): that triple tells the definition from the two orders in which band 2 meets band 0 first.  The second triple, -2^23 in
    the place of -2^24, tells it from all four."""
    import itertools
    centres = [(3, 7)] * 3
    hs = [HS[0]] * 3
    n = T + 40
    x = gaussian_stream(n, 9)
    xs = np.stack([x * np.float32(s) for s in scales])[None]
    rig = Rig(oracle, xs)
    ys = band_refs(oracle, hs, 4, rig.x[0], 2, centres)
    want = sum_in_order(ys).view(np.uint32)
    for order in itertools.permutations(range(3)):
        other = sum_in_order(ys, order).view(np.uint32)
        if order in differ:
            assert np.count_nonzero(other != want) > want.size // 2, order
        else:
            assert np.array_equal(other, want), order
    same(rig.call(plan_of(centres, kernel, hs=hs), 0, n, name), want.reshape(1, -1), "the definition's order")


# ---- 4. twin bands -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,name", [(KERNEL_TILED, TILED), (KERNEL_GENERIC, GENERIC)])
def test_twin_bands_double(oracle, kernel, name):
    import torch
    num, den = 123, 1000
    n = 2 * T + 17
    x = gaussian_stream(n, 10)
    rig = Rig(oracle, np.stack([x, x])[None])
    got = rig.call(plan_of([(num, den)] * 2, kernel, hs=[HS[1]] * 2), 0, n, name).view(np.float32)
    one = TranslatingInterpolator(HS[1], 4, num, den)
    one.set_kernel(kernel)
    y = one.process(torch.from_numpy(x).cuda()).cpu().numpy().view(np.float32)
    assert np.array_equal(got[0], np.float32(2.0) * y), "twice the single plan's, as floats"


# ---- 5. CF16 and S32: the generic kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaps,L,fmt,jsplit", [(128, 4, "CF16", 2), (128, 4, "S32", 2), (35, 5, "CF16", 1), (96, 3, "S32", 2), (35, 5, "CF32", 1)])
def test_generic_formats_and_shapes(oracle, ntaps, L, fmt, jsplit):
    centres = [(3, 7), (123, 1000), (5, 7)]
    hs = [design_bandpass(ntaps, L, 0, 1, gain=L) for _ in centres] if fmt == "S32" else [random_taps_cx(ntaps, 70 + k) for k in range(3)]
    n = 300 + 3
    x = streams(2, 3, n, 11)
    if fmt == "S32":
        x = x * np.float32(0.0625)          # (exact; the outputs stay inside the wire words' range)
    rig = Rig(oracle, x, fmt, layout="channels")
    plan = plan_of(centres, nchan=2, hs=hs, L=L, fmt=fmt)
    assert tuple(plan.contract) == (jsplit, 1) and plan.contract.rot == 0
    g = plan.geometry(n)
    assert not g["tiled"] and g["kernel"] == GENERIC, g
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_kernel(KERNEL_TILED)
    assert ei.value.code == EUNSUPPORTED
    if fmt == "S32":
        # a non-default threshold that leaves outputs on both sides of the keying rule
        y = combiner_ref(oracle, hs, L, rig.x[0], jsplit, centres)
        assert max(np.abs(y.real).max(), np.abs(y.imag).max()) < 1.0
        rig.thr2 = float(np.float32(np.median(y.real.astype(np.float32) ** 2 + y.imag.astype(np.float32) ** 2)))
        assert rig.thr2 != 1.0e-6
        plan.set_tx_threshold(rig.thr2)
    ref = rig.ref(hs, L, jsplit, centres)
    if fmt == "S32":
        keyed = (ref[0].view(np.int32).reshape(-1, 2)[:, 0] & 3) == 3
        assert 0 < keyed.sum() < keyed.size
    if fmt == "CF16":
        # one rounding, after the last add: rounding every band to half first gives other words
        early = sum_in_order([oracle.f16_to_f32(oracle.f32_to_f16(y.view(np.float32))).view(np.complex64)
                              for y in band_refs(oracle, hs, L, rig.x[0], jsplit, centres)])
        assert np.count_nonzero(rig.words(early) != ref[0]) > 0
    same(rig.stream(plan, [n], [GENERIC]), ref, "one call")
    again = plan_of(centres, nchan=2, hs=hs, L=L, fmt=fmt)
    if fmt == "S32":
        again.set_tx_threshold(rig.thr2)
    same(rig.stream(again, [37, 1, n - 38], [GENERIC] * 3), ref, "three calls")


# ---- 6. the walk ---------------------------------------------------------------------------------------------------------------------
def _walk_size(n_tiles):
    """Inputs of a call of n_tiles tiles whose last tile is ragged (half a tile and five samples)."""
    return (n_tiles - 1) * T + T // 2 + 5


@pytest.mark.parametrize("centres", [[(3, 7), (65534, 65535)], [(1, 3), (65535, 65536)]])
def test_a_waves_third_tile(oracle, centres):
    """2 resident + 3 tiles with K = 2 under a forced TILED: one generation of waves, so every wave walks to a second tile and three to a
    THIRD -- every band's word moved on by stride_step twice, the counted wait behind a tile's stores and the full wait between its
    bands in turn, the histories carried over by a wave on its third tile."""
    plan = plan_of(centres, KERNEL_TILED)
    resident = plan.geometry(T)["resident"]
    n = _walk_size(2 * resident + 3)
    g = plan.geometry(n)
    print("%s: resident %d, workgroups %d, %d tiles, %d inputs per band" % (centres, resident, g["workgroups"], g["n_tiles"], n))
    assert g["kernel"] == TILED and g["workgroups"] == resident and g["n_tiles"] == 2 * resident + 3, g
    rig = Rig(oracle, streams(1, 2, n + T + 8, 19), pad=3)
    ref = rig.ref(HS[:2], 4, 2, centres, threads=oracle.max_threads())
    same(rig.call(plan, 0, n, TILED), ref[:, :2 * 4 * n], "2 resident + 3 tiles")
    same(rig.call(plan, n, T + 8, TILED), ref[:, 2 * 4 * n:], "the call after it: the histories a third tile's wave left")


def test_more_tiles_than_workgroups_three_channels(oracle):
    """Three channels: the grid per channel is a third of the resident waves, no multiple of 8, so the tiles are dealt plainly strided,
    and a call of that many tiles + 4 per channel has more tiles than waves."""
    centres = [(123, 1000), (3, 7)]
    plan = plan_of(centres, KERNEL_TILED, nchan=3)
    per = plan.geometry(T)["resident"] // 3
    n = _walk_size(per + 4)
    g = plan.geometry(n)
    G = g["workgroups"] // 3
    print("3 channels: resident %d, %d workgroups per channel, %d tiles per channel, %d inputs per band" % (g["resident"], G, g["n_tiles"], n))
    assert g["kernel"] == TILED and g["workgroups"] == 3 * G and G == per and g["n_tiles"] == G + 4 and G < g["n_tiles"], g
    rig = Rig(oracle, streams(3, 2, n, 29), pad=41 - n % 2)
    same(rig.call(plan, 0, n, TILED), rig.ref(HS[:2], 4, 2, centres, threads=oracle.max_threads()), "three channels, groups + 4 tiles each")


@pytest.mark.parametrize("where,lead,cls,den", [((1 << 40) + 21, 64, "max", 65535), (5, 21, "one", 65535)])
def test_placed_streams(oracle, where, lead, cls, den):
    """A stream placed with set_position(where) on a fresh plan: a first call of `lead` inputs, shorter than the 32-sample history or
    longer, then resident + 3 tiles from an odd position whose halo reaches back into the histories the first call left (a combiner
    takes no sxfir_set_history).  From 2^40 + 21: the 64-bit reduction of every band's phase (t = 1 on den 65535, and den 7).  From 5
    with s = 1 (the largest t, 65534): the first call's halo has the indices -27 .. 4, reduced from below 0, and the second call's
    reaches through the 21 carried samples into them."""
    num = rc.mixer_num(cls, den, None, 4)
    centres = [(num, den), (3, 7)]
    assert back_step(num, den, 4) == {"max": 1, "one": den - 1}[cls] and where * back_step(num, den, 4) % den != 0
    plan = plan_of(centres, KERNEL_TILED)
    resident = plan.geometry(T)["resident"]
    n = _walk_size(resident + 3)
    rig = Rig(oracle, streams(1, 2, lead + n, 23), pad=3)
    plan.set_position(where)
    assert plan.position == (where, 4 * where)
    g = plan.geometry(n)
    assert g["kernel"] == TILED and g["workgroups"] == resident and g["n_tiles"] == resident + 3, g
    ref = rig.ref(HS[:2], 4, 2, centres, m_first=where, threads=oracle.max_threads())
    same(rig.call(plan, 0, lead, TILED), ref[:, :2 * 4 * lead], "the first call")
    same(rig.call(plan, lead, n, TILED), ref[:, 2 * 4 * lead:], "resident + 3 tiles from input %d" % (where + lead))


@pytest.mark.parametrize("ntaps,L,fmt,kernel", [(128, 4, "CF32", KERNEL_GENERIC), (35, 5, "CF32", KERNEL_AUTO)])
def test_generic_call_longer_than_the_table(oracle, ntaps, L, fmt, kernel):
    """ONE generic call of den + 300 inputs on den = 65535 with the largest step the ratio allows: only a call of more than den inputs
    makes `q % den` wrap, only a large t brings `(q % den) * t` near 65535^2 (tests/test_gpu_mix_tx.py has the argument)."""
    den = 65535
    num = rc.mixer_num("one", den, None, L)
    t = back_step(num, den, L)
    n = den + 300
    assert t == den - np.gcd(L, den) and (den - 1) * t < 2 ** 32 <= (n - 1) * t
    centres = [(3, 7), (num, den)]
    hs = HS[:2] if ntaps == 128 else [random_taps_cx(ntaps, 80 + k) for k in range(2)]
    rig = Rig(oracle, streams(1, 2, n, 31), fmt)
    plan = plan_of(centres, kernel, hs=hs, L=L, fmt=fmt)
    jsplit = plan.contract[0]
    same(rig.stream(plan, [n], [GENERIC]), rig.ref(hs, L, jsplit, centres, threads=oracle.max_threads()), "one generic call of den + 300 inputs")


# ---- 7. state ------------------------------------------------------------------------------------------------------------------------
def test_reset_and_set_history(oracle):
    import torch
    centres = [(3, 7), (123, 1000)]
    n = T + 40
    rig = Rig(oracle, streams(1, 2, n, 12))
    ref = rig.ref(HS[:2], 4, 2, centres)
    plan = plan_of(centres)
    same(rig.call(plan, 0, n, TILED), ref, "first pass")
    assert plan.position == (n, 4 * n)
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        plan.set_history_ptr(rig.xg.data_ptr(), 64, rig.row, torch.cuda.current_stream().cuda_stream)
    assert ei.value.code == EUNSUPPORTED and plan.position == (n, 4 * n)
    plan.reset()
    assert plan.position == (0, 0)
    same(rig.call(plan, 0, n, TILED), ref, "after reset: every band's phase and history start again")


def test_refused_calls_leave_everything_alone(oracle):
    centres = [(3, 7), (123, 1000)]
    n, n1 = T + 60, 50
    rig = Rig(oracle, streams(3, 2, n, 13), pad=42 - n % 2)
    assert rig.row % 2 == 0
    ref = rig.ref(HS[:2], 4, 2, centres)
    plan = plan_of(centres, KERNEL_TILED, nchan=3)
    same(rig.call(plan, 0, n1, TILED), ref[:, :2 * 4 * n1], "first block")
    m = n - n1
    rig.call(plan, n1, m, expect=EINVAL, band_stride=m - 1)                       # band_stride < n_in
    rig.call(plan, n1, m, expect=EINVAL, band_stride=rig.in_stride)               # overlap: band 1 of a channel is band 0 of the next
    rig.call(plan, n1, m, expect=EINVAL, out_stride=4 * m - 2)                    # a short out_stride
    rig.call(plan, n1, m, TILED, odd_stride=True, expect=EUNSUPPORTED)            # an odd out_stride under a forced TILED
    rig.call(plan, n1, m, TILED, offset=1, expect=EUNSUPPORTED)                   # an unaligned output
    # the failed calls left the phases, the histories and the position where they were
    same(rig.call(plan, n1, m, TILED), ref[:, 2 * 4 * n1:], "the call after the refused ones")
    # the same calls under AUTO run the generic kernel: the same bits
    auto = plan_of(centres, nchan=3)
    same(rig.call(auto, 0, n1, TILED), ref[:, :2 * 4 * n1], "first block under AUTO")
    same(rig.call(auto, n1, 7, odd_stride=True), ref[:, 2 * 4 * n1:2 * 4 * (n1 + 7)], "odd stride under AUTO")
    same(rig.call(auto, n1 + 7, m - 7, offset=1), ref[:, 2 * 4 * (n1 + 7):], "offset output under AUTO")


def test_overlapping_bands_and_channels(oracle):
    """sxfir_synthesize's layout rule with K - 1 in the place of 3: with three channels and K = 3, bands inside channels need
    in_stride >= 2 band_stride + n, channels inside bands band_stride >= 2 in_stride + n."""
    import torch
    centres = [(3, 7), (123, 1000), (1, 4)]
    n = 100
    plan = plan_of(centres, nchan=3)
    x = torch.zeros(16 * n, dtype=torch.complex64, device="cuda")
    out = torch.zeros(3 * 4 * n, dtype=torch.complex64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ok = [(3 * n, n), (n, 3 * n), (2 * n + n, n)]
    bad = [(3 * n - 1, n), (n, 3 * n - 1), (2 * n, 2 * n), (n, n)]
    for in_stride, band_stride in bad:
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            plan.process_ptr(x.data_ptr(), n, in_stride, band_stride, out.data_ptr(), 4 * n, st)
        assert ei.value.code == EINVAL and plan.position == (0, 0), (in_stride, band_stride)
    torch.cuda.synchronize()
    assert float(out.abs().max().item()) == 0.0
    for in_stride, band_stride in ok:
        plan.reset()
        assert plan.process_ptr(x.data_ptr(), n, in_stride, band_stride, out.data_ptr(), 4 * n, st) == 4 * n


# ---- 8. refusals across plans -----------------------------------------------------------------------------------------------------------
def test_frame(oracle):
    import torch
    lib = sxxcvr_amd.load_sxfir()
    vp = C.c_void_p
    centres = [(123, 1000), (1000 * 7 + 5, 7)]
    n = T + 40
    rig = Rig(oracle, streams(1, 2, n, 14))
    plan = plan_of(centres)
    q, a, b = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.sxfir_taps_are_complex(plan._plan, C.byref(q)) == 0 and q.value == 1
    assert lib.sxfir_plan_bank_tx(plan._plan, C.byref(q)) == 0 and q.value == 2
    assert lib.sxfir_plan_bank_tx_band(plan._plan, 1, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (5, 7)
    for band in (-1, 2):
        assert lib.sxfir_plan_bank_tx_band(plan._plan, band, C.byref(a), C.byref(b)) == EINVAL
    # the other kinds' queries answer zeros
    assert lib.sxfir_plan_bank(plan._plan, C.byref(q)) == 0 and q.value == 0
    assert lib.sxfir_plan_bank_band(plan._plan, 0, C.byref(a), C.byref(b)) == EINVAL
    for query in ("sxfir_plan_translation", "sxfir_plan_translation_tx", "sxfir_plan_rational"):
        a.value = b.value = -1
        assert getattr(lib, query)(plan._plan, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0), query
    for query in ("sxfir_plan_bands", "sxfir_plan_oversampling", "sxfir_plan_synthesis_bands", "sxfir_plan_synthesis_oversampling"):
        q.value = -1
        assert getattr(lib, query)(plan._plan, C.byref(q)) == 0 and q.value == 0, query
    # every other processing entry point refuses the plan, which stays where it was
    pos = plan.position
    out = torch.full((8 * n,), 0.0, dtype=torch.complex64, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    got, ms = C.c_size_t(77), C.c_float()
    io = (plan._plan, vp(rig.xg.data_ptr()), n, rig.in_stride, vp(out.data_ptr()), 8 * n)
    refused = {
        "sxfir_interpolate": lambda: lib.sxfir_interpolate(*io, C.byref(got), None),
        "sxfir_interpolate_keyed": lambda: lib.sxfir_interpolate_keyed(*io, C.byref(got), 0, n, vp(counter.data_ptr()), None),
        "sxfir_time_interpolate": lambda: lib.sxfir_time_interpolate(*io, 1, None, C.byref(ms)),
        "sxfir_decimate": lambda: lib.sxfir_decimate(*io, C.byref(got), None),
        "sxfir_time_decimate": lambda: lib.sxfir_time_decimate(*io, 1, None, C.byref(ms)),
        "sxfir_decimate_bank": lambda: lib.sxfir_decimate_bank(*io, 2 * n, C.byref(got), None),
        "sxfir_channelize": lambda: lib.sxfir_channelize(*io, 2 * n, C.byref(got), None),
        "sxfir_synthesize": lambda: lib.sxfir_synthesize(*io[:4], rig.band_stride, *io[4:], C.byref(got), None),
        "sxfir_resample": lambda: lib.sxfir_resample(*io, C.byref(got), None),
        "sxfir_resample_arbitrary": lambda: lib.sxfir_resample_arbitrary(*io, C.byref(got), None),
    }
    for name, fn in refused.items():
        got.value = 77
        assert fn() == EINVAL, name
        assert plan.position == pos and got.value in (0, 77), name
    torch.cuda.synchronize()
    assert float(out.abs().max().item()) == 0.0 and int(counter.item()) == 0
    # sxfir_interpolate_bank refuses every other plan
    h4 = design_lowpass(128, 4)
    others = {"resampler": Resampler(INTERPOLATE, h4, 4), "decimator": Resampler(DECIMATE, h4, 4),
              "translating interpolator": TranslatingInterpolator(HS[0], 4, 3, 7),
              "tuner bank": TranslatingBank(np.stack(HS[:2]), 4, [(3, 7), (1, 4)]), "synthesizer": Synthesizer(design_lowpass(128, 4, gain=4.0))}
    for name, p in others.items():
        ppos = p.position
        got.value = 77
        assert lib.sxfir_interpolate_bank(p._plan, vp(rig.xg.data_ptr()), 64, rig.in_stride, rig.band_stride, vp(out.data_ptr()), 8 * n,
                                          C.byref(got), None) == EINVAL, name
        assert lib.sxfir_time_interpolate_bank(p._plan, vp(rig.xg.data_ptr()), 64, rig.in_stride, rig.band_stride, vp(out.data_ptr()), 8 * n,
                                               1, None, C.byref(ms)) == EINVAL, name
        assert p.position == ppos and got.value == 0, name
        assert lib.sxfir_plan_bank_tx(p._plan, C.byref(q)) == 0 and q.value == 0, name
        assert lib.sxfir_plan_bank_tx_band(p._plan, 0, C.byref(a), C.byref(b)) == EINVAL, name
    torch.cuda.synchronize()
    assert float(out.abs().max().item()) == 0.0
    # the timed entry point leaves the position, the histories and the phases as they were
    ref = rig.ref(HS[:2], 4, 2, centres)
    n1 = 61
    same(rig.call(plan, 0, n1, TILED), ref[:, :2 * 4 * n1], "first block")
    assert plan.time_ptr(rig.xg.data_ptr() + 8 * n1, n - n1, rig.in_stride, rig.band_stride, out.data_ptr(), 8 * n, 2) > 0.0
    torch.cuda.synchronize()
    assert plan.position == (n1, 4 * n1)
    same(np.ascontiguousarray(out.cpu().numpy()[:4 * (n - n1)]).view(np.uint32).reshape(1, -1), ref[:, 2 * 4 * n1:], "what the timed passes wrote")
    same(rig.call(plan, n1, n - n1, TILED), ref[:, 2 * 4 * n1:], "the call after the refused and the timed ones")
