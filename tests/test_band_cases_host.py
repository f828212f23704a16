"""tests/band_cases.py on the CPU: the generator covers what the GPU sweep (tests/test_gpu_band_sweep.py) is there for, its draws
are calls the entry points accept, and the float32 references the sweep compares against ARE the fp64 definitions of the headers,
numerically, before any kernel runs."""
import numpy as np
import pytest

import band_cases as bc
from band_cases import AUTO, GENERIC, KINDS, SWEEP_COUNT, SWEEP_SEED, TILED
from gpu_util import assert_bands, chan_os_ref, chan_ref, random_taps

TX_KINDS = [k for k in KINDS if not KINDS[k].decim]


def _labels(kind, case):
    return [bc.expected_kernel(kind, case, i) for i in range(len(case.calls))]


def coverage(kind, cases):
    """The counts the issue's conditions are about, from the predictor alone."""
    K = KINDS[kind]
    c = dict.fromkeys(("all tiled", "generic by shape", "tiled-generic-tiled", "refused calls", "CF16", "S32", "CF16 nchan>1", "S32 nchan>1",
                       "nchan>1", "bands inside channels", "channels inside bands", "call of 0", "call of 1", "call below history",
                       "output offset", "odd out_stride", "odd band_stride"), 0)
    for case in cases:
        labels = _labels(kind, case)
        produced = [x for x in labels if x != "history only"]
        hist = bc.hist_of(kind, case.ntaps, case.ratio)
        c["all tiled"] += bool(produced) and all(x == "tiled" for x in produced)
        c["generic by shape"] += case.fmt == "CF32" and (case.ntaps, case.ratio) not in K.tiled_shapes
        c["tiled-generic-tiled"] += any(produced[i:i + 3] == ["tiled", "generic", "tiled"] for i in range(len(produced) - 2))
        c["refused calls"] += labels.count("refused")
        for fmt in ("CF16", "S32"):
            c[fmt] += case.fmt == fmt
            c[fmt + " nchan>1"] += case.fmt == fmt and case.nchan > 1
        c["nchan>1"] += case.nchan > 1
        if case.nchan > 1 and (K.banded_in or K.banded_out):
            for nesting in ("bands inside channels", "channels inside bands"):
                c[nesting] += any(call.nesting == nesting and call.n > 0 for call in case.calls)
        c["call of 0"] += any(call.n == 0 for call in case.calls)
        c["call of 1"] += any(call.n == 1 for call in case.calls)
        c["call below history"] += any(0 < call.n < hist for call in case.calls)
        c["output offset"] += any(call.out_off == 1 and x != "history only" for call, x in zip(case.calls, labels))
        c["odd out_stride"] += case.nchan > 1 and any(call.out_stride % 2 == 1 and x != "history only" for call, x in zip(case.calls, labels))
        c["odd band_stride"] += K.banded_out and any(call.band_stride % 2 == 1 and x != "history only" for call, x in zip(case.calls, labels))
    return c


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_sweep_covers_what_it_is_for(kind):
    K = KINDS[kind]
    cases = bc.cases(kind, SWEEP_SEED, SWEEP_COUNT)
    assert len(cases) == SWEEP_COUNT and len({c.ident for c in cases}) == SWEEP_COUNT
    assert cases == bc.cases(kind, SWEEP_SEED, SWEEP_COUNT), "the generator is a function of its seed"
    c = coverage(kind, cases)
    print("%s: %s" % (kind, ", ".join("%s %d" % kv for kv in c.items())))
    assert c["all tiled"] >= 6 and c["generic by shape"] >= 6 and c["tiled-generic-tiled"] >= 3 and c["refused calls"] >= 2, c
    assert c["CF16"] >= 3 and c["S32"] >= 3 and c["CF16 nchan>1"] >= 1 and c["S32 nchan>1"] >= 1 and c["nchan>1"] >= 4, c
    if K.banded_in or K.banded_out:
        assert c["bands inside channels"] >= 1 and c["channels inside bands"] >= 1, c
    for what in ("call of 0", "call of 1", "call below history", "output offset", "odd out_stride"):
        assert c[what] >= 2, (what, c)
    assert not K.banded_out or c["odd band_stride"] >= 2, c


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_draw_is_a_call_the_entry_point_accepts(kind):
    """The argument checks of sxfir_decimate / sxfir_interpolate (check_io), sxfir_channelize and sxfir_synthesize, restated: legal
    shapes and formats, a stream of six tiles at the most, strides that hold the block, bands and channels that do not overlap."""
    K = KINDS[kind]
    for case in bc.cases(kind, SWEEP_SEED, SWEEP_COUNT):
        assert case.fmt in ("CF32", "CF16", "S32") and case.nchan in (1, 2, 3) and 1 <= len(case.calls) <= 5, case.ident
        assert case.ratio == K.ratio or (K.ratio is None and case.ratio in bc.CX_RATIOS), case.ident
        least = case.ratio if kind == "interpolate_cx" else 4
        assert least <= case.ntaps <= 300 and (kind == "decimate_cx" or case.ntaps % least == 0), case.ident
        assert 0 < sum(call.n for call in case.calls) <= 6 * bc.tile_of(kind, case.ratio), case.ident
        pos = 0
        for call in case.calls:
            n_out = bc.outputs_for(kind, case.ratio, pos, call.n)
            pos += call.n
            assert call.request in (AUTO, TILED, GENERIC) and call.out_off in (0, 1) and call.skew >= 0, case.ident
            for banded, n, chan, band in ((K.banded_in, call.n, call.in_stride, call.band_stride), (K.banded_out, n_out, call.out_stride, call.band_stride)):
                if not banded:
                    assert chan >= n, (case.ident, call)
                    continue
                assert band >= n, (case.ident, call)
                bands_inside = chan >= 3 * band + n
                channels_inside = chan >= n and band >= (case.nchan - 1) * chan + n
                assert case.nchan == 1 or bands_inside or channels_inside, (case.ident, call)
                if case.nchan > 1:
                    assert (call.nesting == "bands inside channels") == bands_inside or n == 0, (case.ident, call)


def test_the_predictor_on_hand_made_calls():
    """The headers' rules on calls written out by hand: one tiled shape of every position rule, every reason to leave the tiled kernel."""
    def case(kind, calls, ntaps=128, ratio=None, fmt="CF32", nchan=2):
        ratio = ratio or KINDS[kind].ratio or 4
        return bc.Case("hand", ntaps, ratio, 0, nchan, fmt, 0, "hand", tuple(calls))

    def call(n, request=AUTO, out_off=0, out_stride=4096, band_stride=1024):
        return bc.Call(n, request, out_off, out_stride, 0, 4096, band_stride, "bands inside channels")

    for kind in KINDS:
        assert bc.expected_kernel(kind, case(kind, [call(512)]), 0) == "tiled"
        assert bc.expected_kernel(kind, case(kind, [call(512, GENERIC)]), 0) == "generic"
        assert bc.expected_kernel(kind, case(kind, [call(512, out_off=1)]), 0) == "generic"
        assert bc.expected_kernel(kind, case(kind, [call(512, TILED, out_off=1)]), 0) == "refused"
        assert bc.expected_kernel(kind, case(kind, [call(512, TILED, out_off=1)]), 0, request=AUTO) == "generic"
        assert bc.expected_kernel(kind, case(kind, [call(512, TILED, out_off=1)]), 0, assume_aligned=True) == "tiled"
        assert bc.expected_kernel(kind, case(kind, [call(512, out_stride=4097)]), 0) == "generic"
        assert bc.expected_kernel(kind, case(kind, [call(512, out_stride=4097)], nchan=1), 0) == "tiled"
        assert bc.expected_kernel(kind, case(kind, [call(512, band_stride=1025)]), 0) == ("generic" if KINDS[kind].banded_out else "tiled")
        assert bc.expected_kernel(kind, case(kind, [call(512)], fmt="CF16"), 0) == "generic"
        assert bc.expected_kernel(kind, case(kind, [call(512, TILED)], fmt="S32"), 0) == "refused"
        assert bc.expected_kernel(kind, case(kind, [call(512, TILED)], ntaps=64), 0) == "refused"
        assert bc.expected_kernel(kind, case(kind, [call(0, TILED)]), 0) == "history only"
    for kind in ("decimate_cx", "channelize"):
        c = case(kind, [call(5), call(2), call(2, TILED), call(3), call(512, TILED)])
        assert [bc.expected_kernel(kind, c, i) for i in range(5)] == ["tiled", "history only", "refused", "history only", "tiled"]
    c = case("channelize_os", [call(6), call(1, TILED), call(1), call(512, TILED), call(2), call(512)])
    assert [bc.expected_kernel("channelize_os", c, i) for i in range(6)] == ["tiled", "refused", "history only", "tiled", "tiled", "generic"]
    for kind in TX_KINDS:
        c = case(kind, [call(5), call(1, TILED), call(512)])
        assert [bc.expected_kernel(kind, c, i) for i in range(3)] == ["tiled"] * 3
    assert bc.expected_kernel("interpolate_cx", case("interpolate_cx", [call(64)], ntaps=256, ratio=8), 0) == "tiled"
    assert bc.expected_kernel("interpolate_cx", case("interpolate_cx", [call(64)], ntaps=256, ratio=4), 0) == "generic"


@pytest.mark.parametrize("kind,label,ntaps,ratio", [(k,) + s for k in KINDS for s in bc.anchor_shapes(k)])
def test_the_float32_reference_is_the_fp64_definition(oracle, kind, label, ntaps, ratio):
    """The float32 construct the GPU is compared with bit for bit (chan_ref, syn_ref, chan_os_ref, syn_os_ref, the two cx_ref), against
    the header's formula in fp64 by np.convolve alone, on about 3000 random samples with components uniform in [-1, 1), random taps.
    Bound: 2e-6 sum|h| B (band_cases.fp64_bound), B = 4 for the synthesizers.

    Measured max |reference - fp64| against that bound (tiled shape; generic shape):
      decimate_cx     9.65e-08 of 4.87e-06; 4.10e-08 of 1.28e-06 (/5 x 35)
      interpolate_cx  3.44e-08 of 4.87e-06 (x4), 3.97e-08 of 9.63e-06 (x8); 1.06e-08 of 1.46e-06 (x5 x 40)
      channelize      5.08e-08 of 2.94e-06; 2.04e-08 of 9.13e-07 (40 taps)
      channelize_os   5.92e-08 of 2.94e-06; 1.80e-08 of 9.13e-07
      synthesize      7.49e-08 of 1.18e-05; 2.89e-08 of 3.65e-06
      synthesize_os   9.88e-08 of 1.18e-05; 3.65e-08 of 3.65e-06
    No kind's reference comes within a factor 4 of its bound: the closest is the complex decimator at /5 x 35, 31 times below it."""
    h = bc.taps_of(kind, ntaps, 5)
    N = bc.anchor_length(kind, ratio)
    rng = np.random.default_rng(1234 + ntaps + ratio)
    shape = (4, N) if KINDS[kind].banded_in else (N,)
    x = (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(np.complex64)
    ref = bc.reference(kind, oracle, h, ratio, x)
    want = bc.definition_fp64(kind, h, ratio, x)
    assert ref.shape == want.shape and ref.size >= 500
    err, bound = float(np.abs(ref.astype(np.complex128) - want).max()), bc.fp64_bound(kind, h)
    print("%s %s: max |float32 reference - fp64 definition| = %.3g, bound %.3g (%.1f times below it)" % (kind, label, err, bound, bound / max(err, 1e-300)))
    assert err <= bound
    assert float(np.abs(want).max()) > 100 * bound, "the comparison is not about zeros"


@pytest.mark.parametrize("step", [4, 2])
def test_the_phase_tap_reference_has_chan_refs_bits(oracle, step):
    """chan_ref_phase_taps (each branch sum over its own phase's taps alone: what the non-finite test compares against) gives the bits
    of chan_ref / chan_os_ref on finite samples, at every length mod 4."""
    for ntaps in (128, 40):
        h = random_taps(ntaps, 3)
        for n in (1, 2, 3, 4, 701, 702, 703, 704):
            rng = np.random.default_rng(n)
            x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
            want = chan_ref(oracle, h, x) if step == 4 else chan_os_ref(oracle, h, x)
            assert_bands(bc.chan_ref_phase_taps(oracle, h, x, step), want, "%d taps, %d samples, step %d" % (ntaps, n, step))


@pytest.mark.parametrize("kind", TX_KINDS)
def test_s32_tx_inputs_stay_inside_the_wire_words(oracle, kind):
    """The S32 cases of the TX kinds: the input scale is a power of two (exact), the reference stays below 1.0 per component (so
    convert_tx's saturating corner is never met) and the median threshold leaves outputs on both sides of the keying rule."""
    s32 = [c for c in bc.cases(kind, SWEEP_SEED, SWEEP_COUNT) if c.fmt == "S32"]
    assert len(s32) >= 3
    for case in s32:
        h = bc.taps_of(kind, case.ntaps, case.tap_seed)
        scale = float(bc.tx_scale(kind, h, case.ratio))
        assert scale == 2.0 ** round(np.log2(scale)) and scale <= 1.0, case.ident
        raw, xs = bc.stream_input(kind, case, oracle)
        assert np.array_equal(raw.view(np.float32).reshape(-1), xs.view(np.float32).reshape(-1))
        assert float(np.abs(xs.view(np.float32)).max()) < scale
        for c in range(case.nchan):
            ref = bc.reference(kind, oracle, h, case.ratio, xs[c])
            assert max(float(np.abs(ref.real).max()), float(np.abs(ref.imag).max())) < 1.0, case.ident
            thr2 = bc.keying_threshold(ref)
            words = bc.stored_words(kind, oracle, "S32", ref, thr2)
            keyed = (words[:, 0] & 3) == 3
            assert 0 < keyed.sum() < keyed.size, (case.ident, c)
