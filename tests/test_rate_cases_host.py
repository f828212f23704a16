"""tests/rate_cases.py on the CPU: the generator covers what the GPU sweep (tests/test_gpu_rate_sweep.py) is there for, its draws
are calls the entry points accept, the predictor says what the headers say, and the reference of a PLACED stream is the fp64
definition at the true 64-bit position, numerically, before any kernel runs."""
import collections
import math

import numpy as np
import pytest

import rate_cases as rc
from band_cases import AUTO, CX_RATIOS, GENERIC, TILED, Call
from bank_cases import bank_f64
from mix_cases import bound as mix_bound, mix_f64, step
from mix_tx_cases import back_step, bound as mix_tx_bound, mix_tx_f64
from rate_cases import KINDS, SWEEP_COUNT, SWEEP_SEED
from rational_cases import bound as rational_bound, n_out_for, rational_f64


# translate_tx: the mixers that must meet the tiled AND the generic kernel -- the smallest step t above 0 on the largest odd and the
# largest even table, and the largest t of all (s = 1: t = den - 1)
TX_LIMITS = ("s = den - gcd, den 65535", "s = den - gcd, den 65536", "s = 1, den 65535")


def _labels(kind, case):
    return [rc.expected_kernel(kind, case, i) for i in range(len(case.calls))]


def coverage(kind, cases):
    """The counts the conditions below are about: cases, unless the name says calls."""
    c = collections.Counter()
    for case in cases:
        labels = _labels(kind, case)
        form = rc.has_form(kind, case)
        produced = [x for x in labels if x != "history only"]
        c["calls"] += len(labels)
        for x in ("tiled", "generic", "history only", "refused"):
            c["%s calls" % x] += labels.count(x)
        c[case.fmt] += 1
        c["%d ch" % case.nchan] += 1
        if case.style == "seam":
            c["seam by %s" % case.how] += any(produced[i:i + 3] == ["tiled", "generic", "tiled"] for i in range(len(produced) - 2))
        c["CF16 placed"] += case.fmt == "CF16" and case.place != "start"
        c["S32 placed"] += case.fmt == "S32" and case.place != "start"
        c["3 ch with a seam"] += case.nchan == 3 and case.style == "seam"
        c["refused in mid-stream on an odd stride"] += any(x == "refused" and form and 0 < i
                                                           and ((call.out_stride % 2 == 1 and case.nchan > 1) or call.band_stride % 2 == 1)
                                                           for i, (x, call) in enumerate(zip(labels, case.calls)))
        if case.place != "start":
            c["placed"] += 1
            c["place %s" % case.place] += 1
            if form and KINDS[kind].tx:
                # no start rule: the tiled kernel takes any position, and must take one of this stream's calls
                c["placed on a tiled shape, c0 %s" % ("even" if case.c0 % 2 == 0 else "odd")] += 1
                c["placed on a tiled shape without a tiled call"] += "tiled" not in labels
            elif form:
                c["placed, start rule %s" % ("kept" if case.c0 % KINDS[kind].start_multiple == 0 else "broken")] += 1
        for index, log2, i in rc.crossings(case):
            c["%s passes 2^%d" % (index, log2)] += 1
            c["%s passes 2^%d in a %s call" % (index, log2, labels[i])] += 1
        if kind == "bank":
            bank_coverage(c, case, labels)
        elif kind != "rational":
            c["den %d" % case.den] += 1
            for cls in rc.s_classes(case):
                c[cls] += 1
                name = cls if cls.startswith("s = den") else "%s, den %d" % (cls, case.den)
                if KINDS[kind].tx and name in TX_LIMITS:
                    for label in ("tiled", "generic"):
                        c["%s, on a %s call" % (name, label)] += label in labels
            c["den below 8 on the tiled kernel"] += case.den < 8 and "tiled" in labels
        else:
            c["pair %d/%d" % (case.up, case.down)] += 1
        if kind not in ("translate", "bank"):
            c["odd taps per phase"] += rc.hist_of(case) % 2 == 1
        if KINDS[kind].tx and form:
            c["%dx%d %s" % (case.ntaps, case.up, case.style)] += 1
            c["%dx%d placed" % (case.ntaps, case.up)] += case.place != "start"
    return c


BANK_CLASSES = ("s = den - gcd, den 65535", "s = den - gcd, den 65536", "s = 1", "s = 0", "negative num", "num above den")


def bank_coverage(c, case, labels):
    """The bank's own counts: per band what a translating case counts once, and what only a plan with bands can show."""
    nb, form = rc.nbands_of(case), rc.has_form("bank", case)
    assert nb == len(case.centres) >= 1
    c["K %d" % nb] += 1
    c["K %d on %s" % (nb, "the tiled shape" if form else "a generic shape")] += 1
    c["K %d on %s" % (nb, case.fmt)] += 1
    seen = set()
    for num, den in case.centres:
        seen |= rc.centre_classes(num, den, case.down)
        c["den %d" % den] += 1
        c["den below 8 on the tiled kernel"] += den < 8 and "tiled" in labels
    for cls in seen:
        c[cls] += 1
        c["%s, at another ratio than 4" % cls] += case.down != 4
        for label in ("tiled", "generic"):
            c["%s, on a %s call" % (cls, label)] += label in labels
    c["two bands share a den and differ in num"] += any(a[1] == b[1] and a[0] % a[1] != b[0] % b[1]
                                                        for i, a in enumerate(case.centres) for b in case.centres[i + 1:])
    if case.twin:
        j, k = case.twin
        assert j != k and case.centres[j] == case.centres[k] and np.array_equal(rc.taps_of("bank", case)[j], rc.taps_of("bank", case)[k])
        c["twin bands"] += 1
        c["twin bands on a %s call" % ("tiled" if "tiled" in labels else "generic")] += 1
    for i, (label, call) in enumerate(zip(labels, case.calls)):
        inside = call.nesting if case.nchan > 1 else "bands inside channels"         # (one channel: the strides name one nesting alone)
        c["%s on a %s call" % (inside, label)] += 1
        c["a skewed input on a %s call" % label] += call.skew > 0
        c["input off the 16-byte raster on a %s call" % label] += (call.skew * (4 if case.fmt == "CF16" else 8)) % 16 != 0
        c["an odd band stride leaves the tiled kernel in mid-stream"] += i > 0 and form and call.band_stride % 2 == 1 and label in ("generic", "refused") \
            and "tiled" in labels[:i]
        c["more than two bands and more than two channels on a %s call" % label] += nb > 2 and case.nchan > 2
        c["sixteen bands on a %s call" % label] += nb == 16


def needed(kind):
    """What must occur in at least one case (for "... calls": in one call)."""
    need = ["tiled calls", "generic calls", "history only calls", "refused calls", "1 ch", "2 ch", "3 ch", "CF16 placed", "3 ch with a seam",
            "refused in mid-stream on an odd stride"]
    need += sorted(set(KINDS[kind].formats)) + ["seam by %s" % how for how in rc.SEAMS[kind]] + ["place %s" % p for p in rc.PLACES[kind]]
    need += ["%s passes 2^%s" % tuple(p.split()) for p in rc.PLACES[kind] if p != "far"]
    if KINDS[kind].tx:
        need += ["S32 placed", "placed on a tiled shape, c0 even", "placed on a tiled shape, c0 odd"]
        need += ["%s passes 2^%s in a tiled call" % tuple(p.split()) for p in rc.PLACES[kind] if p != "far"]
        need += ["%dx%d %s" % (s[0], s[1], what) for s in KINDS[kind].tiled_shapes for what in ("clean", "seam", "placed")]
        need += ["%s, on a %s call" % (cls, label) for cls in TX_LIMITS for label in ("tiled", "generic")]
    else:
        need += ["placed, start rule kept", "placed, start rule broken"]
    if kind != "rational":
        need += ["den %d" % d for d in rc.DENS]
        need += ["s = den - gcd, den 65535", "s = den - gcd, den 65536", "s = 1", "s = 0", "negative num", "num above den", "den below 8 on the tiled kernel"]
    else:
        need += ["pair %d/%d" % p for p in rc.RATIONAL_PAIRS]
    if kind not in ("translate", "bank"):
        need += ["odd taps per phase"]
    if kind == "bank":
        need += ["K %d" % k for k in rc.BANK_KS] + ["K 16 on the tiled shape", "K 16 on a generic shape"]
        need += ["%s, on a %s call" % (cls, label) for cls in BANK_CLASSES for label in ("tiled", "generic")]
        need += ["%s, at another ratio than 4" % cls for cls in BANK_CLASSES]
        need += ["%s on a %s call" % (nesting, label) for nesting in ("bands inside channels", "channels inside bands") for label in ("tiled", "generic")]
        need += ["a skewed input on a tiled call", "input off the 16-byte raster on a tiled call", "two bands share a den and differ in num",
                 "twin bands on a tiled call", "twin bands on a generic call", "an odd band stride leaves the tiled kernel in mid-stream",
                 "more than two bands and more than two channels on a tiled call", "more than two bands and more than two channels on a generic call",
                 "sixteen bands on a tiled call", "sixteen bands on a generic call"]
    return need


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_sweep_covers_what_it_is_for(kind):
    cases = rc.cases(kind, SWEEP_SEED, SWEEP_COUNT)
    assert len(cases) == SWEEP_COUNT and len({c.ident for c in cases}) == SWEEP_COUNT
    assert cases == rc.cases(kind, SWEEP_SEED, SWEEP_COUNT), "the generator is a function of its seed"
    c = coverage(kind, cases)
    print("%s, seed %d: %s" % (kind, SWEEP_SEED, ", ".join("%s %d" % (k, c[k]) for k in sorted(c))))
    missing = [what for what in needed(kind) if c[what] < 1]
    assert not missing, missing
    # band_cases' deck
    assert c["CF32"] == 22 and c["placed"] == 12 and sum(rc.has_form(kind, x) for x in cases) == 11, c
    assert sum(x.style == "seam" for x in cases) == 4 and sum(x.style == "clean" for x in cases) == 7, c
    if KINDS[kind].tx:
        assert c["placed on a tiled shape, c0 even"] == 2 and c["placed on a tiled shape, c0 odd"] == 2, c
        assert c["placed on a tiled shape without a tiled call"] == 0, c
        # no call with inputs is "history only": every input makes L outputs
        assert all(call.n == 0 for x in cases for call, label in zip(x.calls, _labels(kind, x)) if label == "history only")
        for x in cases:
            assert 0 <= step(x.num, x.den, x.up) < x.den <= 65536 and x.ntaps % x.up == 0 and x.down == 1, x.ident
    else:
        assert c["placed, start rule kept"] == 2 and c["placed, start rule broken"] == 2, c
    # at most a quarter of all calls compute nothing (refused calls and calls that complete no output -- translate_tx: n = 0 -- together)
    assert 4 * (c["refused calls"] + c["history only calls"]) <= c["calls"], c
    if kind == "bank":
        assert c["K 16 on CF16"] + c["K 16 on S32"] >= 1, c
        for x in cases:
            assert all(0 <= step(num, den, x.down) < den <= 65536 for num, den in x.centres), x.ident
    if kind == "translate":
        # the mixer at its limits: num 65535 at /4 on den 65536 has s = 65532, as the tiled kernel's comments count on
        assert rc.mixer_num("max", 65536, None, 4) == 65535 and step(65535, 65536, 4) == 65532
        assert step(rc.mixer_num("max", 65535, None, 4), 65535, 4) == 65534 and step(rc.mixer_num("one", 65535, None, 4), 65535, 4) == 1
        for x in cases:
            assert 0 <= step(x.num, x.den, x.down) < x.den <= 65536, x.ident


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_draw_is_a_call_the_entry_point_accepts(kind):
    """The argument checks of sxfir_create_translating / sxfir_create_rational and of sxfir_decimate / sxfir_resample (check_buffers),
    restated: legal shapes and formats, a stream of six tiles at the most, strides that hold the block, a position that
    sxfir_set_position takes and whose product with `up` stays below 2^62, a lead that sxfir_set_history takes.
    sxfir_create_translating_interpolator: ntaps % ratio == 0, den in 1 .. 65536, and (c0 + 6 tile) L < 2^62 for the output count."""
    K = KINDS[kind]
    for case in rc.cases(kind, SWEEP_SEED, SWEEP_COUNT):
        assert case.fmt in K.formats and case.nchan in (1, 2, 3) and 1 <= len(case.calls) <= 6, case.ident
        if kind == "translate":
            assert case.up == 1 and case.down in CX_RATIOS and 4 <= case.ntaps <= 300 and 1 <= case.den <= 65536, case.ident
            assert -2 ** 31 <= case.num < 2 ** 31, case.ident
        elif kind == "bank":
            # sxfir_create_bank: nbands in 1 .. 16, every den in 1 .. 65536, num any int
            assert case.up == 1 and case.down in CX_RATIOS and 4 <= case.ntaps <= 300 and (case.num, case.den) == (0, 0), case.ident
            assert 1 <= rc.nbands_of(case) <= 16 and rc.nbands_of(case) in rc.BANK_KS, case.ident
            assert all(1 <= den <= 65536 and -2 ** 31 <= num < 2 ** 31 for num, den in case.centres), case.ident
            assert rc.taps_of(kind, case).shape == (rc.nbands_of(case), case.ntaps), case.ident
        elif kind == "translate_tx":
            assert case.down == 1 and case.up in CX_RATIOS and case.ntaps % case.up == 0 and 1 <= case.ntaps // case.up, case.ident
            assert (case.ntaps <= 300 or (case.ntaps, case.up, case.down) in K.tiled_shapes) and 1 <= case.den <= 65536, case.ident
            assert -2 ** 31 <= case.num < 2 ** 31, case.ident
            assert tuple(rc.contract(kind, case)) == ((2, 1) if (case.ntaps // case.up) % 2 == 0 else (1, 1)), case.ident
        else:
            assert case.fmt != "S32" and (case.num, case.den) == (0, 0), case.ident
            assert 2 <= case.up <= 4096 and 2 <= case.down <= 4096 and math.gcd(case.up, case.down) == 1, case.ident
            assert case.ntaps % case.up == 0 and 1 <= case.ntaps // case.up <= 40, case.ident
            assert ((case.up, case.down) in rc.RATIONAL_PAIRS), case.ident
        assert 0 < sum(call.n for call in case.calls) <= 6 * rc.tile_of(kind, case), case.ident
        assert 0 <= case.c0 and (case.c0 + 6 * rc.tile_of(kind, case)) * case.up < 2 ** 62, case.ident
        assert (case.c0 == 0) == (case.place == "start"), case.ident
        lead = rc.lead_of(case)
        assert (lead == 0 and case.c0 == 0) or (rc.hist_len(case) <= lead <= case.c0 and (case.c0 - lead) % case.down == 0), case.ident
        assert rc.hist_len(case) >= rc.hist_of(case) >= 1
        pos = case.c0
        for call in case.calls:
            n_out = n_out_for(call.n, case.up, case.down, pos)
            pos += call.n
            assert call.request in (AUTO, TILED, GENERIC) and call.out_off in (0, 1) and call.skew >= 0, case.ident
            assert call.in_stride >= call.n and call.out_stride >= n_out, (case.ident, call)
            if kind != "bank":
                assert call.band_stride == 0, case.ident
                continue
            # check_bank_io and check_band_layout (sxfir_bank.hip.h, sxfir_launch.hip.h), restated: a band stride that holds the
            # block, and one of the two nestings
            nb, nc = rc.nbands_of(case), case.nchan
            assert call.band_stride >= n_out, (case.ident, call)
            bands_inside = call.out_stride >= (nb - 1) * call.band_stride + n_out
            channels_inside = call.out_stride >= n_out and call.band_stride >= (nc - 1) * call.out_stride + n_out
            assert nc == 1 or bands_inside or channels_inside, (case.ident, call)
            if nc > 1:                                      # (the nesting the call was drawn with is the one its strides state)
                assert channels_inside if call.nesting == "channels inside bands" else bands_inside, (case.ident, call)
                assert n_out == 0 or nb == 1 or bands_inside != channels_inside, (case.ident, call)


def test_the_predictor_on_hand_made_calls():
    """The headers' rules on calls written out by hand: every reason to leave the tiled kernel, both start rules, from the stream's
    start and from a placed position."""
    def case(kind, calls, fmt="CF32", nchan=2, c0=0, shape=None):
        ntaps, up, down = shape or KINDS[kind].tiled_shapes[0]
        return rc.Case("hand", ntaps, up, down, 3, 7, 0, nchan, fmt, 0, "hand", None, "start" if c0 == 0 else "far", c0, tuple(calls))

    def call(n, request=AUTO, out_off=0, out_stride=4096):
        return Call(n, request, out_off, out_stride, 0, 4096, 0, "bands inside channels")

    for kind in KINDS:
        q = KINDS[kind].start_multiple
        one = lambda *a, **kw: rc.expected_kernel(kind, case(kind, [call(*a, **kw)]), 0)                          # noqa: E731
        assert one(640) == "tiled"                                                                                  # 1
        assert one(640, GENERIC) == "generic"                                                                       # 2
        assert one(640, out_off=1) == "generic" and one(640, TILED, out_off=1) == "refused"                         # 3, 4
        assert rc.expected_kernel(kind, case(kind, [call(640, TILED, out_off=1)]), 0, request=AUTO) == "generic"    # 5
        assert rc.expected_kernel(kind, case(kind, [call(640, TILED, out_off=1)]), 0, assume_aligned=True) == "tiled"           # 6
        assert one(640, out_stride=4097) == "generic"                                                               # 7
        assert rc.expected_kernel(kind, case(kind, [call(640, out_stride=4097)], nchan=1), 0) == "tiled"            # 8
        assert rc.expected_kernel(kind, case(kind, [call(640)], fmt="CF16"), 0) == "generic"                        # 9
        assert rc.expected_kernel(kind, case(kind, [call(640, TILED)], fmt="CF16"), 0) == "refused"                 # 10
        assert one(0, TILED) == "history only"                                                                      # 11
        if KINDS[kind].tx:
            # no position rule: "at any stream position" (sxfir_translate_tx.h), even, odd, beyond 2^32
            for c0 in (2 ** 40 + 3, 2 ** 40 + 20, 2 ** 31 - 1, 5):
                assert rc.expected_kernel(kind, case(kind, [call(640, TILED)], c0=c0), 0) == "tiled", (kind, c0)
            continue
        # a placed stream: the rule is about the ABSOLUTE position
        for c0, want in ((q * (2 ** 40 + 3), "tiled"), (q * 2 ** 40 + 1, "generic"), (2 ** 31, "tiled" if 2 ** 31 % q == 0 else "generic")):
            assert rc.expected_kernel(kind, case(kind, [call(640)], c0=c0), 0) == want, (kind, c0)                   # 12, 13, 14
        assert rc.expected_kernel(kind, case(kind, [call(640, TILED)], c0=q * 2 ** 40 + 1), 0) == "refused"         # 15
    # translate, /4: 5 samples make 2 outputs and leave the stream one past a boundary; 2 more complete none; 1 brings it back
    c = case("translate", [call(5), call(2), call(2, TILED), call(3), call(512, TILED)])
    assert [rc.expected_kernel("translate", c, i) for i in range(5)] == ["tiled", "history only", "refused", "history only", "tiled"]
    # rational, 4/5: ceil(4 c / 5) outputs exist after c inputs -- 5, 8, 12, 12, 13, 525, 528, 529 after 6, 10, 14, 15, 16, 656, 660,
    # 661: the fifth input of every period (14) completes none, and the calls at 10, 15 and 660 start on the period
    c = case("rational", [call(6), call(4, TILED), call(4), call(1, TILED), call(1), call(640, TILED), call(4), call(1)])
    assert [n_out_for(x.n, 4, 5, rc.position_before(c, i)) for i, x in enumerate(c.calls)] == [5, 3, 4, 0, 1, 512, 3, 1]
    assert [rc.expected_kernel("rational", c, i) for i in range(8)] == ["tiled", "refused", "tiled", "history only", "tiled", "refused", "generic", "tiled"]
    # a shape without a tiled kernel
    assert rc.expected_kernel("translate", case("translate", [call(640, TILED)], shape=(64, 1, 4)), 0) == "refused"
    assert rc.expected_kernel("rational", case("rational", [call(640)], shape=(64, 4, 5)), 0) == "generic"
    assert rc.expected_kernel("rational", case("rational", [call(1)], shape=(24, 3, 8), c0=1), 0) == "history only"
    # translate_tx: every input makes L outputs, so a call of ANY size above 0 computes, at any position; n = 0 does nothing, whatever
    # was asked for; the only refusals in mid-stream are the output's alignment and an odd out_stride with nchan > 1; both shapes
    tx = "translate_tx"
    c = case(tx, [call(1), call(2, TILED), call(0, TILED, out_off=1), call(31, GENERIC), call(3, TILED, out_off=1), call(3, TILED, out_stride=4097),
                  call(300, TILED)], c0=2 ** 40 + 21)
    assert [rc.outputs_for(c, rc.position_before(c, i), x.n) for i, x in enumerate(c.calls)] == [4, 8, 0, 124, 12, 12, 1200]
    assert [rc.expected_kernel(tx, c, i) for i in range(7)] == ["tiled", "tiled", "history only", "generic", "refused", "refused", "tiled"]
    assert rc.expected_kernel(tx, c._replace(nchan=1), 5) == "tiled"                        # (one channel: the stride is not used)
    assert rc.expected_kernel(tx, case(tx, [call(640, TILED)], shape=(256, 8, 1)), 0) == "tiled"
    assert rc.expected_kernel(tx, case(tx, [call(640, TILED)], shape=(128, 8, 1)), 0) == "refused"
    assert rc.expected_kernel(tx, case(tx, [call(640)], shape=(35, 5, 1), c0=7), 0) == "generic"
    assert rc.expected_kernel(tx, case(tx, [call(0, TILED)], shape=(35, 5, 1)), 0) == "refused"      # (sxfir_set_kernel's refusal comes first)


def test_crossings_on_hand_made_streams():
    def case(up, down, c0, sizes):
        calls = tuple(Call(n, AUTO, 0, 4096, 0, 4096, 0, "bands inside channels") for n in sizes)
        return rc.Case("hand", 128, up, down, 0, 0, 0, 1, "CF32", 0, "hand", None, "far", c0, calls)

    assert rc.crossings(case(1, 4, 2 ** 31 - 10, [10, 10])) == set()                       # the mark lies between two calls
    assert rc.crossings(case(1, 4, 2 ** 31 - 10, [5, 10])) == {("input", 31, 1)}
    assert rc.crossings(case(1, 4, 4 * 2 ** 32 - 4, [4, 8])) == set()                      # output 2^32 - 1 in one call, 2^32 in the next
    assert rc.crossings(case(1, 4, 4 * 2 ** 32 - 8, [4, 8])) == {("output", 32, 1)}       # outputs 2^32 - 1 (input 2^34 - 4) and 2^32
    assert rc.crossings(case(1, 4, 4 * 2 ** 32, [8])) == set()
    # 4/5: output m belongs to input floor(5 m / 4); m = ceil(2^31 / 5) = 429496730 is the first with 5 m >= 2^31, its input 536870912
    assert rc.crossings(case(4, 5, 536870911, [2])) == {("raster", 31, 0)}
    assert rc.crossings(case(4, 5, 536870912, [2])) == set()
    # x4 and x8 (down = 1): a call of inputs [a, b) makes the outputs [L a, L b) -- ma = a up / down holds without a remainder --, so
    # output 2^32 belongs to input 2^30 at x4 and output 2^31 to input 2^28 at x8; no "raster" of its own
    assert rc.crossings(case(4, 1, 2 ** 30 - 2, [2, 2])) == set()                          # outputs .. 2^32 - 1, then 2^32 ..: between two calls
    assert rc.crossings(case(4, 1, 2 ** 30 - 1, [2])) == {("output", 32, 0)}
    assert rc.crossings(case(4, 1, 2 ** 30, [2])) == set()
    assert rc.crossings(case(8, 1, 2 ** 28 - 3, [2, 2, 2])) == {("output", 31, 1)}
    assert rc.crossings(case(8, 1, 2 ** 31 - 10, [5, 10])) == {("input", 31, 1)}
    assert rc.crossings(case(4, 1, 2 ** 32 - 1, [1, 1])) == set() and rc.crossings(case(4, 1, 2 ** 32 - 1, [2])) == {("input", 32, 0)}
    assert rc.crossings(case(2, 1, 2 ** 31 - 1, [2])) == {("input", 31, 0), ("output", 32, 0)}     # (x2: both marks in one call)


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_placed_reference_is_the_plain_one_at_the_lead(oracle, kind):
    """At c0 = lead the placed stream IS the tail of one pass from zero history: the same bits, the lead's outputs dropped."""
    for case in [c for c in rc.cases(kind, SWEEP_SEED, SWEEP_COUNT) if c.place != "start"][:4]:
        lead = rc.lead_of(case)
        near = case._replace(c0=lead)
        assert rc.lead_of(near) == lead
        h = rc.taps_of(kind, case)
        raw, xs = rc.stream_input(kind, case, oracle)
        whole = rc.plain_reference(kind, oracle, case, h, xs[0])
        got = rc.reference(kind, oracle, near, h, xs[0])
        assert got.shape[-1] == n_out_for(xs.shape[1] - lead, case.up, case.down, lead) and got.shape[-1] == whole.shape[-1] - n_out_for(lead, case.up, case.down)
        assert np.array_equal(got.view(np.uint32), whole[..., whole.shape[-1] - got.shape[-1]:].view(np.uint32)), case.ident
        if kind == "translate" and (case.c0 - lead) // case.down * step(case.num, case.den, case.down) % case.den:
            far = rc.reference(kind, oracle, case, h, xs[0])
            assert far.shape == got.shape and not np.array_equal(far.view(np.uint32), got.view(np.uint32)), "the far phase is not the near one"
        if kind == "bank":
            far = rc.reference(kind, oracle, case, h, xs[0])
            assert far.shape == got.shape == (rc.nbands_of(case), got.shape[-1])
            for k, (num, den) in enumerate(case.centres):
                if (case.c0 - lead) // case.down * step(num, den, case.down) % den:
                    assert not np.array_equal(far[k].view(np.uint32), got[k].view(np.uint32)), "band %d: the far phase is not the near one" % k
        if kind == "translate_tx" and back_step(case.num, case.den, case.up):
            far = rc.reference(kind, oracle, case, h, xs[0])
            assert far.shape == got.shape and np.count_nonzero(far.view(np.uint32) != got.view(np.uint32)) > got.size // 2, "the far phase is not the near one"
    if kind == "translate_tx":
        # the generator's promise for EVERY placed case: wherever the kernels step at all (t != 0), the lead's first sample has another
        # table entry than at c0 = lead, so a plan that lost its 64-bit position cannot pass
        placed = [c for c in rc.cases(kind, SWEEP_SEED, SWEEP_COUNT) if c.place != "start"]
        assert len(placed) == 12 and {rc.has_form(kind, c) for c in placed if back_step(c.num, c.den, c.up)} == {True, False}
        for case in placed:
            t = back_step(case.num, case.den, case.up)
            assert rc.lead_of(case) == rc.hist_len(case), case.ident                        # the fewest samples that fill the history
            assert t == 0 or (case.c0 - rc.lead_of(case)) * t % case.den != 0, case.ident


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_placed_reference_is_the_fp64_definition(oracle, kind):
    """Three placed cases per kind, channel 0: the float32 reference the GPU is compared with bit for bit against the header's formula
    in fp64 with the TRUE absolute index of the first output (translate_tx: of the first input) -- mix_cases.mix_f64 /
    rational_cases.rational_f64 / mix_tx_cases.mix_tx_f64 over the lead and the stream, the lead's outputs dropped -- within the
    project's bounds (mix_cases.bound, rational_cases.bound, mix_tx_cases.bound)."""
    placed = [c for c in rc.cases(kind, SWEEP_SEED, SWEEP_COUNT) if c.place != "start"]
    assert len(placed) >= 3
    for case in placed[:3]:
        lead = rc.lead_of(case)
        h = rc.taps_of(kind, case)
        raw, xs = rc.stream_input(kind, case, oracle)
        x = xs[0]
        got = rc.reference(kind, oracle, case, h, x).astype(np.complex128)
        skip = n_out_for(lead, case.up, case.down)
        if kind == "translate":
            m_true = -(-case.c0 // case.down)                                   # ceil(c0 / ratio): sxfir_set_position's `produced`
            want = mix_f64(h, case.down, case.num, case.den, x, m_true - skip)[skip:]
            b = mix_bound(h, x, want)
        elif kind == "bank":                                                    # the translating decimator's definition and bound, band by band
            m_true = -(-case.c0 // case.down)
            want = bank_f64(h, case.down, x, case.centres, m_true - skip)[:, skip:]
            b = np.stack([mix_bound(h[k], x, want[k]) for k in range(rc.nbands_of(case))])
        elif kind == "translate_tx":
            # the first sample of x is input c0 - lead of the stream: the true index, a Python int of 41 bits in the "far" cases
            want = mix_tx_f64(h, case.up, case.num, case.den, x, case.c0 - lead)[skip:]
            b = np.full(want.shape, mix_tx_bound(h, x))
        else:
            want = rational_f64(h, case.up, case.down, x)[skip:]
            b = np.full(want.shape, rational_bound(h, x))
        assert got.shape == want.shape and got.size > 0, case.ident
        err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) if kind != "rational" else np.abs(got - want)
        print("%s %s from %d: worst error %.3g, bound there %.3g" % (kind, case.ident, case.c0, err.max(), b.ravel()[err.argmax()]))
        assert np.all(err <= b), case.ident


def test_the_tx_wire_words_stay_in_range_and_hold_both_keying_states(oracle):
    """translate_tx on S32: CF32 in, convert_tx words out.  The input's scale (rate_cases.tx_scale, an exact power of two) keeps
    every component of the reference below 1.0, and the threshold -- the median |y|^2 of channel 0's reference -- leaves words of
    both keying states in EVERY channel's reference: a plan that lost its threshold, or keyed on the raw input, cannot pass."""
    kind = "translate_tx"
    s32 = [c for c in rc.cases(kind, SWEEP_SEED, SWEEP_COUNT) if c.fmt == "S32"]
    assert s32
    for case in s32:
        h = rc.taps_of(kind, case)
        raw, xs = rc.stream_input(kind, case, oracle)
        scale = rc.tx_scale(h)
        assert float(np.log2(scale)) == int(np.log2(scale)) and float(np.abs(h.astype(np.complex128)).sum()) * float(np.abs(xs).max()) < 1.0, case.ident
        refs = [rc.reference(kind, oracle, case, h, xs[c]) for c in range(case.nchan)]
        thr2 = rc.keying_threshold(refs[0])
        for ref in refs:
            assert max(np.abs(ref.real).max(), np.abs(ref.imag).max()) < 1.0, case.ident
            words = rc.stored_words(oracle, case.fmt, ref, thr2)
            keyed = (words.view(np.int32)[:, 0] & 3) == 3
            assert 0 < keyed.sum() < keyed.size, (case.ident, int(keyed.sum()), keyed.size)
        assert not np.array_equal(rc.stored_words(oracle, case.fmt, refs[0], thr2), rc.stored_words(oracle, case.fmt, refs[0], np.float32(0.0)))
