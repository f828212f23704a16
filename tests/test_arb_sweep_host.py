"""tests/arb_sweep_cases.py on the CPU: the generator covers what the GPU sweep (tests/test_gpu_arb_sweep.py) is there for, its draws
are calls the entry points accept, the predictor says what the header says, and the chunked reference of a PLACED stream is the plain
blend of arb_cases at the lead, before any kernel runs."""
import collections

import numpy as np

import arb_sweep_cases as ac
from arb_cases import MASK, ONE, STEP_MAX, STEP_MIN, Stream, arb_ref, blend_at, position
from arb_sweep_cases import SWEEP_COUNT, SWEEP_SEED, TILED_MAX, TILED_MIN
from band_cases import AUTO, GENERIC, TILED, Call


def _labels(case):
    return [ac.expected_kernel(case, st) for st in ac.walk(case)]


def _after_refusal(case, st):
    """the kernel that computes the call: a refused one is made again under AUTO"""
    label = ac.expected_kernel(case, st)
    return ac.expected_kernel(case, st, request=AUTO) if label == "refused" else label


def coverage(cases):
    """The counts the conditions below are about: cases, unless the name says calls."""
    c = collections.Counter()
    for case in cases:
        steps, labels = ac.walk(case), _labels(case)
        ran = [_after_refusal(case, st) for st in steps]
        form = ac.has_form(case)
        produced = [x for x in labels if x != "history only"]
        c["calls"] += len(labels)
        for x in ("tiled", "generic", "history only", "refused"):
            c["%s calls" % x] += labels.count(x)
        c[case.fmt] += 1
        c["%d ch" % case.nchan] += 1
        c["P %d" % case.P] += 1
        c["T %d" % case.T] += 1
        c["contract (%d, 1)" % ac.jsplit_of(case)] += 1
        c["tiled shape on CF16"] += (case.P, case.T, case.fmt) == (128, 32, "CF16")
        c["more than one segment"] += len(case.segments) > 1
        if case.style == "seam":
            c["seam by %s" % case.how] += any(produced[i:i + 3] == ["tiled", "generic", "tiled"] for i in range(len(produced) - 2))
            c["refused in mid-stream, seam by %s" % case.how] += any(x == "refused" and 0 < i for i, x in enumerate(labels))
        for st, label, kernel in zip(steps, labels, ran):
            call = st.call
            if st.n_out:
                if st.step in ac.EDGE_STEPS:
                    c["step %#x on a %s call" % (st.step, kernel)] += 1
                if form and not TILED_MIN <= st.step <= TILED_MAX:
                    c["step %#x on the tiled shape: %s" % (st.step, label)] += 1
                c["first output in the history, on a %s call" % kernel] += (st.t >> 32) == st.consumed - 1
                c["last phase, on a %s call" % kernel] += ac.last_phase(case, st) > 0
                c["2^32 / step outputs per input and more on a %s call" % kernel] += st.n_out > st.call.n
            c["calls of samples that yield nothing"] += call.n > 0 and st.n_out == 0
            if label == "tiled":
                c["an even offset other than 0 on a tiled call"] += call.out_off == 2
                c["a padded even out_stride with three channels on a tiled call"] += case.nchan == 3 and call.out_stride % 2 == 0 and call.out_stride > st.n_out
                c["a skewed input on a tiled call"] += call.skew > 0
            for log2 in (31, 32):
                if st.consumed < 2 ** log2 <= st.consumed + call.n - 1:
                    c["input passes 2^%d on a %s call" % (log2, kernel)] += 1
        if case.place != "start":
            c["placed"] += 1
            c["place %s" % case.place] += 1
            first = next(i for i, st in enumerate(steps) if st.n_out)
            c["place %s, the first outputs on a %s call" % (case.place, ran[first])] += 1
            if case.place == "ahead":
                st = steps[first]
                assert first >= 1 and all(s.call.n > 0 and s.n_out == 0 for s in steps[:first]), case.ident
                assert (case.t_index - case.consumed) >= sum(s.call.n for s in steps[:first]), case.ident
                assert (st.t >> 32) > st.consumed and st.t - ((st.consumed - 1) << 32) >= 2 << 32, case.ident      # arb_rel: two samples and more
                c["ahead over %d calls" % first] += 1
            if case.place == "last phase":
                calls, step = case.segments[0]
                assert step == ONE and case.t_frac >= (1 << 32) - (1 << 32) // case.P, case.ident
                mine = [st for st in steps if st.segment == 0]
                assert sum(st.n_out for st in mine) > 0 and all(ac.last_phase(case, st) == st.n_out for st in mine), case.ident
            if case.place == "far":
                assert case.consumed >= 2 ** 40 and case.t_index in (case.consumed - 1, case.consumed), case.ident
                c["far with a fraction"] += case.t_frac != 0
            if case.place.startswith("input"):
                B = 2 ** int(case.place.split()[1])
                assert any(st.consumed < B <= st.consumed + st.call.n - 1 and st.n_out for st in steps), case.ident
    return c


def needed():
    """What must occur in at least one case (for "... calls": in one call)."""
    need = ["tiled calls", "generic calls", "history only calls", "refused calls", "1 ch", "2 ch", "3 ch", "CF32", "CF16", "tiled shape on CF16",
            "contract (1, 1)", "contract (2, 1)", "more than one segment", "calls of samples that yield nothing", "far with a fraction",
            "an even offset other than 0 on a tiled call", "a padded even out_stride with three channels on a tiled call", "a skewed input on a tiled call"]
    need += ["P %d" % p for p in ac.GENERIC_P] + ["T %d" % t for t in ac.GENERIC_T]
    need += ["seam by %s" % how for how in ac.SEAMS] + ["refused in mid-stream, seam by %s" % how for how in ("offset", "out_stride", "rate")]
    need += ["step %#x on a generic call" % s for s in ac.EDGE_STEPS]
    need += ["step %#x on a tiled call" % s for s in ac.FORM_STEPS if s != "log"]
    need += ["step %#x on the tiled shape: %s" % (s, label) for s, label in ((TILED_MIN - 1, "generic"), (TILED_MAX + 1, "refused"))]
    need += ["place %s, the first outputs on a %s call" % (p, k) for p in ac.PLACES for k in ("tiled", "generic")]
    need += ["input passes 2^%d on a %s call" % (b, k) for b in (31, 32) for k in ("tiled", "generic")]
    need += ["%s, on a %s call" % (what, k) for what in ("first output in the history", "last phase") for k in ("tiled", "generic")]
    return need


def test_the_sweep_covers_what_it_is_for():
    cases = ac.cases(SWEEP_SEED, SWEEP_COUNT)
    assert len(cases) == SWEEP_COUNT == 36 and len({c.ident for c in cases}) == SWEEP_COUNT
    assert cases == ac.cases(SWEEP_SEED, SWEEP_COUNT), "the generator is a function of its seed"
    c = coverage(cases)
    print("seed %d: %s" % (SWEEP_SEED, ", ".join("%s %d" % (k, c[k]) for k in sorted(c))))
    missing = [what for what in needed() if c[what] < 1]
    assert not missing, missing
    # the other sweeps' deck
    assert c["CF32"] == 22 and c["CF16"] == 14 and c["placed"] == 12 and sum(ac.has_form(x) for x in cases) == 11, c
    assert sum(x.style == "seam" for x in cases) == 4 and sum(x.style == "clean" for x in cases) == 7, c
    assert c["tiled shape on CF16"] == 7, c
    assert not any((x.P, x.T, x.fmt) == ac.FORM for x in cases if x.style == "mixed")
    # the ends of the header's range, each created
    for what in ("P 2", "P 4096", "T 1", "T 2"):
        assert c[what] >= 1, what
    # at most a quarter of all calls compute nothing (refused calls and calls that yield no output together)
    assert 4 * (c["refused calls"] + c["history only calls"]) <= c["calls"], c


def test_every_draw_is_a_call_the_entry_point_accepts():
    """The argument checks of sxfir_create_arbitrary, sxfir_set_rate, sxfir_set_time, sxfir_set_history and sxfir_resample_arbitrary
    (check_arbitrary_io, check_buffers), restated: legal shapes, formats and steps, a time not below consumed - 1, a lead that
    fills the history, strides that hold the block, calls of fewer than 2^31 inputs, streams within the budgets."""
    for case in ac.cases(SWEEP_SEED, SWEEP_COUNT):
        steps = ac.walk(case)
        assert case.fmt in ("CF32", "CF16") and case.nchan in (1, 2, 3) and 2 <= case.P <= 4096 and 1 <= case.T <= 40, case.ident
        assert ac.taps_of(case).size == case.P * case.T <= 65536 and 1 <= len(steps) <= 12, case.ident      # (ntaps in 1 .. 65536)
        assert all(STEP_MIN <= step <= STEP_MAX for _, step in case.segments), case.ident
        assert all(a[1] != b[1] for a, b in zip(case.segments, case.segments[1:])), case.ident            # (every set_rate changes the rate)
        assert 0 <= case.consumed < 2 ** 62 and case.t_index >= case.consumed - 1 and 0 <= case.t_frac < 2 ** 32, case.ident
        assert (case.place == "start") == ((case.consumed, case.t_index, case.t_frac, case.lead) == (0, 0, 0, 0)), case.ident
        assert case.lead == 0 or (case.lead == ac.hist_len(case) >= case.T and case.lead <= case.consumed), case.ident
        n_in, n_out = sum(st.call.n for st in steps), sum(st.n_out for st in steps)
        assert 0 < n_out <= ac.out_budget(case.P) <= 6 * ac.TILE and n_in <= ac.INPUT_BUDGET, (case.ident, n_in, n_out)
        model = Stream(case.segments[0][1], case.consumed, (case.t_index << 32) | case.t_frac)
        for st in steps:
            call = st.call
            model.step = st.step
            assert (model.consumed, model.t) == (st.consumed, st.t) and len(model.call(call.n)) == st.n_out, case.ident
            assert call.request in (AUTO, TILED, GENERIC) and call.out_off in (0, 1, 2) and call.skew >= 0 and call.band_stride == 0, case.ident
            assert 0 <= call.n < 2 ** 31 and call.in_stride >= call.n and call.out_stride >= st.n_out, (case.ident, call)


def test_the_predictor_on_hand_made_calls():
    """The header's rules on calls written out by hand: every reason to leave the tiled kernel."""
    def case(calls, step=ac.SQRT2, fmt="CF32", nchan=2, shape=(128, 32), consumed=0, t=0):
        return ac.Case("hand", shape[0], shape[1], 0, nchan, fmt, 0, "hand", None, "start", consumed, t >> 32, t & MASK, 0, ((tuple(calls), step),))

    def call(n, request=AUTO, out_off=0, out_stride=4096):
        return Call(n, request, out_off, out_stride, 0, 4096, 0, "bands inside channels")

    def one(*a, **kw):
        kw_case = {k: kw.pop(k) for k in list(kw) if k in ("step", "fmt", "nchan", "shape", "consumed", "t")}
        c = case([call(*a, **kw)], **kw_case)
        return ac.expected_kernel(c, ac.walk(c)[0])

    assert one(640) == "tiled" and one(640, TILED) == "tiled" and one(640, GENERIC) == "generic"
    assert one(640, out_off=1) == "generic" and one(640, TILED, out_off=1) == "refused" and one(640, TILED, out_off=2) == "tiled"
    assert one(640, out_stride=4097) == "generic" and one(640, TILED, out_stride=4097) == "refused" and one(640, TILED, out_stride=4097, nchan=1) == "tiled"
    assert one(640, fmt="CF16") == "generic" and one(640, TILED, fmt="CF16") == "refused" and one(0, TILED, fmt="CF16") == "refused"
    assert one(640, TILED, shape=(128, 33)) == "refused" and one(640, shape=(4, 8)) == "generic"
    for step, want in ((TILED_MIN, "tiled"), (TILED_MAX, "tiled"), (TILED_MIN - 1, "refused"), (TILED_MAX + 1, "refused"), (STEP_MIN, "refused"), (STEP_MAX, "refused")):
        assert one(640, TILED, step=step) == want and one(640, step=step) == ("tiled" if want == "tiled" else "generic"), hex(step)
    # no start rule: any position and time; a call that yields nothing is the history's alone, whatever was asked for
    assert one(640, TILED, consumed=2 ** 40 + 3, t=((2 ** 40 + 2) << 32) + 5) == "tiled"
    assert one(1, TILED) == "history only" and one(0) == "history only" and one(2, TILED) == "tiled"
    assert one(100, TILED, t=120 << 32) == "history only" and one(122, TILED, t=120 << 32) == "tiled"
    c = case([call(640, TILED, out_off=1)])
    st = ac.walk(c)[0]
    assert ac.expected_kernel(c, st, request=AUTO) == "generic" and ac.expected_kernel(c, st, assume_aligned=True) == "tiled"


def test_the_chunked_reference_is_the_plain_blend(oracle):
    """blend_chunked against arb_cases.blend_at over the whole stream in one piece, wherever the x P raster of the whole stream is
    small enough to compute: the same bits, from the start and placed."""
    done = 0
    for case in ac.cases(SWEEP_SEED, SWEEP_COUNT):
        n = sum(c.n for calls, _ in case.segments for c in calls)
        if (case.lead + n) * case.P > 1 << 22:
            continue
        h = ac.taps_of(case)
        raw, xs = ac.stream_input(case, oracle)
        got = ac.reference(oracle, case, h, xs[0])
        want = blend_at(oracle, h, case.P, ac.times_of(case), xs[0], ac.jsplit_of(case), case.consumed - case.lead)
        assert got.size == sum(st.n_out for st in ac.walk(case)) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), case.ident
        done += 1
    assert done >= 30, done


def test_the_placed_reference_is_the_plain_one_at_the_lead(oracle):
    """At consumed = lead the placed stream IS a stream from zero history whose first samples are the lead's: arb_cases.blend_at over
    the lead and the stream in one piece, nothing in front.  And the far stream has the near one's bits exactly: the time's fraction
    and its distance to `consumed` are all an output sees of the position."""
    placed = [c for c in ac.cases(SWEEP_SEED, SWEEP_COUNT) if c.place != "start"]
    assert len(placed) == 12
    for case in placed:
        near = case._replace(consumed=case.lead, t_index=case.t_index - case.consumed + case.lead)
        h = ac.taps_of(case)
        raw, xs = ac.stream_input(case, oracle)
        got = ac.reference(oracle, near, h, xs[0])
        far = ac.reference(oracle, case, h, xs[0])
        assert got.shape == far.shape and np.array_equal(got.view(np.uint32), far.view(np.uint32)), case.ident
        if len(case.segments) == 1 and xs.shape[1] * case.P <= 1 << 22:
            # arb_cases' own blend, in one piece, of a stream whose sample 0 is the lead's first
            times = ac.times_of(near)
            whole = blend_at(oracle, h, case.P, times, xs[0], ac.jsplit_of(case), 0)
            assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), case.ident
            assert all(position(t, case.P)[0] >= case.lead - 1 for t in times), case.ident
    # the reference in arb_cases' own words, from a start: arb_ref cuts the stream into the same calls
    for case in [c for c in ac.cases(SWEEP_SEED, SWEEP_COUNT) if c.place == "start" and c.P <= 128][:6]:
        h = ac.taps_of(case)
        raw, xs = ac.stream_input(case, oracle)
        steps = [(c.n, step) for calls, step in case.segments for c in calls]
        want = arb_ref(oracle, h, case.P, steps, xs[0], ac.jsplit_of(case))
        assert np.array_equal(ac.reference(oracle, case, h, xs[0]).view(np.uint32), want.view(np.uint32)), case.ident
