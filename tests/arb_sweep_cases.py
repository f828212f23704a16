"""The arbitrary-rate resamplers (include/sxfir_arbitrary.h) as tests/rate_cases.py has the rate-changing kinds: a seeded generator of
streams, a predictor of the kernel each call takes and the float32 reference of a whole stream, from zero history or PLACED
(sxfir_set_history + sxfir_set_time) anywhere in a 64-bit stream.  The count rule is driven by the time, not by up / down, so the
generator is this module's own; the calls (Call, their strides and placements) and the sizes' menu are band_cases', the model
(Stream, count) and the blend (blend_at) arb_cases'.  CPU only: torch is never imported.  tests/test_arb_sweep_host.py checks the
generator's coverage and the references; tests/test_gpu_arb_sweep.py runs the cases."""
import collections
import math

import numpy as np

from arb_cases import MASK, ONE, STEP_MAX, STEP_MIN, Stream, arb_taps, blend_at, count, position
from band_cases import AUTO, GENERIC, GUARD, TILED, Call, _make_call, _sizes                # noqa: F401

SWEEP_SEED, SWEEP_COUNT = 0, 36                             # what the GPU sweep runs; tests/test_arb_sweep_host.py holds them to the coverage
TILE = 256                                                  # OUTPUTS per tile of resample_arb_kernel
TILE_BUDGET = 6                                             # a stream: six tiles of outputs at the most ...
INPUT_BUDGET = TILE_BUDGET * TILE * 16                      # ... and, at the large steps, fewer inputs than six tiles take at step 16
FORM = (128, 32, "CF32")                                    # (P, T, format) of the tiled kernel
TILED_MIN, TILED_MAX = 1 << 31, 1 << 33                     # the steps the tiled kernel takes
TILED_KERNEL, GENERIC_KERNEL = "resample_arb_kernel", "resample_arb_generic_kernel"
SQRT2 = 0x16A09E667
# the generic shapes, dealt in turn (the T's turn moves on by one with every round of the P's, so that the pairs change); (128, 32)
# on CF32 has the tiled kernel and is skipped there.  The ends of the header's range: P = 2 and 4096; T = 1 and 2 -- a history of 2
# samples, the contracts (1, 1) and (2, 1)
GENERIC_P = (2, 3, 4, 7, 128, 129, 1000, 4096)
GENERIC_T = (1, 2, 3, 8, 31, 32, 33, 40)
NTAPS_MAX = 65536                                           # sxfir_create_arbitrary: P T taps at the most; a pair above it takes the next smaller T that fits
# the steps, dealt in turn; "log": drawn uniformly in log scale.  The tiled shape on CF32 takes the first deck -- the ends of the
# tiled range, unity and its neighbours, sqrt 2 --, every other plan the second: the tiled range's outer neighbours, the ends of the
# allowed range, and the first deck's
FORM_STEPS = (TILED_MIN, TILED_MAX, ONE, ONE + 1, ONE - 1, SQRT2, "log")
ALL_STEPS = (TILED_MIN - 1, TILED_MAX + 1, STEP_MIN, STEP_MAX, TILED_MIN, TILED_MAX, ONE, ONE + 1, ONE - 1, SQRT2, "log", "log")
EDGE_STEPS = tuple(s for s in ALL_STEPS if s != "log")
# where a placed stream starts.  "far": consumed = 2^40 + k, the first output in the history or on the first new sample, any
# fraction.  "input 31" / "input 32": the input index passes 2^31 / 2^32 inside the stream's largest call.  "ahead": the time lies
# beyond the first one or two calls, which yield nothing and only carry history; the first output falls in the middle of a later
# call.  "last phase": a fraction in the last 1 / P of a sample under a unit step -- every output of the first segment has p = P - 1
PLACES = ("far", "input 31", "input 32", "ahead", "last phase")
# how the four "seam" cases leave the tiled kernel in mid-stream: the output one sample in, an odd channel stride, a forced GENERIC,
# and sxfir_set_rate to the tiled range's outer neighbours (2^31 - 1 under AUTO, then 2^33 + 1 under a forced TILED) and back
SEAMS = ("offset", "out_stride", "generic", "rate")

KIND = collections.namedtuple("Kind", "banded_in banded_out")(False, False)                  # what band_cases._make_call asks of a kind
Case = collections.namedtuple("Case", "ident P T tap_seed nchan fmt data_seed style how place consumed t_index t_frac lead segments")
# segments: ((calls, step), ...) -- sxfir_set_rate(step) in front of every segment but the first, whose step the plan is created
# with.  place: "start" (consumed = t = 0, no lead) or one of PLACES; consumed, t_index, t_frac: what sxfir_set_time takes; lead:
# the samples in front of the stream that sxfir_set_history takes.
Step = collections.namedtuple("Step", "segment index call step consumed t n_out")
# one call of a stream as the model sees it: the state in front of it (step, consumed, t as one Q.32 integer) and its outputs


def has_form(case):
    return (case.P, case.T, case.fmt) == FORM


def jsplit_of(case):
    """The contract: (2, 1) when T is even, else (1, 1)."""
    return 2 if case.T % 2 == 0 else 1


def hist_len(case):
    """What sxfir_set_history asks for: T rounded up to even."""
    return (case.T + 1) & ~1


def out_budget(P):
    """Outputs of a stream: six tiles; correspondingly fewer for a plan whose x P raster is finer than 1024 samples per input."""
    return TILE_BUDGET * TILE * (1024 if P > 1024 else P) // P


def taps_of(case):
    return arb_taps(case.P, case.T, case.tap_seed)


def make_plan(case, h):
    import sxxcvr_amd
    return sxxcvr_amd.ArbitraryResampler(h, case.P, step=case.segments[0][1], nchan=case.nchan, fmt=case.fmt)


def walk(case):
    """[Step]: every call of the stream in order, with the model's state in front of it."""
    model = Stream(case.segments[0][1], case.consumed, (case.t_index << 32) | case.t_frac)
    out = []
    for s, (calls, step) in enumerate(case.segments):
        model.step = step
        for call in calls:
            before = (model.consumed, model.t)
            n_out = len(model.call(call.n))
            out.append(Step(s, len(out), call, step, before[0], before[1], n_out))
    return out


def times_of(case):
    """The absolute times (Q.32) of all outputs of the stream."""
    return [st.t + m * st.step for st in walk(case) for m in range(st.n_out)]


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _log_step(rng, lo, hi):
    return int(min(max(round(2.0 ** rng.uniform(math.log2(lo), math.log2(hi))), lo), hi))


def tile_inputs(step):
    """The input span of a tile of 256 outputs at a step, one at the least."""
    return max((TILE * step) >> 32, 1)


def _one_case(rng, index, slot, shape, dealt_step, place, clean_turn):
    shape_tiled, fmt, style, how = slot
    P, T = shape
    form = (P, T, fmt) == FORM
    lo, hi = (TILED_MIN, TILED_MAX) if form else (STEP_MIN, STEP_MAX)
    step0 = _log_step(rng, lo, hi) if dealt_step == "log" else dealt_step
    nchan = 3 if how == "out_stride" or (style == "clean" and clean_turn % 3 == 2) else int(rng.choice([1, 1, 2, 3]))
    budget_out, budget_in = out_budget(P), INPUT_BUDGET * out_budget(P) // (TILE_BUDGET * TILE)
    # the time in front of the first call, relative to consumed = 0 (the place moves the stream, not its counts)
    t_rel, ahead = 0, []
    if place == "far":
        t_rel = (int(rng.integers(-1, 1)) << 32) + int(rng.integers(0, 1 << 32))
    elif place in ("input 31", "input 32"):
        t_rel = (int(rng.integers(-1, 1)) << 32) + int(rng.integers(1, 1 << 32))
    elif place == "last phase":
        t_rel = (int(rng.integers(-1, 1)) << 32) + (1 << 32) - int(rng.integers(1, (1 << 32) // P + 1))
    segments, calls = [], []
    first_step = ONE if place == "last phase" else step0
    model = Stream(first_step, 0, 0)
    T_in = tile_inputs(step0)
    if place == "ahead":
        # one or two calls that yield nothing, then a gap into the call after them
        ahead = [int(rng.choice([1, 3, T + 5, T_in]))] + ([int(rng.choice([2, max(T - 1, 1)]))] if rng.integers(0, 2) else [])
        ahead = [min(n, budget_in // 8) for n in ahead]
        gap = int(rng.integers(1, max(min(T_in, budget_in // 4), 2)))
        t_rel = ((sum(ahead) + gap) << 32) + int(rng.integers(0, 1 << 32))
    model.t = t_rel

    def fits(n):
        k = count(model.t, model.step, model.consumed, n)[0]
        return model.produced + k <= budget_out and model.consumed + n <= budget_in

    def add(n, request, perturb, off=None):
        call = _make_call(rng, KIND, None, nchan, None, n, request, perturb, "bands inside channels",
                          n_out=count(model.t, model.step, model.consumed, n)[0])
        calls.append(call if off is None else call._replace(out_off=off))
        model.call(n)

    def set_rate(step):
        nonlocal calls
        segments.append((tuple(calls), model.step))
        calls = []
        model.step = step

    for n in ahead:
        assert count(model.t, model.step, model.consumed, n)[0] == 0
        add(n, int(rng.choice([AUTO, TILED])) if form else AUTO, None if style != "mixed" else "any")
    extra = (model.t >> 32) - model.consumed + 2 if ahead else 0             # what the call after them needs to reach the first output
    if place == "last phase":
        # the first segment: a unit step, every output of the last phase; then on to the dealt step
        n = int(rng.integers(T + 3, T + 60))
        add(n, AUTO, None if style != "mixed" else "any")
        if step0 != ONE:
            set_rate(step0)
    if style == "clean":
        # every call on the tiled kernel's terms: aligned, even strides -- at an even offset of 0 or (every other clean case) 2 samples
        sizes = [T_in, int(rng.integers(2, 4)) * T_in + int(rng.integers(1, T_in)), max(T - 1, 1), T_in + 1, 1, 0, T_in - 1, 3]
        offs = (0, 2) if clean_turn % 2 == 0 else (0, 0)
        add(sizes[int(rng.integers(0, 2))] + extra, int(rng.choice([AUTO, TILED])), None, offs[1])
        for j in range(int(rng.integers(1, 5))):
            n = sizes[int(rng.integers(len(sizes)))]
            if j == 1 and rng.integers(0, 2):
                set_rate(_log_step(rng, lo, hi))
            if fits(n):
                add(n, int(rng.choice([AUTO, AUTO, TILED])), None, offs[j % 2])
    elif style == "seam":
        # tiled, generic, tiled in the middle of one stream
        a = T_in + int(rng.integers(0, T_in))
        b = int(rng.integers(1, T_in // 2 + 20))
        add(a + extra, int(rng.choice([AUTO, TILED])), None)
        if how == "rate":
            set_rate(TILED_MIN - 1)
        add(b, GENERIC if how == "generic" else AUTO, how if how in ("offset", "out_stride") else None)
        if how == "rate":
            set_rate(step0)
        add(int(rng.choice([T_in, T_in + 1, 2 * T_in])), int(rng.choice([AUTO, TILED])), None)
        if how != "generic":
            if how == "rate":
                set_rate(TILED_MAX + 1)
            add(int(rng.integers(1, 60)), TILED, how if how != "rate" else None)        # under a forced TILED: refused in mid-stream
            if how == "rate":
                set_rate(step0)
                add(T_in + int(rng.integers(0, 40)), TILED, None)
        menu = _sizes(rng, T_in, T) if T_in > 1 else [0, 1, 2, 3]
        for _ in range(int(rng.integers(0, 3))):
            n = menu[int(rng.integers(len(menu)))]
            if fits(n):
                add(n, int(rng.choice([AUTO, AUTO, GENERIC, TILED])), "any")
    else:
        menu = _sizes(rng, max(T_in, 2), T)
        change = int(rng.integers(1, 6)) if rng.integers(0, 3) == 0 else None
        if extra:
            add(extra + int(rng.integers(1, T_in + 2)), AUTO, "any")
        for j in range(int(rng.integers(2, 7))):
            if j == change and model.produced:
                set_rate(_log_step(rng, lo, hi))
            n = menu[int(rng.choice([0, 1, 2, 3] + 3 * [4, 5, 6, 7, 8]))]
            if not fits(n):
                n = menu[int(rng.integers(0, 5))]
            if fits(n):
                add(n, int(rng.choice([AUTO, AUTO, AUTO, AUTO, GENERIC, GENERIC, GENERIC, TILED])), "any")
        if model.produced < 8:
            set_rate(step0)
            n = min(T_in + 2, budget_in - model.consumed)
            while not fits(n):
                n -= max(n // 8, 1)
            add(n, AUTO, "any")                             # (every stream computes something at its dealt step)
    segments.append((tuple(calls), model.step))
    segments = [s for s in segments if s[0] or s is segments[0]]
    assert 0 < model.produced <= budget_out and model.consumed <= budget_in + extra, (index, model.produced, model.consumed)
    # the place: where consumed = 0 of the model lies in the 64-bit stream
    if place == "start":
        consumed = 0
    elif place == "far":
        consumed = 2 ** 40 + int(rng.integers(0, 1000))
    elif place in ("input 31", "input 32"):
        B = 2 ** int(place.split()[1])
        flat = [c for seg in segments for c in seg[0]]
        j = max(range(len(flat)), key=lambda i: flat[i].n)
        p, n = sum(c.n for c in flat[:j]), flat[j].n
        assert n >= 4, (index, n)
        consumed = B - p - n // 2                           # input B - 1 and input B are the call's: consumed + p < B <= consumed + p + n - 1
    else:
        consumed = int(rng.integers(1, 5000))
    t = (consumed << 32) + t_rel
    lead = 0 if place == "start" else (T + 1) & ~1
    shape = "%dx%d" % (P, T)
    ident = "%02d-%s-%s-%dch-%s" % (index, shape, fmt, nchan, style) + ("" if place == "start" else "-" + place.replace(" ", ""))
    return Case(ident, P, T, 100 + index, nchan, fmt, 7000 + index, style, how, place, consumed, t >> 32, t & MASK, lead, tuple(segments))


def cases(seed, n):
    """n seeded cases, as plain tuples.  The other sweeps' deck: of 36 slots, the tiled shape on CF32 in 11 -- seven keep to the tiled
    kernel's terms in every call ("clean"), four leave it and come back in mid-stream ("seam", one by each of SEAMS) --, a generic
    shape on CF32 in 11 and CF16 in 14, on the tiled and a generic shape in turn ("mixed": every call's size, kernel request and
    placement drawn).  A third of the slots are PLACED streams: five of the clean ones, four of the generic eleven and three of the
    fourteen.  What must occur at least once is dealt in turn over the cases, not drawn: the places (to the tiled shape on CF32 and
    to all others apart, so that each meets both kernels), the generic shapes, the steps."""
    rng = np.random.default_rng([seed, 200])
    deck = []
    for i in range(n):
        slot = i % 36
        placed = slot in (1, 3, 4, 6, 7, 12, 15, 18, 21, 23, 26, 29)
        if slot < 11:
            seam = (2, 5, 8, 10).index(slot) if slot in (2, 5, 8, 10) else None
            deck.append(((True, "CF32", "clean" if seam is None else "seam", None if seam is None else SEAMS[seam]), placed))
        elif slot < 22:
            deck.append(((False, "CF32", "mixed", None), placed))
        else:
            deck.append(((slot % 2 == 0, "CF16", "mixed", None), placed))
    order = rng.permutation(n)
    out = []
    turn = collections.Counter()
    for i in range(n):
        slot, placed = deck[int(order[i])]
        form = "form" if slot[0] and slot[1] == "CF32" else "other"
        shape = FORM[:2]
        while not slot[0]:
            g = turn["generic"]
            P, j = GENERIC_P[g % 8], (g + g // 8) % 8
            while P * GENERIC_T[j] > NTAPS_MAX:             # (4096 phases: 16 taps per phase at the most, so 8 of GENERIC_T)
                j = (j - 1) % 8
            shape = (P, GENERIC_T[j])
            turn["generic"] += 1
            if shape + (slot[1],) != FORM:
                break
        steps = FORM_STEPS if form == "form" else ALL_STEPS
        place = PLACES[turn["placed " + form] % len(PLACES)] if placed else "start"
        out.append(_one_case(rng, i, slot, shape, steps[turn[form] % len(steps)], place, turn["clean"]))
        turn[form] += 1
        turn["placed " + form] += placed
        turn["clean"] += slot[2] == "clean"
    return out


# ---- the predictor ---------------------------------------------------------------------------------------------------------------
def expected_kernel(case, st, request=None, assume_aligned=False):
    """"tiled" | "generic" | "history only" | "refused" for the call `st` (a Step of walk(case)), every call before it having been made
    (a refused one again under AUTO).  The header's rule: the tiled kernel runs when the shape and format have one (128 x 32 on
    CF32), the request is not GENERIC, the step lies in [2^31, 2^33], the output is 16-byte aligned and out_stride is even with
    nchan > 1 -- at any stream position and time; under a forced TILED "refused" replaces "generic" -- sxfir_set_kernel's own refusal
    where the plan has no tiled kernel at all.  A call that yields no output only carries its samples into the history, whatever
    was asked for.  `request`: another request than the call's own (AUTO: the call repeated after a refusal); `assume_aligned`: what
    sxfir_launch_geometry answers, which takes the output's placement for good."""
    call = st.call
    request = call.request if request is None else request
    form = has_form(case)
    if request == TILED and not form:
        return "refused"
    if st.n_out == 0:
        return "history only"
    aligned = assume_aligned or (call.out_off % 2 == 0 and (case.nchan == 1 or call.out_stride % 2 == 0))
    if form and request != GENERIC and aligned and TILED_MIN <= st.step <= TILED_MAX:
        return "tiled"
    return "refused" if request == TILED else "generic"


# ---- a stream's data -------------------------------------------------------------------------------------------------------------
def stream_input(case, oracle):
    """(raw, xs): the lead and the stream behind it, lead + N samples per channel, as stored words, int32 [nchan, lead + N, words per
    sample], and as the complex64 values the kernels filter.  CF32: components uniform in [-1, 1); CF16: the same rounded to half
    (the stored halves are the input, exactly)."""
    rng = np.random.default_rng(case.data_seed)
    shape = (case.nchan, case.lead + sum(c.n for calls, _ in case.segments for c in calls))
    x = rng.uniform(-1, 1, size=shape + (2,)).astype(np.float32)
    if case.fmt == "CF16":
        halves = oracle.f32_to_f16(x)
        raw = np.ascontiguousarray(halves).view(np.uint32).view(np.int32)
        return raw.reshape(shape + (1,)), np.ascontiguousarray(oracle.f16_to_f32(halves)).view(np.complex64).reshape(shape)
    return np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(x).view(np.complex64).reshape(shape)


RASTER = 1 << 20                                            # samples of the x P raster one oracle.interp_f32 call computes, at the most
SPARSE = 64                                                 # outputs further apart than this on the raster are computed one by one


def blend_chunked(oracle, h, P, times, x, jsplit, x0):
    """arb_cases.blend_at over the times in chunks of outputs: blend_at computes the x P raster between a chunk's first and last
    output, which for a whole stream is inputs x P samples -- 10^8 at 4096 phases and step 16, for 1500 outputs that read two of
    them each.  A chunk ends where the raster's span would pass RASTER, or where the next output lies more than SPARSE raster
    samples on.  Each chunk sees the samples its chains read alone: T + 1 in front of its first output's (tests/test_gpu_arb.py's
    window), or all there are -- below x0 the stream is zeros, as blend_at has it."""
    T = len(h) // P
    x = np.ascontiguousarray(x, dtype=np.complex64)
    out, i = [], 0
    k = [(t * P) >> 32 for t in times]
    while i < len(times):
        j = i + 1
        while j < len(times) and k[j] - k[j - 1] <= SPARSE and k[j] - k[i] < RASTER:
            j += 1
        lo = max((times[i] >> 32) - T - 1, x0)
        hi = (times[j - 1] >> 32) + 2
        out.append(blend_at(oracle, h, P, times[i:j], x[lo - x0:hi - x0], jsplit, lo))
        i = j
    return np.concatenate(out) if out else np.zeros(0, dtype=np.complex64)


def reference(oracle, case, h, x):
    """The float32 reference of one channel's stream, x = the lead then the stream (stream_input): blend_at over the model's times.

    A stream placed at (consumed, t) is DEFINED as the same samples behind the lead with zeros in front of the lead.  No output
    sees the zeros: floor(t) >= consumed - 1 for every output, its chains reach T - 1 samples back from there, and the lead is T
    samples or more.  The time is a Python int throughout; arb_cases.position splits it."""
    assert case.lead == 0 or case.lead >= case.T
    return blend_chunked(oracle, h, case.P, times_of(case), x, jsplit_of(case), case.consumed - case.lead)


def stored_words(oracle, fmt, ref):
    """The reference as the plan stores it, uint32 [n_out, words per sample]: CF16: one rounding to half, after the blend."""
    ref = np.ascontiguousarray(ref, dtype=np.complex64)
    if fmt == "CF16":
        return np.ascontiguousarray(oracle.f32_to_f16(ref.view(np.float32))).view(np.uint32).reshape(ref.shape + (1,))
    return ref.view(np.uint32).reshape(ref.shape + (2,))


def last_phase(case, st):
    """How many of the call's outputs are of the last phase, p = P - 1: their second chain is phase 0 of the next input."""
    return sum(1 for m in range(st.n_out) if position(st.t + m * st.step, case.P)[1] == case.P - 1)
