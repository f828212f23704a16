"""The two plan kinds that change the rate by more than a band plan does -- frequency-translating decimators
(include/sxfir_translate.h, "translate") and rational resamplers (include/sxfir_rational.h, "rational") -- as tests/band_cases.py has
the six band kinds: a seeded generator of streams, a predictor of the kernel each call takes, and the float32 reference of a whole
stream, from zero history or PLACED (sxfir_set_history + sxfir_set_position) anywhere in a 64-bit stream.  CPU only: torch is never
imported.  tests/test_rate_cases_host.py checks the generator's coverage and the references; tests/test_gpu_rate_sweep.py runs the
cases.  The calls (Call, their strides and placements) and the sizes' menu are band_cases' own.

One description serves both kinds: `up` outputs for every `down` inputs (translate: up = 1, down = the ratio), so after c inputs
ceil(c up / down) outputs exist (rational_cases.n_out_for)."""
import collections
import math

import numpy as np

from band_cases import AUTO, CX_RATIOS, GENERIC, GUARD, TILED, Call, Contract, _layout, _make_call, _sizes, _stride     # noqa: F401
from band_cases import contract as band_contract
from gpu_util import random_taps_cx
from mix_cases import mix_ref, step
from rational_cases import n_out_for, rational_ref, rational_taps

SWEEP_SEED, SWEEP_COUNT = 0, 36                             # what the GPU sweep runs; tests/test_rate_cases_host.py holds them to the coverage

Kind = collections.namedtuple("Kind", "name tiled_shape tile start_multiple tiled generic formats banded_in banded_out")
# tiled_shape: (ntaps, up, down) with a tiled kernel, on CF32.  tile: its inputs per tile.  start_multiple: the tiled kernel takes a
# call whose stream position is a multiple of it.  formats: CF32, CF16 and the kind's third -- S32 wire words in (CF32 out) for
# translate; rational refuses S32, CF16 again.  banded_*: what band_cases._make_call asks of a kind (no bands on either side).
KINDS = collections.OrderedDict((k.name, k) for k in (
    Kind("translate", (128, 1, 4), 2048, 4, "decim4_mix_kernel", "decim_mix_generic_kernel", ("CF32", "CF16", "S32"), False, False),
    Kind("rational", (128, 4, 5), 1280, 5, "resample45_kernel", "resample_generic_kernel", ("CF32", "CF16", "CF16"), False, False),
))
# rational, generic: the coprime pairs, dealt in turn; taps per phase drawn from 1..40 -- four for the two pairs with a side above 64
RATIONAL_PAIRS = ((2, 3), (3, 2), (3, 4), (5, 4), (7, 5), (3, 8), (8, 3), (4, 5), (125, 128), (128, 125))
# the mixer, dealt in turn: (class, den, num or None).  "max": the num whose s = num ratio mod den is the largest the ratio allows,
# den - gcd(ratio, den) (at /4 with den 65536: num 65535, s 65532); "one": the smallest s above 0, gcd(ratio, den) (1 where the two
# are coprime); "zero": s = 0.  The others name their num: negative, above den, plain.
MIXERS = (("max", 65536, None), ("max", 65535, None), ("one", 7, None), ("one", 65535, None), ("zero", 1, None), ("zero", 8, None),
          ("zero", 4096, None), ("negative", 7, -3), ("negative", 1000, -123), ("negative", 2, -1), ("above", 5, 13),
          ("above", 65535, 70000), ("above", 3, 11), ("plain", 2, 1), ("plain", 3, 1), ("plain", 5, 2), ("plain", 7, 3), ("plain", 8, 5),
          ("plain", 1000, 123), ("plain", 4096, 1001), ("plain", 65536, 12345), ("plain", 65536, 49380), ("plain", 65535, 65534))
DENS = (1, 2, 3, 5, 7, 8, 1000, 4096, 65535, 65536)
# where a placed stream starts: 2^40 + k, or so that the named index passes 2^31 / 2^32 INSIDE the case's largest call
PLACES = {"translate": ("far", "input 31", "output 31", "input 32", "output 32"),
          "rational": ("far", "input 31", "output 31", "raster 31", "input 32", "output 32", "raster 32")}
SEAMS = ("offset", "out_stride", "generic", "position")      # how the four "seam" cases leave the tiled kernel in mid-stream

Case = collections.namedtuple("Case", "ident ntaps up down num den tap_seed nchan fmt data_seed style how place c0 calls")
# ntaps: all taps (rational: up times the taps per phase).  num, den: the mixer (rational: 0, 0).  how: a seam case's perturbation.
# place: "start" (c0 = 0) or one of PLACES; c0: the stream position of the first call.


def hist_of(case):
    """Samples of the stream a call still needs from before it: ntaps for translate, the taps per phase for rational."""
    return case.ntaps // case.up


def hist_len(case):
    """What sxfir_set_history asks for: hist_of rounded up to even (sxfir_plan.hip.h, sxfir_rational.hip.h: hist_len)."""
    return (hist_of(case) + 1) & ~1


def lead_of(case):
    """Samples in front of a placed stream that the test hands to sxfir_set_history: the fewest that fill the plan's history and
    leave lead = c0 modulo `down`, the filter part's period in input samples."""
    if case.place == "start":
        return 0
    lead = hist_len(case)
    return lead + (case.c0 - lead) % case.down


def has_form(kind, case):
    return case.fmt == "CF32" and (case.ntaps, case.up, case.down) == KINDS[kind].tiled_shape


def contract(kind, case):
    """The numeric contract the plan must report.  translate: the complex-tap decimator's of the shape (sxfir_translate.h: "z[m] has
    the bits of the sxfir_create_complex plan of the same shape").  rational: the x up interpolator's -- a phase's taps in two halves
    when their count is even, else one chain (sxfir_rational.h)."""
    if kind == "translate":
        return band_contract("decimate_cx", case.ntaps, case.down)
    return Contract((2 if hist_of(case) % 2 == 0 else 1, 1))


def taps_of(kind, case):
    """Random taps without symmetry: complex for translate, real for rational."""
    if kind == "translate":
        return random_taps_cx(case.ntaps, case.tap_seed)
    return rational_taps(case.up, case.ntaps // case.up, case.tap_seed)


def make_plan(kind, case, h):
    import sxxcvr_amd
    if kind == "translate":
        return sxxcvr_amd.TranslatingDecimator(h, case.down, case.num, case.den, nchan=case.nchan, fmt=case.fmt)
    return sxxcvr_amd.RationalResampler(h, case.up, case.down, nchan=case.nchan, fmt=case.fmt)


def outputs_for(case, consumed, n):
    """Outputs of a call of n inputs at the absolute stream position `consumed`."""
    return n_out_for(n, case.up, case.down, consumed)


def position_before(case, call_index):
    """The absolute stream position in front of call `call_index`."""
    return case.c0 + sum(c.n for c in case.calls[:call_index])


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def mixer_num(cls, den, num, ratio):
    """The num of a MIXERS entry at a ratio."""
    if num is not None:
        return num
    g = math.gcd(ratio, den)
    if cls == "zero":
        return den // g                                     # num ratio = (ratio / g) den
    inv = pow(ratio // g, -1, den // g) if den // g > 1 else 0                 # (ratio / g) inv = 1 modulo den / g: num ratio = g modulo den
    return inv if cls == "one" else (den // g - inv) % (den // g) + (den // g) * (g - 1)        # (the largest such num below den)


def s_classes(case):
    """The classes of MIXERS a translate case's (num, den) falls into, from the numbers themselves."""
    s, g = step(case.num, case.den, case.down), math.gcd(case.down, case.den)
    out = set()
    if case.den >= 65535 and s == case.den - g:
        out.add("s = den - gcd, den %d" % case.den)
    if s == 1:
        out.add("s = 1")
    if s == 0:
        out.add("s = 0")
    if case.num < 0:
        out.add("negative num")
    if case.num > case.den:
        out.add("num above den")
    return out


def _first_position(rng, K, up, down, calls, r, place):
    """c0 = r modulo `down` for a place of PLACES.  An index passes B = 2^31 / 2^32 inside the largest call, [c0 + p, c0 + p + n):
    "input": c0 + p < B <= c0 + p + n - 1.  "output": outputs B - 1 and B are the call's; output m is made when its newest input,
    floor(m down / up), arrives.  "raster": as "output" for the first m with m down >= B, the x up raster's index of output m."""
    if place == "far":
        mid = 2 ** 40 + int(rng.integers(0, 1000))
    else:
        index, log2 = place.split()
        B = 2 ** int(log2)
        j = max(range(len(calls)), key=lambda i: calls[i].n)
        p, n = sum(c.n for c in calls[:j]), calls[j].n
        if index == "input":
            lo, hi = B - p - (n - 1), B - p - 1
        else:
            m = B if index == "output" else -(-B // down)
            lo, hi = m * down // up - p - (n - 1), (m - 1) * down // up - p
        mid = (lo + hi) // 2
        assert hi - lo >= 2 * down, (place, n)
    return mid - (mid - r) % down


def _one_case(rng, kind, index, slot, pair, mixer, place):
    K = KINDS[kind]
    shape_tiled, fmt, style, how, keep_rule = slot
    num = den = 0
    if kind == "translate":
        ntaps, up, down = K.tiled_shape
        while not shape_tiled and (ntaps, up, down) == K.tiled_shape:
            ntaps, down = int(rng.integers(4, 301)), int(rng.choice(CX_RATIOS))         # any count
        cls, den, num = mixer
        num = mixer_num(cls, den, num, down)
    elif shape_tiled:
        ntaps, up, down = K.tiled_shape
    else:
        up, down = pair
        while True:
            per_phase = 4 if max(up, down) > 64 else int(rng.integers(1, 41))
            if (up * per_phase, up, down) != K.tiled_shape:
                break
        ntaps = up * per_phase
    form = shape_tiled and fmt == "CF32"
    nchan = 3 if how == "out_stride" else int(rng.choice([1, 1, 2, 3]))        # (an odd out_stride leaves the tiled kernel with nchan > 1 only)
    T, hist, q = K.tile, ntaps // up, K.start_multiple
    # the stream's first position modulo `down`: what the calls' output counts depend on, and for a plan with a tiled kernel
    # (down = q) whether the start rule holds
    if place == "start" or (form and keep_rule):
        r = 0
    elif form:
        r = int(rng.integers(1, q))
    else:
        r = int(rng.integers(0, down))
    budget = 6 * T
    calls, consumed = [], 0

    def add(n, request, perturb):
        nonlocal consumed, budget
        calls.append(_make_call(rng, K, None, nchan, None, n, request, perturb, "bands inside channels", n_out=n_out_for(n, up, down, r + consumed)))
        consumed += n
        budget -= n

    if style == "clean":
        # every call on the tiled kernel's terms: aligned, even strides, sizes that keep the stream on its positions
        sizes = [T, int(rng.integers(2, 4)) * T + q * int(rng.integers(1, T // q)), q * max((hist - 1) // q, 1), T + q, q, 0, T - q]
        add(sizes[int(rng.integers(0, 2))], int(rng.choice([AUTO, TILED])), None)
        for _ in range(int(rng.integers(0, 5))):
            n = sizes[int(rng.integers(len(sizes)))]
            if n <= budget:
                add(n, int(rng.choice([AUTO, AUTO, TILED])), None)
    elif style == "seam":
        # tiled, generic, tiled in the middle of one stream: the history goes from the tiled kernel to history_kernel and back
        a = T + q * int(rng.integers(0, T // q))
        b = q * int(rng.integers(1, (T + 40) // q))
        if how == "position":
            # the first call ends off the tiled kernel's positions, the second brings the stream back onto them
            off = int(rng.integers(1, q))
            a, b = a + off, b + q - off
        add(a, int(rng.choice([AUTO, TILED])), None)
        add(b, GENERIC if how == "generic" else AUTO, how if how in ("offset", "out_stride") else None)
        add(int(rng.choice([T, T + q, 2 * T])), int(rng.choice([AUTO, TILED])), None)
        if how in ("offset", "out_stride"):
            add(q * int(rng.integers(1, 60)), TILED, how)   # the same placement under a forced TILED: refused in mid-stream
        menu = _sizes(rng, T, hist)
        for _ in range(int(rng.integers(0, 3))):
            n = menu[int(rng.integers(len(menu)))]
            if n <= budget:
                add(n, int(rng.choice([AUTO, AUTO, GENERIC, TILED])), "any")
    else:
        # (the menu's four smallest sizes at a third of the others' weight and a forced TILED in one call of eight: most of these plans
        # have no tiled kernel, and at /16 a call of three samples seldom completes an output -- three calls of four compute something)
        menu = _sizes(rng, T, hist)
        for _ in range(int(rng.integers(1, 6))):
            n = menu[int(rng.choice([0, 1, 2, 3] + 3 * [4, 5, 6, 7, 8]))]
            if n > budget:
                n = menu[int(rng.integers(0, 5))]
            if n <= budget:
                add(n, int(rng.choice([AUTO, AUTO, AUTO, AUTO, GENERIC, GENERIC, GENERIC, TILED])), "any")
        if consumed == 0 or (place != "start" and max(c.n for c in calls) < T - 1):
            add(T + 1, AUTO, "any")                         # (a placed stream has a call the index can pass its mark in)
    c0 = 0 if place == "start" else _first_position(rng, K, up, down, calls, r, place)
    shape = "%dx%d" % (ntaps, down) if kind == "translate" else "%dx%d:%d" % (ntaps, up, down)
    ident = "%02d-%s-%s-%dch-%s" % (index, shape, fmt, nchan, style) + ("" if place == "start" else "-" + place.replace(" ", ""))
    return Case(ident, ntaps, up, down, num, den, 100 + index, nchan, fmt, 7000 + index, style, how, place, c0, tuple(calls))


def cases(kind, seed, n):
    """n seeded cases of one kind, as plain tuples.  band_cases' deck: of 36 slots, the tiled shape on CF32 in 11 -- seven keep to
    the tiled kernel's terms in every call ("clean"), four leave it and come back in mid-stream ("seam", one by each of SEAMS) --, a
    generic shape on CF32 in 11 and CF16 and the kind's third format in turn in 14, on the tiled and a generic shape in turn
    ("mixed": every call's size, kernel request and placement drawn).  A third of the slots are PLACED streams, four of each eleven
    and of the fourteen; of the four on the tiled kernel's shape two keep its start rule and two break it.  What must occur at least
    once is dealt in turn over the cases, not drawn: the places of PLACES, the rational pairs, the mixers."""
    K = KINDS[kind]
    rng = np.random.default_rng([seed, 100 + list(KINDS).index(kind)])
    deck = []
    for i in range(n):
        slot = i % 36
        placed = slot in (1, 4, 5, 7, 12, 15, 18, 21, 23, 26, 29, 32)      # (1, 5 keep the start rule; 4, 7 -- no seam case -- break it)
        if slot < 11:
            seam = (2, 5, 8, 10).index(slot) if slot in (2, 5, 8, 10) else None
            deck.append(((True, "CF32", "clean" if seam is None else "seam", None if seam is None else SEAMS[seam], slot in (1, 5)), placed))
        elif slot < 22:
            deck.append(((False, "CF32", "mixed", None, False), placed))
        else:
            deck.append(((slot % 2 == 0, K.formats[1 + (slot // 2) % 2], "mixed", None, False), placed))
    order = rng.permutation(n)
    out, n_generic, n_placed = [], 0, 0
    for i in range(n):
        slot, placed = deck[int(order[i])]
        place = PLACES[kind][n_placed % len(PLACES[kind])] if placed else "start"
        out.append(_one_case(rng, kind, i, slot, RATIONAL_PAIRS[n_generic % len(RATIONAL_PAIRS)], MIXERS[i % len(MIXERS)], place))
        n_generic += not slot[0]
        n_placed += placed
    assert all(sum(c.n for c in case.calls) <= 6 * K.tile for case in out)
    return out


# ---- the predictor ---------------------------------------------------------------------------------------------------------------
def expected_kernel(kind, case, call_index, request=None, assume_aligned=False):
    """"tiled" | "generic" | "history only" | "refused" for call `call_index` of the stream, every call before it having been made
    (a refused one again under AUTO).  The headers' rules: the tiled kernel runs when the shape and format have one and the request is
    not GENERIC, the output is 16-byte aligned, out_stride is even with nchan > 1 and the stream position is a multiple of 4
    (translate) or 5 (rational); under a forced TILED "refused" replaces "generic" -- sxfir_set_kernel's own refusal where the plan
    has no tiled kernel at all.  A call that completes no output only carries its samples into the history, whatever was asked for.
    `request`: another request than the call's own (AUTO: the call repeated after a refusal); `assume_aligned`: what
    sxfir_launch_geometry answers, which takes the output's placement for good."""
    call = case.calls[call_index]
    request = call.request if request is None else request
    form = has_form(kind, case)
    if request == TILED and not form:
        return "refused"
    consumed = position_before(case, call_index)
    if outputs_for(case, consumed, call.n) == 0:
        return "history only"
    aligned = assume_aligned or (call.out_off % 2 == 0 and (case.nchan == 1 or call.out_stride % 2 == 0))
    if form and request != GENERIC and aligned and consumed % KINDS[kind].start_multiple == 0:
        return "tiled"
    return "refused" if request == TILED else "generic"


def crossings(case):
    """{(index, log2 B, call)}: the calls inside which an index passes B = 2^31 or 2^32 -- two of the call's inputs, or two of its
    outputs, lie on either side of B.  "input": the absolute input index; "output": the absolute output index m; "raster": m down,
    the index on the x up raster that resample_generic_kernel computes (rational alone)."""
    out = set()
    for i, call in enumerate(case.calls):
        a = position_before(case, i)
        b = a + call.n
        ma, mb = -(-a * case.up // case.down), -(-b * case.up // case.down)       # the call's outputs: [ma, mb)
        for log2 in (31, 32):
            B = 2 ** log2
            if a < B <= b - 1:
                out.add(("input", log2, i))
            if ma < B <= mb - 1:
                out.add(("output", log2, i))
            if case.up > 1 and mb - ma >= 2 and ma * case.down < B <= (mb - 1) * case.down:
                out.add(("raster", log2, i))
    return out


# ---- a stream's data -------------------------------------------------------------------------------------------------------------
def stream_input(kind, case, oracle):
    """(raw, xs): the lead and the stream behind it, lead_of(case) + N samples per channel, as stored words, int32 [nchan, lead + N,
    words per sample], and as the complex64 values the kernels filter.  CF32: components uniform in [-1, 1); CF16: the same rounded
    to half (the stored halves are the input, exactly); S32: random wire words (convert_rx)."""
    rng = np.random.default_rng(case.data_seed)
    shape = (case.nchan, lead_of(case) + sum(c.n for c in case.calls))
    if case.fmt == "S32":
        raw = rng.integers(-2 ** 31, 2 ** 31, size=shape + (2,), dtype=np.int64).astype(np.int32)
        return raw, oracle.convert_rx(raw.ravel()).reshape(shape)
    x = rng.uniform(-1, 1, size=shape + (2,)).astype(np.float32)
    if case.fmt == "CF16":
        halves = oracle.f32_to_f16(x)
        raw = np.ascontiguousarray(halves).view(np.uint32).view(np.int32)
        return raw.reshape(shape + (1,)), np.ascontiguousarray(oracle.f16_to_f32(halves)).view(np.complex64).reshape(shape)
    return np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(x).view(np.complex64).reshape(shape)


def plain_reference(kind, oracle, case, h, x, m_first=0):
    """complex64: one pass over x from zero history, its first output at the absolute index m_first (translate: the mixer's phase;
    nothing else of either kind sees it)."""
    if kind == "translate":
        return mix_ref(oracle, h, case.down, x, contract(kind, case), case.num, case.den, m_first)
    return rational_ref(oracle, h, case.up, case.down, x, contract(kind, case)[0])


def reference(kind, oracle, case, h, x):
    """The float32 reference of one channel's stream, x = the lead then the stream (stream_input): the outputs of the stream alone.

    A stream placed at c0 is DEFINED as the same samples behind the lead from zero history, the lead's outputs dropped.  This is the
    definition and no approximation of it: output m reaches hist_of(case) - 1 samples back at the most, and the lead is longer, so
    no output of the stream sees what lay in front of the lead; the filter part sees the position only modulo its period -- `down`
    input samples, which are `up` outputs --, and lead = c0 modulo down keeps it; the translating plan's rotation alone sees the
    absolute output index m, and mix_ref takes that as a Python int: the first output of x has m = (c0 - lead) / down, so that the
    stream's first has the true ceil(c0 / down)."""
    lead = lead_of(case)
    assert (case.c0 - lead) % case.down == 0 and (lead == 0 or lead >= hist_len(case))
    y = plain_reference(kind, oracle, case, h, x, (case.c0 - lead) // case.down)
    return y[n_out_for(lead, case.up, case.down):]


def stored_words(oracle, fmt, ref):
    """The reference as the plan stores it, uint32 [n_out, words per sample]: CF16: one rounding to half; CF32, and S32 in: CF32."""
    ref = np.ascontiguousarray(ref, dtype=np.complex64)
    if fmt == "CF16":
        return np.ascontiguousarray(oracle.f32_to_f16(ref.view(np.float32))).view(np.uint32).reshape(ref.shape + (1,))
    return ref.view(np.uint32).reshape(ref.shape + (2,))
