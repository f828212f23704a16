"""The four plan kinds that change the rate by more than a band plan does, or turn the stream while they do -- frequency-translating
decimators (include/sxfir_translate.h, "translate"), rational resamplers (include/sxfir_rational.h, "rational"),
frequency-translating interpolators (include/sxfir_translate_tx.h, "translate_tx") and tuner banks (include/sxfir_bank.h, "bank": K
translating decimators over one stream) -- as tests/band_cases.py has the six band kinds: a
seeded generator of streams, a predictor of the kernel each call takes, and the float32 reference of a whole stream, from zero
history or PLACED (sxfir_set_history + sxfir_set_position) anywhere in a 64-bit stream.  CPU only: torch is never imported.
tests/test_rate_cases_host.py checks the generator's coverage and the references; tests/test_gpu_rate_sweep.py runs the cases
(tests/test_gpu_bank_sweep.py the bank's).  The calls (Call, their strides and placements) and the sizes' menu are band_cases' own.

One description serves the four kinds: `up` outputs for every `down` inputs (translate and bank: up = 1, down = the ratio;
translate_tx: up = the ratio L, down = 1), so after c inputs ceil(c up / down) outputs exist (rational_cases.n_out_for)."""
import collections
import math

import numpy as np

from band_cases import AUTO, CX_RATIOS, GENERIC, GUARD, TILED, Call, Contract, _layout, _make_call, _sizes, _stride     # noqa: F401
from band_cases import contract as band_contract
from band_cases import keying_threshold                    # noqa: F401  (the TX kind's S32 cases: the median |y|^2 of a reference)
from bank_cases import bank_ref
from gpu_util import random_taps_cx
from mix_cases import mix_ref, step
from mix_tx_cases import back_step, mix_tx_ref
from rational_cases import n_out_for, rational_ref, rational_taps

SWEEP_SEED, SWEEP_COUNT = 0, 36                             # what the GPU sweep runs; tests/test_rate_cases_host.py holds them to the coverage

Kind = collections.namedtuple("Kind", "name tiled_shapes tile start_multiple tiled generic formats banded_in banded_out tx")
# tiled_shapes: every (ntaps, up, down) with a tiled kernel, on CF32.  tile: the inputs per tile of that kernel, by (up, down); the
# first figure serves a shape without one (tile_of).  start_multiple: the tiled kernel takes a call whose stream position is a
# multiple of it (translate_tx: anywhere).  formats: CF32, CF16 and the kind's third -- S32 wire words in (CF32 out) for translate;
# rational refuses S32, CF16 again; translate_tx, a TX kind: CF32 in, convert_tx wire words out under the plan's keying threshold,
# as in band_cases; bank: translate's.  banded_*: what band_cases._make_call asks of a kind (bands on the bank's output side alone: K
# rows per channel, the channelizer's layout).  tx: an interpolator of the translating kind -- the mixer turns the INPUT, by its
# absolute index.
KINDS = collections.OrderedDict((k.name, k) for k in (
    Kind("translate", ((128, 1, 4),), {(1, 4): 2048}, 4, "decim4_mix_kernel", "decim_mix_generic_kernel", ("CF32", "CF16", "S32"), False, False, False),
    Kind("rational", ((128, 4, 5),), {(4, 5): 1280}, 5, "resample45_kernel", "resample_generic_kernel", ("CF32", "CF16", "CF16"), False, False, False),
    Kind("translate_tx", ((128, 4, 1), (256, 8, 1)), {(4, 1): 256, (8, 1): 128}, 1, "interp_mix_pass_kernel", "interp_mix_generic_kernel",
         ("CF32", "CF16", "S32"), False, False, True),
    Kind("bank", ((128, 1, 4),), {(1, 4): 2048}, 4, "decim4_bank_kernel", "decim_bank_generic_kernel", ("CF32", "CF16", "S32"), False, True, False),
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
# translate_tx: the class names keep their meaning for s = num L mod den, but interp_mix_pass_kernel and interp_mix_generic_kernel
# step by t = (den - s) mod den: "one" (s = 1 where L and den are coprime) is the LARGEST t, "max" the smallest above 0.
# where a placed stream starts: 2^40 + k, or so that the named index passes 2^31 / 2^32 INSIDE the case's largest call (translate_tx:
# "output" is the absolute output index L m + r; on a shape with a tiled kernel the largest call that the tiled kernel takes)
PLACES = {"translate": ("far", "input 31", "output 31", "input 32", "output 32"),
          "rational": ("far", "input 31", "output 31", "raster 31", "input 32", "output 32", "raster 32"),
          "translate_tx": ("far", "input 31", "input 32", "output 31", "output 32")}
PLACES["bank"] = PLACES["translate"]
# how the four "seam" cases leave the tiled kernel in mid-stream.  translate_tx has no position rule; its fourth seam is "short": a
# GENERIC call of 1 .. 31 inputs, fewer than the 32-sample history, so that the next history is part old history, part new input
SEAMS = {"translate": ("offset", "out_stride", "generic", "position"), "rational": ("offset", "out_stride", "generic", "position"),
         "translate_tx": ("offset", "out_stride", "generic", "short")}
# the bank's are translate's.  Its "out_stride" seam has a second odd stride to show, the band's: of the seam's two perturbed calls
# (the one that leaves the tiled kernel under AUTO, the one that is refused under a forced TILED) one has an odd out_stride and the
# other an odd band_stride, in turn over the seeds
SEAMS["bank"] = SEAMS["translate"]
# bank: the band count, dealt in turn to the cases of each of the deck's three parts (the tiled shape on CF32, a generic shape on
# CF32, CF16 / S32): every part has eight slots or more, so every count meets the tiled kernel, the generic one and the 16-bit and
# wire formats.  The centres are MIXERS, dealt per band, continuing from case to case: one turn for the cases whose calls the tiled
# kernel takes (the tiled shape on CF32 under the start rule) and one for all others, so that both kernels see every class.  The
# first case of each turn with three bands or more has its last band a TWIN of band 0, taps and centre.
BANK_KS = (1, 2, 3, 4, 5, 8, 15, 16)

Case = collections.namedtuple("Case", "ident ntaps up down num den tap_seed nchan fmt data_seed style how place c0 calls")
# ntaps: all taps (rational, translate_tx: up times the taps per phase).  num, den: the mixer (rational: 0, 0).  how: a seam case's
# perturbation.  place: "start" (c0 = 0) or one of PLACES; c0: the stream position of the first call.
BankCase = collections.namedtuple("BankCase", Case._fields + ("centres", "twin"))
# a bank's case: num = den = 0; centres: K (num, den) pairs; twin: None, or (j, k) -- band k has band j's taps and centre.


def nbands_of(case):
    """The bands on the output side: K of a bank's case, none of any other."""
    return len(case.centres) if isinstance(case, BankCase) else 0


def ratio_of(case):
    """The ratio of a translating plan: `down` of a decimator (up = 1), `up` of an interpolator (down = 1)."""
    return case.up * case.down


def tile_of(kind, case):
    """Inputs of one tile; the kind's first figure for a shape without a tiled kernel."""
    tile = KINDS[kind].tile
    return tile.get((case.up, case.down), next(iter(tile.values())))


def hist_of(case):
    """Samples of the stream a call still needs from before it: ntaps for translate, the taps per phase for rational and
    translate_tx."""
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
    return case.fmt == "CF32" and (case.ntaps, case.up, case.down) in KINDS[kind].tiled_shapes


def contract(kind, case):
    """The numeric contract the plan must report.  translate: the complex-tap decimator's of the shape (sxfir_translate.h: "z[m] has
    the bits of the sxfir_create_complex plan of the same shape").  rational and translate_tx: the x up interpolator's -- a phase's
    taps in two halves when their count is even, else one chain (sxfir_rational.h, sxfir_complex_tx.h)."""
    if kind in ("translate", "bank"):
        return band_contract("decimate_cx", case.ntaps, case.down)
    return Contract((2 if hist_of(case) % 2 == 0 else 1, 1))


def taps_of(kind, case):
    """Random taps without symmetry: complex for the translating kinds, real for rational.  bank: [K, ntaps], band k's from the
    seed tap_seed + k -- a twin's from its sibling's."""
    if kind == "bank":
        seeds = [case.tap_seed + k for k in range(nbands_of(case))]
        if case.twin:
            seeds[case.twin[1]] = seeds[case.twin[0]]
        return np.stack([random_taps_cx(case.ntaps, s) for s in seeds])
    if kind != "rational":
        return random_taps_cx(case.ntaps, case.tap_seed)
    return rational_taps(case.up, case.ntaps // case.up, case.tap_seed)


def make_plan(kind, case, h):
    import sxxcvr_amd
    if kind == "translate":
        return sxxcvr_amd.TranslatingDecimator(h, case.down, case.num, case.den, nchan=case.nchan, fmt=case.fmt)
    if kind == "bank":
        return sxxcvr_amd.TranslatingBank(h, case.down, case.centres, nchan=case.nchan, fmt=case.fmt)
    if kind == "translate_tx":
        return sxxcvr_amd.TranslatingInterpolator(h, case.up, case.num, case.den, nchan=case.nchan, fmt=case.fmt)
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
    """The classes of MIXERS a translating case's (num, den) falls into, from the numbers themselves."""
    return centre_classes(case.num, case.den, ratio_of(case))


def centre_classes(num, den, ratio):
    """s_classes of one (num, den) at a ratio: a bank has one per band."""
    s, g = step(num, den, ratio), math.gcd(ratio, den)
    out = set()
    if den >= 65535 and s == den - g:
        out.add("s = den - gcd, den %d" % den)
    if s == 1:
        out.add("s = 1")
    if s == 0:
        out.add("s = 0")
    if num < 0:
        out.add("negative num")
    if num > den:
        out.add("num above den")
    return out


def _first_position(rng, K, up, down, calls, r, place, period=None, among=None):
    """c0 = r modulo `period` (`down` unless given) for a place of PLACES.  An index passes B = 2^31 / 2^32 inside the largest call
    (of those in `among`, if given), [c0 + p, c0 + p + n): "input": c0 + p < B <= c0 + p + n - 1.  "output": outputs B - 1 and B are
    the call's; output m is made when its newest input, floor(m down / up), arrives.  "raster": as "output" for the first m with
    m down >= B, the x up raster's index of output m."""
    period = down if period is None else period
    if place == "far":
        mid = 2 ** 40 + int(rng.integers(0, 1000))
    else:
        index, log2 = place.split()
        B = 2 ** int(log2)
        j = max(range(len(calls)) if among is None else among, key=lambda i: calls[i].n)
        p, n = sum(c.n for c in calls[:j]), calls[j].n
        if index == "input":
            lo, hi = B - p - (n - 1), B - p - 1
        else:
            m = B if index == "output" else -(-B // down)
            lo, hi = m * down // up - p - (n - 1), (m - 1) * down // up - p
        mid = (lo + hi) // 2
        assert hi - lo >= 2 * period, (place, n)            # (translate_tx may move c0 one period up from the middle, _one_case)
    return mid - (mid - r) % period


def _one_case(rng, kind, index, slot, pair, mixer, place, bank=None):
    """`pair`: what is dealt in turn to a case that draws its shape -- a rational pair; translate_tx: the parity of the taps per
    phase, so that the contracts (2, 1) and (1, 1) both occur.  `bank`: (the bank's mixers, one per band; whether the last band is
    band 0's twin; whether the "out_stride" seam's refused call, not its AUTO call, has the odd out_stride)."""
    K = KINDS[kind]
    shape_tiled, fmt, style, how, keep_rule, which = slot
    num = den = 0
    nbands, centres = 0, ()
    if kind in ("translate", "bank"):
        ntaps, up, down = K.tiled_shapes[which]
        while not shape_tiled and (ntaps, up, down) in K.tiled_shapes:
            ntaps, down = int(rng.integers(4, 301)), int(rng.choice(CX_RATIOS))         # any count
        if kind == "translate":
            cls, den, num = mixer
            num = mixer_num(cls, den, num, down)
        else:
            mixers, twin, swap = bank
            centres = tuple((mixer_num(cls, d, n, down), d) for cls, d, n in mixers)
            centres += (centres[0],) if twin else ()
            nbands = len(centres)
    elif shape_tiled:
        ntaps, up, down = K.tiled_shapes[which]
    elif K.tx:
        down = 1
        while True:
            up = int(rng.choice(CX_RATIOS))
            most = 300 // up                                # whole phases, 300 taps at the most (sxfir_translate_tx.h: "ntaps % ratio")
            per_phase = int(rng.integers(1, most + 1))
            if per_phase % 2 != pair:
                per_phase += 1 if per_phase < most else -1
            if (up * per_phase, up, down) not in K.tiled_shapes:
                break
        ntaps = up * per_phase
    else:
        up, down = pair
        while True:
            per_phase = 4 if max(up, down) > 64 else int(rng.integers(1, 41))
            if (up * per_phase, up, down) not in K.tiled_shapes:
                break
        ntaps = up * per_phase
    if K.tx:
        cls, den, num = mixer
        num = mixer_num(cls, den, num, up)
    form = shape_tiled and fmt == "CF32"
    nchan = 3 if how == "out_stride" else int(rng.choice([1, 1, 2, 3]))        # (an odd out_stride leaves the tiled kernel with nchan > 1 only)
    T, hist, q = K.tile.get((up, down), next(iter(K.tile.values()))), ntaps // up, K.start_multiple
    # the stream's first position modulo `down`: what the calls' output counts depend on, and for a plan with a tiled kernel
    # (down = q) whether the start rule holds.  translate_tx has neither: on a shape with a tiled kernel the PARITY of c0 is dealt
    # (keep_rule: even; the header promises the tiled kernel "at any stream position")
    period = down
    if K.tx:
        period = 2 if form else 1
        r = 0 if place == "start" or keep_rule or not form else 1
    elif place == "start" or (form and keep_rule):
        r = 0
    elif form:
        r = int(rng.integers(1, q))
    else:
        r = int(rng.integers(0, down))
    budget = 6 * T
    calls, consumed = [], 0

    def add(n, request, perturb):
        nonlocal consumed, budget
        nesting = "bands inside channels"
        if nbands:                                          # (a draw of the bank's alone: the other kinds' streams stay as they were)
            nesting = str(rng.choice(["bands inside channels", "channels inside bands"]))
        calls.append(_make_call(rng, K, None, nchan, None, n, request, perturb, nesting, n_out=n_out_for(n, up, down, r + consumed),
                                bands=max(nbands, 1)))
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
        if how == "short":
            b = int(rng.integers(1, hist))                  # fewer inputs than the history holds: the next one is part old, part new
        # (bank, "out_stride": the odd stride of the call that leaves the tiled kernel and of the refused one -- SEAMS)
        hows = (how, how) if not (nbands and how == "out_stride") else ("band_stride", how) if swap else (how, "band_stride")
        add(a, int(rng.choice([AUTO, TILED])), None)
        add(b, GENERIC if how in ("generic", "short") else AUTO, hows[0] if how in ("offset", "out_stride") else None)
        add(int(rng.choice([T, T + q, 2 * T])), int(rng.choice([AUTO, TILED])), None)
        if how in ("offset", "out_stride"):
            add(q * int(rng.integers(1, 60)), TILED, hows[1])              # the same placement under a forced TILED: refused in mid-stream
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
    if place == "start":
        c0 = 0
    elif not K.tx:
        c0 = _first_position(rng, K, up, down, calls, r, place)
    else:
        # the mark is passed inside a call that the tiled kernel takes, where the plan has one; and the phase of the lead's first
        # sample, (c0 - lead) t mod den, is not 0 wherever t is not: the far stream's bits are not the near one's
        tiled = [i for i, c in enumerate(calls)
                 if c.n > 0 and c.request != GENERIC and c.out_off % 2 == 0 and (nchan == 1 or c.out_stride % 2 == 0)]
        assert tiled or not form
        c0 = _first_position(rng, K, up, down, calls, r, place, period, tiled if form else None)
        t, lead = back_step(num, den, up), (hist + 1) & ~1
        if t and (c0 - lead) * t % den == 0:
            c0 += period
        assert t == 0 or (c0 - lead) * t % den != 0, (num, den, up, c0)
    shape = "%dx%d" % (ntaps, up * down) if kind != "rational" else "%dx%d:%d" % (ntaps, up, down)
    ident = "%02d-%s-%s-%dch-%s" % (index, shape, fmt, nchan, style) + ("" if place == "start" else "-" + place.replace(" ", ""))
    case = Case(ident, ntaps, up, down, num, den, 100 + index, nchan, fmt, 7000 + index, style, how, place, c0, tuple(calls))
    if kind != "bank":
        return case
    return BankCase(*case._replace(ident=ident.replace("-%s-" % fmt, "-%s-K%d-" % (fmt, nbands), 1)), centres, (0, nbands - 1) if twin else None)


def cases(kind, seed, n):
    """n seeded cases of one kind, as plain tuples.  band_cases' deck: of 36 slots, the tiled shape on CF32 in 11 -- seven keep to
    the tiled kernel's terms in every call ("clean"), four leave it and come back in mid-stream ("seam", one by each of SEAMS) --, a
    generic shape on CF32 in 11 and CF16 and the kind's third format in turn in 14, on the tiled and a generic shape in turn
    ("mixed": every call's size, kernel request and placement drawn).  A third of the slots are PLACED streams, four of each eleven
    and of the fourteen; of the four on the tiled kernel's shape two keep its start rule and two break it.  What must occur at least
    once is dealt in turn over the cases, not drawn: the places of PLACES, the rational pairs, the mixers.

    translate_tx has two tiled shapes, dealt in turn over the slots (each is in clean, seam and placed cases), and two turns of its
    own, because only 11 of the 36 cases can reach the tiled kernel: the mixers are dealt to those 11 and to the other 25 apart --
    the first 11 of MIXERS hold both "max" rows and "one" on den 65535 and four dens below 8, the 25 see all of MIXERS --,
    and the four placed cases among the 11 take the four crossings of PLACES, one each (the other eight every place in turn).  Of
    those four two start at an even c0 and two at an odd one.

    bank is translate's deck with K and K centres on top (BANK_KS), and the output's nesting drawn per call."""
    K = KINDS[kind]
    rng = np.random.default_rng([seed, 100 + list(KINDS).index(kind)])
    deck = []
    for i in range(n):
        slot = i % 36
        placed = slot in (1, 4, 5, 7, 12, 15, 18, 21, 23, 26, 29, 32)      # (1, 5 keep the start rule; 4, 7 -- no seam case -- break it)
        which = (slot % 2 if slot < 22 else (slot // 2) % 2) % len(K.tiled_shapes)          # the tiled shape, where the slot has one
        if slot < 11:
            seam = (2, 5, 8, 10).index(slot) if slot in (2, 5, 8, 10) else None
            deck.append(((True, "CF32", "clean" if seam is None else "seam", None if seam is None else SEAMS[kind][seam], slot in (1, 5), which), placed))
        elif slot < 22:
            deck.append(((False, "CF32", "mixed", None, False, which), placed))
        else:
            deck.append(((slot % 2 == 0, K.formats[1 + (slot // 2) % 2], "mixed", None, False, which), placed))
    order = rng.permutation(n)
    out, n_generic, n_placed = [], 0, 0
    turn = collections.Counter()
    for i in range(n):
        slot, placed = deck[int(order[i])]
        if K.tx:
            form = "form" if slot[0] and slot[1] == "CF32" else "other"
            menu = PLACES[kind][1:] if form == "form" else PLACES[kind]        # (the four crossings; all five places)
            place = menu[turn["placed " + form] % len(menu)] if placed else "start"
            out.append(_one_case(rng, kind, i, slot, n_generic % 2, MIXERS[turn[form] % len(MIXERS)], place))
            turn[form] += 1
            turn["placed " + form] += placed
        elif kind == "bank":
            part = "form" if slot[0] and slot[1] == "CF32" else "generic" if slot[1] == "CF32" else "other"
            side = "tiled" if part == "form" and (not placed or slot[4]) else "not tiled"        # (the mixers' turn: BANK_KS)
            nb = BANK_KS[turn[part] % len(BANK_KS)]
            twin = nb >= 3 and not turn["twin " + side]
            mixers = tuple(MIXERS[(turn[side] + k) % len(MIXERS)] for k in range(nb - twin))
            place = PLACES[kind][n_placed % len(PLACES[kind])] if placed else "start"
            out.append(_one_case(rng, kind, i, slot, None, None, place, (mixers, twin, (seed + i // 36) % 2 == 1)))
            turn[part] += 1
            turn[side] += nb - twin
            turn["twin " + side] += twin
        else:
            place = PLACES[kind][n_placed % len(PLACES[kind])] if placed else "start"
            out.append(_one_case(rng, kind, i, slot, RATIONAL_PAIRS[n_generic % len(RATIONAL_PAIRS)], MIXERS[i % len(MIXERS)], place))
        n_generic += not slot[0]
        n_placed += placed
    assert all(sum(c.n for c in case.calls) <= 6 * tile_of(kind, case) for case in out)
    return out


# ---- the predictor ---------------------------------------------------------------------------------------------------------------
def expected_kernel(kind, case, call_index, request=None, assume_aligned=False):
    """"tiled" | "generic" | "history only" | "refused" for call `call_index` of the stream, every call before it having been made
    (a refused one again under AUTO).  The headers' rules: the tiled kernel runs when the shape and format have one and the request is
    not GENERIC, the output is 16-byte aligned, out_stride is even with nchan > 1 and the stream position is a multiple of 4
    (translate; bank, which asks for an even band_stride as well) or 5 (rational) -- translate_tx: any position, so its refused rule is the output's alignment and the even out_stride
    alone; under a forced TILED "refused" replaces "generic" -- sxfir_set_kernel's own refusal where the plan
    has no tiled kernel at all.  A call that completes no output only carries its samples into the history, whatever was asked for
    (translate_tx: every input makes L outputs, so this is the call with n = 0 alone, which does nothing).
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
    aligned = assume_aligned or (call.out_off % 2 == 0 and (case.nchan == 1 or call.out_stride % 2 == 0)
                                 and (not KINDS[kind].banded_out or call.band_stride % 2 == 0))
    if form and request != GENERIC and aligned and consumed % KINDS[kind].start_multiple == 0:
        return "tiled"
    return "refused" if request == TILED else "generic"


def crossings(case):
    """{(index, log2 B, call)}: the calls inside which an index passes B = 2^31 or 2^32 -- two of the call's inputs, or two of its
    outputs, lie on either side of B.  "input": the absolute input index; "output": the absolute output index m (translate_tx:
    L m + r, the call's outputs are [L a, L b)); "raster": m down, the index on the x up raster that resample_generic_kernel
    computes (rational alone)."""
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
            if case.up > 1 and case.down > 1 and mb - ma >= 2 and ma * case.down < B <= (mb - 1) * case.down:
                out.add(("raster", log2, i))
    return out


# ---- a stream's data -------------------------------------------------------------------------------------------------------------
def tx_scale(h):
    """The power of two that keeps every output component of translate_tx inside the wire words' range for input components below
    1.0: sum|h| max|x| < 1 with max|x| < sqrt 2 -- an output is at most sum|h| max|xr|, and the rotation leaves |xr| <= (1 + 2^-20)
    |x| (mix_tx_cases.bound), which the 1 % of margin covers."""
    bound = float(np.abs(np.asarray(h).astype(np.complex128)).sum()) * math.sqrt(2.0) * 1.01
    k = 0
    while 2.0 ** k <= bound:
        k += 1
    return np.float32(2.0 ** -k)


def stream_input(kind, case, oracle):
    """(raw, xs): the lead and the stream behind it, lead_of(case) + N samples per channel, as stored words, int32 [nchan, lead + N,
    words per sample], and as the complex64 values the kernels filter.  CF32: components uniform in [-1, 1); CF16: the same rounded
    to half (the stored halves are the input, exactly); S32: random wire words (convert_rx) -- out of translate_tx, a TX kind: CF32
    input scaled by tx_scale."""
    rng = np.random.default_rng(case.data_seed)
    shape = (case.nchan, lead_of(case) + sum(c.n for c in case.calls))
    if case.fmt == "S32" and not KINDS[kind].tx:
        raw = rng.integers(-2 ** 31, 2 ** 31, size=shape + (2,), dtype=np.int64).astype(np.int32)
        return raw, oracle.convert_rx(raw.ravel()).reshape(shape)
    x = rng.uniform(-1, 1, size=shape + (2,)).astype(np.float32)
    if case.fmt == "S32":
        x = x * tx_scale(taps_of(kind, case))               # exact: a power of two
    if case.fmt == "CF16":
        halves = oracle.f32_to_f16(x)
        raw = np.ascontiguousarray(halves).view(np.uint32).view(np.int32)
        return raw.reshape(shape + (1,)), np.ascontiguousarray(oracle.f16_to_f32(halves)).view(np.complex64).reshape(shape)
    return np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(x).view(np.complex64).reshape(shape)


def plain_reference(kind, oracle, case, h, x, m_first=0):
    """complex64: one pass over x from zero history, its first output at the absolute index m_first (translate: the mixer's phase;
    translate_tx: the absolute index of the first INPUT, the mixer's phase again; nothing else of any kind sees it)."""
    if kind == "translate":
        return mix_ref(oracle, h, case.down, x, contract(kind, case), case.num, case.den, m_first)
    if kind == "bank":                                      # [K, n_out]: band k is the translating decimator of its taps and centre
        return bank_ref(oracle, h, case.down, x, contract(kind, case), case.centres, m_first)
    if kind == "translate_tx":
        return mix_tx_ref(oracle, h, case.up, x, contract(kind, case)[0], case.num, case.den, m_first)
    return rational_ref(oracle, h, case.up, case.down, x, contract(kind, case)[0])


def reference(kind, oracle, case, h, x):
    """The float32 reference of one channel's stream, x = the lead then the stream (stream_input): the outputs of the stream alone.

    A stream placed at c0 is DEFINED as the same samples behind the lead from zero history, the lead's outputs dropped.  This is the
    definition and no approximation of it: output m reaches hist_of(case) - 1 samples back at the most, and the lead is longer, so
    no output of the stream sees what lay in front of the lead; the filter part sees the position only modulo its period -- `down`
    input samples, which are `up` outputs --, and lead = c0 modulo down keeps it; the translating plan's rotation alone sees the
    absolute output index m, and mix_ref takes that as a Python int: the first output of x has m = (c0 - lead) / down, so that the
    stream's first has the true ceil(c0 / down).  A bank is that per band ([K, n_out]: bank_cases.bank_ref).

    translate_tx (mix_tx_cases.mix_tx_ref over the lead and the stream with m_first = c0 - lead, the lead's L lead outputs dropped):
    the same holds with less to say.  The filter -- the complex-tap interpolator over the rotated input -- sees the position not at
    all: every input makes its L outputs, whatever its index.  The rotation alone sees the absolute INPUT index m, and takes it as
    a Python int: table_index reduces m_first modulo den in integers of any size before a numpy array is made.  What the test hands
    to sxfir_set_history is the lead RAW, as the header says the history is kept; the reference rotates the lead's samples by their
    own indices c0 - lead .. c0 - 1."""
    lead = lead_of(case)
    assert (case.c0 - lead) % case.down == 0 and (lead == 0 or lead >= hist_len(case))
    y = plain_reference(kind, oracle, case, h, x, (case.c0 - lead) // case.down)
    return y[..., n_out_for(lead, case.up, case.down):]


def stored_words(oracle, fmt, ref, thr2=None):
    """The reference as the plan stores it, uint32 [n_out, words per sample]: CF16: one rounding to half; CF32, and S32 in: CF32; S32
    out of translate_tx (thr2 given): convert_tx of the CF32 result under the keying threshold thr2."""
    ref = np.ascontiguousarray(ref, dtype=np.complex64)
    if fmt == "CF16":
        return np.ascontiguousarray(oracle.f32_to_f16(ref.view(np.float32))).view(np.uint32).reshape(ref.shape + (1,))
    if fmt == "S32" and thr2 is not None:
        return oracle.convert_tx(ref.ravel(), thr2).view(np.uint32).reshape(ref.shape + (2,))
    return ref.view(np.uint32).reshape(ref.shape + (2,))
