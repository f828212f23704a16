"""The six band-plan kinds as one table, a seeded generator of streams over them, a predictor of the kernel each call takes, the
float32 reference of a whole stream and the fp64 definition of each kind.  CPU only: nothing here needs a GPU, and torch is never
imported (sxxcvr_amd only where a plan is made).  tests/test_band_cases_host.py checks the generator's coverage and the references
here; tests/test_gpu_band_sweep.py runs the cases.

The kinds (include/sxfir_complex.h, sxfir_complex_tx.h, sxfir_channelizer.h, sxfir_channelizer_os.h, sxfir_synthesizer.h,
sxfir_synthesizer_os.h): "decimate_cx", "interpolate_cx", "channelize", "channelize_os", "synthesize", "synthesize_os"."""
import collections

import numpy as np

from gpu_util import chan_os_ref, chan_ref, cx_decim_ref, cx_interp_ref, random_taps, random_taps_cx, syn_os_ref, syn_ref

AUTO, TILED, GENERIC = 0, 1, 2                              # SXFIR_KERNEL_* (include/sxfir.h)
BANDS = 4
GUARD = 4                                                   # samples of fill in front of every output buffer (16 bytes at the least)
SWEEP_SEED, SWEEP_COUNT = 0, 36                             # what the GPU sweep runs; tests/test_band_cases_host.py holds them to the coverage

Kind = collections.namedtuple("Kind", "name decim complex_taps banded_in banded_out ratio tiled_shapes tile start_multiple tiled generic")
# ratio: None where the case draws it.  tiled_shapes: (ntaps, ratio) with a tiled kernel, on CF32.  tile: inputs (per band) of one
# tile of that kernel, by ratio.  start_multiple: the tiled kernel takes a call whose stream position is a multiple of it (the
# decimator kinds: the call starts on an output boundary; the oversampled channelizer: on one of EVEN index; the TX kinds: anywhere).
# Formats: every kind takes CF32, CF16 (halves in and out) and S32 -- wire words IN for the RX kinds (convert_rx, CF32 out), wire
# words OUT under the plan's keying threshold for the TX kinds (CF32 in, convert_tx of the CF32 result).
KINDS = collections.OrderedDict((k.name, k) for k in (
    Kind("decimate_cx", True, True, False, False, None, ((128, 4),), {4: 2048}, 4, "decim4_cx_kernel", "decim_cx_generic_kernel"),
    Kind("interpolate_cx", False, True, False, False, None, ((128, 4), (256, 8)), {4: 256, 8: 128}, 1, "interp_cx_pass_kernel", "interp_cx_generic_kernel"),
    Kind("channelize", True, False, False, True, 4, ((128, 4),), {4: 2048}, 4, "chan4_kernel", "chan_generic_kernel"),
    Kind("channelize_os", True, False, False, True, 2, ((128, 2),), {2: 2048}, 4, "chan4x2_kernel", "chan4x2_generic_kernel"),
    Kind("synthesize", False, False, True, False, 4, ((128, 4),), {4: 256}, 1, "synthesis4_kernel", "synthesis_generic_kernel"),
    Kind("synthesize_os", False, False, True, False, 2, ((128, 2),), {2: 512}, 1, "synthesis4x2_kernel", "synthesis_os_generic_kernel"),
))
CX_RATIOS = (2, 3, 4, 5, 8, 16)

Call = collections.namedtuple("Call", "n request out_off out_stride skew in_stride band_stride nesting")
# n: inputs (per band).  out_off, skew: samples between the buffer's aligned start and the call's first output / input.  Strides in
# samples of the side's format; band_stride is the banded side's (a channelizer's output, a synthesizer's input; 0 for the complex
# kinds).  nesting: "bands inside channels" or "channels inside bands" on the banded side.
Case = collections.namedtuple("Case", "ident ntaps ratio tap_seed nchan fmt data_seed style calls")


class Contract(tuple):
    """(jsplit, cw) with rot beside it, as sxxcvr_amd.resampler.Contract: what the references of gpu_util take."""
    rot = 0


def tile_of(kind, ratio):
    """Inputs (per band) of one tile; the x4 figure for a complex interpolator of a ratio without a tiled kernel."""
    return KINDS[kind].tile.get(ratio, 256)


def hist_of(kind, ntaps, ratio):
    """Samples (per band) of the stream a call still needs from before it: ntaps for the RX kinds, the taps per phase for the TX
    kinds (ntaps / 4 for the synthesizer, ntaps / 2 for the oversampled one)."""
    K = KINDS[kind]
    return ntaps if K.decim else ntaps // ratio


def has_form(kind, case):
    return case.fmt == "CF32" and (case.ntaps, case.ratio) in KINDS[kind].tiled_shapes


def contract(kind, ntaps, ratio):
    """The numeric contract the plan must report.  Channelizers: one chain per branch sum (sxfir_channelizer.h).  Complex
    decimator: the real-tap plan's of the shape (two row halves and column groups of 4 when the rows are whole, even
    in number and the ratio / 4 column groups a power of two; else one chain over all taps).  TX kinds: a phase's taps in two halves
    when their count is even."""
    K = KINDS[kind]
    if K.banded_out:
        return Contract((1, 1))
    if not K.decim:
        return Contract((2 if (ntaps // ratio) % 2 == 0 else 1, 1))
    ncol4 = ratio // 4
    pow2 = ratio % 4 == 0 and ncol4 & (ncol4 - 1) == 0 and ncol4 <= 32
    if ntaps % ratio == 0 and pow2 and (ntaps // ratio) % 2 == 0:
        return Contract((2, 4))
    return Contract((1, ratio))


def taps_of(kind, ntaps, seed):
    """Random taps without symmetry: complex for the complex kinds."""
    return random_taps_cx(ntaps, seed) if KINDS[kind].complex_taps else random_taps(ntaps, seed)


def make_plan(kind, h, ratio, nchan=1, fmt="CF32"):
    import sxxcvr_amd
    from sxxcvr_amd.resampler import DECIMATE
    if kind == "decimate_cx":
        return sxxcvr_amd.Resampler(DECIMATE, np.asarray(h, dtype=np.complex64), ratio, nchan=nchan, fmt=fmt)
    if kind == "interpolate_cx":
        return sxxcvr_amd.ComplexInterpolator(h, ratio, nchan=nchan, fmt=fmt)
    cls = sxxcvr_amd.Channelizer if KINDS[kind].banded_out else sxxcvr_amd.Synthesizer
    return cls(h, nchan=nchan, fmt=fmt, oversample=BANDS // ratio)


def outputs_for(kind, ratio, consumed, n):
    """Outputs (per band) of a call of n inputs at stream position `consumed`."""
    if not KINDS[kind].decim:
        return n * ratio
    return (consumed + n + ratio - 1) // ratio - (consumed + ratio - 1) // ratio


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _stride(rng, need, mode):
    """A stride of at least `need` samples: "tight", or padded to an even or to an odd figure."""
    if mode == "tight":
        return need
    s = need + int(rng.choice([2, 6, 26]))
    return s + 1 if (s % 2 == 1) != (mode == "odd") else s


def _layout(rng, nchan, n, banded, chan_mode, band_mode, nesting, bands=BANDS):
    """(channel stride, band stride) of one side of a call with n samples per row and `bands` bands."""
    if not banded:
        return _stride(rng, n, chan_mode), 0
    if nchan == 1 or nesting == "bands inside channels":
        band = _stride(rng, n, band_mode)
        return _stride(rng, (bands - 1) * band + n, chan_mode), band
    chan = _stride(rng, n, chan_mode)
    return chan, _stride(rng, (nchan - 1) * chan + n, band_mode)


def _make_call(rng, kind, ratio, nchan, consumed, n, request, perturb, nesting, n_out=None, bands=BANDS):
    """One call of n inputs.  perturb: None (an aligned output, even strides on the output side), "offset" (the output starts one
    sample in), "out_stride" / "band_stride" (that stride odd) or "any" (every placement drawn).  The input side is always drawn: a
    view `skew` samples into its buffer, strides padded by nothing, to an even or to an odd figure -- no header asks more of the
    input than one sample's alignment (sxfir_channelizer.hip.h / sxfir_synthesizer.hip.h: "buffers must be aligned to one complex
    sample"; sxfir_synthesizer.h: "an odd in_stride or band_stride stays with the tiled kernel").  n_out: the call's outputs where
    the kind is not one of KINDS (tests/rate_cases.py: `kind` is then a Kind of its own; its "bank" has `bands` bands on the output
    side, tests/arb_sweep_cases.py's kind none)."""
    K = KINDS[kind] if n_out is None else kind
    n_out = outputs_for(kind, ratio, consumed, n) if n_out is None else n_out
    modes = ("tight", "even", "odd")
    out_off = 0
    chan_mode, band_mode = "even", "even"
    if perturb == "offset":
        out_off = 1
    elif perturb == "out_stride":
        chan_mode = "odd"
    elif perturb == "band_stride":
        band_mode = "odd"
    elif perturb == "any":
        out_off = int(rng.choice([0, 0, 1]))
        chan_mode, band_mode = str(rng.choice(modes)), str(rng.choice(modes))
    out_stride, out_band = _layout(rng, nchan, n_out, K.banded_out, chan_mode, band_mode, nesting, bands)
    skew = int(rng.choice([0, 0, 1, 3, 6]))
    in_stride, in_band = _layout(rng, nchan, n, K.banded_in, str(rng.choice(modes)), str(rng.choice(modes)), nesting, bands)
    return Call(n, request, out_off, out_stride, skew, in_stride, out_band if K.banded_out else in_band, nesting)


def _sizes(rng, T, hist):
    """The menu of call sizes: the smallest at which the seams exist."""
    return [0, 1, 2, 3, max(hist - 1, 0), T - 1, T, T + 1, int(rng.integers(2, 6)) * T + int(rng.integers(1, T))]


def _one_case(rng, kind, index, shape_tiled, fmt, style):
    K = KINDS[kind]
    if shape_tiled:
        ntaps, ratio = K.tiled_shapes[int(rng.integers(len(K.tiled_shapes)))]
    else:
        while True:
            ratio = K.ratio or int(rng.choice(CX_RATIOS))
            if kind == "decimate_cx":
                ntaps = int(rng.integers(4, 301))                           # any count
            elif kind == "interpolate_cx":
                ntaps = ratio * int(rng.integers(1, 300 // ratio + 1))      # whole phases (sxfir_complex_tx.h: "ntaps must be a multiple of ratio")
            else:
                ntaps = BANDS * int(rng.integers(1, 76))                    # ntaps % nbands == 0 (sxfir_channelizer.h, sxfir_synthesizer.h)
            if (ntaps, ratio) not in K.tiled_shapes:
                break
    nchan = int(rng.choice([1, 1, 2, 3]))
    T, hist = tile_of(kind, ratio), hist_of(kind, ntaps, ratio)
    budget = 6 * T
    q = 4 if K.decim else 1                                 # sizes that keep an RX stream on the tiled kernels' positions
    calls, consumed = [], 0

    def add(n, request, perturb):
        nonlocal consumed, budget
        nesting = str(rng.choice(["bands inside channels", "channels inside bands"]))
        calls.append(_make_call(rng, kind, ratio, nchan, consumed, n, request, perturb, nesting))
        consumed += n
        budget -= n

    def odd_stride_perturbations():
        p = ["offset", "generic"]
        if nchan > 1:
            p.append("out_stride")
        if K.banded_out:
            p.append("band_stride")
        if K.decim:
            p.append("position")
        return p

    if style == "clean":
        # every call on the tiled kernel's terms (where the plan has one): aligned, even strides, the position rule kept
        sizes = [T, int(rng.integers(2, 4)) * T + q * int(rng.integers(1, T // q)), q * max((hist - 1) // q, 1), T + q, q, 0, T - q]
        add(sizes[int(rng.integers(0, 2))], int(rng.choice([AUTO, TILED])), None)
        for _ in range(int(rng.integers(0, 5))):
            n = sizes[int(rng.integers(len(sizes)))]
            if n <= budget:
                add(n, int(rng.choice([AUTO, AUTO, TILED])), None)
    elif style == "seam":
        # tiled, generic, tiled in the middle of one stream: the history goes from a tiled kernel to history_kernel /
        # synthesis_history_kernel and back
        how = str(rng.choice(odd_stride_perturbations()))
        a = T + q * int(rng.integers(0, T // q))
        b = q * int(rng.integers(1, (T + 40) // q))
        if how == "position":
            # the first call ends off the tiled kernel's positions, the second brings the stream back onto them
            off = 2 if kind == "channelize_os" else int(rng.choice([1, 2, 3]))
            a, b = a + off, b + 4 - off
        add(a, int(rng.choice([AUTO, TILED])), None)
        add(b, GENERIC if how == "generic" else AUTO, how if how in ("offset", "out_stride", "band_stride") else None)
        add(int(rng.choice([T, T + q, 2 * T])), int(rng.choice([AUTO, TILED])), None)
        menu = _sizes(rng, T, hist)
        for _ in range(int(rng.integers(0, 3))):
            n = menu[int(rng.integers(len(menu)))]
            if n <= budget:
                add(n, int(rng.choice([AUTO, AUTO, GENERIC, TILED])), "any")
    else:
        menu = _sizes(rng, T, hist)
        for _ in range(int(rng.integers(1, 6))):
            n = menu[int(rng.integers(len(menu)))]
            if n > budget:
                n = menu[int(rng.integers(0, 5))]
            if n <= budget:
                add(n, int(rng.choice([AUTO, AUTO, GENERIC, TILED])), "any")
        if consumed == 0:
            add(T + 1, AUTO, "any")
    ident = "%02d-%dx%d-%s-%dch-%s" % (index, ntaps, ratio, fmt, nchan, style)
    return Case(ident, ntaps, ratio, 100 + index, nchan, fmt, 7000 + index, style, tuple(calls))


def cases(kind, seed, n):
    """n seeded cases of one kind, as plain tuples.  Shape and format come from a shuffled deck, so that their shares are what they
    are meant to be at any n: the tiled shape in half the cases, CF32 in 22 of 36, CF16 and S32 in turn in the rest; of eleven cases
    the tiled kernel can take (tiled shape on CF32) seven keep to its terms in every call ("clean") and four leave it and come back
    in mid-stream ("seam"); everything else draws every call's size, kernel request and placement freely ("mixed")."""
    K = KINDS[kind]
    rng = np.random.default_rng([seed, list(KINDS).index(kind)])
    deck = []
    for i in range(n):
        slot = i % 36
        if slot < 11:
            deck.append((True, "CF32", "seam" if slot in (2, 5, 8, 10) else "clean"))
        elif slot < 22:
            deck.append((False, "CF32", "mixed"))
        else:
            deck.append((slot % 2 == 0, "CF16" if (slot // 2) % 2 == 0 else "S32", "mixed"))
    order = rng.permutation(n)
    out = [_one_case(rng, kind, i, *deck[int(order[i])]) for i in range(n)]
    assert all(sum(c.n for c in case.calls) <= 6 * tile_of(K.name, case.ratio) for case in out)
    return out


# ---- the predictor ---------------------------------------------------------------------------------------------------------------
def position_before(case, call_index):
    return sum(c.n for c in case.calls[:call_index])


def expected_kernel(kind, case, call_index, request=None, assume_aligned=False):
    """"tiled" | "generic" | "history only" | "refused" for call `call_index` of the stream, every call before it having been made
    (a refused one again under AUTO).  The headers' rules: the tiled kernel runs when the shape and format have one and the request is
    not GENERIC, the output is 16-byte aligned, out_stride is even with nchan > 1, a channelizer's band_stride is even and the kind's
    position rule holds; under a forced TILED "refused" replaces "generic" -- sxfir_set_kernel's own refusal where the plan has no
    tiled kernel at all.  A call that completes no output only carries its samples into the history, whatever was asked for.
    `request`: another request than the call's own (AUTO: the call repeated after a refusal); `assume_aligned`: what
    sxfir_launch_geometry answers, which takes the output's placement for good."""
    K = KINDS[kind]
    call = case.calls[call_index]
    request = call.request if request is None else request
    form = has_form(kind, case)
    if request == TILED and not form:
        return "refused"
    consumed = position_before(case, call_index)
    if outputs_for(kind, case.ratio, consumed, call.n) == 0:
        return "history only"
    aligned = assume_aligned or (call.out_off % 2 == 0 and (case.nchan == 1 or call.out_stride % 2 == 0)
                                 and (not K.banded_out or call.band_stride % 2 == 0))
    if form and request != GENERIC and aligned and consumed % K.start_multiple == 0:
        return "tiled"
    return "refused" if request == TILED else "generic"


# ---- a stream's data -------------------------------------------------------------------------------------------------------------
def tx_scale(kind, h, ratio):
    """The power of two that keeps every output component of a TX kind below 1.0 for input components below 1.0: a component of
    the output is at most the largest phase's sum of |tap| (both parts, for complex taps) times the components added into one
    input of the filter (the synthesizers' butterflies add four)."""
    K = KINDS[kind]
    assert not K.decim
    h = np.asarray(h).astype(np.complex128)
    bound = max(float((np.abs(h[r::ratio].real) + np.abs(h[r::ratio].imag)).sum()) for r in range(ratio))
    bound *= BANDS if K.banded_in else 1
    k = 0
    while 2.0 ** k <= bound:
        k += 1
    return np.float32(2.0 ** -k)


def stream_input(kind, case, oracle):
    """(raw, xs): the stream's input as stored words, int32 [nchan, (4,) N, words per sample], and as the complex64 values the
    kernels filter, [nchan, (4,) N].  CF32: components uniform in [-1, 1); CF16: the same rounded to half (the stored halves are
    the input, exactly); S32 into an RX kind: random wire words (convert_rx); S32 out of a TX kind: CF32 input scaled by tx_scale."""
    K = KINDS[kind]
    rng = np.random.default_rng(case.data_seed)
    N = sum(c.n for c in case.calls)
    shape = (case.nchan, BANDS, N) if K.banded_in else (case.nchan, N)
    if case.fmt == "S32" and K.decim:
        raw = rng.integers(-2 ** 31, 2 ** 31, size=shape + (2,), dtype=np.int64).astype(np.int32)
        xs = oracle.convert_rx(raw.ravel()).reshape(shape)
        return raw, xs
    x = rng.uniform(-1, 1, size=shape + (2,)).astype(np.float32)
    if case.fmt == "S32":
        x = x * tx_scale(kind, taps_of(kind, case.ntaps, case.tap_seed), case.ratio)          # exact: a power of two
    if case.fmt == "CF16":
        halves = oracle.f32_to_f16(x)
        raw = np.ascontiguousarray(halves).view(np.uint32).view(np.int32)
        xs = np.ascontiguousarray(oracle.f16_to_f32(halves)).view(np.complex64).reshape(shape)
        return raw.reshape(shape + (1,)), xs
    return np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(x).view(np.complex64).reshape(shape)


def reference(kind, oracle, h, ratio, x):
    """The float32 reference of one channel's whole stream from zero history: [n_out], or [4, n_out] for the channelizers.  x: [N], or
    [4, N] for the synthesizers.  The constructs of gpu_util under the contract the plan must report."""
    ct = contract(kind, len(h), ratio)
    if kind == "decimate_cx":
        return cx_decim_ref(oracle, h, ratio, x, ct)
    if kind == "interpolate_cx":
        return cx_interp_ref(oracle, h, ratio, x, ct[0])
    if kind == "channelize":
        return chan_ref(oracle, h, x)
    if kind == "channelize_os":
        return chan_os_ref(oracle, h, x)
    if kind == "synthesize":
        return syn_ref(oracle, h, x, ct[0])
    return syn_os_ref(oracle, h, x, ct[0])


def keying_threshold(ref):
    """The median squared magnitude of a TX reference, in float32: outputs on both sides of convert_tx's keying rule."""
    ref = np.ascontiguousarray(ref, dtype=np.complex64)
    return np.float32(np.median(ref.real ** 2 + ref.imag ** 2))


def stored_words(kind, oracle, fmt, ref, thr2=None):
    """The reference as the plan stores it, uint32 [..., n_out, words per sample]: CF32 as it is; CF16: one rounding to half; S32 out
    of a TX kind: convert_tx of the CF32 result under thr2 (S32 into an RX kind leaves CF32)."""
    ref = np.ascontiguousarray(ref, dtype=np.complex64)
    if fmt == "CF16":
        return np.ascontiguousarray(oracle.f32_to_f16(ref.view(np.float32))).view(np.uint32).reshape(ref.shape + (1,))
    if fmt == "S32" and not KINDS[kind].decim:
        return oracle.convert_tx(ref.ravel(), thr2).view(np.uint32).reshape(ref.shape + (2,))
    return ref.view(np.uint32).reshape(ref.shape + (2,))


# ---- the reference of a channelizer without the zero taps ------------------------------------------------------------------------
def _butterflies_rx(a):
    re = [np.ascontiguousarray(v.real) for v in a]
    im = [np.ascontiguousarray(v.imag) for v in a]
    s0re, s0im, s1re, s1im = re[0] + re[2], im[0] + im[2], re[0] - re[2], im[0] - im[2]
    t0re, t0im, t1re, t1im = re[1] + re[3], im[1] + im[3], re[1] - re[3], im[1] - im[3]
    assert s0re.dtype == np.float32 and t1im.dtype == np.float32
    y = np.empty((4, a[0].size), dtype=np.complex64)
    y[0].real, y[0].imag = s0re + t0re, s0im + t0im
    y[1].real, y[1].imag = s1re - t1im, s1im + t1re
    y[2].real, y[2].imag = s0re - t0re, s0im - t0im
    y[3].real, y[3].imag = s1re + t1im, s1im - t1re
    return y


def chan_ref_phase_taps(oracle, h, x, step):
    """chan_ref (step 4) / chan_os_ref (step 2) with every branch sum taken over the taps of its phase ALONE, as the headers state the
    contract: u_r[m] = sum_j h[4j + r] x[step m - 4j - r] is the chain of the taps h[r::4] over the stream x[step m - r] taken every
    4th sample.  chan_ref leaves the other phases' taps in the chain as +0.0, which changes nothing while the samples are finite
    (asserted in tests/test_band_cases_host.py) and turns an infinite sample into a NaN the kernels never compute."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.complex64)
    n_out = (x.size + step - 1) // step
    u = np.zeros((4, n_out), dtype=np.complex64)
    for r in range(4):
        for first in range(4 // step):                      # step 2: the even and the odd outputs are two streams of their own
            m = np.arange(first, n_out, 4 // step)
            if m.size == 0:
                continue
            at = step * m - r                               # the stream's samples: x[at], every 4th sample of x; x[<0] = +0.0
            s = np.where(at >= 0, x[np.maximum(at, 0)], np.complex64(0)).astype(np.complex64)
            u[r, m] = oracle.decim_f32(np.ascontiguousarray(h[r::4]), 1, s, 1, 1)
    if step == 4:
        return _butterflies_rx([u[r] for r in range(4)])
    odd = (np.arange(n_out) & 1) == 1
    return _butterflies_rx([np.where(odd, u[(r + 2) % 4], u[r]) for r in range(4)])


# ---- the definitions in fp64 -----------------------------------------------------------------------------------------------------
QUARTER = np.array([1, 1j, -1, -1j])                        # exact quarter turns


def _up(x, L):
    u = np.zeros(x.size * L, dtype=np.complex128)
    u[::L] = x
    return u


def definition_fp64(kind, h, ratio, x):
    """The headers' formulas with np.convolve alone, complex128: no oracle, no butterflies, no polyphase split.  Channelizer band
    k: convolve(x, h j^(k n)) taken every 4th sample; oversampled: every 2nd, times (-1)^(k m).  Synthesizer: sum_k j^(k n)
    (h * up4 x_k)[n]; oversampled: up2, n the absolute output index.  Complex kinds: complex h convolved directly."""
    K = KINDS[kind]
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.complex128 if K.complex_taps else np.float64)
    N = x.shape[-1]
    t = np.arange(h.size)
    if kind == "decimate_cx":
        return np.convolve(x, h)[:N:ratio]
    if kind == "interpolate_cx":
        return np.convolve(_up(x, ratio), h)[:N * ratio]
    if K.banded_out:
        y = np.stack([np.convolve(x, h * QUARTER[(k * t) % 4])[:N:ratio] for k in range(4)])
        if kind == "channelize_os":
            m = np.arange(y.shape[1])
            for k in range(4):
                y[k] *= np.where((k * m) % 2 == 1, -1.0, 1.0)
        return y
    n = np.arange(N * ratio)
    return sum(QUARTER[(k * n) % 4] * np.convolve(_up(x[k], ratio), h)[:N * ratio] for k in range(4))


def anchor_shapes(kind):
    """(label, ntaps, ratio) of the shapes the fp64, non-finite and subnormal tests run: every tiled shape and one generic shape."""
    K = KINDS[kind]
    out = [("tiled-%dx%d" % s, s[0], s[1]) for s in K.tiled_shapes]
    generic = {"decimate_cx": (35, 5), "interpolate_cx": (40, 5)}.get(kind, (40, K.ratio))
    return out + [("generic-%dx%d" % generic,) + generic]


def anchor_length(kind, ratio):
    """About 3000 inputs (per band): two tiles plus a ragged tail for the 2048-sample kinds."""
    T = tile_of(kind, ratio)
    return 2 * T + 37 * 3 if T == 2048 else 3000 + 3


def fp64_bound(kind, h):
    """2e-6 sum|h| B: the project's figure for a float32 pass against fp64 (test_every_configuration_against_scipy_fp64), B the
    input streams added into one output (4 for the synthesizers)."""
    return 2.0e-6 * float(np.abs(np.asarray(h).astype(np.complex128)).sum()) * (BANDS if KINDS[kind].banded_in else 1)
