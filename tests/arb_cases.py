"""The arbitrary-rate resamplers' model, references and bound (include/sxfir_arbitrary.h), shared by tests/test_arb_host.py and
tests/test_gpu_arb.py.

The model is the header's definition in Python's big integers: the count rule, the position of an output, a stream that is cut into
calls.  The bit-exact reference needs nothing new of the oracle: an output is a blend of samples k and k + 1 of the x P interpolator's
output, so it is the oracle's order-matched interpolator pass over the needed window, two samples of it per output, blended in
float32.  The fp64 definition is the same sum in float64 with the same 24-bit alpha."""
import numpy as np

from rational_cases import BOUND

ONE = 1 << 32
MASK = ONE - 1
STEP_MIN, STEP_MAX = 1 << 28, 1 << 36
# the steps the issue names: unity (alpha = 0, p = 0 throughout), 5/4, 1 + 1e-6, the two ends of the range, sqrt(2)
STEPS = [ONE, 5 << 30, ONE + 4295, STEP_MIN, STEP_MAX, 0x16A09E667]


def count(t, step, consumed, n_in):
    """(n_out, t after): a call of n_in inputs on a stream that has consumed `consumed`, the next output at time t (Q.32)."""
    limit = (consumed + n_in - 1) << 32
    n = max(0, -(-(limit - t) // step))
    return n, t + n * step


def locate(rel, step, m, P):
    """(n_rel, p, alpha24) of output m of a call whose first output lies at rel (Q.32, relative to input consumed - 1)."""
    pos = rel + m * step
    z = (pos & MASK) * P
    return pos >> 32, z >> 32, (z & MASK) >> 8


def position(t, P):
    """(n, p, alpha24) of the output at absolute time t."""
    return locate(t, ONE, 0, P)


class Stream:
    """A stream cut into calls: .call(n_in) gives the absolute times of the call's outputs."""

    def __init__(self, step, consumed=0, t=None):
        self.step, self.consumed, self.t, self.produced = step, consumed, consumed << 32 if t is None else t, 0

    def call(self, n_in):
        n, after = count(self.t, self.step, self.consumed, n_in)
        times = [self.t + i * self.step for i in range(n)]
        assert not times or (times[-1] >> 32) + 1 <= self.consumed + n_in - 1, "an output without its look-ahead sample"
        self.t, self.consumed, self.produced = after, self.consumed + n_in, self.produced + n
        assert (self.t >> 32) >= self.consumed - 1
        return times


def times_of(steps, n, consumed=0, t=None):
    """The output times of a stream of n inputs.  `steps`: one step, or [(n_in, step), ...] -- calls of n_in inputs, the step set
    before each; the calls' inputs add up to n."""
    if isinstance(steps, int):
        steps = [(n, steps)]
    assert sum(k for k, _ in steps) == n
    s = Stream(steps[0][1], consumed, t)
    out = []
    for k, step in steps:
        s.step = step
        out += s.call(k)
    return out


def arb_taps(P, T, seed=23):
    """Real taps with no symmetry to lean on."""
    return (np.random.default_rng(seed + P + 1000 * T).standard_normal(P * T) / 16.0).astype(np.float32)


def fma_f32(alpha, d, a):
    """float32 fmaf(alpha, d, a), elementwise, alpha a 24-bit fraction: the product of two 24-bit significands is exact in float64;
    the float64 sum is made sticky (rounded to odd, from the exact error of the addition) so that the second rounding, to float32,
    rounds the exact value: 53 bits are two more than float32's 24 plus the sticky bit need."""
    alpha = np.asarray(alpha, dtype=np.float64)
    d = np.asarray(d, dtype=np.float32).astype(np.float64)
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = alpha * d
        s = prod + a
        bb = s - prod
        err = (prod - (s - bb)) + (a - bb)                   # TwoSum: exact for finite operands
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix & (err > 0), np.nextafter(s, np.inf), np.where(fix & (err < 0), np.nextafter(s, -np.inf), s))
        return s.astype(np.float32)


def _located(times, P):
    pos = [position(t, P) for t in times]
    n = np.array([q[0] for q in pos], dtype=np.int64)
    p = np.array([q[1] for q in pos], dtype=np.int64)
    alpha = np.array([q[2] for q in pos], dtype=np.float64) * 2.0 ** -24
    return n, p, alpha


def arb_ref(oracle, h, P, steps, x, jsplit, consumed=0, t=None):
    """complex64 [n_out]: the outputs of the stream x (its first sample at absolute index `consumed`, zero history in front) under the
    x P interpolator's contract: samples k, k + 1 of oracle.interp_f32 over the needed window, blended in float32."""
    return blend_at(oracle, h, P, times_of(steps, len(x), consumed, t), x, jsplit, consumed)


def blend_at(oracle, h, P, times, x, jsplit, x0=0):
    """complex64 [len(times)]: the outputs at the absolute times `times` (Q.32) of a stream whose sample x0 + i is x[i] and whose
    samples below x0 are zeros."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.complex64)
    consumed = x0
    if not times:
        return np.zeros(0, dtype=np.complex64)
    n, p, alpha = _located(times, P)
    assert n.max() + 1 <= x0 + len(x) - 1, "an output without its look-ahead sample"
    k = (n - consumed) * P + p                          # on the x P raster of x alone
    # an output in the history (floor(t) = consumed - 1) reads u below x's first sample: a stream of zeros in front stands for it
    T = h.size // P
    lead = T + 1
    xz = np.concatenate([np.zeros(lead, dtype=np.complex64), x])
    k = k + lead * P
    k0 = int(k.min())
    u = oracle.interp_f32(h, P, xz, jsplit, n0=k0, n_out=int(k.max()) + 2 - k0)
    a, b = u[k - k0], u[k + 1 - k0]
    y = np.empty(len(times), dtype=np.complex64)
    with np.errstate(invalid="ignore", over="ignore"):
        y.real = fma_f32(alpha, b.real - a.real, a.real)     # (b - a: float32, one rounding)
        y.imag = fma_f32(alpha, b.imag - a.imag, a.imag)
    return y


def arb_f64(h, P, steps, x, consumed=0, t=None):
    """complex128: the definition in float64 with the same 24-bit alpha."""
    h = np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.complex128)
    T = h.size // P
    times = times_of(steps, len(x), consumed, t)
    n, p, alpha = _located(times, P)
    k = (n - consumed) * P + p
    xz = np.concatenate([np.zeros(T + 1, dtype=np.complex128), x, np.zeros(1, dtype=np.complex128)])

    def u(kk):
        q, r = kk // P, kk % P
        j = np.arange(T)
        return (h[j[None, :] * P + r[:, None]] * xz[q[:, None] - j[None, :] + T + 1]).sum(axis=1)
    a, b = u(k), u(k + 1)
    return a + alpha * (b - a)


def bound(h, x):
    """(BOUND + 3 * 2^-24) sum|h| max|x|: the project's bound on a float32 chain against fp64 for u[k] and u[k + 1], and three
    roundings of the blend -- the subtraction (operands within sum|h| max|x| each, so its result within twice that: one ulp of it
    is two of the unit) and the fma (its result within the operands' range: one)."""
    return (BOUND + 3 * 2.0 ** -24) * float(np.abs(np.asarray(h, dtype=np.float64)).sum()) * float(np.abs(np.asarray(x, dtype=np.complex128)).max())
