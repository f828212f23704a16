"""The rational resamplers' references and shapes (include/sxfir_rational.h), shared by tests/test_rational_host.py and
tests/test_gpu_rational.py.

The bit-exact reference needs nothing new of the oracle: y[m] is sample m * down of the x up interpolator's output, so it is the
oracle's order-matched interpolator pass, every down-th sample of it.  The fp64 definition is numpy's convolution of the
zero-stuffed stream with the taps, sampled the same way."""
import numpy as np

# (up, down, taps per phase): the shapes the float32 reference was checked against fp64 at
SHAPES = [(4, 5, 32), (2, 3, 32), (3, 4, 8), (5, 4, 32), (3, 2, 16), (7, 5, 4)]
BOUND = 2e-6            # the project's bound on a float32 chain against fp64: BOUND * sum|h| * max|x|


def n_out_for(n_in, up, down, consumed=0):
    """Outputs of a call of n_in inputs on a plan that has consumed `consumed`: ceil((c + n) up / down) - ceil(c up / down)."""
    return -(-(consumed + n_in) * up // down) - -(-consumed * up // down)


def rational_taps(up, taps_per_phase, seed=11):
    """Real taps with no symmetry to lean on."""
    return (np.random.default_rng(seed + up).standard_normal(up * taps_per_phase) / 16.0).astype(np.float32)


def gaussian_stream(n, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def rational_ref(oracle, h, up, down, x, jsplit):
    """complex64 [ceil(len(x) up / down)]: one pass over x from zero history under the x up interpolator's contract."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.complex64)
    return np.ascontiguousarray(oracle.interp_f32(h, up, x, jsplit)[::down][:n_out_for(len(x), up, down)])


def rational_f64(h, up, down, x):
    """complex128: the definition, np.convolve of the zero-stuffed stream, sampled every `down`."""
    x = np.asarray(x, dtype=np.complex128)
    z = np.zeros(len(x) * up, dtype=np.complex128)
    z[::up] = x
    return np.convolve(z, np.asarray(h, dtype=np.float64))[:len(z)][::down][:n_out_for(len(x), up, down)]


def bound(h, x):
    return BOUND * float(np.abs(np.asarray(h, dtype=np.float64)).sum()) * float(np.abs(np.asarray(x, dtype=np.complex128)).max())
