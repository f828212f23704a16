"""The frequency-translating decimators' references (include/sxfir_translate.h), shared by tests/test_mix_host.py and
tests/test_gpu_mix.py.

The bit-exact reference needs nothing new of the oracle: z is the complex-tap decimator's reference (gpu_util.cx_decim_ref), and the
rotation is six float32 operations per output, each a numpy ufunc call of its own (numpy never fuses a product into a sum), on the
table that sxfir_design_rotator makes -- the table the plan itself uploads.  The fp64 definition uses neither the library's table nor
its reference."""
import numpy as np

from gpu_util import cx_decim_ref

BOUND = 2e-6                # the project's bound on a float32 chain against fp64: BOUND * sum|h| * max|x| (tests/rational_cases.py)
ROT_UNITS = 4.0             # the rotation's share: 4 * 2^-24 * (|z.re| + |z.im|) per component -- to first order 3 (table, product, sum)


def step(num, den, ratio):
    """s: table entries per output."""
    return (int(num) % int(den)) * int(ratio) % int(den)


def table_index(m_first, n, s, den):
    """int64 [n]: ((m_first + i) mod den) * s mod den, exact (m_first: a Python int of any size)."""
    m = (int(m_first) % int(den) + np.arange(n, dtype=np.int64)) % int(den)
    return (m * int(s)) % int(den)


def rotate_f32(z, w, m_first, s, den):
    """complex64 [.., n]: z[i] * w[((m_first + i) mod den) s mod den] in float32 -- two products and one subtraction or addition per
    component, one rounding each."""
    z = np.ascontiguousarray(z, dtype=np.complex64)
    w = np.ascontiguousarray(w, dtype=np.complex64)
    assert w.shape == (den,)
    idx = table_index(m_first, z.shape[-1], s, den)
    wre, wim = np.ascontiguousarray(w.real[idx]), np.ascontiguousarray(w.imag[idx])
    zre, zim = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    with np.errstate(all="ignore"):
        rr, ii = np.multiply(zre, wre), np.multiply(zim, wim)
        ri, ir = np.multiply(zre, wim), np.multiply(zim, wre)
        assert rr.dtype == np.float32 and ir.dtype == np.float32
        y = np.empty(z.shape, dtype=np.complex64)
        y.real = np.subtract(rr, ii)
        y.imag = np.add(ri, ir)
    return y


def mix_ref(oracle, h, ratio, x, contract, num, den, m_first=0, threads=None):
    """complex64: one translating pass over x from zero history, its first output at the absolute index m_first."""
    from sxxcvr_amd import design_rotator
    z = cx_decim_ref(oracle, h, ratio, x, contract, threads=threads)
    return rotate_f32(z, design_rotator(den), m_first, step(num, den, ratio), den)


def decim_f64(h, ratio, x):
    """complex128: z[m] = sum_k h[k] x[m ratio - k], x[<0] = 0."""
    x = np.asarray(x, dtype=np.complex128)
    return np.convolve(x, np.asarray(h, dtype=np.complex128))[:len(x)][::ratio]


def rotor_f64(m_first, n, s, den):
    """complex128 [n]: exp(-2j pi ((m_first + i) s mod den) / den), the index reduced in integers."""
    return np.exp(-2j * np.pi * table_index(m_first, n, s, den).astype(np.float64) / float(den))


def mix_f64(h, ratio, num, den, x, m_first=0):
    """complex128: the definition -- z in fp64, times exp(-2j pi num ratio m / den) with m the absolute 64-bit output index."""
    z = decim_f64(h, ratio, x)
    return z * rotor_f64(m_first, z.size, step(num, den, ratio), den)


def bound(h, x, z):
    """Per component of an output: the complex anchors' bound on z plus the rotation's term."""
    chain = BOUND * float(np.abs(np.asarray(h).astype(np.complex128)).sum()) * float(np.abs(np.asarray(x, dtype=np.complex128)).max())
    z = np.asarray(z, dtype=np.complex128)
    return chain + ROT_UNITS * 2.0 ** -24 * (np.abs(z.real) + np.abs(z.imag))
