"""CPU-side checks of the arbitrary-rate resamplers (include/sxfir_arbitrary.h): the extension's symbols and bindings, the refusals
of sxfir_create_arbitrary that need no GPU, the two host-only functions -- the count rule and the kernels' own index arithmetic --
against the big-integer model of tests/arb_cases.py, the float32 reference against the fp64 definition, and the shipped code object
of the new kernels."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_arbitrary, design_lowpass
from arb_cases import MASK, ONE, STEP_MAX, STEP_MIN, STEPS, Stream, arb_f64, arb_ref, arb_taps, bound, count, fma_f32, locate, times_of
from rational_cases import gaussian_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -5
NAMES = ["sxfir_arbitrary_abi_version", "sxfir_arbitrary_locate", "sxfir_arbitrary_outputs", "sxfir_create_arbitrary",
         "sxfir_plan_arbitrary", "sxfir_resample_arbitrary", "sxfir_set_rate", "sxfir_set_time", "sxfir_time_resample_arbitrary"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sxfir_[a-z0-9_]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_bound():
    assert _declared("sxfir_arbitrary.h") == NAMES
    lib = sxxcvr_amd.load_sxfir()
    prof = sxxcvr_amd.load_sxfir(profiling=True)
    for n in NAMES:
        assert hasattr(lib, n), "libsxfir.so does not export " + n
        assert n in lib._sx_signatures, "no prototype bound for " + n
        assert hasattr(prof, n) and n in prof._sx_signatures, "libsxfir_prof.so / its binding lacks " + n
    assert lib.sxfir_arbitrary_abi_version() == 1 and prof.sxfir_arbitrary_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "sxfir_arbitrary.h")).read()
    assert int(re.search(r"^#define\s+SXFIR_ARBITRARY_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 1
    # the base ABI's number is the header's, untouched by the extension
    text = open(os.path.join(ROOT, "include", "sxfir.h")).read()
    assert lib.sxfir_abi_version() == int(re.search(r"^#define\s+SXFIR_ABI_VERSION\s+(\d+)", text, re.M).group(1))
    assert sxxcvr_amd.ArbitraryResampler.__mro__[1] is sxxcvr_amd.Resampler
    assert "ArbitraryResampler" in sxxcvr_amd.__all__ and "design_arbitrary" in sxxcvr_amd.__all__
    # the bindings' argument lists are the header's: as many arguments, the scalars of the header's types
    ctype = {"int": C.c_int, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "size_t": C.c_size_t}
    body = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sxfir_arbitrary.h")).read(), flags=re.S)
    seen = []
    for m in re.finditer(r"\bint\s+(sxfir_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body):
        name, args = m.group(1), [a.strip() for a in m.group(2).split(",") if a.strip() != "void"]
        got = lib._sx_signatures[name][1]
        assert len(got) == len(args), (name, got, args)
        for g, a in zip(got, args):
            if "*" not in a:
                assert g is ctype[a.split()[0]], (name, a, g)
        seen.append(name)
    assert sorted(seen) == NAMES


def test_create_refusals_need_no_gpu():
    lib = sxxcvr_amd.load_sxfir()
    create = lib.sxfir_create_arbitrary
    taps = np.ones(4096, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    CF32, CF16, S32 = 0, 1, 2
    assert create(None, tp, 4096, 128, ONE, 1, CF32, -1) == EINVAL
    # (taps, ntaps, nphases, step, nchan, fmt) -> code and a word of the message, in the order the creator checks them
    cases = [((None, 4096, 128, ONE, 1, CF32), EINVAL, b"NULL"),
             ((tp, 0, 128, ONE, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 65537, 128, ONE, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 4096, 1, ONE, 1, CF32), EINVAL, b"nphases"),
             ((tp, 4096, 4097, ONE, 1, CF32), EINVAL, b"nphases"),
             ((tp, 4095, 128, ONE, 1, CF32), EINVAL, b"ntaps % nphases"),
             ((tp, 4096, 128, STEP_MIN - 1, 1, CF32), EINVAL, b"step"),
             ((tp, 4096, 128, STEP_MAX + 1, 1, CF32), EINVAL, b"step"),
             ((tp, 4096, 128, 0, 1, CF32), EINVAL, b"step"),
             ((tp, 4096, 128, ONE, 0, CF32), EINVAL, b"nchan"),
             ((tp, 4096, 128, ONE, 1, 9), EINVAL, b"format"),
             ((tp, 4096, 128, ONE, 1, S32), EUNSUPPORTED, b"neither wire side"),
             # two bad arguments at once: the earlier check answers
             ((tp, 0, 1, ONE, 1, CF32), EINVAL, b"ntaps"),
             ((tp, 4095, 1, ONE, 1, CF32), EINVAL, b"nphases"),
             ((tp, 4095, 128, 0, 1, CF32), EINVAL, b"ntaps % nphases"),
             ((tp, 4096, 128, 0, 0, CF32), EINVAL, b"step"),
             ((tp, 4096, 128, ONE, 0, 9), EINVAL, b"nchan"),
             ((tp, 4096, 128, 0, 1, S32), EINVAL, b"step"),
             ((tp, 4096, 128, ONE, 0, S32), EINVAL, b"nchan")]
    for args, code, word in cases:
        plan.value = 0xDEAD if args[0] is not None else None
        assert create(C.byref(plan), *args, -1) == code, args
        assert word in lib.sxfir_last_error(), (args, lib.sxfir_last_error())
        assert not plan.value, args
    # the S32 refusal is the rational plan's, word for word
    rat = C.c_void_p()
    assert lib.sxfir_create_rational(C.byref(rat), tp, 128, 4, 5, 1, S32, -1) == EUNSUPPORTED
    words = lib.sxfir_last_error()
    assert create(C.byref(plan), tp, 4096, 128, ONE, 1, S32, -1) == EUNSUPPORTED and lib.sxfir_last_error() == words
    n = C.c_int(-1)
    lib.sxfir_device_count(C.byref(n))
    if n.value > 0:
        return          # (with a GPU the valid call succeeds: tests/test_gpu_arb.py)
    # no GPU: refused as the real-tap create refuses, never computed on the host
    for fmt in (CF32, CF16):
        assert create(C.byref(plan), tp, 4096, 128, ONE, 1, fmt, -1) == ENODEVICE and not plan.value
    with pytest.raises(sxxcvr_amd.NativeError) as ei:
        sxxcvr_amd.ArbitraryResampler(design_arbitrary(128), 128, rate=1.0)
    assert ei.value.code == ENODEVICE


def _outputs(lib, t, step, consumed, n_in):
    n, ti, tf = C.c_uint64(), C.c_int64(), C.c_uint32()
    assert lib.sxfir_arbitrary_outputs(t >> 32, t & MASK, step, consumed, n_in, C.byref(n), C.byref(ti), C.byref(tf)) == 0, lib.sxfir_last_error()
    return n.value, (ti.value << 32) | tf.value


def _brute(t, step, consumed, n_in):
    """The walk the rule stands for: outputs while x[floor(t) + 1] has been delivered."""
    n = 0
    while (t >> 32) + 1 <= consumed + n_in - 1:
        t += step
        n += 1
    return n, t


def test_outputs_against_the_model():
    lib = sxxcvr_amd.load_sxfir()
    rng = np.random.default_rng(2024)
    steps = STEPS + [int(s) for s in rng.integers(STEP_MIN, STEP_MAX, 6, endpoint=True)] + [int(s) for s in rng.integers(1 << 31, 1 << 33, 6)]
    cases = 0
    for step in steps:
        for trial in range(12):
            length = int(rng.integers(0, 400))
            # starts: the stream's start; placed so that consumed and floor(t) pass 2^31 and 2^32 inside a call
            start = [0, (1 << 31) - length // 2, (1 << 32) - length // 2, (1 << 32) - 3][trial % 4]
            frac = int(rng.integers(0, ONE)) if trial % 3 else 0
            t0 = (start << 32) + frac + (int(rng.integers(0, 3)) << 32)
            if trial % 5 == 4:
                t0 = ((start - 1) << 32) + frac                  # the first output lies in the history
            if start == 0:
                t0 = max(t0, 0) if trial % 2 else frac
            # one call
            want, after = count(t0, step, start, length)
            assert (want, after) == _outputs(lib, t0, step, start, length), (step, start, length, t0)
            if want < 5000:
                assert (want, after) == _brute(t0, step, start, length)
            # any split: the same count, the same time; floor(t) >= consumed - 1 after every call
            k = int(rng.integers(1, 7))
            cuts = sorted(int(c) for c in rng.integers(0, length + 1, k))
            sizes = [b - a for a, b in zip([0] + cuts, cuts + [length])] + [0, 1, 1]      # zero-length and one-sample calls too
            model = Stream(step, start, t0)
            t, c, total = t0, start, 0
            for n_in in sizes:
                got, t_next = _outputs(lib, t, step, c, n_in)
                assert got == len(model.call(n_in)) and t_next == model.t, (step, sizes, n_in)
                t, c, total = t_next, c + n_in, total + got
                assert (t >> 32) >= c - 1
            assert (total, t) == count(t0, step, start, length + 2), (step, sizes)
            cases += 1
    assert cases >= 200
    n, ti, tf = C.c_uint64(7), C.c_int64(7), C.c_uint32(7)
    for bad in [(-2, 0, ONE, 0, 5), (0, 0, STEP_MIN - 1, 0, 5), (0, 0, STEP_MAX + 1, 0, 5), (0, 0, ONE, -1, 5), (1 << 62, 0, ONE, 0, 5), (0, 0, ONE, 0, 1 << 62)]:
        assert lib.sxfir_arbitrary_outputs(*bad, C.byref(n), C.byref(ti), C.byref(tf)) == EINVAL, bad
        assert n.value == 0
    assert lib.sxfir_arbitrary_outputs(0, 0, ONE, 0, 5, None, C.byref(ti), C.byref(tf)) == EINVAL


def _locate(lib, rel, step, m, P):
    n, p, a = C.c_int64(), C.c_int(), C.c_float()
    assert lib.sxfir_arbitrary_locate(rel, step, m, P, C.byref(n), C.byref(p), C.byref(a)) == 0, lib.sxfir_last_error()
    a24 = a.value * 2.0 ** 24
    assert a24 == int(a24) and 0 <= a24 < 1 << 24
    return n.value, p.value, int(a24)


def test_locate_against_the_model():
    lib = sxxcvr_amd.load_sxfir()
    rng = np.random.default_rng(7)
    # m * step above 2^64
    m, step = (1 << 28) + 1, STEP_MAX
    assert m * step > 1 << 64
    for rel in (0, 1, MASK, ONE + 12345, (3 << 32) | 0xFF800000):
        for P in (2, 4, 7, 128, 4096):
            assert _locate(lib, rel, step, m, P) == locate(rel, step, m, P), (rel, P)
    # p == P - 1, by construction and by a walk
    for P in (4, 7, 128, 4096):
        rel = (5 << 32) | (MASK - 3)
        got = _locate(lib, rel, ONE, 0, P)
        assert got == locate(rel, ONE, 0, P) and got[1] == P - 1
    hits = 0
    for m in range(4096):
        got = _locate(lib, 0, 0x16A09E667, m, 128)
        assert got == locate(0, 0x16A09E667, m, 128)
        hits += got[1] == 127
    assert hits == 32
    # seeded cases over the whole range; the carry from the low half into the high one
    for _ in range(3000):
        step = int(rng.integers(STEP_MIN, STEP_MAX, endpoint=True))
        m = int(rng.integers(0, 1 << int(rng.integers(1, 30))))
        rel = int(rng.integers(0, 1 << int(rng.integers(1, 62))))
        P = int(rng.integers(2, 4097))
        assert _locate(lib, rel, step, m, P) == locate(rel, step, m, P), (rel, step, m, P)
    assert _locate(lib, (1 << 64) - 1, STEP_MAX, 1 << 27, 128) == locate((1 << 64) - 1, STEP_MAX, 1 << 27, 128)
    n, p, a = C.c_int64(), C.c_int(), C.c_float()
    assert lib.sxfir_arbitrary_locate(0, ONE, 0, 1, C.byref(n), C.byref(p), C.byref(a)) == EINVAL
    assert lib.sxfir_arbitrary_locate(0, 1, 0, 4, C.byref(n), C.byref(p), C.byref(a)) == EINVAL
    assert lib.sxfir_arbitrary_locate(0, ONE, 0, 4, None, C.byref(p), C.byref(a)) == EINVAL


def test_fma_model_is_fmaf():
    """tests/arb_cases.py fma_f32 against exact rational arithmetic rounded once (and math.fma where Python has it)."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    n = 4000
    alpha = rng.integers(0, 1 << 24, n).astype(np.float64) * 2.0 ** -24
    d = rng.standard_normal(n).astype(np.float32)
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 3, n)).astype(np.float32)
    # ties of the second rounding, by construction: alpha * d a quarter ulp of a beside a half-way case
    a[:200] = np.float32(1.0)
    d[:200] = np.float32(2.0 ** -24) * (1 + rng.integers(0, 1 << 20, 200).astype(np.float32) * np.float32(2.0 ** -22))
    alpha[:200] = 0.5 + rng.integers(0, 2, 200) * 2.0 ** -24
    got = fma_f32(alpha, d, a)

    def rn32(fr):
        """Fraction -> float32, round to nearest even"""
        if fr == 0:
            return np.float32(0.0)
        s, v = (-1, -fr) if fr < 0 else (1, fr)
        e = max(v.numerator.bit_length() - v.denominator.bit_length(), -126 - 1)
        while Fraction(2) ** e > v and e > -126:
            e -= 1
        while Fraction(2) ** (e + 1) <= v:
            e += 1
        e = max(e, -126)
        q = v / Fraction(2) ** (e - 23)
        k = q.numerator // q.denominator
        r = q - k
        if r > Fraction(1, 2) or (r == Fraction(1, 2) and k & 1):
            k += 1
        return np.float32(s * float(k) * 2.0 ** (e - 23))
    for i in range(n):
        want = rn32(Fraction(float(alpha[i])) * Fraction(float(d[i])) + Fraction(float(a[i])))
        assert got[i] == want, (i, alpha[i], d[i], a[i], got[i], want)
        if hasattr(math, "fma"):
            s = math.fma(float(alpha[i]), float(d[i]), float(a[i]))         # (rounded to float64 once: not yet fmaf)
            assert abs(float(got[i]) - s) <= abs(s) * 2.0 ** -23


@pytest.mark.parametrize("P,T", [(P, T) for P in (4, 128) for T in (8, 32, 33)])
def test_reference_against_fp64(oracle, P, T):
    """The float32 reference against the definition in fp64, within (2e-6 + 3 * 2^-24) sum|h| max|x|, under jsplit 1 and, where T is
    even, 2; one step below 1, one above, one with set_rate in mid-stream."""
    h = arb_taps(P, T)
    x = gaussian_stream(1500)
    for steps in (0x16A09E667, 3 << 30, [(700, ONE + 4295), (800, 0x16A09E667)]):
        want = arb_f64(h, P, steps, x)
        assert want.size == len(times_of(steps, x.size)) > 0
        for jsplit in (1, 2) if T % 2 == 0 else (1,):
            got = arb_ref(oracle, h, P, steps, x, jsplit)
            assert got.dtype == np.complex64 and got.shape == want.shape
            err = float(np.abs(got.astype(np.complex128) - want).max())
            print("%d x %d jsplit %d: error %.3g, bound %.3g (%.0f times inside)" % (P, T, jsplit, err, bound(h, x), bound(h, x) / err))
            assert err <= bound(h, x)


def test_design_arbitrary_is_the_lowpass_it_stands_for():
    for P, tpp, rate, beta in [(128, 32, 1.0, 8.0), (128, 32, 0.8, 8.0), (4, 32, 0.8, 8.0), (7, 8, 1.25, 6.5), (128, 32, 2048.0 / 2400.0, 8.0)]:
        a = design_arbitrary(P, tpp, rate, beta)
        b = design_lowpass(P * tpp, int(math.ceil(P * max(1.0, 1.0 / rate))), beta, float(P))
        assert a.dtype == np.float32 and a.size == P * tpp
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (P, rate)
    assert design_arbitrary(128).size == 4096
    assert sxxcvr_amd.ArbitraryResampler._step_of(0.8, None) == 5 << 30
    assert sxxcvr_amd.ArbitraryResampler._step_of(1.0, None) == ONE
    assert sxxcvr_amd.ArbitraryResampler._step_of(None, 12345) == 12345


def test_shipped_code_object_of_the_arbitrary_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shipped_isa
    rows = shipped_isa.kernels()
    tiled = [r for r in rows if "resample_arb_kernel" in r["name"]]
    assert len(tiled) == 1, [r["name"] for r in rows]
    t = tiled[0]
    print(t)
    assert t["scratch_bytes"] == 0 and t["v_mfma"] == 0 and t["vgpr"] <= 128, t
    assert t["ds_read_b128"] > 0 and t["lds_bytes"] == 4 * (129 * 36) + 4 * 8 * (2 * 256 + 32 + 8), t
    generic = sorted(r["name"] for r in rows if "resample_arb_generic_kernel<" in r["name"])
    assert generic == ["resample_arb_generic_kernel<sxfir::CF16>", "resample_arb_generic_kernel<sxfir::CF32>"], generic
    for r in rows:
        if "resample_arb_generic_kernel" in r["name"]:
            assert r["scratch_bytes"] == 0 and r["v_mfma"] == 0, r
