"""Helpers shared by the -m gpu parity tests."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.complex64).view(np.uint64)


def assert_bit_exact(got, ref, what=""):
    got = np.ascontiguousarray(got, dtype=np.complex64)
    ref = np.ascontiguousarray(ref, dtype=np.complex64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.nonzero(bits(got).ravel() != bits(ref).ravel())[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: %d of %d outputs differ, first at %d: got %r want %r" % (
            what, bad.size, got.size, i, got.ravel()[i], ref.ravel()[i]))


def ulp_distance(a, b):
    a = np.ascontiguousarray(a, dtype=np.complex64).view(np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.complex64).view(np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def to_gpu(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_cpu(t):
    return t.cpu().numpy()


# ---- the band plans' inputs (tests/test_gpu_channelizer.py, test_gpu_synthesizer.py and their _os files: each binds its own
# SEED with functools.partial and names the result `source`) --------------------------------------------------------------------
def random_taps(n, seed=5):
    """Real taps with no symmetry to lean on."""
    return (np.random.default_rng(seed).standard_normal(n) / 64.0).astype(np.float32)


def wideband_source(oracle, channel, n, start=0, seed=0):
    """The synthetic source on the GPU and its CPU twin: a channelizer's input."""
    import torch
    import sxxcvr_amd
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, seed, channel, start)
    return x, oracle.synth_iq(seed, channel, start, n)


def four_band_source(oracle, channel, n, start=0, seed=0):
    """Four bands of the synthetic source on the GPU (channels channel .. channel + 3) and their CPU twin: a synthesizer's input."""
    import torch
    import sxxcvr_amd
    x = torch.empty((4, n), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, seed, channel, start)
    return x, np.stack([oracle.synth_iq(seed, channel + k, start, n) for k in range(4)])


def run(plan, xg, **kw):
    """One process() call, waited for, on the CPU."""
    import torch
    y = plan.process(xg, **kw)
    torch.cuda.synchronize()
    return to_cpu(y)


def band_proto(gain=1.0):
    """The 128-tap prototype of the 4-band plans, the /4 band edge: gain 1 for a channelizer (critically sampled or oversampled),
    4 for the synthesizer (as for any x4 interpolator), 2 for the oversampled synthesizer (a x2 interpolator's)."""
    import sxxcvr_amd
    return sxxcvr_amd.design_lowpass(128, 4, 8.0, gain)


# ---- the band plans' references (tests/test_gpu_channelizer.py, test_gpu_synthesizer.py and their _os files, test_gpu_call_frame.py,
# tests/band_cases.py) ---------------------------------------------------------------------------------------------------------
def chan_ref(oracle, h, x, threads=None):
    """[4, n_out] complex64: the four bands of one channelizer pass over x from zero history."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    u = []
    for r in range(4):
        hr = np.zeros_like(h)                               # +0.0
        hr[r::4] = h[r::4]
        u.append(oracle.decim_f32(hr, 4, x, 1, 1, threads=threads))
    f = np.float32
    s0re, s0im, s1re, s1im = u[0].real + u[2].real, u[0].imag + u[2].imag, u[0].real - u[2].real, u[0].imag - u[2].imag
    t0re, t0im, t1re, t1im = u[1].real + u[3].real, u[1].imag + u[3].imag, u[1].real - u[3].real, u[1].imag - u[3].imag
    assert s0re.dtype == f and t1im.dtype == f
    y = np.empty((4, u[0].size), dtype=np.complex64)
    y[0].real, y[0].imag = s0re + t0re, s0im + t0im
    y[1].real, y[1].imag = s1re - t1im, s1im + t1re
    y[2].real, y[2].imag = s0re - t0re, s0im - t0im
    y[3].real, y[3].imag = s1re + t1im, s1im - t1re
    return y


def assert_bands(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for k in range(4):
        assert_bit_exact(got[k], ref[k], "%s, band %d" % (what, k))


def butterflies_f32(x):
    """[4, n] complex64 -> the four streams v_r of the synthesizer, float32 arithmetic."""
    f = np.float32
    re = [np.ascontiguousarray(x[k].real) for k in range(4)]
    im = [np.ascontiguousarray(x[k].imag) for k in range(4)]
    a0re, a0im, a1re, a1im = re[0] + re[2], im[0] + im[2], re[0] - re[2], im[0] - im[2]
    b0re, b0im, b1re, b1im = re[1] + re[3], im[1] + im[3], re[1] - re[3], im[1] - im[3]
    assert a0re.dtype == f and b1im.dtype == f
    v = np.empty((4, x.shape[1]), dtype=np.complex64)
    v[0].real, v[0].imag = a0re + b0re, a0im + b0im
    v[1].real, v[1].imag = a1re - b1im, a1im + b1re
    v[2].real, v[2].imag = a0re - b0re, a0im - b0im
    v[3].real, v[3].imag = a1re + b1im, a1im - b1re
    return v


def syn_ref(oracle, h, x, jsplit, threads=None):
    """[4 n] complex64: one synthesizer pass over the four bands x [4, n] from zero history."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.complex64)
    v = butterflies_f32(x)
    w = np.empty(4 * x.shape[1], dtype=np.complex64)
    for r in range(4):
        y = oracle.interp_f32(h, 4, v[r], jsplit) if threads is None else oracle.interp_f32_mt(h, 4, v[r], jsplit, threads=threads)
        w[r::4] = y[r::4]
    return w


def chan_os_ref(oracle, h, x, threads=None):
    """[4, ceil(n / 2)] complex64: the four bands of one 2x oversampled channelizer pass over x from zero history (the butterflies
    on (u0, u1, u2, u3) in the even columns and on (u2, u3, u0, u1) in the odd ones)."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    u = []
    for r in range(4):
        hr = np.zeros_like(h)                               # +0.0
        hr[r::4] = h[r::4]
        u.append(oracle.decim_f32(hr, 2, x, 1, 1, threads=threads))
    odd = (np.arange(u[0].size) & 1) == 1
    a = [np.where(odd, u[(r + 2) % 4], u[r]) for r in range(4)]          # odd times: the branch sums shifted by two
    re = [np.ascontiguousarray(v.real) for v in a]
    im = [np.ascontiguousarray(v.imag) for v in a]
    s0re, s0im, s1re, s1im = re[0] + re[2], im[0] + im[2], re[0] - re[2], im[0] - im[2]
    t0re, t0im, t1re, t1im = re[1] + re[3], im[1] + im[3], re[1] - re[3], im[1] - im[3]
    assert s0re.dtype == np.float32 and t1im.dtype == np.float32
    y = np.empty((4, u[0].size), dtype=np.complex64)
    y[0].real, y[0].imag = s0re + t0re, s0im + t0im
    y[1].real, y[1].imag = s1re - t1im, s1im + t1re
    y[2].real, y[2].imag = s0re - t0re, s0im - t0im
    y[3].real, y[3].imag = s1re + t1im, s1im - t1re
    return y


def syn_os_ref(oracle, h, x, jsplit, m0=0, threads=None):
    """[2 n] complex64: one 2x oversampled synthesizer pass over the four bands x [4, n] from zero history, the first input at the
    absolute per-band index m0."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.complex64)
    v = butterflies_f32(x)
    n = np.arange(2 * x.shape[1])
    w = np.empty(n.size, dtype=np.complex64)
    for r in range(4):
        y = oracle.interp_f32(h, 2, v[r], jsplit) if threads is None else oracle.interp_f32_mt(h, 2, v[r], jsplit, threads=threads)
        pick = ((n + 2 * m0) & 3) == r
        w[pick] = y[pick]
    return w


# ---- the complex-tap plans' taps and references (tests/test_gpu_complex_taps.py, test_gpu_complex_interp.py) --------------------
def random_taps_cx(n, seed=5):
    """Complex taps with no structure to lean on."""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / 64.0).astype(np.complex64)


def _cx_combine(A, B):
    ref = np.empty(A.shape, dtype=np.complex64)
    ref.real = A.real - B.imag                          # float32, one rounding each
    ref.imag = A.imag + B.real
    return ref


def cx_decim_ref(oracle, h, D, x, contract, threads=None):
    """A complex-tap decimator pass: two real-tap oracle passes (Re h, Im h) under `contract` (with its .rot), combined in float32."""
    rot = contract.rot                                  # (read first: the pair alone does not state a rotated contract)
    js, cw = contract
    a = np.ascontiguousarray(h.real, dtype=np.float32)
    b = np.ascontiguousarray(h.imag, dtype=np.float32)
    A = oracle.decim_f32(a, D, x, js, cw, rot=rot, threads=threads)
    B = oracle.decim_f32(b, D, x, js, cw, rot=rot, threads=threads)
    return _cx_combine(A, B)


def cx_interp_ref(oracle, h, L, x, jsplit, threads=None):
    """A complex-tap interpolator pass: two real-tap oracle passes (Re h, Im h) under jsplit, combined in float32."""
    a = np.ascontiguousarray(h.real, dtype=np.float32)
    b = np.ascontiguousarray(h.imag, dtype=np.float32)
    if threads is None:
        A, B = oracle.interp_f32(a, L, x, jsplit), oracle.interp_f32(b, L, x, jsplit)
    else:
        A, B = oracle.interp_f32_mt(a, L, x, jsplit, threads=threads), oracle.interp_f32_mt(b, L, x, jsplit, threads=threads)
    return _cx_combine(A, B)


# ---- the (tile, block) join of the decimators by 48 and 96 (decim_blocks_kernel<..., SPLIT>) --------------------------------
# One checker for tests/test_gpu_join.py and tools/soak_split.py.  The dealt form hands 4 KiB block values from workgroup to
# workgroup through the plan's scratch; what could go wrong there is a joiner that reads a block value of an EARLIER launch (stale),
# half of one (torn) or none, or an arrival counter that is not zero when a launch starts.  So: several DIFFERENT inputs of one
# geometry in turn (a stale value is then another input's and differs), the scratch poisoned with NaNs before every launch where
# the library has the hook (a value that was never stored, or is read before it lands, is then a NaN), the destination prefilled
# with NaNs (an output that was never stored shows), call sizes that change the slots' meaning, a second stream that loads the
# chip unevenly, back-to-back launches with no host synchronisation, and EVERY output word of every launch compared -- on the GPU,
# against the bits of another kernel instance (the walking form: one workgroup adds a tile's blocks in registers) which, for CF32,
# is itself checked against the CPU oracle.
JOIN_POISON = 0x7FC00000          # a quiet NaN in every fp32 lane of the scratch
OUT_FILL = 0x7FC07FC0             # a NaN as one fp32 word and as two halves: no kernel output of random data is this word
TILE_OUT = 512


def plan_knobs(**knobs):
    """Context manager: the environment holds exactly these SXFIR_* knobs (the profiling build reads them when a plan is created)
    and is put back afterwards."""
    import contextlib
    import os

    @contextlib.contextmanager
    def cm():
        keep = ("SXFIR_NO_TORCH", "SXFIR_PROF_LIB")
        saved = {k: v for k, v in os.environ.items() if k.startswith("SXFIR_") and k not in keep}
        for k in saved:
            del os.environ[k]
        os.environ.update({k: str(v) for k, v in knobs.items()})
        try:
            yield
        finally:
            for k in knobs:
                os.environ.pop(k, None)
            os.environ.update(saved)
    return cm()


def join_taps(D):
    """Asymmetric random taps, 32 per phase."""
    return (np.random.default_rng(D + 1).standard_normal(32 * D) / 64.0).astype(np.float32)


_load_rig = None


def _join_load_rig():
    """The neighbour of the soak: a /4, 128-tap plan of the product library with 2^26 samples of input (made once per process)."""
    global _load_rig
    if _load_rig is None:
        import torch
        import sxxcvr_amd
        from sxxcvr_amd.resampler import DECIMATE, KERNEL_TILED
        plan = sxxcvr_amd.Resampler(DECIMATE, sxxcvr_amd.design_lowpass(128, 4, 8.0, 1.0), 4)
        plan.set_kernel(KERNEL_TILED)
        x = torch.empty(1 << 26, dtype=torch.complex64, device="cuda")
        sxxcvr_amd.synth_fill(x, 0x10AD, 0, 0)
        y = torch.empty(1 << 24, dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        _load_rig = (plan, x, y, torch.cuda.Stream())
    return _load_rig


class JoinSoak:
    """Inputs and references of one case (ratio D, format, channels, outputs per channel of the full call); run() soaks a plan.

    Inputs: n_inputs windows of one buffer, each `shift` = 4 D x 37 samples after the one before (a multiple of 4 D, no multiple of
    a tile: what a slot of the scratch held in the last launch is never what it gets in this one).  Call sizes: "full", "one"
    (one tile) and "few" (five tiles, the last ragged) over the same windows.  References: the walking form of the PROFILING
    library (SXFIR_BLOCKS_SPLIT=0), one launch per (input, size), kept as whole destination images (the NaN prefill beyond the
    call's outputs included: a store past the end shows too); for CF32 with `oracle` those are checked against
    decim_f32 under the contract the plan reports -- everywhere when the call is small, else over five windows of 3000 outputs
    with the first and the last."""

    def __init__(self, D, fmt, nchan, n_out, oracle=None, n_inputs=3, seed=0x51255):
        import torch
        import sxxcvr_amd
        from sxxcvr_amd.resampler import DECIMATE, KERNEL_TILED
        assert n_out % 4 == 0 and n_out > 5 * TILE_OUT and n_inputs >= 2
        self.D, self.fmt, self.nchan, self.n_inputs = D, fmt, nchan, n_inputs
        self.h = join_taps(D)
        self.sizes = {"full": n_out, "one": TILE_OUT, "few": 4 * TILE_OUT + 76}
        self.n_tiles = (n_out + TILE_OUT - 1) // TILE_OUT
        self.shift = 4 * D * 37
        assert self.shift % (4 * D) == 0 and self.shift % (TILE_OUT * D) != 0
        self.total = n_out * D + (n_inputs - 1) * self.shift
        self.sb = 4 if fmt == "CF16" else 8               # bytes per input sample
        self.wpo = 1 if fmt == "CF16" else 2              # 32-bit words per output sample
        if fmt == "S32":
            g = torch.Generator(device="cuda")
            g.manual_seed(seed)
            self.buf = torch.randint(-2 ** 31, 2 ** 31, (nchan, self.total, 2), generator=g, device="cuda").to(torch.int32)
        elif fmt == "CF16":
            self.buf = torch.empty((nchan, self.total), dtype=torch.int32, device="cuda")
            sxxcvr_amd.synth_fill(self.buf, seed, 90, 0, fmt="CF16")
        else:
            self.buf = torch.empty((nchan, self.total), dtype=torch.complex64, device="cuda")
            sxxcvr_amd.synth_fill(self.buf, seed, 90, 0)
        self.y = torch.empty((nchan, n_out * self.wpo), dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())
        with plan_knobs(SXFIR_BLOCKS_SPLIT=0):
            walk = sxxcvr_amd.Resampler(DECIMATE, self.h, D, nchan=nchan, fmt=fmt, profiling=True)
        walk.set_kernel(KERNEL_TILED)
        contract = walk.contract
        rot = contract.rot                              # (read first: the pair alone does not state a rotated contract)
        self.contract = tuple(contract) + (rot,)
        assert self.contract == (2, 4, 1), self.contract
        self.refs = {}
        for i in range(n_inputs):
            for size, n in self.sizes.items():
                g = walk.geometry(n * D)
                assert g["kernel"] == "decim_blocks_kernel" and g["split"] == 1, g
                self.launch(walk, i, size)
                with torch.cuda.stream(self.stream):
                    self.refs[i, size] = self.y.clone()
        self.stream.synchronize()
        walk.close()
        for (i, size), r in self.refs.items():
            n = self.sizes[size] * self.wpo
            assert int((r[:, :n] == _i32(OUT_FILL)).sum()) == 0, "the walking form left outputs unstored (input %d, %s)" % (i, size)
            assert int((r[:, n:] != _i32(OUT_FILL)).sum()) == 0, "the walking form stored past its outputs (input %d, %s)" % (i, size)
        self.oracle_outputs = 0
        if oracle is not None and fmt == "CF32":
            self._check_refs(oracle)

    def in_ptr(self, i):
        return self.buf.data_ptr() + self.sb * self.shift * i

    def launch(self, plan, i, size, poison=False):
        """Prefill the destination, reset, (poison,) one call of `size` over input i: all on the soak's stream, nothing waits."""
        import torch
        s = self.stream.cuda_stream
        with torch.cuda.stream(self.stream):
            self.y.fill_(_i32(OUT_FILL))
        plan.reset(s)
        if poison:
            plan.join_poison(JOIN_POISON, s)
        n = self.sizes[size]
        got = plan.process_ptr(self.in_ptr(i), n * self.D, self.total, self.y.data_ptr(), self.sizes["full"], s)
        assert got == n

    def _check_refs(self, oracle):
        js, cw, rot = self.contract
        D = self.D
        th = oracle.max_threads()
        for (i, size), r in sorted(self.refs.items()):
            n = self.sizes[size]
            if n <= 40000:
                windows = [(0, n)]
            else:
                k = 3000
                windows = [(0, k)] + [((n * j // 4) | 1, k) for j in (1, 2, 3)] + [(n - k, k)]
            ref = r.cpu().numpy()
            for c in range(self.nchan):
                for m0, k in windows:
                    lead = min(m0, 32)                     # rows of history in front of the window (zero history before the stream)
                    s0 = self.shift * i + (m0 - lead) * D
                    x = self.buf[c, s0:s0 + (lead + k) * D].cpu().numpy()
                    want = oracle.decim_f32(self.h, D, x, js, cw, m0=lead, n_out=k, rot=rot, threads=th)
                    got = ref[c, 2 * m0:2 * (m0 + k)].view(np.complex64)
                    assert_bit_exact(got, want, "/%d walking form against the oracle, input %d (%s) channel %d outputs %d.." % (D, i, size, c, m0))
                    self.oracle_outputs += k

    def check_geometry(self, plan):
        """Every call size the soak uses takes the dealt form on this plan."""
        for size, n in self.sizes.items():
            g = plan.geometry(n * self.D)
            assert g["kernel"] == "decim_blocks_kernel" and g["split"] == self.D // 16, (size, g)

    def run(self, plan, launches, poison, load, mixed=True, per_tile=False, seconds=None):
        """`launches` launches (or, with `seconds`, batches of 100 until that long has passed), inputs in turn, every 7th with
        another call size (mixed); returns {"launches", "bad_words", "counters" (profiling plans, else None)} and, with per_tile
        (full-size calls only), per launch the number of tiles with a differing word and of tiles whose every word is a NaN."""
        import time
        import torch
        self.check_geometry(plan)
        if poison and not plan.profiling:
            raise ValueError("the product library has no poison hook")
        assert not (per_tile and (mixed or self.fmt == "CF16"))
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        self.stream.wait_stream(torch.cuda.current_stream())
        tiles_bad, tiles_nan = [], []
        if load:
            lplan, lx, ly, lstream = _join_load_rig()
            order = np.random.default_rng(7).integers(22, 27, size=997)       # 2^22 .. 2^26 samples, a fixed order
        other = ("one", "few")
        k, t0 = 0, time.time()
        while k < launches or (seconds is not None and time.time() - t0 < seconds):
            for _ in range(min(100, launches - k) if seconds is None else 100):
                i = k % self.n_inputs
                size = other[(k // 7) % 2] if (mixed and k % 7 == 6) else "full"
                if load:
                    lplan.process_ptr(lx.data_ptr(), 1 << int(order[k % order.size]), 1 << 26, ly.data_ptr(), 1 << 24, lstream.cuda_stream)
                self.launch(plan, i, size, poison)
                with torch.cuda.stream(self.stream):
                    diff = self.y != self.refs[i, size]
                    bad += diff.sum()
                    if per_tile:
                        nan = torch.isnan(self.y.view(torch.float32))
                        tiles_bad.append(self._by_tile(diff, False).any(-1).sum())
                        tiles_nan.append(self._by_tile(nan, True).all(-1).sum())
                k += 1
        torch.cuda.synchronize()
        res = {"launches": k, "bad_words": int(bad.item()),
               "counters": plan.join_counters(self.stream.cuda_stream) if plan.profiling else None}
        if per_tile:
            res["tiles_bad"] = [int(t) for t in tiles_bad]
            res["tiles_nan"] = [int(t) for t in tiles_nan]
        return res

    def _by_tile(self, flags, fill):
        """[nchan, words] flags as [nchan, tiles, words per tile], the ragged last tile filled up with `fill`."""
        import torch
        per = flags.shape[1] // self.sizes["full"] * TILE_OUT
        out = torch.full((self.nchan, self.n_tiles * per), fill, dtype=torch.bool, device=flags.device)
        out[:, :flags.shape[1]] = flags
        return out.view(self.nchan, self.n_tiles, per)

    def inputs_differ_tiles(self, i, j):
        """How many (channel, tile) pairs of the full call see different input in windows i and j (their own 512 D samples)."""
        import torch
        n = self.sizes["full"] * self.D

        def words(k):
            w = self.buf[:, self.shift * k:self.shift * k + n]
            if w.dtype == torch.complex64:
                w = torch.view_as_real(w).view(torch.int32)
            return w.reshape(self.nchan, -1)
        return int(self._by_tile(words(i) != words(j), False).any(-1).sum())


def _i32(word):
    return word - (1 << 32) if word >= 1 << 31 else word
