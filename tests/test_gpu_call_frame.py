"""The streaming call of every plan kind, through each of the nine ways into it (sxfir_launch.hip.h: stream_call): a stream
cut anywhere gives the oracle's bits and the arithmetic positions, a refused call leaves the plan and the output alone, and
destroying a plan gives its device memory back.

The nine ways: sxfir_decimate on real taps (/4 x 128) and on complex taps (/4 x 128), sxfir_channelize (4 x 128, critically
sampled and 2x oversampled), sxfir_interpolate on real and on complex taps (x4 x 128), sxfir_interpolate_keyed (x8 x 256) and
sxfir_synthesize (4 x 128, critically sampled and 2x oversampled); CF32, one channel.

Cut anywhere: the calls are [0, 1, 2, 1, T, 3, T + 4, rest] with T the tiled kernel's input tile (2048 for the decimator kinds;
256 for x4 and the synthesizer, 512 for the oversampled synthesizer, 128 for x8).  The decimator kinds' stream is 2 * 2048 + 11
samples, which the seven calls use up (the rest is a second call of nothing, off an output boundary).  The interpolator kinds'
stream is 3 T + 3 inputs per band (3 * 256 + 3 at x8): the seven calls take 2 T + 11 inputs, more than two tiles and three, and
the rest is a ragged call of its own.  The oversampled channelizer, whose tiled kernel takes a stream position that is a multiple
of 4, has calls of its own, [0, 1, 2, 1, T, 2, T + 4, 3, rest] on 2 * 2048 + 15 samples: the calls of T + 4 and of 3 start ON an
output boundary at a position = 2 mod 4 -- an odd output index -- and run the generic kernel for that alone."""
import ctypes as C

import numpy as np
import pytest

import sxxcvr_amd
from sxxcvr_amd import design_bandpass, design_lowpass
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE
from gpu_util import assert_bands, assert_bit_exact, chan_os_ref, chan_ref, cx_decim_ref, cx_interp_ref, syn_os_ref, syn_ref, to_cpu

pytestmark = pytest.mark.gpu

SEED = 0xF4A3E
THR2 = np.float32(0.49)
WAYS = ["decimate", "decimate_cx", "channelize", "interpolate", "interpolate_keyed", "synthesize", "channelize_os", "synthesize_os",
        "interpolate_cx"]
ENTRIES = ["sxfir_decimate", "sxfir_interpolate", "sxfir_interpolate_keyed", "sxfir_channelize", "sxfir_synthesize",
           "sxfir_time_decimate", "sxfir_time_interpolate"]
EINVAL, EUNSUPPORTED = -1, -4


class Way:
    """One way into the frame: how its plan is made, which entry points take that plan, and its oracle."""

    def __init__(self, name):
        self.name = name
        self.decim = name in ("decimate", "decimate_cx", "channelize", "channelize_os")
        self.banded_in = name in ("synthesize", "synthesize_os")            # input [4, n]
        self.banded_out = name in ("channelize", "channelize_os")           # output [4, n_out]
        self.oversampled = name.endswith("_os")
        self.ratio = 8 if name == "interpolate_keyed" else 2 if self.oversampled else 4
        self.tile = 2048 if self.decim else 512 if name == "synthesize_os" else (128 if self.ratio == 8 else 256)
        self.stream = 2 * 2048 + 11 if self.decim else 3 * max(self.tile, 256) + 3
        self.cuts = [0, 1, 2, 1, self.tile, 3, self.tile + 4]
        if name == "channelize_os":
            self.stream = 2 * 2048 + 15
            self.cuts = [0, 1, 2, 1, self.tile, 2, self.tile + 4, 3]
        if name == "decimate_cx":
            self.taps = design_bandpass(128, 4, 1, 4)
        elif name == "interpolate_cx":
            self.taps = design_bandpass(128, 4, 1, 4, gain=4.0)
        elif self.decim:
            self.taps = design_lowpass(128, 4)
        elif name == "synthesize_os":
            self.taps = design_lowpass(128, 4, 8.0, 2.0)    # a x2 interpolator's low-pass with the /4 band edge
        else:
            self.taps = design_lowpass(32 * self.ratio, self.ratio, 8.0, float(self.ratio))
        self.own = {"decimate": {"sxfir_decimate", "sxfir_time_decimate"},
                    "decimate_cx": {"sxfir_decimate", "sxfir_time_decimate"},
                    "channelize": {"sxfir_channelize"},
                    "interpolate": {"sxfir_interpolate", "sxfir_interpolate_keyed", "sxfir_time_interpolate"},
                    "interpolate_keyed": {"sxfir_interpolate", "sxfir_interpolate_keyed", "sxfir_time_interpolate"},
                    "synthesize": {"sxfir_synthesize"},
                    "channelize_os": {"sxfir_channelize"},
                    "synthesize_os": {"sxfir_synthesize"},
                    "interpolate_cx": {"sxfir_interpolate", "sxfir_interpolate_keyed", "sxfir_time_interpolate"}}[name]
        self.entry = "sxfir_" + name.replace("_cx", "").replace("_os", "")

    def plan(self, nchan=1):
        if self.banded_out:
            return sxxcvr_amd.Channelizer(self.taps, nchan=nchan, oversample=2 if self.oversampled else 1)
        if self.banded_in:
            return sxxcvr_amd.Synthesizer(self.taps, nchan=nchan, oversample=2 if self.oversampled else 1)
        if self.name == "interpolate_cx":
            p = sxxcvr_amd.ComplexInterpolator(self.taps, self.ratio, nchan=nchan)
            p.set_tx_threshold(float(THR2))
            return p
        p = sxxcvr_amd.Resampler(DECIMATE if self.decim else INTERPOLATE, self.taps, self.ratio, nchan=nchan)
        if not self.decim:
            p.set_tx_threshold(float(THR2))
        return p

    def source(self, oracle, n):
        """The synthetic source on the GPU ([n], or [4, n] for the synthesizer) and its CPU twin."""
        import torch
        shape = (4, n) if self.banded_in else (n,)
        x = torch.empty(shape, dtype=torch.complex64, device="cuda")
        sxxcvr_amd.synth_fill(x, SEED, 3, 0)
        xs = np.stack([oracle.synth_iq(SEED, 3 + k, 0, n) for k in range(4)]) if self.banded_in else oracle.synth_iq(SEED, 3, 0, n)
        return x, xs

    def n_out(self, n_in, consumed=0):
        if not self.decim:
            return n_in * self.ratio
        r = self.ratio
        return (consumed + n_in + r - 1) // r - (consumed + r - 1) // r

    def reference(self, oracle, plan, xs):
        if self.name == "decimate":
            return oracle.decim_f32(self.taps, 4, xs, *plan.contract)
        if self.name == "decimate_cx":
            return cx_decim_ref(oracle, self.taps, 4, xs, plan.contract)
        if self.name == "interpolate_cx":
            return cx_interp_ref(oracle, self.taps, 4, xs, plan.contract[0])
        if self.name == "channelize":
            return chan_ref(oracle, self.taps, xs)
        if self.name == "channelize_os":
            return chan_os_ref(oracle, self.taps, xs)
        if self.name == "synthesize":
            return syn_ref(oracle, self.taps, xs, plan.contract[0])
        if self.name == "synthesize_os":
            return syn_os_ref(oracle, self.taps, xs, plan.contract[0])
        return oracle.interp_f32(self.taps, self.ratio, xs, plan.contract[0])

    def call(self, lib, entry, plan, x, n, in_stride, band_in, out, out_stride, band_out, n_out, key=None):
        """One raw call of `entry` (any of ENTRIES) on `plan` (a ctypes pointer or None); pointers as integers."""
        vp = C.c_void_p
        if entry == "sxfir_channelize":
            return lib.sxfir_channelize(plan, vp(x), n, in_stride, vp(out), out_stride, band_out, C.byref(n_out), None)
        if entry == "sxfir_synthesize":
            return lib.sxfir_synthesize(plan, vp(x), n, in_stride, band_in, vp(out), out_stride, C.byref(n_out), None)
        if entry == "sxfir_interpolate_keyed":
            first, count, counter = key
            return lib.sxfir_interpolate_keyed(plan, vp(x), n, in_stride, vp(out), out_stride, C.byref(n_out), first, count, vp(counter), None)
        if entry.startswith("sxfir_time_"):
            ms = C.c_float()
            return getattr(lib, entry)(plan, vp(x), n, in_stride, vp(out), out_stride, 1, None, C.byref(ms))
        return getattr(lib, entry)(plan, vp(x), n, in_stride, vp(out), out_stride, C.byref(n_out), None)


def keyed_count(xs, lo, hi):
    """Samples of xs[lo:hi] whose squared magnitude reaches the threshold: two products and one sum, each rounded to float32."""
    v = np.ascontiguousarray(xs[lo:hi]).view(np.float32).reshape(-1, 2)
    return int(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) >= THR2).sum())


@pytest.mark.parametrize("name", WAYS)
def test_cut_anywhere(oracle, name):
    import torch
    w = Way(name)
    lib = sxxcvr_amd.load_sxfir()
    T = w.tile
    plan = w.plan()
    probe = plan.geometry(4 * 2048)
    assert probe["tiled"] and probe["tile_samples"] == (T if w.decim else T * w.ratio), probe
    x, xs = w.source(oracle, w.stream)
    calls = list(w.cuts)
    calls.append(w.stream - sum(calls))
    assert calls[-1] >= 0
    total_out = w.n_out(w.stream)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    x_row = x.stride(0) if w.banded_in else 0
    pos_in = pos_out = want_keyed = 0
    kernels, outs = set(), []
    for n in calls:
        asked = plan.outputs_for(n)
        assert asked == w.n_out(n, pos_in)
        kernels.add(plan.geometry(n)["kernel"] if asked or not w.decim else "history only")
        if w.decim and asked:       # the tiled kernels' position rule: a multiple of 4, for /4 an output boundary, for the oversampled channelizer one of even index
            assert plan.geometry(n)["tiled"] == (pos_in % 4 == 0), (n, pos_in)
        # a buffer of its own for every call, the empty ones included: 16-byte aligned, an even band stride (the tiled stores)
        row = max(asked + (asked & 1), 2)
        out = torch.zeros((4, row) if w.banded_out else (row,), dtype=torch.complex64, device="cuda")
        key = None
        if name == "interpolate_keyed":
            first = n // 3
            key = (first, (n - first + 1) // 2, counter.data_ptr())
            want_keyed += keyed_count(xs, pos_in + first, pos_in + first + key[1])
        n_out = C.c_size_t(77)
        rc = w.call(lib, w.entry, plan._plan, x.data_ptr() + 8 * pos_in, n, n, x_row, out.data_ptr(), row, row, n_out, key)
        assert rc == 0, (n, lib.sxfir_last_error())
        assert n_out.value == asked, (n, n_out.value, asked)
        pos_in += n
        pos_out += asked
        assert plan.position == (pos_in, pos_out), n
        outs.append((out, asked))
    torch.cuda.synchronize()
    assert pos_in == w.stream and pos_out == total_out
    if w.decim:         # the tiled kernel, the generic one (a call that starts off an output boundary) and the history pass alone
        assert len(kernels) == 3 and "history only" in kernels, kernels
    ref = w.reference(oracle, plan, xs)
    for out, asked in outs:
        assert np.all(to_cpu(out)[..., asked:].view(np.uint64) == 0), "something was written behind a call's outputs"
    got = np.concatenate([to_cpu(out)[..., :asked] for out, asked in outs], axis=-1)
    if w.banded_out:
        assert_bands(got, ref, name)
    else:
        assert_bit_exact(got, ref, name)
    if name == "interpolate_keyed":
        assert 0 < want_keyed < w.stream
        assert int(counter.item()) == want_keyed
    plan.close()


@pytest.mark.parametrize("name", WAYS)
def test_refusals_leave_the_plan_alone(oracle, name):
    import torch
    w = Way(name)
    lib = sxxcvr_amd.load_sxfir()
    n = w.tile
    n_o = w.n_out(n)
    x, xs = w.source(oracle, n)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    key = (0, n, counter.data_ptr())

    def rig(nchan):
        """A fresh plan of `nchan` channels, an input buffer that would do for a good call and a zeroed output buffer."""
        plan = w.plan(nchan)
        xin = torch.zeros((nchan, 4, n) if w.banded_in else (nchan, n), dtype=torch.complex64, device="cuda")
        out = torch.zeros((nchan, 4, n_o) if w.banded_out else (nchan, n_o), dtype=torch.complex64, device="cuda")
        return plan, xin, out

    def refused(plan, out, entry, handle, xp, in_stride, band_in, op, out_stride, band_out, code=EINVAL):
        n_out = C.c_size_t(77)
        rc = w.call(lib, entry, handle, xp, n, in_stride, band_in, op, out_stride, band_out, n_out, key)
        what = (entry, xp != 0, in_stride, band_in, op != 0, out_stride, band_out)
        assert rc == code, (what, rc, lib.sxfir_last_error())
        assert len(lib.sxfir_last_error()) > 0, what
        assert entry.startswith("sxfir_time_") or n_out.value == 0, what
        assert plan.position == (0, 0), what
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(torch.view_as_real(out))) == 0, what

    plan, _, out = rig(1)
    xp, op = x.data_ptr(), out.data_ptr()
    # the strides of a good call
    band_in = n if w.banded_in else 0
    band_out = n_o if w.banded_out else 0
    good = (n, band_in, op, n_o, band_out)
    refused(plan, out, w.entry, plan._plan, 0, *good)                                        # NULL input
    refused(plan, out, w.entry, plan._plan, xp, n, band_in, 0, n_o, band_out)                # NULL output
    for entry in ENTRIES:                                                                    # NULL plan, whichever way in
        refused(plan, out, entry, None, xp, *good)
    refused(plan, out, w.entry, plan._plan, xp + 4, *good)                                   # half a sample off
    refused(plan, out, w.entry, plan._plan, xp, n, band_in, op + 4, n_o, band_out)
    for entry in ENTRIES:                                                                    # every entry point that is not this kind's
        if entry not in w.own:
            refused(plan, out, entry, plan._plan, xp, *good)
    if w.banded_in:
        with pytest.raises(sxxcvr_amd.NativeError) as ei:
            plan.set_history_ptr(xp, n, n)
        assert ei.value.code == EUNSUPPORTED and plan.position == (0, 0)
    assert int(counter.item()) == 0
    # two channels: a channel stride one short; a band plan's overlapping layout
    two, x2, out2 = rig(2)
    x2p, o2p = x2.data_ptr(), out2.data_ptr()
    in2, o2 = (4 * n if w.banded_in else n), (4 * n_o if w.banded_out else n_o)              # bands inside channels
    refused(two, out2, w.entry, two._plan, x2p, in2 - 1 if not w.banded_in else n - 1, band_in, o2p, o2, band_out)
    refused(two, out2, w.entry, two._plan, x2p, in2, band_in, o2p, o2 - 1 if not w.banded_out else n_o - 1, band_out)
    if w.banded_out:
        refused(two, out2, w.entry, two._plan, x2p, in2, band_in, o2p, 2 * n_o, n_o)
    if w.banded_in:
        refused(two, out2, w.entry, two._plan, x2p, 2 * n, n, o2p, o2, band_out)
    two.close()
    ref = w.reference(oracle, plan, xs)
    # the timing entry that takes this kind (a complex-tap plan is a decimator to sxfir_time_decimate) accepts it: the same tile,
    # filtered from the same empty history into a buffer of its own, and no position moves
    for entry in sorted(e for e in w.own if e.startswith("sxfir_time_")):
        timed = torch.zeros_like(out)
        assert w.call(lib, entry, plan._plan, xp, n, n, band_in, timed.data_ptr(), n_o, band_out, C.c_size_t(77), key) == 0, \
            (entry, lib.sxfir_last_error())
        torch.cuda.synchronize()
        assert plan.position == (0, 0) and int(torch.count_nonzero(torch.view_as_real(out))) == 0
        assert_bit_exact(to_cpu(timed)[0], ref, entry)
    # one good call of one tile
    n_out = C.c_size_t(77)
    assert w.call(lib, w.entry, plan._plan, xp, n, *good, n_out, key) == 0, lib.sxfir_last_error()
    torch.cuda.synchronize()
    assert n_out.value == n_o and plan.position == (n, n_o)
    if w.banded_out:
        assert_bands(to_cpu(out)[0], ref, name)
    else:
        assert_bit_exact(to_cpu(out)[0], ref, name)
    if name == "interpolate_keyed":
        assert int(counter.item()) == keyed_count(xs, 0, n)
    plan.close()


def _owned_bytes(kind, ntaps, ratio, nchan, resident):
    """What one plan holds on the device: two tap tables at the most, two history buffers and, for /96, the join scratch (eight
    times the chip's workgroup slots in tiles: six block values of 4 KiB and one arrival counter each)."""
    hist = 4 * ((ntaps // 4 + 1) & ~1) if kind == "synthesize" else (ntaps + 1) & ~1
    join = 8 * resident * (6 * 4096 + 4) if ratio == 96 else 0
    return 2 * 4 * ntaps + 2 * 8 * hist * nchan + join


@pytest.mark.parametrize("kind", ["real", "complex", "channelize", "synthesize", "real96"])
def test_destroy_gives_the_memory_back(kind):
    """Twenty plans created and destroyed in a row leave the device's free memory where it was, to within one plan's own
    allocation (a condition: a leaked member would cost twenty).  One plan is created and destroyed before the first reading, so
    that what the allocator keeps for itself on a first allocation is not counted.

    The four small kinds own a few KiB each, and the device hands memory out in far larger pieces: twenty leaked buffers of that
    size need not move `mem_get_info` at all, so those four cases can pass over a leak.  The /96 case is the one that sees it:
    its join scratch is some 96 MiB a plan, and twenty leaked plans are unmistakable."""
    import torch

    def make():
        if kind == "complex":
            return sxxcvr_amd.Resampler(DECIMATE, design_bandpass(128, 4, 1, 4), 4)
        if kind == "channelize":
            return sxxcvr_amd.Channelizer(design_lowpass(128, 4))
        if kind == "synthesize":
            return sxxcvr_amd.Synthesizer(design_lowpass(128, 4, 8.0, 4.0))
        r = 96 if kind == "real96" else 4
        return sxxcvr_amd.Resampler(DECIMATE, design_lowpass(32 * r, r), r)

    first = make()
    r = first.ratio
    resident = first.geometry(r * 512)["resident"]
    assert kind != "real96" or first.geometry(r * 512)["kernel"] == "decim_blocks_kernel"
    first.close()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        make().close()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    cap = _owned_bytes(kind, 32 * r, r, 1, resident)
    print("%s: free before %d, after %d (difference %d), one plan owns %d bytes" % (kind, before, after, before - after, cap))
    assert kind != "real96" or cap > 90 << 20
    assert before - after <= cap
