"""The launch geometry of every shape in the kernel table, field by field against a recorded table.

sxfir_create resolves a plan's kernels and occupancy once (sxfir_plan.hip.h) and decim_geom / interp_geom turn a call size
into tiles and workgroups (sxfir_launch.hip.h).  tests/golden/launch_geometry.json holds what Resampler.geometry() reported
for every shape and call size below BEFORE the two were rewritten around one kernel table; the figures depend on the chip's
compute-unit count, which the table stores.  Geometry is host arithmetic: the only kernel this file launches is the one
small call that takes a decimator off its output boundary.

    python tests/test_gpu_launch_table.py --record [path]     # writes the table from the library that is importable
"""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_geometry.json")
FIELDS = ["kernel", "tiled", "split", "tile_samples", "n_tiles", "workgroups", "resident"]
FMTS = ["CF32", "CF16", "S32"]
NCHAN = [1, 2, 3]

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> (mode, ratio, taps): both modes at ratios 4 .. 96 with 32 taps per phase, /4 with 64 taps, /4 with 128 taps
    that are not bit-symmetric, one shape only the generic kernels take, the two complex-tap plans, and the band plans
    ("chan...": created through Channelizer, "syn...": through Synthesizer; "...os...": with oversample=2, where `ratio` is the
    stream's 2 and the bands are 4) with the tiled kernels' 128 taps and with 64."""
    import sxxcvr_amd
    from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE
    out = {}
    for r in (4, 8, 16, 32, 48, 96):
        out["decim%d" % r] = (DECIMATE, r, sxxcvr_amd.design_lowpass(32 * r, r))
        out["interp%d" % r] = (INTERPOLATE, r, sxxcvr_amd.design_lowpass(32 * r, r, 8.0, float(r)))
    out["decim4x64"] = (DECIMATE, 4, sxxcvr_amd.design_lowpass(64, 4))
    asym = np.array(sxxcvr_amd.design_lowpass(128, 4), dtype=np.float32)
    asym[3] *= 1.5
    out["decim4asym"] = (DECIMATE, 4, asym)
    out["decim5x40"] = (DECIMATE, 5, sxxcvr_amd.design_lowpass(40, 5))
    out["interp5x40"] = (INTERPOLATE, 5, sxxcvr_amd.design_lowpass(40, 5, 8.0, 5.0))
    out["cx4x128"] = (DECIMATE, 4, sxxcvr_amd.design_bandpass(128, 4, 1, 4))
    out["cx8x256"] = (DECIMATE, 8, sxxcvr_amd.design_bandpass(256, 8, 1, 8))
    for n in (128, 64):
        out["chan4x%d" % n] = (DECIMATE, 4, sxxcvr_amd.design_lowpass(n, 4))
        out["syn4x%d" % n] = (INTERPOLATE, 4, sxxcvr_amd.design_lowpass(n, 4, 8.0, 4.0))
        # 2x oversampled: 4 bands on a /2, x2 stream
        out["chanos4x%d" % n] = (DECIMATE, 2, sxxcvr_amd.design_lowpass(n, 4))
        out["synos4x%d" % n] = (INTERPOLATE, 2, sxxcvr_amd.design_lowpass(n, 4, 8.0, 2.0))
    return out


SHAPE_NAMES = ["decim%d" % r for r in (4, 8, 16, 32, 48, 96)] + ["interp%d" % r for r in (4, 8, 16, 32, 48, 96)] + \
              ["decim4x64", "decim4asym", "decim5x40", "interp5x40", "cx4x128", "cx8x256"] + \
              ["chan4x128", "chan4x64", "syn4x128", "syn4x64"] + \
              ["chanos4x128", "chanos4x64", "synos4x128", "synos4x64"]


def call_sizes(plan, mode, ratio, nchan):
    """Input sample counts either side of every rule in the geometry code, from the plan's own tile and slot figures."""
    from sxxcvr_amd.resampler import DECIMATE
    g = plan.geometry(1 << 20)
    tile_in = g["tile_samples"] if mode == DECIMATE else g["tile_samples"] // ratio      # input samples per tile
    r = g["resident"]
    tiles = {1, 2, r + 3}
    # generations(): g = tiles * nchan [* phase blocks] / (4 * resident) reaches k; the /48, /96 join holds 8 * resident tiles
    # over all channels; the x32 .. x96 items are dealt up to 4 * resident tiles
    for k in (1, 2, 8):
        for div in {1, max(1, ratio // 16)}:
            t = 4 * r * k // (nchan * div)
            tiles |= {t - 1, t, t + 1}
    sizes = {tile_in - 1, 1 << 28}
    sizes |= {t * tile_in for t in tiles if t >= 1}
    return sorted(s for s in sizes if s >= 1)


def make_plan(name, fmt, nchan):
    import sxxcvr_amd
    mode, ratio, taps = shapes()[name]
    if name.startswith("chan"):
        return sxxcvr_amd.Channelizer(taps, 4, nchan=nchan, fmt=fmt, oversample=4 // ratio)
    if name.startswith("syn"):
        return sxxcvr_amd.Synthesizer(taps, 4, nchan=nchan, fmt=fmt, oversample=4 // ratio)
    return sxxcvr_amd.Resampler(mode, taps, ratio, nchan=nchan, fmt=fmt)


def rows_for(name, fmt, nchan, sizes=None):
    mode, ratio, taps = shapes()[name]
    plan = make_plan(name, fmt, nchan)
    try:
        sizes = sizes if sizes is not None else call_sizes(plan, mode, ratio, nchan)
        return [[n] + [plan.geometry(n)[f] for f in FIELDS] for n in sizes]
    finally:
        plan.close()


def off_boundary_rows(sizes=None):
    """A /8 x 256 decimator after one call of ratio + 1 samples: every later call starts off an output boundary."""
    import torch
    import sxxcvr_amd
    from sxxcvr_amd.resampler import DECIMATE
    plan = sxxcvr_amd.Resampler(DECIMATE, sxxcvr_amd.design_lowpass(256, 8), 8)
    try:
        x = torch.zeros(9, dtype=torch.complex64, device="cuda")
        plan.process(x)
        torch.cuda.synchronize()
        sizes = sizes if sizes is not None else [7, 8, 1024, 1 << 20]
        return [[n] + [plan.geometry(n)[f] for f in FIELDS] for n in sizes]
    finally:
        plan.close()


def chanos_position_rows(sizes=None):
    """position -> rows of a 2x oversampled channelizer (4 bands x 128 taps, CF32) placed there: every position of the /2 stream's
    raster starts on an output, but chan4x2_kernel also needs that output's index even -- a position that is a multiple of 4."""
    import sxxcvr_amd
    sizes = sizes if sizes is not None else [7, 8, 1024, 1 << 20]
    out = {}
    for pos in (2, 4):
        plan = sxxcvr_amd.Channelizer(sxxcvr_amd.design_lowpass(128, 4), 4, oversample=2)
        try:
            plan.set_position(pos)
            out[str(pos)] = [[n] + [plan.geometry(n)[f] for f in FIELDS] for n in sizes]
        finally:
            plan.close()
    return out


def compute_units():
    import sxxcvr_amd
    cu = C.c_int()
    assert sxxcvr_amd.load_sxfir().sxfir_device_info(0, None, None, C.byref(cu), None) == 0
    return cu.value


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        t = json.load(f)
    cu = compute_units()
    if cu != t["compute_units"]:
        pytest.skip("the table was recorded on a device with %d compute units, this one has %d" % (t["compute_units"], cu))
    return t


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_geometry_matches_recorded(table, name):
    checked = 0
    for fmt in FMTS:
        for nchan in NCHAN:
            want = table["plans"]["%s/%s/%d" % (name, fmt, nchan)]
            got = rows_for(name, fmt, nchan, [row[0] for row in want])
            for w, g in zip(want, got):
                assert g == w, "%s %s nchan %d, n_in %d: %r, recorded %r" % (name, fmt, nchan, w[0], dict(zip(FIELDS, g[1:])), dict(zip(FIELDS, w[1:])))
            checked += len(want)
    assert checked >= 9 * 10


def test_call_sizes_still_straddle_the_rules(table):
    """The recorded call sizes are the ones the rules of today's figures ask for (a changed occupancy would move them)."""
    for name in ("decim32", "decim96", "interp96", "cx4x128"):
        want = table["plans"]["%s/CF32/2" % name]
        assert [row[0] for row in rows_for(name, "CF32", 2)] == [row[0] for row in want], name


def test_off_boundary_falls_to_generic(table):
    want = table["off_boundary"]
    got = off_boundary_rows([row[0] for row in want])
    assert got == want
    assert all(row[1] == "decim_generic_kernel" and not row[2] for row in got)


def test_chanos_position_picks_the_kernel(table):
    want = table["chanos_position"]
    got = chanos_position_rows([row[0] for row in want["2"]])
    assert got == want
    assert all(row[1] == "chan4x2_generic_kernel" and not row[2] for row in got["2"])
    assert all(row[1] == "chan4x2_kernel" and row[2] for row in got["4"])


# ---- kernel-table entries that no other test compares with the oracle bit for bit (which test reaches which entry:
# profiles/launch_table_kernel_trace.txt).  Each with the smallest call that takes its path -- two tiles and a ragged tail, a
# second call on the first one's history, two channels; the walking forms' smallest call is a large one, so its output is
# checked in windows whose input is regenerated on the host from the counter-based source, as tests/test_gpu_kernels.py does
# at the /48, /96 split threshold.
SEED = 0x51255
THR2 = np.float32(0.49)
RATIOS = (4, 8, 16, 32, 48, 96)
# small calls: every keyed instance, and the S32 unkeyed ones (x8 apart: test_s32_wire_front_and_back_end)
INTERP_SMALL = [(L, fmt, keyed) for L in RATIOS for fmt in ("CF32", "S32") for keyed in (False, True) if keyed or (fmt == "S32" and L != 8)]
# walking forms of x32 .. x96 (x48, x96 on CF32 unkeyed: test_gpu_wholestream.py)
INTERP_WALKING = [(L, fmt, keyed) for L in (32, 48, 96) for fmt in ("CF32", "S32") for keyed in (False, True)
                  if not (L > 32 and fmt == "CF32" and not keyed)]
# walking forms of /48, /96 on the other storage formats (CF32: test_blocks_kernel_at_the_split_threshold)
DECIM_WALKING = [(D, fmt) for D in (48, 96) for fmt in ("S32", "CF16")]


def _window_starts(rng, n, w, k):
    return [0, n - w] + [int(v) for v in rng.integers(w, n - 2 * w, k)]


def _run_interp(plan, x, out, keyed, counter):
    """One call over x [2, n] into out [2, >= n L]; returns the counter's growth."""
    import torch
    n = x.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    before = int(counter.item())
    if keyed:
        got = plan.interpolate_keyed_ptr(x.data_ptr(), n, x.stride(0), out.data_ptr(), out.stride(0), 0, n, counter.data_ptr(), st)
    else:
        got = plan.process_ptr(x.data_ptr(), n, x.stride(0), out.data_ptr(), out.stride(0), st)
    torch.cuda.synchronize()
    assert got == n * plan.ratio
    return int(counter.item()) - before


def _interp_case(oracle, L, fmt, keyed, walking):
    import torch
    import sxxcvr_amd
    from sxxcvr_amd.resampler import INTERPOLATE, KERNEL_TILED
    h = sxxcvr_amd.design_lowpass(32 * L, L, 8.0, float(L))
    plan = sxxcvr_amd.Resampler(INTERPOLATE, h, L, nchan=2, fmt=fmt)
    plan.set_kernel(KERNEL_TILED)
    plan.set_tx_threshold(float(THR2))
    g = plan.geometry(1 << 12)
    tile = g["tile_samples"] // L
    assert g["kernel"] == "interp8_pass_kernel"
    # the walking form takes a call of more than 4 x resident tiles over both channels
    lens = [(2 * g["resident"]) * tile + 7, tile + 5] if walking else [2 * tile + 7, tile + 5]
    want_split = [1 if walking or L <= 16 else L // 16, 1 if L <= 16 else L // 16]
    total = sum(lens)
    x = torch.empty((2, total), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, SEED, 40, 0)
    out = torch.empty((2, total * L), dtype=torch.complex64, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    pos = 0
    for n, split in zip(lens, want_split):
        gg = plan.geometry(n)
        assert gg["tiled"] and gg["split"] == split, gg
        grew = _run_interp(plan, x[:, pos:pos + n], out[:, pos * L:], keyed, counter)
        if keyed:
            x0 = oracle.synth_iq(SEED, 40, pos, n)
            assert grew == int(((oracle.convert_tx(x0, THR2).reshape(-1, 2)[:, 0] & 3) == 3).sum())
        pos += n
    W = min(total, 600)                                        # inputs per window
    starts = sorted(set(_window_starts(np.random.default_rng(L), total, W, 6) + [lens[0] - W // 2])) if total > 3 * W else [0]
    for c in range(2):
        for s0 in starts:
            warm = min(s0, 32)                                 # inputs in front of the window: the taps' reach
            xs = oracle.synth_iq(SEED, 40 + c, s0 - warm, min(W, total - s0) + warm)
            ref = oracle.interp_f32(h, L, xs, plan.contract[0], n0=warm * L)
            got = out[c, s0 * L:s0 * L + ref.size].cpu().numpy()
            if fmt == "S32":
                ref = oracle.convert_tx(ref, THR2).view(np.uint64)
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64).ravel()), "x%d %s keyed=%d walking=%d: channel %d, inputs from %d" % (
                L, fmt, keyed, walking, c, s0)
    plan.close()


@pytest.mark.parametrize("L,fmt,keyed", INTERP_SMALL)
def test_interp_entry_small_call_against_oracle(oracle, L, fmt, keyed):
    _interp_case(oracle, L, fmt, keyed, walking=False)


@pytest.mark.parametrize("L,fmt,keyed", INTERP_WALKING)
def test_interp_entry_walking_form_against_oracle(oracle, L, fmt, keyed):
    _interp_case(oracle, L, fmt, keyed, walking=True)


@pytest.mark.parametrize("D,fmt", DECIM_WALKING)
def test_decim_blocks_walking_form_other_formats_against_oracle(oracle, D, fmt):
    import torch
    import sxxcvr_amd
    from sxxcvr_amd.resampler import DECIMATE, KERNEL_TILED
    h = sxxcvr_amd.design_lowpass(32 * D, D)
    plan = sxxcvr_amd.Resampler(DECIMATE, h, D, nchan=2, fmt=fmt)
    plan.set_kernel(KERNEL_TILED)
    assert plan.contract.rot == 1 and tuple(plan.contract) == (2, 4)
    r = plan.geometry(D * 512)["resident"]
    # outputs per channel and call: the smallest call the walking form takes (more than 8 x resident tiles over both channels),
    # then a small one on its history, which is dealt again
    lens = [512 * (4 * r) + 4, 512 + 8]                       # (ragged last tiles; multiples of 4: a channel stride the tiled stores take)
    total = sum(lens)
    x = torch.empty((2, D * total) if fmt == "CF16" else (2, D * total, 2), dtype=torch.int32, device="cuda")
    sxxcvr_amd.synth_fill(x if fmt == "CF16" else torch.view_as_complex(x.view(torch.float32)), SEED, 50, 0, fmt=fmt)
    outs, pos = [], 0
    for n, split in zip(lens, (1, D // 16)):
        gg = plan.geometry(D * n)
        assert gg["kernel"] == "decim_blocks_kernel" and gg["split"] == split, gg
        outs.append(plan.process(x[:, D * pos:D * (pos + n)]))
        pos += n
    torch.cuda.synchronize()
    W = 2000
    starts = sorted(set(_window_starts(np.random.default_rng(D), total, W, 6) + [lens[0] - W // 2]))
    for c in range(2):
        got_all = torch.cat([o[c] for o in outs])
        for m0 in starts:
            warm = min(m0, 32)                                 # outputs of the slice that still see its zero history
            n_w = min(W, total - m0)                           # (the window over the seam runs into the end of the short second call)
            xs = oracle.synth_iq(SEED, 50 + c, (m0 - warm) * D, (n_w + warm) * D)
            if fmt == "CF16":
                xs = oracle.f16_to_f32(oracle.f32_to_f16(xs.view(np.float32))).view(np.complex64)
            ref = oracle.decim_f32(h, D, xs, 2, 4, rot=1, threads=oracle.max_threads())[warm:]
            got = got_all[m0:m0 + n_w].cpu().numpy()
            assert got.shape[0] == n_w == ref.shape[0]
            if fmt == "CF16":
                assert np.array_equal(got.view(np.uint16), oracle.f32_to_f16(ref.view(np.float32)).ravel()), (D, fmt, c, m0)
            else:
                assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (D, fmt, c, m0)
    plan.close()


def test_decim4_tile_kernel_64_taps_against_oracle(oracle):
    """/4 with 64 taps: decim4_tile_kernel<64> (tiles of 256 outputs), two calls, two channels."""
    import torch
    import sxxcvr_amd
    from sxxcvr_amd.resampler import DECIMATE, KERNEL_TILED
    h = sxxcvr_amd.design_lowpass(64, 4)
    plan = sxxcvr_amd.Resampler(DECIMATE, h, 4, nchan=2)
    plan.set_kernel(KERNEL_TILED)
    lens = [4 * (2 * 256 + 38), 4 * (256 + 6)]              # (ragged last tiles; an even channel stride of the output)
    x = torch.empty((2, sum(lens)), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, SEED, 60, 0)
    outs, pos = [], 0
    for n in lens:
        g = plan.geometry(n)
        assert g["kernel"] == "decim4_tile_kernel" and g["tile_samples"] == 1024, g
        outs.append(plan.process(x[:, pos:pos + n]))
        pos += n
    torch.cuda.synchronize()
    for c in range(2):
        ref = oracle.decim_f32(h, 4, oracle.synth_iq(SEED, 60 + c, 0, sum(lens)), *plan.contract)
        got = torch.cat([o[c] for o in outs]).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), "channel %d" % c
    plan.close()


def record(path):
    t = {"compute_units": compute_units(), "fields": ["n_in"] + FIELDS, "plans": {}}
    for name in SHAPE_NAMES:
        for fmt in FMTS:
            for nchan in NCHAN:
                t["plans"]["%s/%s/%d" % (name, fmt, nchan)] = rows_for(name, fmt, nchan)
    t["off_boundary"] = off_boundary_rows()
    t["chanos_position"] = chanos_position_rows()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n \"compute_units\": %d,\n \"fields\": %s,\n \"off_boundary\": %s,\n \"chanos_position\": %s,\n \"plans\": {\n" % (
            t["compute_units"], json.dumps(t["fields"]), json.dumps(t["off_boundary"]), json.dumps(t["chanos_position"])))
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in t["plans"].items()))
        f.write("\n }\n}\n")
    print("recorded %d plans, %d rows, %d compute units -> %s" % (len(t["plans"]), sum(len(v) for v in t["plans"].values()), t["compute_units"], path))


if __name__ == "__main__":
    sys.path.append(ROOT)           # (behind PYTHONPATH: the table is recorded from whichever tree is put in front)
    record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
