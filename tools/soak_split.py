"""Soak of the two dealt forms (round 6).

decim_blocks_kernel<..., SPLIT> hands block values from workgroup to workgroup through HBM with device-scope stores / loads and one
atomic add per item -- the form the microarchitecture guide measured, "not an architectural guarantee".  This is the long form of
tests/test_gpu_join.py, through the same checker (tests/gpu_util.py, JoinSoak): three different inputs in turn (a stale block value
is another input's), the scratch poisoned with NaNs before every launch of the profiling library, the destination prefilled with
NaNs, every 7th launch another call size, a /4 plan of varying call size on a second stream beside it, no host synchronisation
between launches, every output word compared on the GPU with the walking form's (for CF32 itself checked against the CPU oracle),
the arrival counters all zero at the end.  Each case runs on the profiling library (with poison) and on the product library
(without: it has no hooks).

interp8_pass_kernel<..., PBSPLIT> deals phase blocks and joins nothing: its launches are compared with the first one's (itself
checked against the oracle on its first outputs).
    python3 tools/soak_split.py [seconds per case and library]        (default 4)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import sxxcvr_amd
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE, KERNEL_TILED
import oracle_lib
from gpu_util import JoinSoak, join_taps, plan_knobs

oracle_lib.build()
orc = oracle_lib.Oracle()
SECONDS = float(sys.argv[1]) if len(sys.argv) > 1 else 4.0
total_launches = total_bad = 0

# ---- the (tile, block) join: /48, /96
for D, fmt, nchan, lg in [(96, "CF32", 1, 18), (96, "CF32", 1, 22), (96, "CF32", 1, 24), (96, "CF32", 1, 26), (48, "CF32", 1, 20), (48, "CF32", 1, 25),
                          (96, "CF32", 4, 22), (48, "CF32", 8, 23), (48, "CF16", 2, 22), (96, "S32", 1, 22)]:
    n_out = max(((1 << lg) // nchan // D) // 512 * 512 + 76, 6 * 512 + 76)       # per channel; a ragged last tile
    case = JoinSoak(D, fmt, nchan, n_out, oracle=orc)
    for profiling in (True, False):
        with plan_knobs():
            plan = sxxcvr_amd.Resampler(DECIMATE, join_taps(D), D, nchan=nchan, fmt=fmt, profiling=profiling)
        plan.set_kernel(KERNEL_TILED)
        g = plan.geometry(n_out * D)
        res = case.run(plan, 0, poison=profiling, load=True, seconds=SECONDS)
        bad = res["bad_words"] + (res["counters"] or 0)
        print("/%-3d %s %d ch 2^%d (%s library%s): %d tiles x%d, %d workgroups on %d slots; walking form checked against the oracle on %d outputs; "
              "%d launches, %d words differ, %s arrival counters non-zero" % (
                  D, fmt, nchan, lg, "profiling" if profiling else "product", ", poisoned" if profiling else "", g["n_tiles"], g["split"],
                  g["workgroups"], g["resident"], case.oracle_outputs, res["launches"], res["bad_words"],
                  res["counters"] if profiling else "n/a"), flush=True)
        total_launches += res["launches"]; total_bad += bad
        plan.close()
    del case
    torch.cuda.empty_cache()

# ---- the phase-block dealing of the interpolators (nothing is joined)
for mode, ratio, nchan, lg in [(INTERPOLATE, 96, 1, 20), (INTERPOLATE, 96, 1, 24), (INTERPOLATE, 48, 2, 22), (INTERPOLATE, 32, 1, 22)]:
    h = sxxcvr_amd.design_lowpass(32 * ratio, ratio, 8.0, float(ratio))
    plan = sxxcvr_amd.Resampler(mode, h, ratio, nchan=nchan)
    plan.set_kernel(KERNEL_TILED)
    wide = ((1 << lg) // nchan) // (4 * ratio) * (4 * ratio)                     # per channel; aligned channel rows
    n_in, n_out = wide // ratio, wide
    g = plan.geometry(n_in)
    x = torch.empty((nchan, n_in), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y0 = torch.empty((nchan, n_out), dtype=torch.complex64, device="cuda")
    y = torch.empty_like(y0)
    plan.reset(); plan.process(x if nchan > 1 else x[0], out=y0 if nchan > 1 else y0[0]); torch.cuda.synchronize()
    k = min(3000, n_out)
    xs = orc.synth_iq(0x51255, 0, 0, (k + ratio - 1) // ratio)
    ref = orc.interp_f32(h, ratio, xs, 2)[:k]
    ok0 = np.array_equal(y0[0, :k].cpu().numpy().view(np.uint64), ref.view(np.uint64))
    ref_words = torch.view_as_real(y0).view(torch.int32)
    launches = bad = 0
    t0 = time.time()
    while time.time() - t0 < SECONDS:
        for _ in range(20):
            y.zero_()
            plan.reset(); plan.process(x if nchan > 1 else x[0], out=y if nchan > 1 else y[0])
            bad += int((torch.view_as_real(y).view(torch.int32) != ref_words).any().item())
            launches += 1
    print("x%-3d %d ch 2^%d: %s, %d tiles x%d, %d workgroups on %d slots: first launch %s the oracle; %d launches, %d differ" % (
        ratio, nchan, lg, g["kernel"], g["n_tiles"], g["split"], g["workgroups"], g["resident"],
        "equals" if ok0 else "DIFFERS FROM", launches, bad), flush=True)
    total_launches += launches; total_bad += bad + (0 if ok0 else 1)
    plan.close(); del x, y, y0
print("total: %d launches, %d bad" % (total_launches, total_bad))
sys.exit(1 if total_bad else 0)
