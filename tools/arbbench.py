"""The arbitrary-rate 128 x 32 pass (resample_arb_kernel) against the plan's own generic kernel and against the rational 4/5 x 128
plan, which has the same taps per phase and the same rates and half the chains.

    python3 tools/arbbench.py [--log2n 26] [--iters 20] [--rounds 3] [--step 0x140000000]

One process, resident CF32 buffers, sxfir_time_resample_arbitrary / sxfir_time_resample (HIP events around back-to-back launches),
the alternatives alternated round by round on the same box, after a warm-up of each.

  (a) the tiled arbitrary-rate pass over 2^log2n inputs at step 5 * 2^30 (4 outputs for 5 inputs), one channel;
  (b) the same call under SXFIR_KERNEL_GENERIC (resample_arb_generic_kernel);
  (c) the rational 4/5 x 128 plan under SXFIR_KERNEL_GENERIC (resample_generic_kernel) over the same inputs;
  (d) the rational 4/5 x 128 plan under SXFIR_KERNEL_TILED (resample45_kernel) over the same inputs.

Conditions: (a) < (c) in every round; AUTO takes the tiled form only if (a) < (b) in every round.  Reported without a condition:
(a) / (d) -- (d) keeps its taps in SGPRs, this kernel cannot -- and (a)'s algorithmic bytes (8 read per input + 8 written per
output) over its time as a share of 8 TB/s.  profiles/arbitrary.txt keeps the output with the box id.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sxxcvr_amd  # noqa: E402
from sxxcvr_amd.resampler import KERNEL_GENERIC, KERNEL_TILED  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", type=lambda v: int(v, 0), default=5 << 30)
    args = ap.parse_args()
    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    print("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))

    n = 1 << args.log2n
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    ha = sxxcvr_amd.design_arbitrary(128, 32, rate=(1 << 32) / args.step)
    hr = sxxcvr_amd.design_rational(4, 5)
    plans = {"(a) arbitrary tiled": sxxcvr_amd.ArbitraryResampler(ha, 128, step=args.step),
             "(b) arbitrary generic": sxxcvr_amd.ArbitraryResampler(ha, 128, step=args.step),
             "(c) 4/5 generic": sxxcvr_amd.RationalResampler(hr, 4, 5),
             "(d) 4/5 tiled": sxxcvr_amd.RationalResampler(hr, 4, 5)}
    plans["(a) arbitrary tiled"].set_kernel(KERNEL_TILED)
    plans["(b) arbitrary generic"].set_kernel(KERNEL_GENERIC)
    plans["(c) 4/5 generic"].set_kernel(KERNEL_GENERIC)
    plans["(d) 4/5 tiled"].set_kernel(KERNEL_TILED)
    n_out = max(p.outputs_for(n) for p in plans.values())
    y = torch.empty(n_out + 8, dtype=torch.complex64, device="cuda")

    def t(k, iters):
        return plans[k].time_passes_ptr(x.data_ptr(), n, n, y.data_ptr(), y.numel(), iters)

    for k, p in plans.items():
        print("%-22s %s" % (k, p.geometry(n)))
        t(k, 3)                                                          # warm-up
    torch.cuda.synchronize()
    ms = {k: [] for k in plans}
    a, b, c, d = list(plans)
    for r in range(args.rounds):
        for k in plans:
            ms[k].append(t(k, args.iters))
            print("round %d %-22s %.4f ms over 2^%d inputs, %d passes" % (r, k, ms[k][-1], args.log2n, args.iters))
        print("round %d (a)/(c) %.3f (the condition: < 1)   (a)/(b) %.3f (AUTO takes the tiled form if < 1)   (a)/(d) %.3f (reported)" % (
            r, ms[a][-1] / ms[c][-1], ms[a][-1] / ms[b][-1], ms[a][-1] / ms[d][-1]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for other, what in ((c, "the condition"), (b, "AUTO takes the tiled form")):
        print("median %s %.4f ms, %s %.4f ms, ratio %.3f: %s, %s in every round" % (
            a, med[a], other, med[other], med[a] / med[other], what, "met" if all(p < q for p, q in zip(ms[a], ms[other])) else "NOT met"))
    print("median (a)/(d) %.3f (reported: (d) keeps its taps in SGPRs and runs one chain per output)" % (med[a] / med[d]))
    gb = 8.0 * (n + plans[a].outputs_for(n)) / 1e9
    print("(a) %.3f GB read and written in %.4f ms: %.3f of 8 TB/s -- LDS, not HBM, bounds it; %.1f TFLOP/s of FMAs" % (
        gb, med[a], gb * 1e9 / (med[a] * 1e-3) / 8e12, 4.0 * 64 * plans[a].outputs_for(n) / (med[a] * 1e-3) / 1e12))


if __name__ == "__main__":
    main()
