"""The rational 4/5 x 128 pass (resample45_kernel) against what it replaces and against the plan's own generic kernel.

    python3 tools/ratbench.py [--log2n 26] [--log2big 28] [--iters 20] [--rounds 3] [--generations 4,8,16,32]

One process, resident CF32 buffers, sxfir_time_resample / sxfir_time_interpolate (HIP events around back-to-back launches), the
plans alternated round by round on the same box.

  (a) the tiled 4/5 pass over 2^log2n inputs, one channel, against the shipped x4 x 128 real-tap pass (interp8_pass_kernel<4, L = 4>)
      over the same inputs: the x4 pass ALONE is a lower bound of the two-pass route (x4, then /5), which still has to drop four of
      every five samples.  Per round the ratio t(4/5) / t(x4); the condition is < 1.
  (b) the same call under SXFIR_KERNEL_GENERIC (resample_generic_kernel): per round the ratio t(tiled) / t(generic); < 1 or the
      tiled kernel has no reason to ship.
  (c) the tiled pass over 2^log2big inputs: ms, algorithmic bytes (8 read + 6.4 written per input sample), fraction of 8 TB/s.
      Reported, not gated.

--generations: the form row's generations per launch, swept with the profiling library's SXFIR_OVERSUB knob at 2^log2n inputs
(what FORM_RAT45's figure was chosen from).  profiles/rational.txt keeps the output with the box id.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sxxcvr_amd  # noqa: E402
from sxxcvr_amd.resampler import INTERPOLATE, KERNEL_GENERIC, KERNEL_TILED  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--log2big", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--generations", default="")
    args = ap.parse_args()
    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    print("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))

    n, big = 1 << args.log2n, 1 << args.log2big
    x = torch.empty(max(n, big), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty(max(4 * n, -(-4 * big // 5)), dtype=torch.complex64, device="cuda")
    h = sxxcvr_amd.design_rational(4, 5)
    plans = {"4/5 tiled": sxxcvr_amd.RationalResampler(h, 4, 5), "4/5 generic": sxxcvr_amd.RationalResampler(h, 4, 5),
             "x4": sxxcvr_amd.Resampler(INTERPOLATE, sxxcvr_amd.design_lowpass(128, 4, 8.0, 4.0), 4)}
    plans["4/5 tiled"].set_kernel(KERNEL_TILED)
    plans["4/5 generic"].set_kernel(KERNEL_GENERIC)
    plans["x4"].set_kernel(KERNEL_TILED)

    def t(k, count, iters):
        return plans[k].time_passes_ptr(x.data_ptr(), count, count, y.data_ptr(), y.numel(), iters)

    for k, p in plans.items():
        print("%-12s %s" % (k, p.geometry(n)))
        t(k, n, 3)                                                       # warm-up
    torch.cuda.synchronize()
    ms = {k: [] for k in plans}
    for r in range(args.rounds):
        for k in plans:
            ms[k].append(t(k, n, args.iters if k != "4/5 generic" else max(2, args.iters // 4)))
            print("round %d %-12s %.4f ms over 2^%d inputs" % (r, k, ms[k][-1], args.log2n))
        print("round %d (a) ratio 4/5 tiled / x4 pass %.3f (the condition: < 1)" % (r, ms["4/5 tiled"][-1] / ms["x4"][-1]))
        print("round %d (b) ratio 4/5 tiled / 4/5 generic %.3f (the condition: < 1)" % (r, ms["4/5 tiled"][-1] / ms["4/5 generic"][-1]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print("median (a) 4/5 tiled %.4f ms, x4 pass %.4f ms, ratio %.3f: %s" % (
        med["4/5 tiled"], med["x4"], med["4/5 tiled"] / med["x4"], "met" if all(a < b for a, b in zip(ms["4/5 tiled"], ms["x4"])) else "NOT met"))
    print("median (b) 4/5 tiled %.4f ms, 4/5 generic %.4f ms, ratio %.3f: %s" % (
        med["4/5 tiled"], med["4/5 generic"], med["4/5 tiled"] / med["4/5 generic"],
        "met" if all(a < b for a, b in zip(ms["4/5 tiled"], ms["4/5 generic"])) else "NOT met"))
    print("(c) %s" % plans["4/5 tiled"].geometry(big))
    t("4/5 tiled", big, 3)
    for r in range(args.rounds):
        v = t("4/5 tiled", big, args.iters)
        gb = 14.4 * big / 1e9
        print("round %d (c) 4/5 tiled %.4f ms over 2^%d inputs  %.3f GB  %.3f of 8 TB/s  %.1f TFLOP/s" % (
            r, v, args.log2big, gb, gb * 1e9 / (v * 1e-3) / 8e12, 0.8 * 128.0 * big / (v * 1e-3) / 1e12))

    if args.generations:
        for g in [int(v) for v in args.generations.split(",")]:
            os.environ["SXFIR_OVERSUB"] = str(g)
            p = sxxcvr_amd.RationalResampler(h, 4, 5, profiling=True)
            del os.environ["SXFIR_OVERSUB"]
            p.set_kernel(KERNEL_TILED)
            p.time_passes_ptr(x.data_ptr(), n, n, y.data_ptr(), y.numel(), 3)
            v = [p.time_passes_ptr(x.data_ptr(), n, n, y.data_ptr(), y.numel(), args.iters) for _ in range(args.rounds)]
            print("generations %-3d workgroups %-6d resident %-5d  %s ms over 2^%d inputs" % (
                g, p.geometry(n)["workgroups"], p.geometry(n)["resident"], " ".join("%.4f" % q for q in v), args.log2n))


if __name__ == "__main__":
    main()
