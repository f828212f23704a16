"""The combiner bank (include/sxfir_bank_tx.h) against the route it replaces: K translating interpolators, one wideband pass each,
and K - 1 add passes.

    python3 tools/combbench.py [--log2n 28] [--iters 10] [--rounds 5] [--bands 1,2,4,8] [--out profiles/bank_tx.txt]

x4 x 128 on CF32 to n = 2^log2n resident OUTPUTS (n / 4 inputs per band), HIP events around back-to-back launches
(sxfir_time_interpolate_bank, sxfir_time_interpolate).  For every K the plans are warmed up, then alternated on the same box in
rounds: (a) the combiner's one pass (interp4_bank_kernel), (b) the K TranslatingInterpolator passes of the same taps and centres over
the same inputs (interp_mix_pass_kernel), one after the other, summed -- a LOWER bound of the old route, whose K - 1 adds are left
out of it --, and (c) one device-to-device copy that moves an add pass's bytes (an add reads two wideband streams and writes one:
24 B per output; the copy reads and writes 1.5 n samples), stated as the floor of one of those K - 1 adds.  The condition is
(a) < (b) in EVERY round at K = 4; (a) / ((b) + (K - 1) (c)) is reported beside it.  Once per K the combiner's generic kernel
(interp_bank_generic_kernel) is timed too: what AUTO's choice of the tiled kernel is worth.

Per run: ms, the algorithmic bytes (8 B per input sample and band read once, 8 B per output written once) and their fraction of
8 TB/s -- derived from the shapes, not measured --, TFLOP/s (256 flop per output and band).  With --out the lines are also written to
that file.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sxxcvr_amd  # noqa: E402
from sxxcvr_amd.resampler import KERNEL_GENERIC, KERNEL_TILED  # noqa: E402

CENTRES = [(123, 1000), (3, 7), (12345, 65536), (5, 16), (77, 256), (1, 3), (65535, 65536), (999, 4093),
           (1, 5), (2, 9), (7, 11), (12, 13), (100, 1001), (9, 31), (4093, 4096), (1, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bands", default="1,2,4,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = 1 << args.log2n
    n_in = n // 4
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    say("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))
    say("tools/combbench.py --log2n %d --iters %d --rounds %d --bands %s" % (args.log2n, args.iters, args.rounds, args.bands))
    bands = [int(k) for k in args.bands.split(",")]
    x = torch.empty((max(bands), n_in), dtype=torch.complex64, device="cuda")
    for k in range(max(bands)):
        sxxcvr_amd.synth_fill(x[k], 0x51255 + k, 0, 0)
    y = torch.empty(n, dtype=torch.complex64, device="cuda")
    # the add-sized copy: 1.5 n samples read and 1.5 n written = the 24 B per output of an add pass
    src = torch.zeros(n + n // 2, dtype=torch.complex64, device="cuda")
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy_ms(iters):
        e0.record()
        for _ in range(iters):
            dst.copy_(src)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    copy_ms(3)
    verdict = {}
    for K in bands:
        centres = CENTRES[:K]
        taps = np.stack([sxxcvr_amd.design_bandpass(128, 4, 0, 1, gain=4.0) for _ in centres])
        comb = sxxcvr_amd.TranslatingCombiner(taps, 4, centres)
        comb.set_kernel(KERNEL_TILED)
        generic = sxxcvr_amd.TranslatingCombiner(taps, 4, centres)
        generic.set_kernel(KERNEL_GENERIC)
        singles = [sxxcvr_amd.TranslatingInterpolator(taps[k], 4, num, den) for k, (num, den) in enumerate(centres)]
        for p in singles:
            p.set_kernel(KERNEL_TILED)
        say("K = %d  combiner %s" % (K, comb.geometry(n_in)))
        say("K = %d  single   %s" % (K, singles[0].geometry(n_in)))
        say("K = %d  generic  %s" % (K, generic.geometry(n_in)))

        def comb_ms(plan, iters):
            return plan.time_ptr(x.data_ptr(), n_in, 0, n_in, y.data_ptr(), n, iters)

        def single_ms(k, iters):
            return singles[k].time_passes_ptr(x[k].data_ptr(), n_in, n_in, y.data_ptr(), n, iters)

        comb_ms(comb, 3)                                            # warm-up of every shape the rounds time
        for k in range(K):
            single_ms(k, 3)
        torch.cuda.synchronize()
        gb = (8.0 + 2.0 * K) * n / 1e9
        ra, rf, ok = [], [], True
        for r in range(args.rounds):
            a = comb_ms(comb, args.iters)
            b = sum(single_ms(k, args.iters) for k in range(K))
            c = copy_ms(args.iters)
            full = b + (K - 1) * c
            ra.append(a / b)
            rf.append(a / full)
            ok = ok and a < b
            say("K = %d round %d (a) combiner %.4f ms (%.3f GB, %.3f of 8 TB/s, %.1f TFLOP/s)  (b) sum of %d single passes %.4f ms  (c) add-sized copy %.4f ms  "
                "(a) / (b) %.4f  (a) / ((b) + %d (c)) %.4f  (a) < (b): %s" % (K, r, a, gb, gb * 1e9 / (a * 1e-3) / 8e12, 256.0 * K * n / (a * 1e-3) / 1e12, K, b, c,
                                                                             a / b, K - 1, a / full, a < b))
        g = comb_ms(generic, 1)
        a = comb_ms(comb, args.iters)
        say("K = %d generic kernel %.4f ms, tiled %.4f ms in the same breath: generic / tiled %.2f" % (K, g, a, g / a))
        say("K = %d median (a) / (b) %.4f  median (a) / ((b) + (K - 1) (c)) %.4f  (a) < (b) in every round: %s" % (
            K, statistics.median(ra), statistics.median(rf), ok))
        verdict[K] = ok
        del comb, generic, singles
    if 4 in verdict:
        say("condition (one combiner pass at K = 4 below the sum of the four single passes, in every round): %s" % ("met" if verdict[4] else "NOT met"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
