"""The tuner bank (include/sxfir_bank.h) against the route it replaces: K translating decimators, one pass each.

    python3 tools/bankbench.py [--log2n 28] [--iters 10] [--rounds 3] [--bands 1,2,4,8] [--out profiles/bank.txt]

/4 x 128 on CF32 over n = 2^log2n resident inputs (n / 4 outputs per band), HIP events around back-to-back launches
(sxfir_time_decimate_bank, sxfir_time_decimate).  For every K the plans are warmed up, then alternated on the same box in rounds:
(a) the bank's one pass (decim4_bank_kernel), (b) the K TranslatingDecimator passes of the same taps and centres over the same
input (decim4_mix_kernel), one after the other -- their SUM is what the bank replaces --, and (c) K times the single pass of band 0.
The condition is (a) < (b) in EVERY round; (a) / (b) and (a) / (c) per round and their medians say what the shared staging saves
(K > 1) and what the band loop and the quarter-tile transposition cost (K = 1).  Once per K the bank's generic kernel
(decim_bank_generic_kernel) is timed too: what AUTO's choice of the tiled kernel is worth.

Per run: ms, the algorithmic bytes (8 B per input sample read once, 8 K / 4 B written) and their fraction of 8 TB/s -- derived from the
shapes, not measured --, TFLOP/s (256 flop per input sample and band).  With --out the lines are also written to that file.
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bands", default="1,2,4,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = 1 << args.log2n
    n_out = n // 4
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    say("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))
    say("tools/bankbench.py --log2n %d --iters %d --rounds %d --bands %s" % (args.log2n, args.iters, args.rounds, args.bands))
    bands = [int(k) for k in args.bands.split(",")]
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty((max(bands), n_out), dtype=torch.complex64, device="cuda")
    verdict = {}
    for K in bands:
        centres = CENTRES[:K]
        taps = np.stack([sxxcvr_amd.design_bandpass(128, 4, num, den) for num, den in centres])
        bank = sxxcvr_amd.TranslatingBank(taps, 4, centres)
        bank.set_kernel(KERNEL_TILED)
        generic = sxxcvr_amd.TranslatingBank(taps, 4, centres)
        generic.set_kernel(KERNEL_GENERIC)
        singles = [sxxcvr_amd.TranslatingDecimator(taps[k], 4, num, den) for k, (num, den) in enumerate(centres)]
        for p in singles:
            p.set_kernel(KERNEL_TILED)
        say("K = %d  bank    %s" % (K, bank.geometry(n)))
        say("K = %d  single  %s" % (K, singles[0].geometry(n)))
        say("K = %d  generic %s" % (K, generic.geometry(n)))

        def bank_ms(plan, iters):
            return plan.time_ptr(x.data_ptr(), n, n, y.data_ptr(), 0, n_out, iters)

        def single_ms(k, iters):
            return singles[k].time_decimate_ptr(x.data_ptr(), n, n, y[k].data_ptr(), n_out, iters)

        bank_ms(bank, 3)                                            # warm-up of every shape the rounds time
        for k in range(K):
            single_ms(k, 3)
        torch.cuda.synchronize()
        gb = (8.0 + 2.0 * K) * n / 1e9
        ra, rc, ok = [], [], True
        for r in range(args.rounds):
            a = bank_ms(bank, args.iters)
            each = [single_ms(k, args.iters) for k in range(K)]
            b = sum(each)
            c = K * each[0]
            ra.append(a / b)
            rc.append(a / c)
            ok = ok and a < b
            say("K = %d round %d (a) bank %.4f ms (%.3f GB, %.3f of 8 TB/s, %.1f TFLOP/s)  (b) sum of %d single passes %.4f ms  (c) %d x single %.4f ms  "
                "(a) / (b) %.4f  (a) / (c) %.4f  (a) < (b): %s" % (K, r, a, gb, gb * 1e9 / (a * 1e-3) / 8e12, 256.0 * K * n / (a * 1e-3) / 1e12, K, b, K, c,
                                                                  a / b, a / c, a < b))
        g = bank_ms(generic, 2)
        a = bank_ms(bank, args.iters)
        say("K = %d generic kernel %.4f ms, tiled %.4f ms in the same breath: generic / tiled %.2f" % (K, g, a, g / a))
        say("K = %d median (a) / (b) %.4f  median (a) / (c) %.4f  (a) < (b) in every round: %s" % (K, statistics.median(ra), statistics.median(rc), ok))
        verdict[K] = ok
        del bank, generic, singles
    if 4 in verdict:
        say("condition (one bank pass at K = 4 below the sum of the four single passes, in every round): %s" % ("met" if verdict[4] else "NOT met"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
