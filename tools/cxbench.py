"""Complex-tap /4 decimator against the only route the real-tap kernels offer for the same band: two real /4 passes.

    python3 tools/cxbench.py [--log2n 28] [--iters 20] [--rounds 3]

2^28 resident CF32 samples, sxfir_time_decimate (HIP events around back-to-back launches).  The complex /4 x 128 plan
(decim4_cx_kernel) and the real /4 x 128 plan (decim4_wide_kernel) are alternated on the same box, three alternations.  Per
run: ms, algorithmic bytes (10 B per input sample, as BASELINE config 2: 8 read, 8/4 written), fraction of 8 TB/s, TFLOP/s
(real: 128 flop per input sample = 128 taps x 2 components x 2 flop / 4; complex: 256).  Last lines: the medians and the ratio
complex / real -- 2.0 is "two real passes", without the combining pass those would still need.
profiles/cx_decim4.txt keeps the output with the box id.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sxxcvr_amd  # noqa: E402
from sxxcvr_amd.resampler import DECIMATE, KERNEL_TILED  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    n = 1 << args.log2n
    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    print("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty(n // 4, dtype=torch.complex64, device="cuda")
    plans = {"real": sxxcvr_amd.Resampler(DECIMATE, sxxcvr_amd.design_lowpass(128, 4), 4),
             "complex": sxxcvr_amd.Resampler(DECIMATE, sxxcvr_amd.design_bandpass(128, 4, 1, 4), 4)}
    flop = {"real": 128.0, "complex": 256.0}
    for k, p in plans.items():
        p.set_kernel(KERNEL_TILED)
        print("%-8s %s" % (k, p.geometry(n)))
        p.time_decimate_ptr(x.data_ptr(), n, n, y.data_ptr(), n // 4, 3)          # warm-up
    torch.cuda.synchronize()
    ms = {"real": [], "complex": []}
    for r in range(args.rounds):
        for k in ("complex", "real"):
            t = plans[k].time_decimate_ptr(x.data_ptr(), n, n, y.data_ptr(), n // 4, args.iters)
            ms[k].append(t)
            print("round %d %-8s %.4f ms  %.3f GB  %.3f of 8 TB/s  %.1f TFLOP/s" % (
                r, k, t, 10.0 * n / 1e9, 10.0 * n / (t * 1e-3) / 8e12, flop[k] * n / (t * 1e-3) / 1e12))
    mr, mc = statistics.median(ms["real"]), statistics.median(ms["complex"])
    print("median real /4 %.4f ms (%.1f TFLOP/s)  complex /4 %.4f ms (%.1f TFLOP/s)  ratio %.3f (two real passes = 2.000)" % (
        mr, 128.0 * n / (mr * 1e-3) / 1e12, mc, 256.0 * n / (mc * 1e-3) / 1e12, mc / mr))


if __name__ == "__main__":
    main()
