"""Complex-tap /4 decimator against the only route the real-tap kernels offer for the same band: two real /4 passes.

    python3 tools/cxbench.py [rx] [--log2n 28] [--iters 20] [--rounds 3]
    python3 tools/cxbench.py tx [--log2n 28] [--iters 20] [--rounds 3]

2^28 resident CF32 samples, sxfir_time_decimate (HIP events around back-to-back launches).  The complex /4 x 128 plan
(decim4_cx_kernel) and the real /4 x 128 plan (decim4_wide_kernel) are alternated on the same box, three alternations.  Per
run: ms, algorithmic bytes (10 B per input sample, as BASELINE config 2: 8 read, 8/4 written), fraction of 8 TB/s, TFLOP/s
(real: 128 flop per input sample = 128 taps x 2 components x 2 flop / 4; complex: 256).  Last lines: the medians and the ratio
complex / real -- 2.0 is "two real passes", without the combining pass those would still need.
profiles/cx_decim4.txt keeps the output with the box id.

`tx`: the complex-tap interpolators (include/sxfir_complex_tx.h) the same way -- x4 x 128 and x8 x 256, 2^28 resident CF32 OUTPUT
samples, sxfir_time_interpolate; the complex plan (interp_cx_pass_kernel) and the real-tap plan of the same shape
(interp8_pass_kernel) alternated three times on the same box.  Per run: ms, algorithmic bytes (8 + 8 / ratio per output sample),
TFLOP/s (real: 128 flop per output sample = 32 taps x 2 components x 2 flop; complex: 256), and per round the ratio complex / real
-- 2.0 is "two real passes", without the combining pass those would still need.  profiles/cx_interp.txt keeps the output.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sxxcvr_amd  # noqa: E402
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE, KERNEL_TILED  # noqa: E402


def tx(args, n):
    """x4 and x8: n output samples, the complex plan against the real-tap plan of the same shape."""
    y = torch.empty(n, dtype=torch.complex64, device="cuda")
    for L in (4, 8):
        n_in = n // L
        x = torch.empty(n_in, dtype=torch.complex64, device="cuda")
        sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
        plans = {"real": sxxcvr_amd.Resampler(INTERPOLATE, sxxcvr_amd.design_lowpass(32 * L, L, 8.0, float(L)), L),
                 "complex": sxxcvr_amd.ComplexInterpolator(sxxcvr_amd.design_bandpass(32 * L, L, 1, L, gain=L), L)}
        flop = {"real": 128.0, "complex": 256.0}
        gb = (8.0 + 8.0 / L) * n / 1e9
        for k, p in plans.items():
            p.set_kernel(KERNEL_TILED)
            print("x%d %-8s %s" % (L, k, p.geometry(n_in)))
            p.time_passes_ptr(x.data_ptr(), n_in, n_in, y.data_ptr(), n, 3)          # warm-up
        torch.cuda.synchronize()
        ms = {"real": [], "complex": []}
        for r in range(args.rounds):
            for k in ("complex", "real"):
                t = plans[k].time_passes_ptr(x.data_ptr(), n_in, n_in, y.data_ptr(), n, args.iters)
                ms[k].append(t)
                print("x%d round %d %-8s %.4f ms  %.3f GB  %.3f of 8 TB/s  %.1f TFLOP/s" % (
                    L, r, k, t, gb, gb * 1e9 / (t * 1e-3) / 8e12, flop[k] * n / (t * 1e-3) / 1e12))
            print("x%d round %d ratio complex / real %.3f" % (L, r, ms["complex"][-1] / ms["real"][-1]))
        mr, mc = statistics.median(ms["real"]), statistics.median(ms["complex"])
        print("x%d median real %.4f ms (%.1f TFLOP/s)  complex %.4f ms (%.1f TFLOP/s)  ratio %.3f (two real passes = 2.000)" % (
            L, mr, 128.0 * n / (mr * 1e-3) / 1e12, mc, 256.0 * n / (mc * 1e-3) / 1e12, mc / mr))
        del x, plans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="rx", choices=["rx", "tx"])
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
    if args.mode == "tx":
        return tx(args, n)
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
