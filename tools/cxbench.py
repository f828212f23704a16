"""Complex-tap /4 decimator against the only route the real-tap kernels offer for the same band: two real /4 passes.

    python3 tools/cxbench.py [rx] [--log2n 28] [--iters 20] [--rounds 3]
    python3 tools/cxbench.py tx [--log2n 28] [--iters 20] [--rounds 3]
    python3 tools/cxbench.py mix [--log2n 28] [--iters 20] [--rounds 3] [--num 123 --den 1000]
    python3 tools/cxbench.py mixtx [--log2n 28] [--iters 20] [--rounds 3] [--num 123 --den 1000]

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

`mix`: the translating /4 x 128 plan (include/sxfir_translate.h, decim4_cx_kernel<MixTileArgs>: the launch geometry's decim4_mix_kernel) against the route it replaces at that route's
lower bound -- per round (a) the translating plan, (b) the complex plan of the same taps (decim4_cx_kernel), (c) a device-to-device
copy of the n / 4 output samples: 8 B read and 8 B written per output, the traffic floor of any separate rotation pass.  The
condition is (a) < (b) + (c) in every round; (a) / (b) per round and its median say what the fused rotation costs.
profiles/cx_mix.txt keeps the output.

`mixtx`: the translating interpolators (include/sxfir_translate_tx.h, interp_cx_pass_kernel<.., InterpMixTileArgs>: the launch geometry's interp_mix_pass_kernel) the same way -- x4 x 128 and x8 x 256,
n CF32 OUTPUT samples, sxfir_time_interpolate, per round (a) the translating plan, (b) the ComplexInterpolator plan of the same taps
(interp_cx_pass_kernel), (c) a device-to-device copy of the call's n / ratio INPUT samples: the traffic floor of the separate
rotation pass the old route needs in front of (b).  The condition is (a) < (b) + (c) in every round.  profiles/cx_mix_tx.txt keeps
the output.
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


def mix(args, n):
    """/4 x 128 on n resident inputs: translating plan, complex plan of the same taps, and a copy of the output."""
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty(n // 4, dtype=torch.complex64, device="cuda")
    y2 = torch.empty_like(y)
    taps = sxxcvr_amd.design_bandpass(128, 4, args.num, args.den)
    plans = {"mix": sxxcvr_amd.TranslatingDecimator(taps, 4, args.num, args.den), "complex": sxxcvr_amd.Resampler(DECIMATE, taps, 4)}
    for k, p in plans.items():
        p.set_kernel(KERNEL_TILED)
        print("%-8s %s" % (k, p.geometry(n)))
        p.time_decimate_ptr(x.data_ptr(), n, n, y.data_ptr(), n // 4, 3)          # warm-up
    print("band centre %d / %d: %d table entries per output" % (plans["mix"].num, plans["mix"].den, plans["mix"].num * 4 % plans["mix"].den))

    def copy_ms(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            y2.copy_(y)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    copy_ms(3)
    torch.cuda.synchronize()
    ratios, ok = [], True
    for r in range(args.rounds):
        a = plans["mix"].time_decimate_ptr(x.data_ptr(), n, n, y.data_ptr(), n // 4, args.iters)
        b = plans["complex"].time_decimate_ptr(x.data_ptr(), n, n, y.data_ptr(), n // 4, args.iters)
        c = copy_ms(args.iters)
        ratios.append(a / b)
        ok = ok and a < b + c
        print("round %d (a) mix %.4f ms  (b) complex %.4f ms  (c) copy of the output %.4f ms (%.3f of 8 TB/s)  (b) + (c) %.4f ms  (a) / (b) %.3f  (a) < (b) + (c): %s" % (
            r, a, b, c, 16.0 * (n // 4) / (c * 1e-3) / 8e12, b + c, a / b, a < b + c))
    print("median (a) / (b) %.3f; (a) < (b) + (c) in every round: %s" % (statistics.median(ratios), ok))


def mixtx(args, n):
    """x4 x 128 and x8 x 256 on n resident outputs: translating plan, complex plan of the same taps, and a copy of the input."""
    y = torch.empty(n, dtype=torch.complex64, device="cuda")
    for L in (4, 8):
        n_in = n // L
        x = torch.empty(n_in, dtype=torch.complex64, device="cuda")
        sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
        x2 = torch.empty_like(x)
        taps = sxxcvr_amd.design_bandpass(32 * L, L, args.num, args.den, gain=L)
        plans = {"mix": sxxcvr_amd.TranslatingInterpolator(taps, L, args.num, args.den), "complex": sxxcvr_amd.ComplexInterpolator(taps, L)}
        for k, p in plans.items():
            p.set_kernel(KERNEL_TILED)
            print("x%d %-8s %s" % (L, k, p.geometry(n_in)))
            p.time_passes_ptr(x.data_ptr(), n_in, n_in, y.data_ptr(), n, 3)          # warm-up
        print("x%d band centre %d / %d: %d table entries per input" % (L, plans["mix"].num, plans["mix"].den, plans["mix"].num * L % plans["mix"].den))

        def copy_ms(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                x2.copy_(x)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        copy_ms(3)
        torch.cuda.synchronize()
        ratios, ok = [], True
        for r in range(args.rounds):
            a = plans["mix"].time_passes_ptr(x.data_ptr(), n_in, n_in, y.data_ptr(), n, args.iters)
            b = plans["complex"].time_passes_ptr(x.data_ptr(), n_in, n_in, y.data_ptr(), n, args.iters)
            c = copy_ms(args.iters)
            ratios.append(a / b)
            ok = ok and a < b + c
            print("x%d round %d (a) mix %.4f ms  (b) complex %.4f ms  (c) copy of the input %.4f ms (%.3f of 8 TB/s)  (b) + (c) %.4f ms  (a) / (b) %.3f  (a) < (b) + (c): %s" % (
                L, r, a, b, c, 16.0 * n_in / (c * 1e-3) / 8e12, b + c, a / b, a < b + c))
        print("x%d median (a) / (b) %.3f; (a) < (b) + (c) in every round: %s" % (L, statistics.median(ratios), ok))
        del x, x2, plans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="rx", choices=["rx", "tx", "mix", "mixtx"])
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--num", type=int, default=123)
    ap.add_argument("--den", type=int, default=1000)
    args = ap.parse_args()
    n = 1 << args.log2n
    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    print("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))
    if args.mode == "tx":
        return tx(args, n)
    if args.mode == "mix":
        return mix(args, n)
    if args.mode == "mixtx":
        return mixtx(args, n)
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
