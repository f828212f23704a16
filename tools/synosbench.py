"""The 2x oversampled 4-band synthesizer against the route the critically sampled one offers for the same bands: two passes.

    python3 tools/synosbench.py [--log2n 28] [--iters 10] [--rounds 3]

2^28 wideband CF32 output samples (2^27 inputs per band at fs/2).  Three legs are alternated on the same box, three alternations:
    real     one real-tap x4 x 128 pass (interp8_pass_kernel<4, ..., 4>), for scale
    2 x syn  two critically sampled synthesizer passes (synthesis4_kernel) over 2^26 inputs per band each -- the even and the odd
             times of the bands -- each writing a full-length wideband stream: the old route's arithmetic and its two wideband
             writes.  A LOWER bound of the old cost: the split into even and odd times, the negation of bands 1 and 3 of the odd
             half and the pass that delays one wideband stream by two samples and adds the two are left out
    syn4x2   one oversampled pass (synthesis4x2_kernel)
Every leg is `iters` back-to-back streaming calls (sxfir_interpolate / sxfir_synthesize) between two HIP events on the launch
stream (StreamTimer); a leg's figure is the mean per set of bands.  Per run: ms and, for the oversampled synthesizer, its
algorithmic bytes (4 x 8/2 B read + 8 B written per output sample: 4 GiB in + 2 GiB out at 2^28; the two passes move 8 GiB) over
time as a fraction of 8 TB/s.  Last lines: the medians, the ratios and the range of the per-round ratio.  profiles/syn4x2.txt
keeps the output with the box id.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sxxcvr_amd  # noqa: E402
from sxxcvr_amd.resampler import INTERPOLATE, KERNEL_TILED, StreamTimer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    n = 1 << args.log2n                                     # wideband output samples
    m = n // 2                                              # inputs per band at fs/2
    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    print("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))
    x = torch.empty((4, m), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty((2, n), dtype=torch.complex64, device="cuda")          # a wideband stream per critically sampled pass
    stream = torch.cuda.current_stream().cuda_stream
    timer = StreamTimer(stream)
    real = sxxcvr_amd.Resampler(INTERPOLATE, sxxcvr_amd.design_lowpass(128, 4, 8.0, 4.0), 4)
    crit = [sxxcvr_amd.Synthesizer(sxxcvr_amd.design_lowpass(128, 4, 8.0, 4.0)) for _ in range(2)]
    syn_os = sxxcvr_amd.Synthesizer(sxxcvr_amd.design_lowpass(128, 4, 8.0, 2.0), oversample=2)
    for label, p, n_in in [("real", real, n // 4), ("syn even", crit[0], n // 4), ("syn odd", crit[1], n // 4), ("syn4x2", syn_os, m)]:
        p.set_kernel(KERNEL_TILED)
        print("%-9s %s" % (label, p.geometry(n_in)))

    def two_passes():
        for k, p in enumerate(crit):                        # (each pass a half of every band: the volume of the even / odd times)
            p.process_ptr(x.data_ptr() + 8 * k * (m // 2), m // 2, 0, m, y.data_ptr() + 8 * k * n, n, stream)

    legs = {"real": lambda: real.process_ptr(x.data_ptr(), n // 4, n // 4, y.data_ptr(), n, stream),
            "2 x syn": two_passes,
            "syn4x2": lambda: syn_os.process_ptr(x.data_ptr(), m, 0, m, y.data_ptr(), n, stream)}

    def timed(leg, iters):
        timer.start()
        for _ in range(iters):
            legs[leg]()
        timer.stop()
        torch.cuda.synchronize()
        return timer.elapsed_ms() / iters

    for leg in legs:
        timed(leg, 2)                                       # warm-up
    os_bytes = 24.0 * n
    ms = {leg: [] for leg in legs}
    for r in range(args.rounds):
        for leg in ("syn4x2", "2 x syn", "real"):
            t = timed(leg, args.iters)
            ms[leg].append(t)
            tail = "  %.3f GB  %.3f of 8 TB/s" % (os_bytes / 1e9, os_bytes / (t * 1e-3) / 8e12) if leg == "syn4x2" else ""
            print("round %d %-8s %.4f ms%s" % (r, leg, t, tail))
    mr, mb, mc = (statistics.median(ms[leg]) for leg in ("real", "2 x syn", "syn4x2"))
    per_round = [c / b for c, b in zip(ms["syn4x2"], ms["2 x syn"])]
    print("median real x4 %.4f ms  2 x synthesizer %.4f ms  oversampled synthesizer %.4f ms (%.3f of 8 TB/s)" % (mr, mb, mc, os_bytes / (mc * 1e-3) / 8e12))
    print("ratio syn4x2 / (2 x syn) %.3f (per round %.3f .. %.3f)   syn4x2 / real %.3f   (2 x syn) / real %.3f" % (
        mc / mb, min(per_round), max(per_round), mc / mr, mb / mr))


if __name__ == "__main__":
    main()
