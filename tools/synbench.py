"""The 4-band synthesizer against the route the real-tap kernels offer for the same four bands: four real x4 passes.

    python3 tools/synbench.py [--log2n 28] [--iters 10] [--rounds 3]

2^28 wideband CF32 output samples (2^26 inputs per band).  Three legs are alternated on the same box, three alternations:
    real     one real-tap x4 x 128 pass (interp8_pass_kernel<4, ..., 4>): the arithmetic the synthesizer does, a quarter of its input
    4 x real four real-tap x4 passes, one per band, each writing a wideband stream of its own: what the synthesis replaces -- a LOWER
             bound of the old cost, which leaves out the caller's rotation of bands 1..3 and the sum of the four streams
    syn      one synthesizer pass (synthesis4_kernel)
Every leg is `iters` back-to-back streaming calls (sxfir_interpolate / sxfir_synthesize) between two HIP events on the launch
stream (StreamTimer); a leg's figure is the mean per set of bands.  Per run: ms and, for the synthesizer, its algorithmic bytes
(4 x 8/4 B read + 8 B written per output sample: 2 GiB in + 2 GiB out at 2^28) over time as a fraction of 8 TB/s.  Last lines:
the medians and the ratios.  profiles/syn4.txt keeps the output with the box id.
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
    m = n // 4                                              # inputs per band
    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    print("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))
    x = torch.empty((4, m), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty((4, n), dtype=torch.complex64, device="cuda")          # a wideband stream per real-tap pass
    stream = torch.cuda.current_stream().cuda_stream
    timer = StreamTimer(stream)
    proto = sxxcvr_amd.design_lowpass(128, 4, 8.0, 4.0)
    real = [sxxcvr_amd.Resampler(INTERPOLATE, proto, 4) for _ in range(4)]
    syn = sxxcvr_amd.Synthesizer(proto)
    for label, p in [("real band %d" % k, p) for k, p in enumerate(real)] + [("syn", syn)]:
        p.set_kernel(KERNEL_TILED)
        print("%-11s %s" % (label, p.geometry(m)))

    def band(k):
        real[k].process_ptr(x.data_ptr() + 8 * k * m, m, m, y.data_ptr() + 8 * k * n, n, stream)

    legs = {"real": lambda: band(0),
            "4 x real": lambda: [band(k) for k in range(4)],
            "syn": lambda: syn.process_ptr(x.data_ptr(), m, 0, m, y.data_ptr(), n, stream)}

    def timed(leg, iters):
        timer.start()
        for _ in range(iters):
            legs[leg]()
        timer.stop()
        torch.cuda.synchronize()
        return timer.elapsed_ms() / iters

    for leg in legs:
        timed(leg, 2)                                       # warm-up
    syn_bytes = 16.0 * n
    ms = {leg: [] for leg in legs}
    for r in range(args.rounds):
        for leg in ("syn", "4 x real", "real"):
            t = timed(leg, args.iters)
            ms[leg].append(t)
            tail = "  %.3f GB  %.3f of 8 TB/s" % (syn_bytes / 1e9, syn_bytes / (t * 1e-3) / 8e12) if leg == "syn" else ""
            print("round %d %-9s %.4f ms%s" % (r, leg, t, tail))
    mr, m4, mh = (statistics.median(ms[leg]) for leg in ("real", "4 x real", "syn"))
    print("median real x4 %.4f ms  4 x real x4 %.4f ms  synthesizer %.4f ms (%.3f of 8 TB/s)" % (mr, m4, mh, syn_bytes / (mh * 1e-3) / 8e12))
    print("ratio synthesizer / (4 x real) %.3f   synthesizer / real %.3f   (4 x real) / real %.3f" % (mh / m4, mh / mr, m4 / mr))


if __name__ == "__main__":
    main()
