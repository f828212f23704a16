"""The 4-band channelizer against the route the complex-tap kernels offer for the same four bands: four complex /4 passes.

    python3 tools/chanbench.py [--log2n 28] [--iters 10] [--rounds 3]

2^28 resident CF32 samples.  Three legs are alternated on the same box, three alternations:
    real     one real-tap /4 x 128 pass (decim4_wide_kernel): the arithmetic the channelizer does, a quarter of its output
    4 x cx   four complex-tap /4 x 128 passes, bands 0..3 (decim4_cx_kernel): the four bands without the channelizer
    chan     one channelizer pass (chan4_kernel)
Every leg is `iters` back-to-back streaming calls (sxfir_decimate / sxfir_channelize) between two HIP events on the launch
stream (StreamTimer); a leg's figure is the mean per set of bands.  Per run: ms and, for the channelizer, its algorithmic bytes
(8 B read + 4 x 8/4 B written per input sample: 2 GiB in + 2 GiB out at 2^28) over time as a fraction of 8 TB/s.  Last lines:
the medians and the ratios.  profiles/chan4.txt keeps the output with the box id.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sxxcvr_amd  # noqa: E402
from sxxcvr_amd.resampler import DECIMATE, KERNEL_TILED, StreamTimer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--iters", type=int, default=10)
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
    y = torch.empty((4, n // 4), dtype=torch.complex64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    timer = StreamTimer(stream)
    proto = sxxcvr_amd.design_lowpass(128, 4)
    real = sxxcvr_amd.Resampler(DECIMATE, proto, 4)
    cx = [sxxcvr_amd.Resampler(DECIMATE, sxxcvr_amd.design_bandpass(128, 4, k, 4), 4) for k in range(4)]
    chan = sxxcvr_amd.Channelizer(proto)
    for label, p in [("real", real)] + [("cx band %d" % k, p) for k, p in enumerate(cx)] + [("chan", chan)]:
        p.set_kernel(KERNEL_TILED)
        print("%-10s %s" % (label, p.geometry(n)))

    def band(p, k):
        p.process_ptr(x.data_ptr(), n, n, y.data_ptr() + 8 * k * (n // 4), n // 4, stream)

    legs = {"real": lambda: band(real, 0),
            "4 x cx": lambda: [band(p, k) for k, p in enumerate(cx)],
            "chan": lambda: chan.process_ptr(x.data_ptr(), n, n, y.data_ptr(), 0, n // 4, stream)}

    def timed(leg, iters):
        timer.start()
        for _ in range(iters):
            legs[leg]()
        timer.stop()
        torch.cuda.synchronize()
        return timer.elapsed_ms() / iters

    for leg in legs:
        timed(leg, 2)                                       # warm-up
    chan_bytes = 16.0 * n
    ms = {leg: [] for leg in legs}
    for r in range(args.rounds):
        for leg in ("chan", "4 x cx", "real"):
            t = timed(leg, args.iters)
            ms[leg].append(t)
            tail = "  %.3f GB  %.3f of 8 TB/s" % (chan_bytes / 1e9, chan_bytes / (t * 1e-3) / 8e12) if leg == "chan" else ""
            print("round %d %-7s %.4f ms%s" % (r, leg, t, tail))
    mr, mc, mh = (statistics.median(ms[leg]) for leg in ("real", "4 x cx", "chan"))
    print("median real /4 %.4f ms  4 x complex /4 %.4f ms  channelizer %.4f ms (%.3f of 8 TB/s)" % (mr, mc, mh, chan_bytes / (mh * 1e-3) / 8e12))
    print("ratio channelizer / (4 x complex) %.3f   channelizer / real %.3f   (4 x complex) / real %.3f" % (mh / mc, mh / mr, mc / mr))


if __name__ == "__main__":
    main()
