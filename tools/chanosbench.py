"""The 2x oversampled 4-band channelizer against the route the critically sampled one offers for the same output: two passes.

    python3 tools/chanosbench.py [--log2n 28] [--iters 10] [--rounds 3]

2^28 resident CF32 samples.  Three legs are alternated on the same box, three alternations:
    real       one real-tap /4 x 128 pass (decim4_wide_kernel): half the arithmetic of the oversampled channelizer
    2 x chan   two critically sampled channelizer passes (chan4_kernel), one on the stream and one on the stream advanced by two
               samples: the same output volume and arithmetic, the input read twice.  A LOWER bound of the old route: the pass
               that interleaves the two results and turns the odd times of bands 1 and 3 (8 GiB of traffic more) is left out
    chan4x2    one oversampled pass (chan4x2_kernel)
Every leg is `iters` back-to-back streaming calls (sxfir_decimate / sxfir_channelize) between two HIP events on the launch
stream (StreamTimer); a leg's figure is the mean per set of bands.  Per run: ms and, for the oversampled channelizer, its
algorithmic bytes (8 B read + 4 x 8/2 B written per input sample: 2 GiB in + 4 GiB out at 2^28) over time as a fraction of
8 TB/s.  Last lines: the medians and the ratios.  profiles/chan4x2.txt keeps the output with the box id.
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
    x = torch.empty(n + 2, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty((4, n // 2), dtype=torch.complex64, device="cuda")       # the two critically sampled passes share it: 2 x [4, n / 4]
    stream = torch.cuda.current_stream().cuda_stream
    timer = StreamTimer(stream)
    proto = sxxcvr_amd.design_lowpass(128, 4)
    real = sxxcvr_amd.Resampler(DECIMATE, proto, 4)
    crit = [sxxcvr_amd.Channelizer(proto) for _ in range(2)]
    chan_os = sxxcvr_amd.Channelizer(proto, oversample=2)
    for label, p in [("real", real), ("chan even", crit[0]), ("chan odd", crit[1]), ("chan4x2", chan_os)]:
        p.set_kernel(KERNEL_TILED)
        print("%-10s %s" % (label, p.geometry(n)))

    def two_passes():
        for k, p in enumerate(crit):                        # (the stream, and the stream advanced by two samples: 16 bytes)
            p.process_ptr(x.data_ptr() + 16 * k, n, n, y.data_ptr() + 8 * k * n, 0, n // 4, stream)

    legs = {"real": lambda: real.process_ptr(x.data_ptr(), n, n, y.data_ptr(), n // 4, stream),
            "2 x chan": two_passes,
            "chan4x2": lambda: chan_os.process_ptr(x.data_ptr(), n, n, y.data_ptr(), 0, n // 2, stream)}

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
        for leg in ("chan4x2", "2 x chan", "real"):
            t = timed(leg, args.iters)
            ms[leg].append(t)
            tail = "  %.3f GB  %.3f of 8 TB/s" % (os_bytes / 1e9, os_bytes / (t * 1e-3) / 8e12) if leg == "chan4x2" else ""
            print("round %d %-8s %.4f ms%s" % (r, leg, t, tail))
    mr, mb, mc = (statistics.median(ms[leg]) for leg in ("real", "2 x chan", "chan4x2"))
    print("median real /4 %.4f ms  2 x channelizer %.4f ms  oversampled channelizer %.4f ms (%.3f of 8 TB/s)" % (mr, mb, mc, os_bytes / (mc * 1e-3) / 8e12))
    print("ratio chan4x2 / (2 x chan) %.3f   chan4x2 / real %.3f   (2 x chan) / real %.3f" % (mc / mb, mc / mr, mb / mr))


if __name__ == "__main__":
    main()
