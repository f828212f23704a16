"""A band plan's one pass against the route the older kernels offer for the same bands, and a real-tap pass for scale.

    python3 tools/bandbench.py {chan|syn|chanos|synos} [--log2n 28] [--iters 10] [--rounds 3]

2^28 wideband CF32 samples (a channelizer's input, a synthesizer's output).  Three legs -- scale, old route, the band plan's
pass -- are alternated on the same box, three alternations.  Every leg is `iters` back-to-back streaming calls (sxfir_decimate /
sxfir_interpolate / sxfir_channelize / sxfir_synthesize) between two HIP events on the launch stream (StreamTimer); a leg's
figure is the mean per set of bands.  Per run: ms and, for the band plan's pass, its algorithmic bytes over time as a fraction
of 8 TB/s.  Last lines: the medians and the ratios.  Each form prints what the tool it replaces printed (chanbench.py,
synbench.py, chanosbench.py, synosbench.py), line for line: the files under profiles/ stay comparable.

chan -- the 4-band channelizer against four complex /4 passes (profiles/chan4.txt)
    real     one real-tap /4 x 128 pass (decim4_wide_kernel): the arithmetic the channelizer does, a quarter of its output
    4 x cx   four complex-tap /4 x 128 passes, bands 0..3 (decim4_cx_kernel): the four bands without the channelizer
    chan     one channelizer pass (chan4_kernel)
Bytes: 8 B read + 4 x 8/4 B written per input sample: 2 GiB in + 2 GiB out at 2^28.

syn -- the 4-band synthesizer against four real x4 passes (profiles/syn4.txt); 2^26 inputs per band
    real     one real-tap x4 x 128 pass (interp8_pass_kernel<4, ..., 4>): the arithmetic the synthesizer does, a quarter of its input
    4 x real four real-tap x4 passes, one per band, each writing a wideband stream of its own: what the synthesis replaces -- a LOWER
             bound of the old cost, which leaves out the caller's rotation of bands 1..3 and the sum of the four streams
    syn      one synthesizer pass (synthesis4_kernel)
Bytes: 4 x 8/4 B read + 8 B written per output sample: 2 GiB in + 2 GiB out at 2^28.

chanos -- the 2x oversampled 4-band channelizer against two critically sampled passes (profiles/chan4x2.txt)
    real       one real-tap /4 x 128 pass (decim4_wide_kernel): half the arithmetic of the oversampled channelizer
    2 x chan   two critically sampled channelizer passes (chan4_kernel), one on the stream and one on the stream advanced by two
               samples: the same output volume and arithmetic, the input read twice.  A LOWER bound of the old route: the pass
               that interleaves the two results and turns the odd times of bands 1 and 3 (8 GiB of traffic more) is left out
    chan4x2    one oversampled pass (chan4x2_kernel)
Bytes: 8 B read + 4 x 8/2 B written per input sample: 2 GiB in + 4 GiB out at 2^28.

synos -- the 2x oversampled 4-band synthesizer against two critically sampled passes (profiles/syn4x2.txt); 2^27 inputs per band at fs/2
    real     one real-tap x4 x 128 pass (interp8_pass_kernel<4, ..., 4>), for scale
    2 x syn  two critically sampled synthesizer passes (synthesis4_kernel) over 2^26 inputs per band each -- the even and the odd
             times of the bands -- each writing a full-length wideband stream: the old route's arithmetic and its two wideband
             writes.  A LOWER bound of the old cost: the split into even and odd times, the negation of bands 1 and 3 of the odd
             half and the pass that delays one wideband stream by two samples and adds the two are left out
    syn4x2   one oversampled pass (synthesis4x2_kernel)
Bytes: 4 x 8/2 B read + 8 B written per output sample: 4 GiB in + 2 GiB out at 2^28; the two passes move 8 GiB.  The ratio line
also gives the range of the per-round ratio.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sxxcvr_amd  # noqa: E402
from sxxcvr_amd.resampler import DECIMATE, INTERPOLATE, KERNEL_TILED, StreamTimer  # noqa: E402

# A form is a function (n, stream) -> its table: "plans" [(label, plan, n_in of the geometry line)], "legs" [(name, call)] in
# the order scale, old route, band plan; "bytes" of the band plan's pass; the words of the two last lines ("median": the three
# legs' names there, "old", "new": the ratio line's); the two column widths; "per_round": the ratio's range too.


def chan(n, st):
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty((4, n // 4), dtype=torch.complex64, device="cuda")
    proto = sxxcvr_amd.design_lowpass(128, 4)
    real = sxxcvr_amd.Resampler(DECIMATE, proto, 4)
    cx = [sxxcvr_amd.Resampler(DECIMATE, sxxcvr_amd.design_bandpass(128, 4, k, 4), 4) for k in range(4)]
    plan = sxxcvr_amd.Channelizer(proto)

    def band(p, k):
        p.process_ptr(x.data_ptr(), n, n, y.data_ptr() + 8 * k * (n // 4), n // 4, st)

    return {"plans": [("real", real, n)] + [("cx band %d" % k, p, n) for k, p in enumerate(cx)] + [("chan", plan, n)],
            "legs": [("real", lambda: band(real, 0)), ("4 x cx", lambda: [band(p, k) for k, p in enumerate(cx)]),
                     ("chan", lambda: plan.process_ptr(x.data_ptr(), n, n, y.data_ptr(), 0, n // 4, st))],
            "bytes": 16.0 * n, "median": ("real /4", "4 x complex /4", "channelizer"), "old": "(4 x complex)", "new": "channelizer",
            "label_width": 10, "leg_width": 7, "per_round": False}


def syn(n, st):
    m = n // 4                                              # inputs per band
    x = torch.empty((4, m), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty((4, n), dtype=torch.complex64, device="cuda")          # a wideband stream per real-tap pass
    proto = sxxcvr_amd.design_lowpass(128, 4, 8.0, 4.0)
    real = [sxxcvr_amd.Resampler(INTERPOLATE, proto, 4) for _ in range(4)]
    plan = sxxcvr_amd.Synthesizer(proto)

    def band(k):
        real[k].process_ptr(x.data_ptr() + 8 * k * m, m, m, y.data_ptr() + 8 * k * n, n, st)

    return {"plans": [("real band %d" % k, p, m) for k, p in enumerate(real)] + [("syn", plan, m)],
            "legs": [("real", lambda: band(0)), ("4 x real", lambda: [band(k) for k in range(4)]),
                     ("syn", lambda: plan.process_ptr(x.data_ptr(), m, 0, m, y.data_ptr(), n, st))],
            "bytes": 16.0 * n, "median": ("real x4", "4 x real x4", "synthesizer"), "old": "(4 x real)", "new": "synthesizer",
            "label_width": 11, "leg_width": 9, "per_round": False}


def chanos(n, st):
    x = torch.empty(n + 2, dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty((4, n // 2), dtype=torch.complex64, device="cuda")       # the two critically sampled passes share it: 2 x [4, n / 4]
    proto = sxxcvr_amd.design_lowpass(128, 4)
    real = sxxcvr_amd.Resampler(DECIMATE, proto, 4)
    crit = [sxxcvr_amd.Channelizer(proto) for _ in range(2)]
    plan = sxxcvr_amd.Channelizer(proto, oversample=2)

    def two_passes():
        for k, p in enumerate(crit):                        # (the stream, and the stream advanced by two samples: 16 bytes)
            p.process_ptr(x.data_ptr() + 16 * k, n, n, y.data_ptr() + 8 * k * n, 0, n // 4, st)

    return {"plans": [("real", real, n), ("chan even", crit[0], n), ("chan odd", crit[1], n), ("chan4x2", plan, n)],
            "legs": [("real", lambda: real.process_ptr(x.data_ptr(), n, n, y.data_ptr(), n // 4, st)), ("2 x chan", two_passes),
                     ("chan4x2", lambda: plan.process_ptr(x.data_ptr(), n, n, y.data_ptr(), 0, n // 2, st))],
            "bytes": 24.0 * n, "median": ("real /4", "2 x channelizer", "oversampled channelizer"), "old": "(2 x chan)", "new": "chan4x2",
            "label_width": 10, "leg_width": 8, "per_round": False}


def synos(n, st):
    m = n // 2                                              # inputs per band at fs/2
    x = torch.empty((4, m), dtype=torch.complex64, device="cuda")
    sxxcvr_amd.synth_fill(x, 0x51255, 0, 0)
    y = torch.empty((2, n), dtype=torch.complex64, device="cuda")          # a wideband stream per critically sampled pass
    real = sxxcvr_amd.Resampler(INTERPOLATE, sxxcvr_amd.design_lowpass(128, 4, 8.0, 4.0), 4)
    crit = [sxxcvr_amd.Synthesizer(sxxcvr_amd.design_lowpass(128, 4, 8.0, 4.0)) for _ in range(2)]
    plan = sxxcvr_amd.Synthesizer(sxxcvr_amd.design_lowpass(128, 4, 8.0, 2.0), oversample=2)

    def two_passes():
        for k, p in enumerate(crit):                        # (each pass a half of every band: the volume of the even / odd times)
            p.process_ptr(x.data_ptr() + 8 * k * (m // 2), m // 2, 0, m, y.data_ptr() + 8 * k * n, n, st)

    return {"plans": [("real", real, n // 4), ("syn even", crit[0], n // 4), ("syn odd", crit[1], n // 4), ("syn4x2", plan, m)],
            "legs": [("real", lambda: real.process_ptr(x.data_ptr(), n // 4, n // 4, y.data_ptr(), n, st)), ("2 x syn", two_passes),
                     ("syn4x2", lambda: plan.process_ptr(x.data_ptr(), m, 0, m, y.data_ptr(), n, st))],
            "bytes": 24.0 * n, "median": ("real x4", "2 x synthesizer", "oversampled synthesizer"), "old": "(2 x syn)", "new": "syn4x2",
            "label_width": 9, "leg_width": 8, "per_round": True}


FORMS = {"chan": chan, "syn": syn, "chanos": chanos, "synos": synos}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("form", choices=sorted(FORMS))
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    n = 1 << args.log2n                                     # wideband samples
    lib = sxxcvr_amd.load_sxfir()
    name, arch, bdf = C.create_string_buffer(64), C.create_string_buffer(32), C.create_string_buffer(16)
    lib.sxfir_device_info(0, name, arch, None, None)
    lib.sxfir_device_pci_bus_id(0, bdf, 16)
    print("box: %s %s %s host %s" % (name.value.decode(), arch.value.decode(), bdf.value.decode(), os.uname().nodename))
    stream = torch.cuda.current_stream().cuda_stream
    timer = StreamTimer(stream)
    f = FORMS[args.form](n, stream)
    for label, p, n_in in f["plans"]:
        p.set_kernel(KERNEL_TILED)
        print("%-*s %s" % (f["label_width"], label, p.geometry(n_in)))
    legs = dict(f["legs"])
    scale, old, new = (leg for leg, _ in f["legs"])

    def timed(leg, iters):
        timer.start()
        for _ in range(iters):
            legs[leg]()
        timer.stop()
        torch.cuda.synchronize()
        return timer.elapsed_ms() / iters

    for leg in legs:
        timed(leg, 2)                                       # warm-up
    nbytes = f["bytes"]
    ms = {leg: [] for leg in legs}
    for r in range(args.rounds):
        for leg in (new, old, scale):
            t = timed(leg, args.iters)
            ms[leg].append(t)
            tail = "  %.3f GB  %.3f of 8 TB/s" % (nbytes / 1e9, nbytes / (t * 1e-3) / 8e12) if leg == new else ""
            print("round %d %-*s %.4f ms%s" % (r, f["leg_width"], leg, t, tail))
    ms_scale, ms_old, ms_new = (statistics.median(ms[leg]) for leg in (scale, old, new))
    print("median %s %.4f ms  %s %.4f ms  %s %.4f ms (%.3f of 8 TB/s)" % (
        f["median"][0], ms_scale, f["median"][1], ms_old, f["median"][2], ms_new, nbytes / (ms_new * 1e-3) / 8e12))
    per_round = [c / b for c, b in zip(ms[new], ms[old])]
    spread = " (per round %.3f .. %.3f)" % (min(per_round), max(per_round)) if f["per_round"] else ""
    print("ratio %s / %s %.3f%s   %s / real %.3f   %s / real %.3f" % (
        f["new"], f["old"], ms_new / ms_old, spread, f["new"], ms_new / ms_scale, f["old"], ms_old / ms_scale))


if __name__ == "__main__":
    main()
