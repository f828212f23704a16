/*
 * sxfir_synthesizer_os.h -- the 2x OVERSAMPLED 4-band synthesizer of the MI355X (gfx950) resampling path: four sub-bands at fs/2
 * each, centred on the /4 raster, into one wideband stream in ONE pass.  The way back from sxfir_channelizer_os.h and, like it, an
 * extension of the C ABI exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION and the other extension headers are
 * unchanged by it: a caller detects the feature by the symbol (dlsym "sxfir_create_synthesizer_os") or by
 * sxfir_synthesizer_os_abi_version() == 1.
 *
 * Why: the bands of the oversampled channelizer leave at fs/2; sxfir_create_synthesizer takes bands at fs/4.  Decimating each
 * band to fs/4 first brings the band-edge alias back (a tone 0.0125 under a band edge returns with an image at -29.9 dB through
 * the critically sampled pair, with nothing above -112 dB through this one); the route through two critically sampled synthesizer
 * passes -- even and odd times apart, bands 1 and 3 of the odd half negated, one result delayed by two samples and added --
 * writes two full-length wideband streams and makes a third pass over them.
 *
 * Definition.  h: the REAL prototype, a x2 interpolator's low-pass with the /4 band edge: sxfir_design_lowpass(ntaps, 4, beta,
 * 2.0), gain 2.  x_k[m]: band k at fs/2, centred at 0 Hz.  n: the ABSOLUTE wideband output index, m: the absolute per-band input
 * index, both counted from the stream's start.
 *
 *   v_r[m] = sum_k (j)^(k r) x_k[m]                                (the radix-2 butterflies of sxfir_synthesizer.h)
 *   w[n]   = sum_i h[2i + (n & 1)] . v_(n & 3)[(n >> 1) - i]       i = 0 .. ntaps/2 - 1,   x_k[<0] = 0
 *
 * Output n is output n of a real-tap x2 interpolation, ntaps / 2 taps per phase, applied to the stream v_(n mod 4).  It equals
 * sum_k (j)^(k n) (h * up2 x_k)[n]: every band interpolated by 2 and placed at k/4 cycles per output sample, the band that band k
 * of sxfir_create_channelizer_os takes out again.  The (-1)^(k m) of that header does not appear as a factor: it is the choice of
 * v_(n mod 4) by the absolute index, so nothing is multiplied.  The analysis prototype has gain 1, this one gain 2.
 *
 * Numeric contract.  The butterflies are exactly those of sxfir_synthesizer.h, one float32 rounding per real operation.  Then the
 * real-tap interpolator's contract, as sxfir_contract reports it for this plan (the contract of a x2 plan of these taps), applied
 * to v_(n & 3): jsplit contiguous ranges of i (2 when ntaps / 2 is even, which ntaps % 4 == 0 makes it; cw = 1, rotation 0), in
 * each range one fmaf chain from +0.0f over i descending, for I and Q each, and the partial sums added as P0 + P1.  SXFIR_CF16
 * input is converted half -> float before the butterflies and the output is rounded to half once, after the last sum; SXFIR_S32
 * output words are convert_tx_buffer's of the CF32 result, with the plan's tx_threshold2.
 *
 * The plan is a x2 INTERPOLATOR in everything about the stream: sxfir_outputs_for, sxfir_position (consumed = inputs PER BAND,
 * produced = wideband outputs), sxfir_set_position, sxfir_reset, sxfir_contract (2, 1), sxfir_contract_rotation (0),
 * sxfir_launch_geometry, sxfir_set_kernel, sxfir_set_tx_threshold and sxfir_destroy take it; sxfir_plan_synthesis_bands answers 4.
 * History is ntaps / 2 samples per band, carried from call to call inside the plan; sxfir_set_history answers SXFIR_EUNSUPPORTED.
 * sxfir_interpolate, sxfir_interpolate_keyed, sxfir_decimate, sxfir_time_decimate, sxfir_time_interpolate and sxfir_channelize
 * refuse the plan with SXFIR_EINVAL and leave it untouched.  sxfir_plan_oversampling keeps answering 0 for every synthesizer plan
 * (it speaks of channelizers); sxfir_plan_synthesis_oversampling below is this header's query.
 *
 * Calls go through sxfir_synthesize (sxfir_synthesizer.h) unchanged, with its band-stride and overlap rules:
 * *n_out = 2 * n_in, and out_stride >= 2 * n_in when nchan > 1.
 *
 * Kernels.  SXFIR_KERNEL_TILED exists for 4 bands x 128 taps on SXFIR_CF32 (synthesis4x2_kernel); every other shape runs
 * synthesis_os_generic_kernel and answers SXFIR_EUNSUPPORTED to sxfir_set_kernel(SXFIR_KERNEL_TILED).  The tiled kernel takes a
 * call that starts at ANY per-band index, odd ones included (the start's parity is an argument of the kernel); it needs a 16-byte
 * aligned output and, with nchan > 1, an even out_stride.  Any other call runs the generic kernel with the same bits under
 * SXFIR_KERNEL_AUTO and answers SXFIR_EUNSUPPORTED under a forced TILED with nothing written.  An odd in_stride or band_stride
 * stays with the tiled kernel.
 */
#ifndef SXFIR_SYNTHESIZER_OS_H
#define SXFIR_SYNTHESIZER_OS_H

#include "sxfir_synthesizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the three entry points below. */
#define SXFIR_SYNTHESIZER_OS_ABI_VERSION 1

int sxfir_synthesizer_os_abi_version(void);

/* taps: ntaps REAL prototype taps (host, copied).  Version 1 accepts nbands == 4 with oversample == 2 only: any other positive
 * nbands or oversample returns SXFIR_EUNSUPPORTED with a message (oversample == 1 is sxfir_create_synthesizer, and the message
 * says so).  Non-positive nbands, oversample, ntaps or nchan, ntaps % nbands != 0, an unknown fmt, NULL pointers: SXFIR_EINVAL.
 * fmt: SXFIR_CF32, SXFIR_CF16 (half in, half out) or SXFIR_S32 (CF32 in, S32_LE wire words out).  Arguments are checked before
 * the device is looked at. */
int sxfir_create_synthesizer_os(sxfir_plan **plan, const float *taps, int ntaps, int nbands, int oversample, int nchan, int fmt,
                                int device);

/* *oversample = 2 for a plan of sxfir_create_synthesizer_os, 1 for a plan of sxfir_create_synthesizer, 0 for any other plan. */
int sxfir_plan_synthesis_oversampling(const sxfir_plan *plan, int *oversample);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_SYNTHESIZER_OS_H */
