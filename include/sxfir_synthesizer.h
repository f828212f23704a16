/*
 * sxfir_synthesizer.h -- the 4-band synthesizer of the MI355X (gfx950) resampling path: four sub-bands of the x4 raster into one
 * wideband stream in ONE pass.  The TX counterpart of sxfir_channelizer.h and, like it, an extension of the C ABI in sxfir.h,
 * exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION, sxfir_complex.h and sxfir_channelizer.h are unchanged by it: a
 * caller detects the feature by the symbol (dlsym "sxfir_create_synthesizer") or by sxfir_synthesizer_abi_version() == 1.
 *
 * What it replaces: four real-tap x4 interpolator plans, one per band, plus kernels of the caller's own that turn band k to k/4
 * cycles per output sample and add the four wideband streams -- four times a real-tap pass's arithmetic and four wideband
 * streams written before the combine.  Band k is placed by h[n] (j)^(k n), h the REAL prototype; with the output index written
 * n = 4m + r the sum over the bands is
 *
 *   w[4m + r] = sum_j h[4j + r] v_r[m - j],     v_r[m] = sum_k (j)^(k r) x_k[m]
 *
 * i.e. a 4-point DFT across the bands, whose twiddles are +-1 and +-j (no multiplication), and then ONE real-tap x4 interpolation
 * in which output phase r reads the stream v_r.  Band k of the input lands at k/4 cycles per output sample: the band that
 * sxfir_create_channelizer's band k takes out again.  The prototype is what any x4 interpolator takes:
 * sxfir_design_lowpass(ntaps, 4, beta, 4.0), gain 4.
 *
 * Numeric contract.  The DFT is radix-2, one float32 rounding per real operation:
 *
 *   a0 = x0 + x2,  a1 = x0 - x2,  b0 = x1 + x3,  b1 = x1 - x3
 *   v0 = a0 + b0,  v2 = a0 - b0
 *   v1 = (a1.re - b1.im, a1.im + b1.re)
 *   v3 = (a1.re + b1.im, a1.im - b1.re)
 *
 * Output 4m + r is the real-tap interpolator's contract, as sxfir_contract reports it for this plan, applied to the stream v_r:
 * jsplit contiguous ranges of j (2 when ntaps / 4 is even, else 1; cw = 1, rotation 0), in each range one fmaf chain from +0.0f
 * over j descending, for I and Q each, and the partial sums added as P0 + P1.  A band's x[<0] = 0, hence v_r[<0] = +0.0.
 * SXFIR_CF16 input is converted half -> float before the butterflies and the output is rounded to half once, after the last sum;
 * SXFIR_S32 output words are convert_tx_buffer's of the CF32 result, with the plan's tx_threshold2.
 *
 * The plan is an ordinary sxfir_plan that behaves as a x4 interpolator for everything about the stream: sxfir_reset,
 * sxfir_set_position, sxfir_position (consumed = inputs PER BAND, produced = wideband outputs), sxfir_outputs_for,
 * sxfir_contract, sxfir_contract_rotation, sxfir_set_kernel, sxfir_set_tx_threshold, sxfir_launch_geometry and sxfir_destroy take
 * it.  History is ntaps / 4 samples per band, carried from call to call inside the plan; sxfir_set_history answers
 * SXFIR_EUNSUPPORTED in version 1 (its single stride cannot name bands and channels).  sxfir_decimate, sxfir_time_decimate,
 * sxfir_interpolate, sxfir_interpolate_keyed, sxfir_time_interpolate and sxfir_channelize refuse it with SXFIR_EINVAL and leave
 * it untouched; sxfir_plan_bands reports 0 for it (it is no channelizer) and sxfir_taps_are_complex 0.  SXFIR_KERNEL_TILED
 * exists for 4 bands x 128 taps on SXFIR_CF32 (synthesis4_kernel); every other shape runs synthesis_generic_kernel and answers
 * SXFIR_EUNSUPPORTED to sxfir_set_kernel(SXFIR_KERNEL_TILED).  The tiled kernel stores 16 bytes at a time: a call whose output
 * pointer is not 16-byte aligned, or whose out_stride is odd with nchan > 1, runs the generic kernel with the same bits under
 * SXFIR_KERNEL_AUTO and answers SXFIR_EUNSUPPORTED under a forced TILED.  Its loads need no more than the one-sample alignment
 * every call must have, so an odd in_stride or band_stride stays with the tiled kernel.
 */
#ifndef SXFIR_SYNTHESIZER_H
#define SXFIR_SYNTHESIZER_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the four entry points below. */
#define SXFIR_SYNTHESIZER_ABI_VERSION 1

int sxfir_synthesizer_abi_version(void);

/* taps: ntaps REAL prototype taps (host, copied).  nbands == 4 in version 1: anything else returns SXFIR_EUNSUPPORTED with a
 * message.  ntaps % nbands == 0, else SXFIR_EINVAL.  fmt: SXFIR_CF32, SXFIR_CF16 (half in, half out) or SXFIR_S32 (CF32 in, S32_LE
 * wire words out).  Arguments are checked before the device is looked at. */
int sxfir_create_synthesizer(sxfir_plan **plan, const float *taps, int ntaps, int nbands, int nchan, int fmt, int device);

/* One call of the stream.  Band k of channel c is read at in_dev + c * in_stride + k * band_stride (complex samples of the input
 * format); n_in = inputs PER BAND; *n_out = 4 * n_in wideband outputs per channel, at out_dev + c * out_stride.  SXFIR_EINVAL if
 * band_stride is smaller than n_in, if two bands or channels of the input would overlap (with nchan > 1 either a channel's bands
 * lie in a row, in_stride >= 3 * band_stride + n_in, or a band's channels do, band_stride >= (nchan - 1) * in_stride + n_in), or
 * if out_stride is smaller than 4 * n_in with nchan > 1. */
int sxfir_synthesize(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, size_t band_stride, void *out_dev,
                     size_t out_stride, size_t *n_out, void *stream);

/* *nbands = 4 for a synthesizer plan, 0 for any other plan. */
int sxfir_plan_synthesis_bands(const sxfir_plan *plan, int *nbands);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_SYNTHESIZER_H */
