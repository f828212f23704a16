/*
 * sxfir_channelizer.h -- the 4-band channelizer of the MI355X (gfx950) resampling path: all four sub-bands of the /4 raster
 * out of one wideband stream in ONE pass.  An extension of the C ABI in sxfir.h, exported by the same libsxfir.so.  sxfir.h,
 * SXFIR_ABI_VERSION and sxfir_complex.h are unchanged by it: a caller detects the feature by the symbol (dlsym
 * "sxfir_create_channelizer") or by sxfir_channelizer_abi_version() == 1.
 *
 * What it replaces: four complex-tap plans (sxfir_create_complex with sxfir_design_bandpass(ntaps, 4, ., ., k, 4, .), k = 0..3),
 * i.e. four reads of the input and eight times a real-tap pass's arithmetic.  With the tap index written n = 4j + r,
 *
 *   y_k[m] = sum_r (j)^(k r) u_r[m],     u_r[m] = sum_j h[4j + r] x[4m - 4j - r]        (h: REAL prototype taps)
 *
 * the four polyphase branch sums u_r together are one real-tap /4 pass, and the 4-point DFT on top has only +-1 and +-j for
 * twiddles: no multiplication.  Band k is the band that sxfir_design_bandpass(ntaps, 4, beta, gain, k, 4, .) centres (k/4 cycles
 * per input sample); it lands at 0 Hz of its output.
 *
 * Numeric contract.  u_r is ONE fmaf chain from +0.0f over j descending, for I and Q each: the real-tap decimator contract
 * with (jsplit, cw) = (1, 1) and rotation 0 -- what sxfir_contract / sxfir_contract_rotation report for the plan -- applied to
 * the taps of phase r alone.  The DFT is radix-2, one float32 rounding per real operation:
 *
 *   s0 = u0 + u2,  s1 = u0 - u2,  t0 = u1 + u3,  t1 = u1 - u3
 *   y0 = s0 + t0,  y2 = s0 - t0
 *   y1 = (s1.re - t1.im, s1.im + t1.re)
 *   y3 = (s1.re + t1.im, s1.im - t1.re)
 *
 * SXFIR_CF16 output is rounded to half once, after the butterflies; SXFIR_S32 input goes through convert_rx_buffer on the way
 * in.  Band 0 is the low-pass output, but under ANOTHER summation order than a real-tap plan's (2, 4): its bits are not the
 * bits sxfir_decimate gives for the same taps.
 *
 * The plan is an ordinary sxfir_plan that behaves as a /4 (/nbands) decimator for everything about the stream: sxfir_reset,
 * sxfir_set_history, sxfir_set_position, sxfir_position (produced = outputs PER BAND), sxfir_outputs_for, sxfir_contract,
 * sxfir_contract_rotation, sxfir_set_kernel, sxfir_launch_geometry and sxfir_destroy take it.  History is ntaps samples,
 * x[<0] = 0.  sxfir_decimate, sxfir_time_decimate and sxfir_interpolate* refuse it with SXFIR_EINVAL and leave it untouched;
 * sxfir_taps_are_complex reports 0.  SXFIR_KERNEL_TILED exists for 4 bands x 128 taps on SXFIR_CF32 (chan4_kernel); every
 * other shape runs chan_generic_kernel and answers SXFIR_EUNSUPPORTED to sxfir_set_kernel(SXFIR_KERNEL_TILED).  A call that
 * starts off an output boundary, or whose output, out_stride or band_stride breaks the 16-byte store alignment, runs the
 * generic kernel with the same bits under SXFIR_KERNEL_AUTO and answers SXFIR_EUNSUPPORTED under a forced TILED.
 */
#ifndef SXFIR_CHANNELIZER_H
#define SXFIR_CHANNELIZER_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the four entry points below. */
#define SXFIR_CHANNELIZER_ABI_VERSION 1

int sxfir_channelizer_abi_version(void);

/* taps: ntaps REAL prototype taps (host, copied).  nbands == 4 in version 1: anything else returns SXFIR_EUNSUPPORTED with a
 * message.  ntaps % nbands == 0, else SXFIR_EINVAL.  fmt: SXFIR_CF32, SXFIR_CF16 or SXFIR_S32 (wire words in, CF32 out).
 * Arguments are checked before the device is looked at. */
int sxfir_create_channelizer(sxfir_plan **plan, const float *taps, int ntaps, int nbands, int nchan, int fmt, int device);

/* One call of the stream.  Band k of channel c starts at out_dev + c * out_stride + k * band_stride (complex samples of the
 * output format); *n_out = outputs PER BAND.  SXFIR_EINVAL if band_stride is smaller than the call's outputs per band, or if
 * two bands or channels would overlap. */
int sxfir_channelize(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                     size_t band_stride, size_t *n_out, void *stream);

/* *nbands = 4 for a channelizer plan, 0 for any other plan. */
int sxfir_plan_bands(const sxfir_plan *plan, int *nbands);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_CHANNELIZER_H */
