/*
 * sxfir_channelizer_os.h -- the 2x OVERSAMPLED 4-band channelizer of the MI355X (gfx950) resampling path: the four bands and
 * centres of sxfir_channelizer.h, each leaving at fs/2 instead of fs/4, out of one wideband stream in ONE pass.  An extension of
 * the C ABI exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION, sxfir_channelizer.h and sxfir_synthesizer.h are
 * unchanged by it: a caller detects the feature by the symbol (dlsym "sxfir_create_channelizer_os") or by
 * sxfir_channelizer_os_abi_version() == 1.
 *
 * Why: the critically sampled channelizer lets every band leave at exactly the band spacing, so the prototype's transition band
 * folds back into the band -- a signal near a band edge appears in the neighbouring band as an alias that nothing there tells
 * from a real signal.  At fs/2 per band the transition band has room: every band is alias-free across its whole width.
 *
 * Definition.  h: the REAL prototype taps, tap index n = 4j + r; m counts outputs at fs/2:
 *
 *   u_r[m] = sum_j h[4j + r] x[2m - 4j - r]                    (x[<0] = 0)
 *   y_k[m] = (-1)^(k m) . sum_r (j)^(k r) u_r[m]
 *
 * Band k is the band that sxfir_design_bandpass(ntaps, 4, beta, gain, k, 4, .) centres (k/4 cycles per input sample); it lands at
 * 0 Hz of its output.
 *
 * Numeric contract.  u_r[m] is ONE fmaf chain from +0.0f over j descending, for I and Q each: the real-tap decimator contract
 * with (jsplit, cw) = (1, 1) and rotation 0 -- what sxfir_contract / sxfir_contract_rotation report for the plan -- applied to
 * the taps of phase r alone, as in sxfir_channelizer.h.  Then the radix-2 butterflies of sxfir_channelizer.h, one float32
 * rounding per real operation:
 *
 *   s0 = a0 + a2,  s1 = a0 - a2,  t0 = a1 + a3,  t1 = a1 - a3
 *   y0 = s0 + t0,  y2 = s0 - t0
 *   y1 = (s1.re - t1.im, s1.im + t1.re)
 *   y3 = (s1.re + t1.im, s1.im - t1.re)
 *
 * with (a0, a1, a2, a3) = (u0, u1, u2, u3) for EVEN m and (u2, u3, u0, u1) for ODD m.  The factor (-1)^(k m) is that circular
 * shift of the branch sums by two: nothing is multiplied, and the result is NOT a negation of the even-time formula -- the signs
 * of zeros are what this operand order gives.  SXFIR_CF16 output is rounded to half once, after the butterflies; SXFIR_S32 wire
 * words go through convert_rx_buffer on the way in, with CF32 out.
 *
 * Two consequences:
 *   * y_k[2m'] has the bits of sxfir_channelize (a plan of sxfir_create_channelizer with the same taps) on the same stream at
 *     output m' (the odd-time outputs are that plan's on the stream advanced by two samples, bands 1 and 3 turned by half a
 *     circle through the operand order above);
 *   * the plan is a /2 DECIMATOR in everything about the stream: sxfir_outputs_for, sxfir_position (produced = outputs PER
 *     BAND), sxfir_set_position, sxfir_set_history (history is ntaps samples), sxfir_reset, sxfir_contract (1, 1),
 *     sxfir_contract_rotation (0), sxfir_launch_geometry, sxfir_set_kernel and sxfir_destroy take it.
 *
 * Calls go through sxfir_channelize (sxfir_channelizer.h) with its band-stride, overlap and *n_out (outputs per band) rules;
 * sxfir_plan_bands answers 4.  sxfir_decimate, sxfir_time_decimate and sxfir_interpolate* refuse the plan with SXFIR_EINVAL and
 * leave it untouched.
 *
 * Kernels.  SXFIR_KERNEL_TILED exists for 4 bands x 128 taps on SXFIR_CF32 (chan4x2_kernel); every other shape runs
 * chan4x2_generic_kernel and answers SXFIR_EUNSUPPORTED to sxfir_set_kernel(SXFIR_KERNEL_TILED).  The tiled kernel takes a call
 * that starts at a stream position that is a multiple of 4 (an EVEN output index), with a 16-byte aligned output and even
 * out_stride and band_stride.  Any other call -- a start at an odd output index included: the tiled kernel has no parity flag --
 * runs the generic kernel with the same bits under SXFIR_KERNEL_AUTO and answers SXFIR_EUNSUPPORTED under a forced TILED with
 * nothing written.
 */
#ifndef SXFIR_CHANNELIZER_OS_H
#define SXFIR_CHANNELIZER_OS_H

#include "sxfir_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the three entry points below. */
#define SXFIR_CHANNELIZER_OS_ABI_VERSION 1

int sxfir_channelizer_os_abi_version(void);

/* taps: ntaps REAL prototype taps (host, copied).  Version 1 accepts nbands == 4 with oversample == 2 only: any other positive
 * nbands or oversample returns SXFIR_EUNSUPPORTED with a message (oversample == 1 is sxfir_create_channelizer, and the message
 * says so).  Non-positive nbands, oversample, ntaps or nchan, ntaps % nbands != 0, an unknown fmt, NULL pointers: SXFIR_EINVAL.
 * fmt: SXFIR_CF32, SXFIR_CF16 or SXFIR_S32 (wire words in, CF32 out).  Arguments are checked before the device is looked at. */
int sxfir_create_channelizer_os(sxfir_plan **plan, const float *taps, int ntaps, int nbands, int oversample, int nchan, int fmt,
                                int device);

/* *oversample = 2 for a plan of sxfir_create_channelizer_os, 1 for a plan of sxfir_create_channelizer, 0 for any other plan. */
int sxfir_plan_oversampling(const sxfir_plan *plan, int *oversample);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_CHANNELIZER_OS_H */
