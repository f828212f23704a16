/*
 * sxfir_translate_tx.h -- frequency-translating interpolators of the MI355X (gfx950) resampling path: an extension of the C ABI in
 * sxfir.h, exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION and the other extension headers are unchanged by it: a
 * caller detects the feature by the symbol (dlsym "sxfir_create_translating_interpolator") or by
 * sxfir_translate_tx_abi_version() == 1.
 *
 * The way back from a translating decimator (sxfir_translate.h).  A complex-tap interpolator (sxfir_complex_tx.h) places a
 * base-band stream on the x ratio raster, at k / ratio cycles per output sample; for a band centred anywhere else the narrowband
 * stream had to be turned in a pass of the caller's own first, read and written once more.  A translating plan does that turn
 * where it reads its input.  The reference (tejeez/sxxcvr, SoapySX/SoapySX.cpp) has no counterpart: the SX1255 interpolates the
 * one band around 0 Hz.
 *
 * Definition.  Let L = ratio, num reduced into [0, den), s = (num * L) mod den and w = sxfir_design_rotator(den), the table
 * w[i] = exp(-j 2 pi i / den) of sxfir_translate.h (no second table, no conjugation).  Then
 *
 *   xr[m] = x[m] * w[(den - (m * s mod den)) mod den]          -- the turn exp(+j 2 pi m s / den)
 *   y     = the complex-tap interpolator's result (sxfir_complex_tx.h) for the same taps over xr
 *
 * With h = sxfir_design_bandpass(ntaps, L, beta, L, num, den) -- gain L, num / den read as cycles per OUTPUT sample -- a base-band
 * input lands centred at num / den cycles per output sample.
 *
 * Stream rules: m is the ABSOLUTE input index -- `consumed` of sxfir_position plus the index within the call -- so the phase is
 * continuous over any split of the stream into calls.  It follows sxfir_set_position, starts again at 0 after sxfir_reset, and a
 * failed call leaves it where it was.  The modulo is the mathematical one: a history sample at a negative index (sxfir_set_history
 * at position 0) gets the entry of its index reduced into [0, den).  The index is reduced exactly, in integers: no drift, however
 * long the stream.  The caller's history (sxfir_set_history) and the history a call leaves behind are RAW, unrotated samples; the
 * rotation is applied where they are read.
 *
 * Numeric contract:
 *
 *   xr.re = fsub_rn(fmul_rn(x.re, w.re), fmul_rn(x.im, w.im))
 *   xr.im = fadd_rn(fmul_rn(x.re, w.im), fmul_rn(x.im, w.re))
 *
 * six roundings, no fused multiply-add: sxfir_translate.h's formula.  y has the bits that the sxfir_create_complex_interpolator
 * plan of the same shape produces when it is fed xr (sxfir_complex_tx.h's contract, in float32 whatever the storage format).
 * SXFIR_CF16: half -> float first, the rotation in float32 and NOT rounded back to half, the output rounded to half once.
 * SXFIR_S32: CF32 in, convert_tx_buffer words of the combined result out, under sxfir_set_tx_threshold.  The keying count of
 * sxfir_interpolate_keyed is taken on the RAW input, under sxfir_count_keyed's rule.  s = 0 (a centre on the output raster)
 * multiplies by (1, +0): that is NOT promised to reproduce the complex interpolator's bits on the raw input -- signed zeros and
 * Inf * 0 differ -- and such a caller wants sxfir_create_complex_interpolator.
 *
 * The plan is an ordinary complex-tap interpolator plan: sxfir_interpolate, sxfir_interpolate_keyed, sxfir_time_interpolate,
 * sxfir_reset, sxfir_set_history, sxfir_set_position, sxfir_position, sxfir_outputs_for, sxfir_contract, sxfir_set_kernel,
 * sxfir_set_tx_threshold, sxfir_launch_geometry and sxfir_destroy take it; sxfir_taps_are_complex answers 1,
 * sxfir_plan_translation (sxfir_translate.h) and the band and rational queries 0; sxfir_decimate and the band and rational entry
 * points refuse it.
 *
 * SXFIR_KERNEL_TILED exists on SXFIR_CF32 for ratio 4 with 128 taps and ratio 8 with 256 taps (interp_mix_pass_kernel): it takes a
 * call whose output is 16-byte aligned with an even channel stride, at any stream position.  Under SXFIR_KERNEL_AUTO any other call
 * of such a plan runs the generic kernel (interp_mix_generic_kernel, the same bits); under SXFIR_KERNEL_TILED it answers
 * SXFIR_EUNSUPPORTED, plan untouched.  Every other shape or format runs the generic kernel and answers SXFIR_EUNSUPPORTED to
 * sxfir_set_kernel(SXFIR_KERNEL_TILED).
 */
#ifndef SXFIR_TRANSLATE_TX_H
#define SXFIR_TRANSLATE_TX_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the three entry points below. */
#define SXFIR_TRANSLATE_TX_ABI_VERSION 1

int sxfir_translate_tx_abi_version(void);

/* As sxfir_create_complex_interpolator, with input m turned by exp(+j 2 pi m s / den), s = (num * ratio) mod den.
 * taps_iq: ntaps interleaved (re, im) float pairs, host, copied.  num: any int, reduced into [0, den); den in 1..65536.
 * Refusals, in this order and before the device is looked at: a NULL argument, ntaps, ratio, nchan, fmt (as
 * sxfir_create_complex_interpolator), den out of range. */
int sxfir_create_translating_interpolator(sxfir_plan **plan, const float *taps_iq, int ntaps, int ratio, int num, int den,
                                          int nchan, int fmt, int device);

/* num mod den and den of a plan of sxfir_create_translating_interpolator; 0, 0 for every other plan. */
int sxfir_plan_translation_tx(const sxfir_plan *plan, int *num, int *den);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_TRANSLATE_TX_H */
