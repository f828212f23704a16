/*
 * sxfir_bank_tx.h -- a bank of frequency-translating interpolators of the MI355X (gfx950) resampling path, the tuner bank's way back:
 * K base-band streams, each turned to its own centre and interpolated x L with its own complex taps, summed into ONE wideband stream
 * in one pass.  An extension of the C ABI in sxfir.h, exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION and the other
 * extension headers are unchanged by it: a caller detects the feature by the symbol (dlsym "sxfir_create_bank_interpolator") or by
 * sxfir_bank_tx_abi_version() == 1.
 *
 * A translating interpolator (sxfir_translate_tx.h) puts one band at one centre; the 4-band synthesizer (sxfir_synthesizer.h) takes
 * the four centres of the x4 raster and one real prototype.  A caller who tuned K narrow channels out of a stream (sxfir_bank.h),
 * worked on them and wants them back ran K translating interpolators, each writing a whole wideband stream, and K - 1 add passes
 * of their own.  A combiner plan writes the output once; no intermediate wideband stream exists.  The reference (tejeez/sxxcvr,
 * SoapySX/SoapySX.cpp) has no counterpart: the SX1255 interpolates what snd_pcm_writei hands it (SoapySX.cpp:1093), one band at 0 Hz.
 *
 * Definition.  Let y_k be, bit for bit, the float32 result of the plan
 *
 *   sxfir_create_translating_interpolator(taps_k, ntaps, ratio, num[k], den[k], nchan, SXFIR_CF32)
 *
 * over band k's stream: sxfir_translate_tx.h's rotation of the input at its ABSOLUTE index (six roundings, no fused multiply-add,
 * the raw history rotated where it is read) on the table of sxfir_design_rotator(den[k]), then the complex-tap interpolator's
 * chains under the contract that plan reports (the combiner reports the same).  The output is
 *
 *   acc = y_0;   acc = fadd_rn(acc, y_k)   for k = 1, 2, .. K - 1 in this order, re and im each.
 *
 * With K = 1 nothing is added: the bits are the translating interpolator's, signed zeros included.  SXFIR_CF16: half -> float on
 * the way in, the rotation and the sum in float32, the output rounded to half ONCE, after the last add.  SXFIR_S32: SXFIR_CF32 in,
 * the convert_tx_buffer words of acc out, under sxfir_set_tx_threshold.  The bits do not depend on how the stream is cut into calls,
 * or on which of the combiner's two kernels ran a call.
 *
 * Input layout (the synthesizer's): band k of channel c starts at in_dev + c * in_stride + k * band_stride, in samples of the input
 * format; n_in counts the inputs PER BAND; *n_out = ratio * n_in outputs per channel go to out_dev + c * out_stride.  band_stride
 * below n_in, two strides under which bands and channels overlap (sxfir_synthesize's rule with K - 1 in the place of 3), or, with
 * nchan > 1, out_stride below ratio * n_in answer SXFIR_EINVAL, plan and output untouched.
 *
 * The plan is a x ratio interpolator for everything about the stream: ONE position -- `consumed` counts inputs per band, every band's
 * phase follows it --, a history of ntaps / ratio RAW samples per band and channel inside the plan; sxfir_reset, sxfir_set_position,
 * sxfir_position, sxfir_outputs_for, sxfir_contract, sxfir_set_kernel, sxfir_set_tx_threshold, sxfir_launch_geometry and sxfir_destroy
 * take it; sxfir_taps_are_complex answers 1.  sxfir_set_history answers SXFIR_EUNSUPPORTED (the synthesizer's reason: one stride
 * cannot name bands and channels).  sxfir_plan_bank, sxfir_plan_translation, sxfir_plan_translation_tx, sxfir_plan_bands,
 * sxfir_plan_synthesis_bands, sxfir_plan_rational and sxfir_plan_arbitrary answer zeros.  Every other processing entry point --
 * sxfir_interpolate, sxfir_interpolate_keyed, sxfir_time_interpolate, sxfir_decimate*, sxfir_decimate_bank, sxfir_channelize,
 * sxfir_synthesize, sxfir_resample* -- refuses it with SXFIR_EINVAL, plan untouched; sxfir_interpolate_bank refuses every other
 * plan the same way.  A failed call leaves position, history and output as they were.
 *
 * SXFIR_KERNEL_TILED exists for ratio 4 with 128 taps on SXFIR_CF32 (interp4_bank_kernel: a tile's K band images are staged, turned
 * and filtered one after the other, the sum is held on chip and the tile is stored once): it takes a call whose output is 16-byte
 * aligned with an even out_stride, at any stream position and with any in_stride or band_stride.  Under SXFIR_KERNEL_AUTO any other
 * call of that plan runs the generic kernel (interp_bank_generic_kernel, the same bits); under SXFIR_KERNEL_TILED it answers
 * SXFIR_EUNSUPPORTED, plan untouched.  Every other shape or format runs the generic kernel and answers SXFIR_EUNSUPPORTED to
 * sxfir_set_kernel(SXFIR_KERNEL_TILED).
 */
#ifndef SXFIR_BANK_TX_H
#define SXFIR_BANK_TX_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the six entry points below. */
#define SXFIR_BANK_TX_ABI_VERSION 1
#define SXFIR_BANK_TX_MAX_BANDS 16

int sxfir_bank_tx_abi_version(void);

/* taps_iq: nbands * ntaps interleaved (re, im) float pairs, band-major, host, copied -- band k's are what
 * sxfir_design_bandpass(ntaps, ratio, ., ., 0, 1) gives (the band is low-pass in front of its rotation), or anything else.  nbands
 * in 1..16.  num[k]: any int, reduced into [0, den[k]); den[k] in 1..65536, per band (tables from sxfir_design_rotator; bands that
 * share a den share one device table).  Refusals, in this order and before the device is looked at: a NULL argument (plan, taps_iq,
 * num, den); ntaps, ratio, nchan, fmt (as sxfir_create_translating_interpolator, ntaps % ratio included); nbands out of 1..16
 * (SXFIR_EINVAL); the first den[k] out of range (SXFIR_EINVAL; the message names k). */
int sxfir_create_bank_interpolator(sxfir_plan **plan, const float *taps_iq, int ntaps, int ratio, int nbands, const int *num,
                                   const int *den, int nchan, int fmt, int device);

/* One call of the stream: n_in samples per band and channel in, *n_out = ratio * n_in outputs per channel. */
int sxfir_interpolate_bank(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, size_t band_stride, void *out_dev,
                           size_t out_stride, size_t *n_out, void *stream);

/* `iters` back-to-back passes of the call's kernel between events on `stream`; the plan's state is untouched (as sxfir_time_interpolate). */
int sxfir_time_interpolate_bank(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, size_t band_stride,
                                void *out_dev, size_t out_stride, int iters, void *stream, float *ms_per_pass);

/* The band count of a plan of sxfir_create_bank_interpolator; 0 for every other plan. */
int sxfir_plan_bank_tx(const sxfir_plan *plan, int *nbands);

/* num[band] mod den[band] and den[band] of a combiner plan; SXFIR_EINVAL for a band off range (every band of another plan is). */
int sxfir_plan_bank_tx_band(const sxfir_plan *plan, int band, int *num, int *den);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_BANK_TX_H */
