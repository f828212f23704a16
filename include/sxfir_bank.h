/*
 * sxfir_bank.h -- a bank of frequency-translating decimators of the MI355X (gfx950) resampling path: K bands at any centres out of
 * one wideband stream in one pass.  An extension of the C ABI in sxfir.h, exported by the same libsxfir.so.  sxfir.h,
 * SXFIR_ABI_VERSION and the other extension headers are unchanged by it: a caller detects the feature by the symbol (dlsym
 * "sxfir_create_bank") or by sxfir_bank_abi_version() == 1.
 *
 * A translating decimator (sxfir_translate.h) takes one band out of the stream and lands it at 0 Hz; the 4-band channelizer
 * (sxfir_channelizer.h) takes the four bands of the /4 raster.  A caller with a handful of narrow channels whose centres lie where the
 * band plan put them ran K translating plans: K histories, K passes over the same input.  A bank plan reads the stream once, keeps
 * ONE history, and gives every band's output.  The reference (tejeez/sxxcvr, SoapySX/SoapySX.cpp) has no counterpart: the SX1255's
 * base-band decimator is fixed and low-pass (register table SoapySX.cpp:180-208).
 *
 * Definition.  Band k of channel c is, bit for bit, the output of the plan
 *
 *   sxfir_create_translating(taps_k, ntaps, ratio, num[k], den[k], nchan, fmt)
 *
 * over the same stream: the chains under the (jsplit, cw) and rotation that sxfir_contract and sxfir_contract_rotation report for
 * that plan (the bank reports the same), sxfir_translate.h's six roundings of the rotation at the ABSOLUTE output index m, on the
 * table of sxfir_design_rotator(den[k]); SXFIR_CF16 output is rounded to half once, after the rotation.  The bits do not depend on
 * how the stream is cut into calls, or on which of the bank's two kernels ran a call.
 *
 * Formats are those of the translating decimator: SXFIR_CF32, SXFIR_CF16, and SXFIR_S32 wire words in with SXFIR_CF32 out.
 * Decimation only.
 *
 * Output layout (the channelizer's): band k of channel c starts at out_dev + c * out_stride + k * band_stride, in samples of the
 * output format; *n_out is the outputs PER BAND.  band_stride below the call's outputs per band, or two strides under which bands
 * and channels overlap (sxfir_channelize's rule), answer SXFIR_EINVAL, plan untouched.
 *
 * The plan is a /ratio decimator for everything about the stream: ONE history of ntaps input samples per channel whatever K is;
 * sxfir_reset, sxfir_set_history, sxfir_set_position (every band's phase follows produced = ceil(consumed / ratio)),
 * sxfir_position, sxfir_outputs_for, sxfir_contract, sxfir_contract_rotation, sxfir_set_kernel, sxfir_launch_geometry and
 * sxfir_destroy take it; sxfir_taps_are_complex answers 1; sxfir_plan_translation, sxfir_plan_bands, sxfir_plan_rational and
 * sxfir_plan_arbitrary answer zeros.  sxfir_decimate, sxfir_time_decimate, sxfir_interpolate*, sxfir_channelize, sxfir_synthesize
 * and sxfir_resample* refuse it with SXFIR_EINVAL, plan untouched; sxfir_decimate_bank refuses every other plan the same way.
 *
 * SXFIR_KERNEL_TILED exists for ratio 4 with 128 taps on SXFIR_CF32 (decim4_bank_kernel: a tile is staged once and walked by every
 * band): it takes a call that starts on an output boundary (a stream position that is a multiple of 4) and whose output is 16-byte
 * aligned with an even out_stride and an even band_stride.  Under SXFIR_KERNEL_AUTO any other call of that plan runs the generic
 * kernel (decim_bank_generic_kernel, the same bits); under SXFIR_KERNEL_TILED it answers SXFIR_EUNSUPPORTED, plan untouched.  Every
 * other shape or format runs the generic kernel and answers SXFIR_EUNSUPPORTED to sxfir_set_kernel(SXFIR_KERNEL_TILED).
 */
#ifndef SXFIR_BANK_H
#define SXFIR_BANK_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the six entry points below. */
#define SXFIR_BANK_ABI_VERSION 1
#define SXFIR_BANK_MAX_BANDS 16

int sxfir_bank_abi_version(void);

/* taps_iq: nbands * ntaps interleaved (re, im) float pairs, band-major, host, copied -- band k's are what
 * sxfir_design_bandpass(ntaps, ratio, ., ., num[k], den[k]) gives, or anything else.  nbands in 1..16.  num[k]: any int, reduced
 * into [0, den[k]); den[k] in 1..65536, per band (tables from sxfir_design_rotator; bands that share a den share one device table).
 * Refusals, in this order and before the device is looked at: a NULL argument (plan, taps_iq, num, den); ntaps, ratio, nchan, fmt
 * (as sxfir_create); nbands out of 1..16 (SXFIR_EINVAL); the first den[k] out of range (SXFIR_EINVAL; the message names k). */
int sxfir_create_bank(sxfir_plan **plan, const float *taps_iq, int ntaps, int ratio, int nbands, const int *num, const int *den,
                      int nchan, int fmt, int device);

/* One call of the stream: n_in samples per channel in, *n_out outputs PER BAND (sxfir_outputs_for) to every band's row. */
int sxfir_decimate_bank(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                        size_t band_stride, size_t *n_out, void *stream);

/* `iters` back-to-back passes of the call's kernel between events on `stream`; the plan's state is untouched (as sxfir_time_decimate). */
int sxfir_time_decimate_bank(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                             size_t band_stride, int iters, void *stream, float *ms_per_pass);

/* The band count of a plan of sxfir_create_bank; 0 for every other plan. */
int sxfir_plan_bank(const sxfir_plan *plan, int *nbands);

/* num[band] mod den[band] and den[band] of a bank plan; SXFIR_EINVAL for a band off range (every band of another plan is). */
int sxfir_plan_bank_band(const sxfir_plan *plan, int band, int *num, int *den);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_BANK_H */
