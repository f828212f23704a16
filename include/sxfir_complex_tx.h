/*
 * sxfir_complex_tx.h -- complex-tap (band-pass) interpolators of the MI355X (gfx950) resampling path: an extension of the C ABI
 * in sxfir.h, exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION and sxfir_complex.h are unchanged by it
 * (sxfir_create_complex keeps refusing SXFIR_INTERPOLATE): a caller detects the feature by the symbol (dlsym
 * "sxfir_create_complex_interpolator") or by sxfir_complex_tx_abi_version() == 1.
 *
 * The way back from a complex-tap decimator (sxfir_complex.h): one narrowband stream is placed at a band of the x ratio raster
 * in ONE pass, where two real-tap interpolator plans (Re h, Im h) and a combining kernel of the caller's own, or a 4-band
 * synthesizer fed three bands of zeros, were needed before.  The reference (tejeez/sxxcvr, SoapySX/SoapySX.cpp) has no
 * counterpart: the SX1255 interpolates the one band around 0 Hz.
 *
 *   y[n] = sum_j h[j*ratio + n mod ratio] x[n / ratio - j],   h[k] = a[k] + j b[k]
 *
 * The band-centre phasors are on the OUTPUT side: sxfir_design_bandpass(ntaps, ratio, beta, ratio, k, ratio, taps) -- gain =
 * ratio, num/den read as cycles per OUTPUT sample -- places the input at sub-band k of the output raster.
 *
 * History, stream positions, x[<0] = 0, the storage formats and the keying threshold are those of a real-tap interpolator of
 * the same shape (ntaps must be a multiple of ratio).
 *
 * Numeric contract: let A = a (*) x and B = b (*) x be the two REAL-tap interpolator results, each under the plan's contract as
 * sxfir_contract reports it (jsplit ranges of j, one fmaf chain from +0.0f over j descending in each, adjacent-pair tree).
 * Then y.re = fsub_rn(A.re, B.im) and y.im = fadd_rn(A.im, B.re), one rounding each.  SXFIR_CF16: inputs converted half ->
 * float first, the output rounded to half once after the combine.  SXFIR_S32: CF32 in, convert_tx_buffer (SoapySX.cpp:116-137)
 * of the combined CF32 result out.
 *
 * The plan is an ordinary interpolator plan: sxfir_interpolate, sxfir_interpolate_keyed, sxfir_time_interpolate, sxfir_reset,
 * sxfir_set_history, sxfir_set_position, sxfir_position, sxfir_outputs_for, sxfir_contract, sxfir_set_kernel,
 * sxfir_set_tx_threshold, sxfir_launch_geometry and sxfir_destroy take it; sxfir_taps_are_complex answers 1; sxfir_decimate
 * refuses it.  SXFIR_KERNEL_TILED exists on SXFIR_CF32 for ratio 4 with 128 taps and ratio 8 with 256 taps
 * (interp_cx_pass_kernel); every other shape runs the generic complex kernel and answers SXFIR_EUNSUPPORTED to
 * sxfir_set_kernel(SXFIR_KERNEL_TILED).
 */
#ifndef SXFIR_COMPLEX_TX_H
#define SXFIR_COMPLEX_TX_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the two entry points below. */
#define SXFIR_COMPLEX_TX_ABI_VERSION 1

int sxfir_complex_tx_abi_version(void);

/* As sxfir_create(SXFIR_INTERPOLATE, ...), with complex taps.  taps_iq: ntaps interleaved (re, im) float pairs, host, copied. */
int sxfir_create_complex_interpolator(sxfir_plan **plan, const float *taps_iq, int ntaps, int ratio, int nchan, int fmt,
                                      int device);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_COMPLEX_TX_H */
