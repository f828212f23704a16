/*
 * sxfir_complex.h -- complex-tap (band-pass) decimators of the MI355X (gfx950) resampling path: an extension of the C ABI
 * in sxfir.h, exported by the same libsxfir.so.  sxfir.h and SXFIR_ABI_VERSION are unchanged by it: a caller detects the
 * feature by the symbol (dlsym "sxfir_create_complex") or by sxfir_complex_abi_version() == 1.
 *
 * What it replaces in the reference (tejeez/sxxcvr, SoapySX/SoapySX.cpp = "SX.cpp"): the SX1255's fixed base-band
 * decimator, which setSampleRate only programs the divider of (register table SX.cpp:180-208).  That filter is low-pass
 * and real: the only band it can take out of the wideband stream is the one around 0 Hz.  With complex taps
 * h = a + j b a plan takes any slice -- sub-band k of the D-channel raster, a one-sided filter -- in ONE pass over the
 * input, where two real-tap plans (Re h, Im h) and a combining kernel of the caller's own were needed before.
 *
 *   y[m] = sum_k h[k] x[m*ratio - k],   h[k] = a[k] + j b[k]
 *
 * History, stream positions, x[<0] = 0 and the storage formats are those of a real-tap plan.
 *
 * Numeric contract: let A = a (*) x and B = b (*) x be the two REAL-tap results, each under the plan's contract as
 * sxfir_contract / sxfir_contract_rotation report it (the same chains from +0.0f, the same trees as a real-tap plan of this
 * shape).  Then y.re = fsub_rn(A.re, B.im) and y.im = fadd_rn(A.im, B.re), one rounding each.  SXFIR_CF16 output is rounded
 * to half once, after the combine; SXFIR_S32 input goes through convert_rx_buffer (SX.cpp:103-112) on the way in.
 *
 * The plan is an ordinary sxfir_plan: sxfir_decimate, sxfir_time_decimate, sxfir_reset, sxfir_set_history,
 * sxfir_set_position, sxfir_position, sxfir_outputs_for, sxfir_contract, sxfir_contract_rotation, sxfir_set_kernel,
 * sxfir_launch_geometry and sxfir_destroy take it.  SXFIR_KERNEL_TILED exists for ratio 4 with 128 taps on SXFIR_CF32
 * (decim4_cx_kernel); every other shape runs the generic complex kernel and answers SXFIR_EUNSUPPORTED to
 * sxfir_set_kernel(SXFIR_KERNEL_TILED).
 */
#ifndef SXFIR_COMPLEX_H
#define SXFIR_COMPLEX_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the four entry points below. */
#define SXFIR_COMPLEX_ABI_VERSION 1

int sxfir_complex_abi_version(void);

/* As sxfir_create, with complex taps.  taps_iq: ntaps interleaved (re, im) float pairs, host, copied.
 * SXFIR_DECIMATE only: SXFIR_INTERPOLATE returns SXFIR_EUNSUPPORTED with a message. */
int sxfir_create_complex(sxfir_plan **plan, int mode, const float *taps_iq, int ntaps, int ratio, int nchan, int fmt,
                         int device);

/* *is_complex = 1 for a plan of sxfir_create_complex, 0 for a plan of sxfir_create. */
int sxfir_taps_are_complex(const sxfir_plan *plan, int *is_complex);

/* Band-pass design: h[n] = lowpass[n] * exp(j*2*pi*((n*num) mod den)/den), where lowpass is the sxfir_design_lowpass
 * prototype in fp64 (same cutoff 0.5/ratio, beta, gain); the phase is reduced in integers and each component is rounded
 * to fp32 once.  num/den = band centre in cycles per INPUT sample (k/ratio = sub-band k of the output raster: it lands at
 * 0 Hz of the output with no rotation needed).  den >= 1.  taps_iq: ntaps (re, im) pairs.  num = 0 gives the low-pass
 * taps bit for bit, with +0.0 imaginary parts. */
int sxfir_design_bandpass(int ntaps, int ratio, double beta, double gain, int num, int den, float *taps_iq);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_COMPLEX_H */
