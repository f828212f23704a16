/*
 * sxfir_translate.h -- frequency-translating decimators of the MI355X (gfx950) resampling path: an extension of the C ABI in
 * sxfir.h, exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION and the other extension headers are unchanged by it: a
 * caller detects the feature by the symbol (dlsym "sxfir_create_translating") or by sxfir_translate_abi_version() == 1.
 *
 * A complex-tap decimator (sxfir_complex.h) takes any slice of the wideband stream in one pass, but leaves it at base-band only
 * when the band centre lies on the output raster, k / ratio: a band centred at num / den cycles per input sample comes out at
 * (num * ratio / den) mod 1 cycles per output sample, and a second pass over the output was needed to turn it down.  A
 * translating plan does that turn in the same pass.  The reference (tejeez/sxxcvr, SoapySX/SoapySX.cpp) has no counterpart: the
 * SX1255's base-band decimator is fixed and low-pass (register table SoapySX.cpp:180-208).
 *
 * Definition.  Let z[m] = sum_k h[k] x[m*ratio - k] be the complex-tap decimator's result for the same taps, and
 * s = (num * ratio) mod den.  Then
 *
 *   y[m] = z[m] * w[(m * s) mod den],   w[i] = exp(-j 2 pi i / den)
 *
 * With h = sxfir_design_bandpass(ntaps, ratio, ., ., num, den) the band centred at num / den lands at 0 Hz of the output.
 *
 * Stream rules: m is the ABSOLUTE output index -- `produced` of sxfir_position plus the index within the call -- so the phase is
 * continuous over any split of the stream into calls.  It follows sxfir_set_position (produced = ceil(consumed / ratio)) and
 * starts again at 0 after sxfir_reset.  The index (m * s) mod den is reduced exactly, in integers, as sxfir_design_bandpass
 * reduces its phase: no drift, however long the stream.  History, x[<0] = 0 and the storage formats are those of
 * sxfir_create_complex: SXFIR_CF32, SXFIR_CF16, and SXFIR_S32 wire words in with SXFIR_CF32 out.  Decimation only.
 *
 * The table: w[i].re = cos(2 pi i / den), w[i].im = -sin(2 pi i / den), each computed in fp64 from the integer i and rounded to
 * fp32 once; the quarter turns are exact (their zeros +0.0f), w[0] = (1.0f, +0.0f).  sxfir_design_rotator is the one function
 * that makes it: the creator calls it and copies the result to the device, so a caller can reproduce a plan's output bit for
 * bit from the complex plan's without a second math library.
 *
 * Numeric contract: z[m] has the bits of the sxfir_create_complex plan of the same shape -- sxfir_complex.h's contract under the
 * (jsplit, cw) and rotation that sxfir_contract and sxfir_contract_rotation report, in float32 whatever the storage format.  Then
 *
 *   y.re = fsub_rn(fmul_rn(z.re, w.re), fmul_rn(z.im, w.im))
 *   y.im = fadd_rn(fmul_rn(z.re, w.im), fmul_rn(z.im, w.re))
 *
 * six roundings, no fused multiply-add; SXFIR_CF16 output is rounded to half once, after the rotation.  s = 0 (a centre on the
 * output raster) multiplies by (1, +0): that is NOT promised to reproduce the complex plan's bits -- signed zeros and Inf * 0
 * differ -- and such a caller wants sxfir_create_complex.
 *
 * The plan is an ordinary complex-tap decimator plan: sxfir_decimate, sxfir_time_decimate, sxfir_reset, sxfir_set_history,
 * sxfir_set_position, sxfir_position, sxfir_outputs_for, sxfir_contract, sxfir_contract_rotation, sxfir_set_kernel,
 * sxfir_launch_geometry and sxfir_destroy take it; sxfir_taps_are_complex answers 1, the band and rational queries 0; the
 * interpolating, band and rational entry points refuse it as they refuse a complex-tap decimator.
 *
 * SXFIR_KERNEL_TILED exists for ratio 4 with 128 taps on SXFIR_CF32 (decim4_mix_kernel): it takes a call that starts on an
 * output boundary (a stream position that is a multiple of 4) and whose output is 16-byte aligned with an even channel stride.
 * Under SXFIR_KERNEL_AUTO any other call of that plan runs the generic kernel (decim_mix_generic_kernel, the same bits); under
 * SXFIR_KERNEL_TILED it answers SXFIR_EUNSUPPORTED, plan untouched.  Every other shape or format runs the generic kernel and
 * answers SXFIR_EUNSUPPORTED to sxfir_set_kernel(SXFIR_KERNEL_TILED).
 */
#ifndef SXFIR_TRANSLATE_H
#define SXFIR_TRANSLATE_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the four entry points below. */
#define SXFIR_TRANSLATE_ABI_VERSION 1

int sxfir_translate_abi_version(void);

/* The rotation table: den (re, im) float pairs, w[i] = exp(-j 2 pi i / den).  den in 1..65536 (at most 512 KiB). */
int sxfir_design_rotator(int den, float *w_iq);

/* As sxfir_create_complex(SXFIR_DECIMATE, ...), with the output turned by w[(m * s) mod den], s = (num * ratio) mod den.
 * taps_iq: ntaps interleaved (re, im) float pairs, host, copied.  num: any int, reduced into [0, den); den in 1..65536.
 * Refusals, in this order and before the device is looked at: a NULL argument, ntaps, ratio, nchan, fmt (as sxfir_create),
 * den out of range. */
int sxfir_create_translating(sxfir_plan **plan, const float *taps_iq, int ntaps, int ratio, int num, int den, int nchan,
                             int fmt, int device);

/* num mod den and den of a plan of sxfir_create_translating; 0, 0 for every other plan. */
int sxfir_plan_translation(const sxfir_plan *plan, int *num, int *den);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_TRANSLATE_H */
