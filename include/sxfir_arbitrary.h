/*
 * sxfir_arbitrary.h -- arbitrary-rate resamplers of the MI355X (gfx950) resampling path: an extension of the C ABI in sxfir.h,
 * exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION and the other extension headers are unchanged by it: a caller
 * detects the feature by the symbol (dlsym "sxfir_create_arbitrary") or by sxfir_arbitrary_abi_version() == 1.
 *
 * Every other plan changes the rate by an integer or by a small fraction up / down (sxfir_rational.h).  An arbitrary-rate plan
 * takes any step of 1/16 .. 16 input samples per output sample, to 2^-32 of a sample, and the step can change in mid-stream without
 * a phase jump: a 20 ppm clock correction, a receiver that tracks a drifting clock, 2.4 MS/s -> 2.048 MS/s.  The reference
 * (tejeez/sxxcvr, SoapySX/SoapySX.cpp) has no counterpart: the SX1255's rates are the master clock over an integer.
 *
 * The plan is a polyphase bank of P = nphases phases x T = ntaps / P taps per phase with linear interpolation between adjacent
 * phases, driven by a 64.32 fixed-point time.
 *
 * Taps: h, ntaps = P * T real floats in the x P interpolator's layout: phase p is h[j*P + p], j = 0..T-1.  A unit-gain design is
 * sxfir_design_lowpass(ntaps, ceil(P * max(1, step / 2^32)), beta, gain = P).
 * Step: input samples per output sample, unsigned Q32.32 (uint64_t), in [2^28, 2^36].
 * Time: t, the time of the next output in input samples, held exactly as (int64 sample index, uint32 fraction).  It starts at 0 and
 * every output adds step.
 *
 * The output at time t.  With z = frac(t) * P, a 44-bit integer product:
 *
 *   n = floor(t)      p = z >> 32      alpha = float((z & 0xffffffff) >> 8) * 2^-24      k = n*P + p  (64 bits)
 *
 *   a = u[k], b = u[k + 1]       u[.] = the output of the x P interpolator of the same taps over the same stream
 *   d = b - a                    one rounding, for I and Q each
 *   y = fmaf(alpha, d, a)
 *
 * alpha has 24 bits and is exact in float.  u[k] has the bits of sxfir_create(SXFIR_INTERPOLATE, taps, ntaps, P, ...) under the
 * contract sxfir_contract reports ((2, 1) when T is even, else (1, 1); rotation 0): within each contiguous range of j one fmaf chain
 * from +0.0f over j descending, for I and Q each, the ranges joined by the adjacent-pair tree.  When p + 1 == P, u[k + 1] is phase 0
 * at input n + 1: no zero tap is invented to make that case uniform, so 0 * Inf does not appear where the interpolator has none.
 * SXFIR_CF16 inputs are converted half -> float first; a SXFIR_CF16 output is rounded to half once, after the blend.  SXFIR_CF32
 * and SXFIR_CF16 (the same storage in and out); SXFIR_S32 is refused: the plan sits on neither wire side.
 *
 * Stream: one sample of look-ahead, uniformly.  The output at t is produced by the call that delivers x[floor(t) + 1], whether or
 * not its alpha and phase need that sample: a call of n_in inputs on a plan that has consumed c yields
 *
 *   max(0, ceil(((c + n_in - 1) * 2^32 - t) / step))
 *
 * outputs (sxfir_arbitrary_outputs) -- possibly none.  The count does not depend on how the stream is cut into calls.  After any
 * call floor(t) >= consumed - 1, so the chains reach at most T samples into the history: hist_len is T rounded up to even, as a
 * rational plan's.  All index arithmetic is 64-bit or wider.
 *
 * State: sxfir_set_rate changes step only -- t stays, so the phase is continuous; sxfir_reset sets t = 0; sxfir_set_position(c) sets
 * t = c * 2^32 and produced = 0 (the count of outputs since then); sxfir_set_time places a stream exactly.  sxfir_set_history,
 * sxfir_position, sxfir_outputs_for, sxfir_contract, sxfir_contract_rotation (0), sxfir_set_kernel, sxfir_launch_geometry and
 * sxfir_destroy take the plan; sxfir_taps_are_complex, sxfir_plan_rational and the band queries answer 0.  sxfir_decimate,
 * sxfir_interpolate, sxfir_interpolate_keyed, sxfir_time_decimate, sxfir_time_interpolate, sxfir_resample, sxfir_time_resample,
 * sxfir_channelize and sxfir_synthesize refuse it with SXFIR_EINVAL and leave it untouched, as sxfir_resample_arbitrary refuses
 * every other plan.
 *
 * SXFIR_KERNEL_TILED exists for 128 phases x 32 taps on SXFIR_CF32 (resample_arb_kernel); it takes a call whose step lies in
 * [2^31, 2^33] (0.5 .. 2 inputs per output) and whose output is 16-byte aligned with an even channel stride, at any stream position
 * and time.  Under SXFIR_KERNEL_AUTO any other call of that plan runs the generic kernel (the same bits); under SXFIR_KERNEL_TILED
 * it answers SXFIR_EUNSUPPORTED, plan untouched.  sxfir_set_rate may move a plan in and out of the range between calls.  Every other
 * shape runs resample_arb_generic_kernel and answers SXFIR_EUNSUPPORTED to sxfir_set_kernel(SXFIR_KERNEL_TILED).
 */
#ifndef SXFIR_ARBITRARY_H
#define SXFIR_ARBITRARY_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the nine entry points below. */
#define SXFIR_ARBITRARY_ABI_VERSION 1

int sxfir_arbitrary_abi_version(void);

/* taps: ntaps real floats, host, copied; nphases in 2..4096; ntaps a multiple of nphases; step in [2^28, 2^36].  Refusals, in this
 * order and before the device is looked at: a NULL argument, ntaps, nphases, ntaps % nphases, step, nchan, the format's range
 * (SXFIR_EINVAL each), SXFIR_S32 (SXFIR_EUNSUPPORTED). */
int sxfir_create_arbitrary(sxfir_plan **plan, const float *taps, int ntaps, int nphases, uint64_t step, int nchan, int fmt, int device);

/* The step of the outputs from now on; the time of the next output stays. */
int sxfir_set_rate(sxfir_plan *plan, uint64_t step);

/* Place the stream: `consumed` inputs taken, the next output at t_index + t_frac * 2^-32.  t_index < consumed - 1 is refused (the
 * output's window would lie below the history); produced = 0.  sxfir_set_history gives the samples in front of `consumed`. */
int sxfir_set_time(sxfir_plan *plan, int64_t consumed, int64_t t_index, uint32_t t_frac);

/* The plan's phases, step and time; zeros for every plan that sxfir_create_arbitrary did not create. */
int sxfir_plan_arbitrary(const sxfir_plan *plan, int *nphases, uint64_t *step, int64_t *t_index, uint32_t *t_frac);

/* As sxfir_resample: n_in inputs per channel, channel c at in_dev + c * in_stride and out_dev + c * out_stride (samples).  A call
 * takes fewer than 2^31 inputs per channel (SXFIR_EINVAL otherwise, plan untouched); so does the timed form below. */
int sxfir_resample_arbitrary(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                             size_t *n_out, void *stream);

/* As sxfir_time_resample: `iters` back-to-back passes from the same filter state; position, time and history stay as they were. */
int sxfir_time_resample_arbitrary(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev,
                                  size_t out_stride, int iters, void *stream, float *ms_per_pass);

/* Host only, no GPU needed: the count rule above in 128-bit arithmetic -- the outputs of a call of n_in inputs on a stream that has
 * consumed `consumed` with the next output at (t_index, t_frac), and the time after it.  t_index >= -1, consumed >= 0, consumed and
 * n_in below 2^62, step in range; SXFIR_EINVAL otherwise.  What the plan itself counts with. */
int sxfir_arbitrary_outputs(int64_t t_index, uint32_t t_frac, uint64_t step, int64_t consumed, uint64_t n_in, uint64_t *n_out,
                            int64_t *t_index_after, uint32_t *t_frac_after);

/* Host only, no GPU needed: where output m of a call lies, relative to the call -- rel_q32 = t - (consumed - 1) * 2^32 of the call's
 * first output (>= 0).  *n_rel = floor(rel_q32 + m * step) (input n_rel - 1 of the call; 0 is the newest history sample), *p and
 * *alpha as defined above.  m * step is taken as high and low halves: it does not fit 64 bits at 2^28 outputs of step 2^36.  The
 * function the kernels call. */
int sxfir_arbitrary_locate(uint64_t rel_q32, uint64_t step, uint64_t m, int nphases, int64_t *n_rel, int *p, float *alpha);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_ARBITRARY_H */
