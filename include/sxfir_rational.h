/*
 * sxfir_rational.h -- rational (up / down) resamplers of the MI355X (gfx950) resampling path: an extension of the C ABI in
 * sxfir.h, exported by the same libsxfir.so.  sxfir.h, SXFIR_ABI_VERSION and the other extension headers are unchanged by it: a
 * caller detects the feature by the symbol (dlsym "sxfir_create_rational") or by sxfir_rational_abi_version() == 1.
 *
 * Every other plan changes the rate by an integer.  A rational plan produces up outputs for every down inputs in ONE pass
 * (2.4 MS/s -> 1.92 MS/s is 4/5), where a x up interpolation pass that writes up times the stream and a / down decimation pass
 * that drops most of it were needed before.  The reference (tejeez/sxxcvr, SoapySX/SoapySX.cpp) has no counterpart: the SX1255's
 * rates are the master clock over an integer.
 *
 * With real taps h, T = ntaps / up taps per phase and x[<0] = 0:
 *
 *   y[m] = sum_{j=0..T-1} h[j*up + (m*down mod up)] * x[floor(m*down / up) - j]
 *
 * -- sample m*down of the x up interpolator's output.  A unit-gain design is sxfir_design_lowpass(ntaps, max(up, down), beta,
 * gain = up).
 *
 * Stream: after c consumed inputs the plan has produced ceil(c*up / down) outputs, so a call of n inputs yields
 * ceil((c + n)*up / down) - ceil(c*up / down) of them -- possibly none when up < down: the samples then only enter the history.
 * The history is an interpolator's (T input samples per channel); all index arithmetic is 64-bit.  SXFIR_CF32 and SXFIR_CF16
 * (the same storage in and out); SXFIR_S32 is refused: a rational plan sits on neither wire side.
 *
 * Numeric contract: that of the real-tap x up interpolator of the same taps, as sxfir_contract reports it ((2, 1) when T is
 * even, else (1, 1); rotation 0): within each contiguous range of j one fmaf chain from +0.0f over j descending, for I and Q
 * each, the ranges joined by the adjacent-pair tree; SXFIR_CF16 inputs converted half -> float first, the output rounded to half
 * once.  y[m] is bit for bit output m*down of sxfir_create(SXFIR_INTERPOLATE, taps, ntaps, up, ...) over the same stream,
 * whichever kernel runs the call.
 *
 * The plan is an ordinary sxfir_plan: sxfir_reset, sxfir_set_history, sxfir_set_position (produced = ceil(consumed*up / down)),
 * sxfir_position, sxfir_outputs_for, sxfir_contract, sxfir_contract_rotation (0), sxfir_set_kernel, sxfir_launch_geometry and
 * sxfir_destroy take it; sxfir_taps_are_complex and the band queries answer 0.  sxfir_decimate, sxfir_interpolate,
 * sxfir_interpolate_keyed, sxfir_time_decimate, sxfir_time_interpolate, sxfir_channelize and sxfir_synthesize refuse it with
 * SXFIR_EINVAL and leave it untouched, as sxfir_resample refuses every other plan.
 *
 * SXFIR_KERNEL_TILED exists for up 4 / down 5 with 128 taps on SXFIR_CF32 (resample45_kernel); it takes a call that starts at a
 * stream position that is a multiple of 5 and whose output is 16-byte aligned with an even channel stride.  Under
 * SXFIR_KERNEL_AUTO any other call of that plan runs the generic kernel (the same bits); under SXFIR_KERNEL_TILED it answers
 * SXFIR_EUNSUPPORTED, plan untouched.  Every other shape runs resample_generic_kernel and answers SXFIR_EUNSUPPORTED to
 * sxfir_set_kernel(SXFIR_KERNEL_TILED).
 */
#ifndef SXFIR_RATIONAL_H
#define SXFIR_RATIONAL_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the five entry points below. */
#define SXFIR_RATIONAL_ABI_VERSION 1

int sxfir_rational_abi_version(void);

/* taps: ntaps real floats, host, copied; up and down in 2..4096, coprime; ntaps a multiple of up. */
int sxfir_create_rational(sxfir_plan **plan, const float *taps, int ntaps, int up, int down, int nchan, int fmt, int device);

/* As sxfir_interpolate: n_in inputs per channel, channel c at in_dev + c * in_stride and out_dev + c * out_stride (samples). */
int sxfir_resample(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                   size_t *n_out, void *stream);

/* As sxfir_time_decimate: `iters` back-to-back passes from the same filter state; position and history stay as they were. */
int sxfir_time_resample(sxfir_plan *plan, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                        int iters, void *stream, float *ms_per_pass);

/* The plan's ratio; 0, 0 for every plan that sxfir_create_rational did not create. */
int sxfir_plan_rational(const sxfir_plan *plan, int *up, int *down);

#ifdef __cplusplus
}
#endif

#endif /* SXFIR_RATIONAL_H */
