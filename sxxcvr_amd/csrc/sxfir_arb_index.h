// Index arithmetic of the arbitrary-rate resamplers (include/sxfir_arbitrary.h): where output m of a call lies (arb_locate: the one
// function the two kernels, sxfir_arbitrary_locate and through it the CPU tests run) and how many outputs a call yields
// (arb_outputs: the one statement of the count rule, behind sxfir_arbitrary_outputs, outputs_for and the commit of a
// call).  Plain C++ but for the high half of a 64 x 64 bit product, which is __umul64hi on the device and a 128-bit
// product on the host.  No HIP header is needed to read it.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SXFIR_HD __host__ __device__
#else
#define SXFIR_HD
#endif

namespace sxfir {

static const uint64_t ARB_STEP_MIN = 1ull << 28, ARB_STEP_MAX = 1ull << 36;     // 1/16 .. 16 inputs per output, Q32.32

SXFIR_HD inline uint64_t arb_mul_hi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// Output m of a call: its time relative to the call is rel + m * step (Q.32; rel = t - (consumed - 1) * 2^32 >= 0 of the call's first
// output), a sum of up to 96 bits -- m * step alone passes 2^64 at 2^28 outputs of step 2^36 -- taken as high and low halves.
// *n_rel = floor of it (input n_rel - 1 of the call; 0 is the newest history sample); with z = frac * nphases, a 44-bit product:
// *p = z >> 32, *alpha = the next 24 bits of z as a float in [0, 1) (exact).
SXFIR_HD inline void arb_locate(uint64_t rel, uint64_t step, uint64_t m, int nphases, long long *n_rel, int *p, float *alpha)
{
    const uint64_t lo = m * step;
    uint64_t hi = arb_mul_hi(m, step);
    const uint64_t sum = rel + lo;
    hi += sum < lo ? 1u : 0u;
    *n_rel = (long long)((hi << 32) | (sum >> 32));
    const uint64_t z = (sum & 0xffffffffull) * (uint64_t)nphases;
    *p = (int)(z >> 32);
    *alpha = (float)(uint32_t)((z & 0xffffffffull) >> 8) * 5.9604644775390625e-08f;       // 2^-24
}

// The count rule.  The output at time t is produced by the call that delivers x[floor(t) + 1]: a call of n_in inputs on a plan that
// has consumed c yields max(0, ceil(((c + n_in - 1) * 2^32 - t) / step)) outputs, every one of which adds step to t.  In 128-bit
// arithmetic; t_index >= -1 and consumed, n_in < 2^62.
inline void arb_outputs(int64_t t_index, uint32_t t_frac, uint64_t step, int64_t consumed, uint64_t n_in, uint64_t *n_out,
                        int64_t *t_index_after, uint32_t *t_frac_after)
{
    typedef __int128 i128;
    const i128 t = ((i128)t_index << 32) + t_frac;
    const i128 limit = ((i128)consumed + (i128)n_in - 1) << 32;
    i128 n = 0;
    if (limit > t) n = (limit - t + (i128)step - 1) / (i128)step;
    const i128 after = t + n * (i128)step;
    *n_out = (uint64_t)n;
    *t_index_after = (int64_t)(after >> 32);
    *t_frac_after = (uint32_t)(after & 0xffffffff);
}

}  // namespace sxfir
