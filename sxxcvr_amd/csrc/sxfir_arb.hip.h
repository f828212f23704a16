// Arbitrary-rate resampling (include/sxfir_arbitrary.h), gfx950: the generic kernel of every shape and the one tiled shape, 128 phases
// x 32 taps on CF32 at 0.5 .. 2 inputs per output.
//
// A polyphase bank of P phases x T taps per phase with linear interpolation between adjacent phases, driven by a fixed-point time
// that advances by `step` per output.  With u[.] the output of the x P interpolator of the same taps over the same stream and k the
// sample of it at or below the output's time (arb_locate, sxfir_arb_index.h):
//
//   y = fmaf(alpha, u[k + 1] - u[k], u[k])            for I and Q each
//
// u[k] and u[k + 1] under the interpolator's contract: per contiguous range of j one fmaf chain from +0.0f over
// j descending, the ranges joined by the adjacent-pair tree.  u[k + 1] of the last phase is phase 0 of the NEXT input: another
// window, not another tap -- no zero tap is invented, so no 0 * Inf appears where the interpolator has none.
//
// The kernels work relative to the call: `rel` is the time of the call's first output less (consumed - 1) * 2^32, so input n_rel - 1
// of the call (n_rel = floor(rel + m * step)) is the newest sample of chain u[k], and n_rel = 0 is the newest history sample.  The
// host has made sure that every output of the call has its look-ahead sample inside the call (arb_outputs).
//
// resample_arb_kernel.  A tile is 256 consecutive outputs of one wave, four consecutive outputs per lane; four waves (one workgroup)
// share the tap table.
//   * the tile's first input follows from rel + tile * 256 * step; the tile's input span (at step 2: 2 * 256 + T + 2 samples) goes
//     into the wave's own LDS image, sample by sample through sample_at, so the history below the call and the call's end need no
//     case of their own and a position needs no alignment;
//   * the (P + 1) x T tap table sits in LDS phase-major with j DESCENDING (ascending image samples), the row for phase P a copy of
//     phase 0's, rows of T + 4 floats: a lane reads four taps per ds_read_b128, and the pad spreads the rows' first banks;
//   * both chains of an output share one window of T + 1 samples in registers; a lane whose phase is the last one takes its second
//     chain's samples one place later (a select per sample, no second read);
//   * per-lane phases: the taps cannot be scalar operands here.  The kernel is LDS-bound by construction;
//   * whole tiles leave as two 16-byte stores per lane; the call's last tile element by element, nothing past n_out;
//   * the history carry-over is the generic path's history_kernel.
// LDS: 18 576 B of taps and 4 x 4416 B of images per workgroup.
//
// New code: the reference's rates are the SX1255's master clock over an integer (SoapySX.cpp:180-208).
#pragma once

#include "sxfir_arb_index.h"
#include "sxfir_common.hip.h"           // f32x4
#include "sxfir_kernels.hip.h"          // GenericArgs, interp_generic_output, sample_at

namespace sxfir {

__device__ __forceinline__ float2 arb_blend(float alpha, float2 a, float2 b)
{
    return make_float2(__builtin_fmaf(alpha, __fsub_rn(b.x, a.x), a.x), __builtin_fmaf(alpha, __fsub_rn(b.y, a.y), a.y));
}

// One output per thread, any P / T / step / format / channel count / stride: two outputs of the interpolator
// (interp_generic_output, the statement of the contract) on the x P interpolator's GenericArgs (ratio = P) with a.arb_rel and
// a.arb_step, and the blend.  FO::store rounds to half once for CF16.
template <typename F>
__global__ __launch_bounds__(256) void resample_arb_generic_kernel(const GenericArgs a)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_out) return;
    const int ch = blockIdx.y;
    const char *in = (const char *)a.in + sizeof(typename F::storage) * a.in_stride * ch;
    const char *hist = (const char *)a.hist + sizeof(typename F::storage) * a.hist_stride * ch;
    char *out = (char *)a.out + sizeof(typename F::storage) * a.out_stride * ch;
    long long n_rel;
    int p;
    float alpha;
    arb_locate(a.arb_rel, a.arb_step, (uint64_t)i, a.ratio, &n_rel, &p, &alpha);
    const bool wrap = p + 1 == a.ratio;
    const float2 A = interp_generic_output<F>(a, a.taps, in, hist, n_rel - 1, p);
    const float2 B = interp_generic_output<F>(a, a.taps, in, hist, wrap ? n_rel : n_rel - 1, wrap ? 0 : p + 1);
    F::store(out, i, arb_blend(alpha, A, B), a.thr2);
}

struct ArbTile {
    static constexpr int P = 128, T = 32;
    static constexpr int TILE = 256;                          // outputs per tile (one wave), 4 per lane
    static constexpr int WAVES = 4;                           // per workgroup
    static constexpr int ROW = T + 4;                         // floats per row of the LDS tap table
    static constexpr int TABLE = (P + 1) * ROW;               // 4644 floats = 1161 chunks of 16 bytes
    static constexpr int IMG = 2 * TILE + T + 8;              // samples per image: 2 * 256 + T + 2 are read at step 2
    static constexpr unsigned long long STEP_MIN = 1ull << 31, STEP_MAX = 1ull << 33;
};

struct ArbTileArgs {
    const void *in, *hist;
    void *out;
    const float *table;             // ArbTile::TABLE floats: row p holds h[(T - 1 - i) * P + p] at i, row P repeats row 0
    long long n_in, n_out;
    long long in_stride, out_stride, hist_stride;
    unsigned long long rel, step;
    int hist_len;
    int n_tiles, n_groups;          // tiles per channel; workgroups per channel
};

__global__ __launch_bounds__(256) void resample_arb_kernel(const ArbTileArgs ka)
{
    using C = ArbTile;
    static_assert(C::TABLE % 4 == 0 && C::ROW % 4 == 0, "the table is copied and read in 16-byte chunks");
    __shared__ __attribute__((aligned(16))) float table[C::TABLE];
    __shared__ __attribute__((aligned(16))) float2 images[C::WAVES][C::IMG];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ch = blockIdx.y;
    const char *in = (const char *)ka.in + sizeof(float2) * ka.in_stride * ch;
    const char *hist = (const char *)ka.hist + sizeof(float2) * ka.hist_stride * ch;
    float *out = (float *)ka.out + 2 * ka.out_stride * ch;
    GenericArgs a{};                                          // what sample_at reads
    a.hist_len = ka.hist_len;

    for (int c = threadIdx.x; c < C::TABLE / 4; c += 256) reinterpret_cast<f32x4 *>(table)[c] = reinterpret_cast<const f32x4 *>(ka.table)[c];
    __syncthreads();

    float2 *img = images[wave];
    for (int tile = blockIdx.x * C::WAVES + wave; tile < ka.n_tiles; tile += ka.n_groups * C::WAVES) {
        const unsigned long long m0 = (unsigned long long)tile * C::TILE;
        long long n0, n_last;
        int p_any;
        float alpha_any;
        arb_locate(ka.rel, ka.step, m0, C::P, &n0, &p_any, &alpha_any);
        arb_locate(ka.rel, ka.step, m0 + C::TILE - 1, C::P, &n_last, &p_any, &alpha_any);
        // image sample i is input n0 - T + i of the call: the oldest sample of the tile's first chain; the last output's second chain
        // reads input n_last at most.  (n_last - n0 <= 2 * 255 at step 2^33.)  Samples past the call's end are read by outputs past
        // n_out alone, which are not stored: zeros.
        const int need = min((int)(n_last - n0) + C::T + 1, C::IMG);
        for (int i = lane; i < need; i += 64) {
            const long long idx = n0 - C::T + i;
            img[i] = idx < ka.n_in ? sample_at<CF32>(a, in, hist, idx) : make_float2(0.0f, 0.0f);
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the image is this wave's own: its LDS operations complete in order)

        f32x4 y[2];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            long long n_rel;
            int p;
            float alpha;
            arb_locate(ka.rel, ka.step, m0 + 4 * lane + o, C::P, &n_rel, &p, &alpha);
            const float2 *win = img + (int)(n_rel - n0);      // window sample i meets tap j = T - 1 - i
            const int wrap = p + 1 == C::P ? 1 : 0;
            const f32x4 *ra = reinterpret_cast<const f32x4 *>(table + p * C::ROW), *rb = ra + C::ROW / 4;
            float2 x[C::T + 1];
#pragma unroll
            for (int i = 0; i <= C::T; ++i) x[i] = win[i];
            // half 1 (j 31 .. 16) is window samples 0 .. 15, half 0 (j 15 .. 0) samples 16 .. 31; each chain from +0
            float2 A[2], B[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float ai = 0.0f, aq = 0.0f, bi = 0.0f, bq = 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 ta = ra[4 * h + g], tb = rb[4 * h + g];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = 16 * h + 4 * g + e;
                        const float2 xa = x[i];
                        const float2 xb = wrap ? x[i + 1] : x[i];
                        ai = __builtin_fmaf(ta[e], xa.x, ai);
                        aq = __builtin_fmaf(ta[e], xa.y, aq);
                        bi = __builtin_fmaf(tb[e], xb.x, bi);
                        bq = __builtin_fmaf(tb[e], xb.y, bq);
                    }
                }
                A[h] = make_float2(ai, aq);
                B[h] = make_float2(bi, bq);
            }
            // P0 + P1, one rounding each, then the blend
            const float2 ua = make_float2(__fadd_rn(A[1].x, A[0].x), __fadd_rn(A[1].y, A[0].y));
            const float2 ub = make_float2(__fadd_rn(B[1].x, B[0].x), __fadd_rn(B[1].y, B[0].y));
            const float2 v = arb_blend(alpha, ua, ub);
            y[o >> 1][2 * (o & 1)] = v.x;
            y[o >> 1][2 * (o & 1) + 1] = v.y;
        }

        const long long m = (long long)m0 + 4 * lane;
        if ((long long)m0 + C::TILE <= ka.n_out) {
            f32x4 *dst = reinterpret_cast<f32x4 *>(out + 2 * m);
            dst[0] = y[0];
            dst[1] = y[1];
        } else {
            // the call's last tile: element by element, nothing past n_out
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (m + o < ka.n_out) reinterpret_cast<float2 *>(out)[m + o] = make_float2(y[o >> 1][2 * (o & 1)], y[o >> 1][2 * (o & 1) + 1]);
        }
        // the next tile's image is written only after these LDS reads have returned
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

}  // namespace sxfir
