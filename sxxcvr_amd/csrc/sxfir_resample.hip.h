// Rational (up / down) resampling (include/sxfir_rational.h), gfx950: the generic kernel of every coprime ratio and the one tiled
// shape, 4/5 x 128 taps on CF32 (2.4 MS/s -> 1.92 MS/s).
//
//   y[m] = sum_{j=0..T-1} h[j*up + (m*down mod up)] * x[floor(m*down / up) - j],   T = ntaps / up
//
// is sample m*down of the x up interpolator's output, and the contract is that interpolator's: per contiguous
// range of j one fmaf chain from +0.0f over j descending, the ranges joined by the adjacent-pair tree -- so both kernels below give
// the bits interp_generic_kernel gives for output m*down.
//
// resample45_kernel.  With m = 4q + p:  y[4q + p] = sum_{j=0..31} h[4j + p] * x[5q + p - j],  p = 0..3 -- four 32-tap filters over
// one window of 35 samples that advances five inputs per period q.
//   * a lane owns whole periods, so at any instant every lane of the wave is on the same (p, j): every v_pk_fma_f32 takes its tap as
//     the SCALAR operand.  128 taps are 64 register pairs, more than the scalar file holds beside the kernel's own scalars, so a tile
//     is walked in two passes by tap half, as decim4_cx_kernel walks its tile: pass 1 = the chains over j 31..16 (taps 64..127 in 32
//     SGPR pairs), pass 0 = the chains over j 15..0 (taps 0..63) -- the contract's two halves, which meet in one add;
//   * tile = 256 periods = 1280 inputs -> 1024 outputs, one wave (= one workgroup) per tile, no barrier: lane l takes periods
//     l, l + 64, l + 128, l + 192 of the tile (four rounds of one period per lane).  In a round the lanes' windows lie 5 samples =
//     10 dwords apart in a LINEAR image (no pad slots): a ds_read_b64's 32 lanes start at 32 different even banks of the 64
//     (tools/lds_bank_model.py rational: 0 extra cycles; two periods per lane, 20 dwords apart, would be two-way);
//   * a half chain of the four phases reads 19 samples: 38 ds_read_b64 per period and 128 packed FMAs;
//   * staging: the tile's 1280 inputs behind a 32-sample halo = 656 chunks of 16 bytes, 11 LDS-DMA instructions (the last for 16
//     lanes); instructions 1..9 -- rows no other tile reads -- non-temporal, 0 (the previous tile's tail) and 10 (the next tile's
//     halo) plain.  Edge tiles chunk by chunk, from the history below the call's first sample (sxfir_common.hip.h);
//   * the 1024 outputs leave as the wide kernel's whole-line stores, transposed through the dead image in two halves of 512
//     (wide_store_full); a call's last tile element by element from the registers, nothing past n_out;
//   * XCD-blocked tile dealing and the fused history carry-over are the /4 kernels' (DecimTileArgs, set_schedule).
// LDS 10 496 B per wave.  Registers of the shipped instance: DESIGN.md 5.11 (tools/shipped_isa.py resample).
//
// New code: the reference's rates are the SX1255's master clock over an integer (SoapySX.cpp:180-208); a rate between them has no
// counterpart there.
#pragma once

#include <utility>

#include "sxfir_decim_wide.hip.h"       // DecimTileArgs, the wide tile's store frame (and, through it, sxfir_common.hip.h)
#include "sxfir_kernels.hip.h"          // GenericArgs, interp_generic_output

namespace sxfir {

// One output per thread, any up / down / taps per phase / channel count / stride / start position: output m is phase m*down mod up
// of input index floor(m*down / up) of the interpolator -- interp_generic_output, the statement of the contract -- on the x up
// interpolator's GenericArgs (ratio = up) with a.down, a.m_first (the absolute index of the call's first output) and a.consumed
// (that of its first input).  The first output
// of a call has floor(m*down / up) >= consumed, so the chain reaches at most T - 1 samples into the history.
template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void resample_generic_kernel(const GenericArgs a)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_out) return;
    const int ch = blockIdx.y;
    const char *in = (const char *)a.in + sizeof(typename F::storage) * a.in_stride * ch;
    const char *hist = (const char *)a.hist + sizeof(typename F::storage) * a.hist_stride * ch;
    char *out = (char *)a.out + sizeof(typename FO::storage) * a.out_stride * ch;
    const long long n = (a.m_first + i) * a.down;           // index on the x up raster (64-bit: past 2^31 at 2^26 inputs and more)
    const long long q = n / a.ratio;
    const int r = (int)(n - q * a.ratio);
    FO::store(out, i, interp_generic_output<F>(a, a.taps, in, hist, q - a.consumed, r), a.thr2);
}

struct Resample45 {
    static constexpr int UP = 4, DOWN = 5, NT = 128;
    static constexpr int ROUNDS = 4;                      // periods per lane and tile
    static constexpr int TILE_Q = 64 * ROUNDS;            // 256 periods
    static constexpr int TILE_IN = TILE_Q * DOWN;         // 1280
    static constexpr int TILE_OUT = TILE_Q * UP;          // 1024
    static constexpr int HALO = 32, HIST = 32;            // (31 samples are read; 32 keeps the image on whole chunks)
    static constexpr int CHUNKS = (TILE_IN + HALO) / 2;   // 656 chunks of two samples, linear
    static constexpr int NI = (CHUNKS + 63) / 64;         // 11 DMA instructions, the last one for LASTL lanes
    static constexpr int LASTL = CHUNKS - 64 * (NI - 1);  // 16
    static constexpr int ROUND_STEP = 64 * DOWN;          // 320 samples between a lane's rounds
    static constexpr int WIN = 19;                        // samples a half chain of the four phases reads
};

// Window sample W (0..18) of a pass: it meets phase p at row jl = 15 + p - W of the pass's sixteen rows, i.e. at tap kl = 4 jl + p
// of the pass's 64 (hs[m] = {h[2m], h[2m + 1]} of that half, SGPR pairs).  Pass 1: x[5q - 31 + W], row j = 16 + jl; pass 0:
// x[5q - 15 + W], row j = jl.  W ascending is j descending for every chain; jl == 15 is a chain's first tap: from +0.
// A function template per sample: every tap index is a compile-time constant, so the taps stay in SGPRs.
template <int W>
__device__ __forceinline__ void rat45_step(const f32x2 &x, const f32x2 (&hs)[32], f32x2 (&acc)[4])
{
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int jl = 15 + p - W;
        if (jl >= 0 && jl <= 15) {
            const int kl = 4 * jl + p;
            if (jl == 15) {
                if (kl & 1) pk_fma_s_hi_first(acc[p], hs[kl >> 1], x);
                else pk_fma_s_lo_first(acc[p], hs[kl >> 1], x);
            } else if (kl & 1) {
                pk_fma_s_hi(acc[p], hs[kl >> 1], x);
            } else {
                pk_fma_s_lo(acc[p], hs[kl >> 1], x);
            }
        }
    }
}

// one period's half chains: `win` is the pass's first window sample of the lane's period
template <int... Ws>
__device__ __forceinline__ void rat45_half(std::integer_sequence<int, Ws...>, const f32x2 *win, const f32x2 (&hs)[32], f32x2 (&acc)[4])
{
    f32x2 x[sizeof...(Ws)];
#pragma unroll
    for (int w = 0; w < (int)sizeof...(Ws); ++w) x[w] = win[w];
    (rat45_step<Ws>(x[Ws], hs, acc), ...);
}

// HBM -> LDS for tile t: 11 LDS-DMA instructions into the linear image, 1..9 non-temporal
__device__ __forceinline__ void rat45_stage(f32x4 *img, const float *in, const float *hist, long long last_chunk, int n_odd, int lane, int t)
{
    using C = Resample45;
    const long long c0 = ((long long)t * C::TILE_IN - C::HALO) >> 1;
    const bool interior = (c0 >= 0) && (c0 + C::CHUNKS - 1 <= last_chunk - n_odd);
    if (interior) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(in) + c0 + lane;
#pragma unroll
        for (int j = 0; j < C::NI; ++j) {
            if (j < C::NI - 1 || lane < C::LASTL) {
                if (j >= 1 && j <= C::NI - 2) glds16<2>(src + 64 * j, img + 64 * j);
                else glds16(src + 64 * j, img + 64 * j);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < C::NI; ++j) {
            long long cc = c0 + 64 * j + lane;
            const f32x4 *src;
            if (cc < 0) {
                src = reinterpret_cast<const f32x4 *>(hist) + (cc + C::HIST / 2);
            } else {
                if (cc > last_chunk) cc = last_chunk;
                src = reinterpret_cast<const f32x4 *>(in) + cc;
            }
            if (j < C::NI - 1 || lane < C::LASTL) stage_edge_chunk(n_odd && cc == last_chunk, lane, src, img + 64 * j);
        }
    }
}

__global__ __launch_bounds__(64) void resample45_kernel(const DecimTileArgs a)
{
    using C = Resample45;
    static_assert(C::TILE_IN % 2 == 0 && C::HALO % 2 == 0, "tiles start on whole chunks");
    static_assert(C::ROUND_STEP * (C::ROUNDS - 1) + C::DOWN * 63 + 1 + 16 + C::WIN <= 2 * C::CHUNKS, "the last lane's last window lies inside the image");
    static_assert(C::CHUNKS >= 512, "the output transposition's two halves fit the dead image");
    __shared__ __attribute__((aligned(16))) f32x4 img[C::CHUNKS];

    const int lane = threadIdx.x;
    const int ch = blockIdx.y;
    const float *in = a.in + 2 * a.in_stride * ch;
    const float *hist = a.hist + 2 * a.hist_stride * ch;
    float *out = a.out + 2 * a.out_stride * ch;
    const long long last_chunk = (a.n_in - 1) >> 1;
    const int n_odd = (int)(a.n_in & 1);

    // the /4 kernels' tile schedule, always XCD-blocked
    const int G = a.n_waves;
    const int b = blockIdx.x;
    int tile = wide_first_tile(b, 0, a.w8);
    if (tile >= a.n_tiles) return;

    if (b == a.hist_wave) carry_history<8, C::HIST>(lane, in, hist, a.hist_out + 2 * a.hist_stride * ch, a.n_in);

    // lane l, round k: period 64k + l of the tile; its pass-1 window starts at image sample 5 (64k + l) + 1 (x[5q - 31] behind the
    // 32-sample halo), its pass-0 window 16 samples on
    const f32x2 *win = reinterpret_cast<const f32x2 *>(img) + C::DOWN * lane + 1;
    // the output transposition: the lane's chunks 2l, 2l + 1 of a round at the wide kernel's swizzled slots
    const int swz_w = ((lane >> 1) & 1) ^ ((lane >> 2) & 3), swz_r = ((lane >> 2) & 1) ^ ((lane >> 3) & 3);
    for (; tile < a.n_tiles; tile += G) {
        rat45_stage(img, in, hist, last_chunk, n_odd, lane, tile);
        SXFIR_WAIT_VMCNT(0);

        f32x2 a1[C::ROUNDS][4], a0[C::ROUNDS][4];
        {
            f32x2 hs[32];
            unsigned long long tp = (unsigned long long)a.taps;
            asm volatile("" : "+s"(tp));
            load_tap_half(tp, 1, hs);
#pragma unroll
            for (int k = 0; k < C::ROUNDS; ++k) rat45_half(std::make_integer_sequence<int, C::WIN>{}, win + C::ROUND_STEP * k, hs, a1[k]);
        }
        {
            f32x2 hs[32];
            unsigned long long tp = (unsigned long long)a.taps;
            // (after pass 1: the second tap set is loaded when the first is dead)
            asm volatile("" : "+s"(tp) : "v"(a1[0][0]), "v"(a1[C::ROUNDS - 1][3]));
            load_tap_half(tp, 0, hs);
#pragma unroll
            for (int k = 0; k < C::ROUNDS; ++k) rat45_half(std::make_integer_sequence<int, C::WIN>{}, win + C::ROUND_STEP * k + 16, hs, a0[k]);
        }
        // y = P0 + P1, one rounding each; chunk e of a round holds phases 2e, 2e + 1
        f32x4 y[C::ROUNDS][2];
#pragma unroll
        for (int k = 0; k < C::ROUNDS; ++k)
#pragma unroll
            for (int e = 0; e < 2; ++e)
                y[k][e] = (f32x4){__fadd_rn(a0[k][2 * e].x, a1[k][2 * e].x), __fadd_rn(a0[k][2 * e].y, a1[k][2 * e].y),
                                  __fadd_rn(a0[k][2 * e + 1].x, a1[k][2 * e + 1].x), __fadd_rn(a0[k][2 * e + 1].y, a1[k][2 * e + 1].y)};

        const long long m0 = (long long)tile * C::TILE_OUT;
        if (m0 + C::TILE_OUT <= a.n_out) {
            // two halves of 512 outputs = 256 chunks: rounds 2h, 2h + 1 through slots [256 h, 256 h + 256) of the dead image
            // (written and read by this wave only: LDS operations of one wave complete in order), then whole-line non-temporal stores
#pragma unroll
            for (int k = 0; k < C::ROUNDS; ++k)
#pragma unroll
                for (int e = 0; e < 2; ++e) img[256 * (k >> 1) + 128 * (k & 1) + ((2 * lane + e) ^ swz_w)] = y[k][e];
            auto store_half = [&](int h) __attribute__((always_inline)) { wide_store_full<0>(img + 256 * h, out, m0 + 512 * h, lane, swz_r); };
            store_half(0);
            store_half(1);
        } else {
            // the call's last tile: element by element, straight from the registers, nothing past n_out
#pragma unroll
            for (int k = 0; k < C::ROUNDS; ++k) store_ragged_from(out, m0 + C::UP * (64 * k + lane), a.n_out, y[k]);
        }
        // the next tile's DMA overwrites the image only after these LDS reads have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

}  // namespace sxfir
