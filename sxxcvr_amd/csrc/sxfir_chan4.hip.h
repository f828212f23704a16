// The 4-band channelizer (include/sxfir_channelizer.h): all four sub-bands of the /4 raster in one pass (gfx950).
//
// With the tap index written n = 4j + r, band k is y_k[m] = sum_r (j)^(k r) u_r[m], u_r[m] = sum_j h[4j + r] x[4m - 4j - r]: the
// four polyphase branch sums are together the 128 real-tap FMAs per output of decim4_wide_kernel, and the 4-point DFT on top has
// only +-1 and +-j for twiddles.  Four bands for one real-tap pass of arithmetic and one read of the input.
//
// Contract: u_r is ONE fmaf chain from +0 over j descending, I and Q each ((jsplit, cw) = (1, 1), rotation 0, on the
// taps of phase r alone); then the radix-2 butterflies, one rounding per real operation:
//   s0 = u0 + u2, s1 = u0 - u2, t0 = u1 + u3, t1 = u1 - u3;  y0 = s0 + t0, y2 = s0 - t0,
//   y1 = (s1.re - t1.im, s1.im + t1.re), y3 = (s1.re + t1.im, s1.im - t1.re).
//
// chan4_kernel -- CF32, 4 bands x 128 taps -- stands on the wide tile as it is (sxfir_decim_wide.hip.h: 2048 inputs + 128-sample
// halo, lane l owns outputs 8l..8l+7, window base chunk 16l), that kernel's frame functions called from here:
//   * window sample w of a lane meets its output i at tap 4i + 128 - w: one phase r = (-w) mod 4 for all eight outputs.  The 1024
//     packed FMAs of a real-tap tile keep their operands, only the accumulator changes: 32 accumulator pairs per lane (4 phases
//     x 8 outputs) instead of 16;
//   * 128 tap floats do not fit the scalar file, so a tile is walked in TWO PASSES by tap half as in decim4_cx_kernel: pass 1 =
//     taps 127..64 (window chunks [0, 47)), pass 0 = taps 63..0 (chunks [32, 79)), the 64 taps of a pass in 32 SGPR pairs,
//     re-loaded per pass behind a laundered pointer.  A chain walks its taps in descending order, i.e. the window in ascending
//     order: pass 0 simply continues in pass 1's accumulator.  Every FMA has a scalar tap operand;
//   * the butterflies (16 real additions per output, 128 per lane and tile) are in registers;
//   * the four bands leave through the dead image, 4 x 256 slots of the 1156, with the wide kernel's swizzles per band, each
//     stored by wide_store_full<0>: every store instruction writes 1 KiB of consecutive addresses, non-temporal.  The ragged last
//     tile goes straight from the registers, band by band (wide_store_ragged).
//
// Per tile of 512 outputs per band: 1024 v_pk_fma_f32, 94 window ds_read_b128 (47 per pass) + 16 of the output transposition, 19
// LDS-DMA instructions, 16 global_store_dwordx4.  LDS 18 496 B per wave -> 8 waves per CU.  Registers of the shipped instance:
// DESIGN.md 5.6 (tools/shipped_isa.py chan4).
//
// chan_generic_kernel -- every other tap count, CF16 storage, S32 wire words, off-boundary or misaligned calls -- is one thread
// per output index: four chains in named registers, the butterflies, four stores (chan_generic_output, which the oversampled
// plan's generic kernel shares).
//
// New code: the reference decimates inside the SX1255, whose base-band decimator takes the one band around 0 Hz
// (SoapySX.cpp:180-208 only programs the divider); the other three bands of the raster have no counterpart there.
#pragma once

#include <utility>

#include "sxfir_decim_wide.hip.h"       // DecimWide and the wide tile's frame: schedule, staging, carry-over, stores
#include "sxfir_kernels.hip.h"          // GenericArgs, sample_at, the storage formats

namespace sxfir {

// The tiled kernel's arguments: DecimTileArgs' stream fields, the XCD-blocked schedule's constants, and the band stride.
struct ChanTileArgs {
    const float *in;        // channel 0, sample 0 of this call
    const float *hist;      // channel 0 history: 128 samples preceding `in`
    float *hist_out;        // where the wave of the last tile leaves the history for the next call
    float *out;             // channel 0, band 0, first output of this call (16-byte aligned)
    const float *taps;      // 128 floats (device)
    long long n_in;         // new input samples per channel
    long long n_out;        // outputs per channel AND BAND
    long long in_stride;    // samples between channels
    long long out_stride;   // outputs between channels (even)
    long long band_stride;  // outputs between the bands of a channel (even)
    long long hist_stride;
    int n_tiles;            // tiles per channel
    int n_waves;            // waves (workgroups) per channel
    int w8;                 // n_waves / 8 when n_waves is a multiple of 8, else 0
    int hist_wave;          // the wave whose tiles include the last one: it carries the history over
};

struct Chan4 {
    static constexpr int NBANDS = 4;
    static constexpr int PCH = 47;                        // window chunks per pass
    static constexpr int P0FROM = 32;                     // pass 0 starts at window chunk 32 (slot 34)
    static constexpr int NB = 16;                         // LDS read-ahead in chunks (the oversampled channelizer's too)
    static constexpr int BAND_SLOTS = 256;                // a band's 512 outputs in the dead image
};

// One window chunk of a pass: chunk CL of the pass is window chunk BASE + CL (BASE: 0 for pass 1 = HALF 1, P0FROM for pass 0; the
// oversampled channelizer's odd times: one more).  Sample w = 2 CL + s of the pass meets output i at tap 64 HALF + kl,
// kl = 4i + 64 - w; hs[m] = {h[64 HALF + 2m], h[64 HALF + 2m + 1]} (SGPR pairs); the tap's phase is kl & 3 and its accumulator
// u[kl & 3][i].  A function template per chunk: every tap index and accumulator index is a compile-time constant.  Taps 127..124
// (HALF = 1, kl >= 60) are the four chains' first: from +0.
template <int CL, int HALF, int BASE, int NB>
__device__ __forceinline__ void chan4_step(const f32x4 *win, f32x4 (&buf)[NB], const f32x2 (&hs)[32], f32x2 (&u)[4][8])
{
    const f32x4 v = buf[CL % NB];
    if constexpr (CL + NB < Chan4::PCH) {
        constexpr int c = BASE + CL + NB;                  // (the image's pad slot after every 16 chunks)
        buf[CL % NB] = win[c + (c >> 4)];
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const f32x2 x = s ? __builtin_shufflevector(v, v, 2, 3) : __builtin_shufflevector(v, v, 0, 1);
        const int w = 2 * CL + s;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kl = 4 * i + 64 - w;
            if (kl >= 0 && kl < 64) {
                if (HALF == 1 && kl >= 60) {
                    if (kl & 1) pk_fma_s_hi_first(u[kl & 3][i], hs[kl >> 1], x);
                    else pk_fma_s_lo_first(u[kl & 3][i], hs[kl >> 1], x);
                } else if (kl & 1) {
                    pk_fma_s_hi(u[kl & 3][i], hs[kl >> 1], x);
                } else {
                    pk_fma_s_lo(u[kl & 3][i], hs[kl >> 1], x);
                }
            }
        }
    }
}

template <int HALF, int BASE, int NB, int... Cs>
__device__ __forceinline__ void chan4_pass(std::integer_sequence<int, Cs...>, const f32x4 *win, const f32x2 (&hs)[32], f32x2 (&u)[4][8])
{
    f32x4 buf[NB];
    fill_read_ahead<BASE>(win, buf);
    (chan4_step<Cs, HALF, BASE, NB>(win, buf, hs, u), ...);
}

// The branch sums of a lane's eight outputs: the two passes by tap half, the window ODD chunks further on (chan4_kernel: 0; the
// oversampled channelizer's odd times: 1).  `taps` (128 floats) is laundered per pass so that the tap loads stay inside the tile
// loop (load_tap_half, sxfir_common.hip.h).
template <int ODD>
__device__ __forceinline__ void chan4_sweep(const f32x4 *win, const float *taps, f32x2 (&u)[4][8])
{
    static_assert(ODD + Chan4::P0FROM + Chan4::PCH == DecimWide::WCH + ODD, "the two passes cover the window");
    {
        f32x2 hs[32];
        unsigned long long tp = (unsigned long long)taps;
        asm volatile("" : "+s"(tp));
        load_tap_half(tp, 1, hs);
        chan4_pass<1, ODD, Chan4::NB>(std::make_integer_sequence<int, Chan4::PCH>{}, win, hs, u);
    }
    {
        f32x2 hs[32];
        unsigned long long tp = (unsigned long long)taps;
        // (after pass 1: the second tap set is loaded when the first is dead)
        asm volatile("" : "+s"(tp) : "v"(u[0][0]), "v"(u[3][7]));
        load_tap_half(tp, 0, hs);
        chan4_pass<0, ODD + Chan4::P0FROM, Chan4::NB>(std::make_integer_sequence<int, Chan4::PCH>{}, win, hs, u);
    }
}

// The radix-2 4-point DFT of one output's branch sums (I, Q pairs), one rounding per real operation.
__device__ __forceinline__ void chan4_butterfly(const f32x2 u0, const f32x2 u1, const f32x2 u2, const f32x2 u3, f32x2 (&y)[4])
{
    const f32x2 s0 = {__fadd_rn(u0.x, u2.x), __fadd_rn(u0.y, u2.y)}, s1 = {__fsub_rn(u0.x, u2.x), __fsub_rn(u0.y, u2.y)};
    const f32x2 t0 = {__fadd_rn(u1.x, u3.x), __fadd_rn(u1.y, u3.y)}, t1 = {__fsub_rn(u1.x, u3.x), __fsub_rn(u1.y, u3.y)};
    y[0] = (f32x2){__fadd_rn(s0.x, t0.x), __fadd_rn(s0.y, t0.y)};
    y[1] = (f32x2){__fsub_rn(s1.x, t1.y), __fadd_rn(s1.y, t1.x)};
    y[2] = (f32x2){__fsub_rn(s0.x, t0.x), __fsub_rn(s0.y, t0.y)};
    y[3] = (f32x2){__fadd_rn(s1.x, t1.y), __fsub_rn(s1.y, t1.x)};
}

__global__ __launch_bounds__(64) void chan4_kernel(const ChanTileArgs a)
{
    using C = DecimWide;
    static_assert(C::CHUNKS % 16 == 0, "whole 16-chunk rows");
    static_assert(Chan4::NBANDS * Chan4::BAND_SLOTS <= C::SLOTS, "the four bands fit the dead image");
    static_assert(2 * Chan4::BAND_SLOTS == C::TILE_OUT, "a band's tile is the wide kernel's");
    __shared__ __attribute__((aligned(16))) f32x4 img[C::SLOTS];

    const int lane = threadIdx.x;
    const int ch = blockIdx.y;
    const float *in = a.in + 2 * a.in_stride * ch;
    const float *hist = a.hist + 2 * a.hist_stride * ch;
    float *out = a.out + 2 * a.out_stride * ch;
    const long long last_chunk = (a.n_in - 1) >> 1;
    const int n_odd = (int)(a.n_in & 1);

    // the wide kernel's tile schedule, always XCD-blocked
    const int G = a.n_waves;
    const int b = blockIdx.x;
    int tile = wide_first_tile(b, 0, a.w8);
    if (tile >= a.n_tiles) return;

    unsigned boff[C::NI];
#pragma unroll
    for (int j = 0; j < C::NI; ++j) boff[j] = slot_source_offset(64u * j + lane, C::CHUNKS);

    // the wide kernel's staging with the shipped policy: instructions 1..16 non-temporal
    auto stage = [&](int t) __attribute__((always_inline)) { wide_stage_cf32<true, 0>(img, in, hist, last_chunk, n_odd, lane, boff, t); };

    if (b == a.hist_wave) carry_history<8, C::HIST>(lane, in, hist, a.hist_out + 2 * a.hist_stride * ch, a.n_in);

    // lane l: outputs 8l..8l+7 of the tile; window from chunk 16l (lane stride 17 slots: conflict free)
    const f32x4 *win = img + 17 * lane;
    const int swz_w = (lane & 1) ^ ((lane >> 1) & 3), swz_r = ((lane >> 2) & 1) ^ ((lane >> 3) & 3);   // the output transposition's swizzles
    for (; tile < a.n_tiles; tile += G) {
        stage(tile);
        SXFIR_WAIT_VMCNT(0);

        f32x2 u[4][8];                                     // u[r][i]: branch sum r of output i
        chan4_sweep<0>(win, a.taps, u);
        f32x4 y[Chan4::NBANDS][4];                         // y[k][q]: outputs 2q, 2q + 1 of band k
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x2 e[4], o[4];
            chan4_butterfly(u[0][2 * q], u[1][2 * q], u[2][2 * q], u[3][2 * q], e);
            chan4_butterfly(u[0][2 * q + 1], u[1][2 * q + 1], u[2][2 * q + 1], u[3][2 * q + 1], o);
#pragma unroll
            for (int k = 0; k < Chan4::NBANDS; ++k) y[k][q] = (f32x4){e[k].x, e[k].y, o[k].x, o[k].y};
        }

        const long long m0 = (long long)tile * C::TILE_OUT;
        if (m0 + C::TILE_OUT <= a.n_out) {
            // band by band through the dead image (the wide kernel's swizzled layout, 256 slots each), then whole-line non-temporal stores
#pragma unroll
            for (int k = 0; k < Chan4::NBANDS; ++k)
#pragma unroll
                for (int q = 0; q < 4; ++q) img[Chan4::BAND_SLOTS * k + 4 * lane + (q ^ swz_w)] = y[k][q];
            auto store_full = [&](int k) __attribute__((always_inline)) {
                wide_store_full<0>(img + Chan4::BAND_SLOTS * k, out + 2 * a.band_stride * k, m0, lane, swz_r);
            };
#pragma unroll
            for (int k = 0; k < Chan4::NBANDS; ++k) store_full(k);
        } else {
#pragma unroll
            for (int k = 0; k < Chan4::NBANDS; ++k) wide_store_ragged(out + 2 * a.band_stride * k, m0, lane, a.n_out, y[k]);
        }
        // the next tile's DMA overwrites the image only after these LDS reads have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// ---- every other shape: one thread per output index, four chains in registers

// Output m of every band of a channelizer plan, critically sampled (OS false: the stream's ratio 4) or 2x oversampled (OS true:
// ratio 2): per tap row j (descending) one FMA of each chain, phases 0..3 by name -- no per-thread array that an index could send
// to scratch -- then the butterflies.  The oversampled plan ALONE shifts their operands by two where the absolute output index
// a.m_first + m is odd (the branch sums shifted in front of the same butterflies); a critically sampled plan never does,
// wherever its call starts.  a.n_out: outputs per band.
template <typename F, typename FO, bool OS>
__device__ __forceinline__ void chan_generic_output(const GenericArgs &a)
{
    constexpr int RATIO = OS ? 2 : 4;
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_out) return;
    const int ch = blockIdx.y;
    const char *in = (const char *)a.in + sizeof(typename F::storage) * a.in_stride * ch;
    const char *hist = (const char *)a.hist + sizeof(typename F::storage) * a.hist_stride * ch;
    const long long newest = a.first + m * RATIO;
    float2 u0 = make_float2(0.0f, 0.0f), u1 = u0, u2 = u0, u3 = u0;
    for (int j = a.ntaps / 4 - 1; j >= 0; --j) {
        const float *t = a.taps + 4 * j;
        const long long at = newest - 4 * j;
        const float2 x0 = sample_at<F>(a, in, hist, at), x1 = sample_at<F>(a, in, hist, at - 1);
        const float2 x2 = sample_at<F>(a, in, hist, at - 2), x3 = sample_at<F>(a, in, hist, at - 3);
        u0 = make_float2(__builtin_fmaf(t[0], x0.x, u0.x), __builtin_fmaf(t[0], x0.y, u0.y));
        u1 = make_float2(__builtin_fmaf(t[1], x1.x, u1.x), __builtin_fmaf(t[1], x1.y, u1.y));
        u2 = make_float2(__builtin_fmaf(t[2], x2.x, u2.x), __builtin_fmaf(t[2], x2.y, u2.y));
        u3 = make_float2(__builtin_fmaf(t[3], x3.x, u3.x), __builtin_fmaf(t[3], x3.y, u3.y));
    }
    const bool odd = OS && ((a.m_first + m) & 1) != 0;
    const float2 a0 = odd ? u2 : u0, a1 = odd ? u3 : u1, a2 = odd ? u0 : u2, a3 = odd ? u1 : u3;
    f32x2 y[4];
    chan4_butterfly((f32x2){a0.x, a0.y}, (f32x2){a1.x, a1.y}, (f32x2){a2.x, a2.y}, (f32x2){a3.x, a3.y}, y);
    // FO::store rounds to half once for CF16
    char *out = (char *)a.out + sizeof(typename FO::storage) * a.out_stride * ch;
    const long long bs = (long long)sizeof(typename FO::storage) * a.band_stride;
    FO::store(out, m, make_float2(y[0].x, y[0].y), a.thr2);
    FO::store(out + bs, m, make_float2(y[1].x, y[1].y), a.thr2);
    FO::store(out + 2 * bs, m, make_float2(y[2].x, y[2].y), a.thr2);
    FO::store(out + 3 * bs, m, make_float2(y[3].x, y[3].y), a.thr2);
}

template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void chan_generic_kernel(const GenericArgs a) { chan_generic_output<F, FO, false>(a); }

}  // namespace sxfir
