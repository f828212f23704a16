// Frequency-translating decimators (include/sxfir_translate.h), gfx950: a complex-tap decimator whose output m is turned by
// w[(m s) mod den], w[i] = exp(-j 2 pi i / den) from a table in device memory, m the ABSOLUTE output index.  Two kernels:
//
//   * decim_mix_generic_kernel<F, FO>: one output per thread, any shape, format, stride and start position -- the work of
//     decim_cx_generic_kernel (sxfir_kernels.hip.h), then the table entry of ((m_first + i) mod den) s mod den and the rotation;
//   * decim4_mix_kernel: /4 x 128 complex taps on CF32, on decim4_cx_kernel's tile (sxfir_decim_cx.hip.h) -- its staging, its two
//     passes, its combine and its stores, called from here unchanged.  Lane l owns outputs 8l..8l+7 of the tile: its first table
//     index is (tile's phase + l (8 s mod den)) mod den, the next seven follow by adding s and taking den off on overflow, all in
//     32 bits (den <= 65536: no sum reaches 2^17).  The tile's phase starts at (call's phase + (tile mod den)(512 s mod den)) mod
//     den and moves by (n_waves 512 s) mod den per stride of the tile loop; the host works the three steps out (mix_tile_args), so
//     the tile loop holds no division.  The eight table reads (8 bytes each, a table of at most 512 KiB that lives in L2) are
//     issued between the two passes, behind the 1024 packed FMAs of pass 0; the rotation sits between the combine and the
//     transposition writes, so the full and the ragged store path both see rotated values.
//
// The rotation (mix_rotate): y.re = fsub_rn(fmul_rn(z.re, w.re), fmul_rn(z.im, w.im)), y.im = fadd_rn(fmul_rn(z.re, w.im),
// fmul_rn(z.im, w.re)): six roundings.  The four products pass through an empty asm statement each, so that no compiler setting
// can contract a product and the sum behind it into a fused multiply-add.
//
// Both kernels have argument structs of their own (the parent's struct plus the mixer): GenericArgs and DecimTileArgs keep their
// size, so every kernel that takes them keeps its text.
//
// New code: the reference has no mixer behind its decimator (the SX1255's is fixed and low-pass, SoapySX.cpp:180-208).
#pragma once

#include "sxfir_decim_cx.hip.h"         // decim4_cx_kernel's tile: DecimCx, fir_cx_pass, load_cx_taps and the wide kernel's frame
#include "sxfir_kernels.hip.h"          // GenericArgs, decim_generic_output, the storage formats

namespace sxfir {

struct Mixer {
    const float *w;         // den (re, im) pairs: w[i] = exp(-j 2 pi i / den) (sxfir_design_rotator)
    unsigned den;           // 1 .. 65536
    unsigned s;             // (num * ratio) mod den: table entries per output
    unsigned phase;         // table index of the call's first output: ((produced mod den) * s) mod den
};

struct MixGenericArgs {
    GenericArgs g;          // m_first: absolute index of the call's first output
    Mixer mix;
};

struct MixTileArgs {
    DecimTileArgs t;
    Mixer mix;
    unsigned lane_step;     // (8 s) mod den: between the first outputs of two lanes
    unsigned tile_step;     // (512 s) mod den: between two tiles
    unsigned stride_step;   // (n_waves * 512 s) mod den: between two tiles of one wave
};

// z * w in six roundings, no fused multiply-add
__device__ __forceinline__ float2 mix_rotate(float2 z, float2 w)
{
    float rr = __fmul_rn(z.x, w.x), ii = __fmul_rn(z.y, w.y);
    float ri = __fmul_rn(z.x, w.y), ir = __fmul_rn(z.y, w.x);
    asm("" : "+v"(rr), "+v"(ii), "+v"(ri), "+v"(ir));
    return make_float2(__fsub_rn(rr, ii), __fadd_rn(ri, ir));
}

// decim_cx_generic_kernel's output, turned: one output per thread.  The table index is reduced exactly, in integers.
template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void decim_mix_generic_kernel(const MixGenericArgs ma)
{
    const GenericArgs &a = ma.g;
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_out) return;
    const int ch = blockIdx.y;
    const char *in = (const char *)a.in + sizeof(typename F::storage) * a.in_stride * ch;
    const char *hist = (const char *)a.hist + sizeof(typename F::storage) * a.hist_stride * ch;
    char *out = (char *)a.out + sizeof(typename FO::storage) * a.out_stride * ch;
    float2 ab[2] = {make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)};
#pragma nounroll
    for (int part = 0; part < 2; ++part) {
        const float2 v = decim_generic_output<F>(a, a.taps + (size_t)part * a.ntaps, in, hist, a.first + m * a.ratio);
        if (part == 0) ab[0] = v;
        else ab[1] = v;
    }
    const float2 z = make_float2(__fsub_rn(ab[0].x, ab[1].y), __fadd_rn(ab[0].y, ab[1].x));
    const unsigned r = (unsigned)((unsigned long long)(a.m_first + m) % ma.mix.den);       // < 2^16
    const unsigned idx = r * ma.mix.s % ma.mix.den;                                        // (65535^2 < 2^32)
    const float2 w = reinterpret_cast<const float2 *>(ma.mix.w)[idx];
    FO::store(out, m, mix_rotate(z, w), a.thr2);
}

__global__ __launch_bounds__(64) void decim4_mix_kernel(const MixTileArgs ma)
{
    using C = DecimWide;
    static_assert(C::CHUNKS % 16 == 0, "whole 16-chunk rows");
    static_assert(DecimCx::P0FROM + DecimCx::PCH == C::WCH, "the two passes cover the window");
    __shared__ __attribute__((aligned(16))) f32x4 img[C::SLOTS];

    const DecimTileArgs &a = ma.t;
    const int lane = threadIdx.x;
    const int ch = blockIdx.y;
    const float *in = a.in + 2 * a.in_stride * ch;
    const float *hist = a.hist + 2 * a.hist_stride * ch;
    float *out = a.out + 2 * a.out_stride * ch;
    const long long last_chunk = (a.n_in - 1) >> 1;
    const int n_odd = (int)(a.n_in & 1);

    // decim4_cx_kernel's tile schedule, staging policy and history carry-over
    const int G = a.n_waves;
    const int b = blockIdx.x;
    int tile = wide_first_tile(b, 0, a.w8);
    if (tile >= a.n_tiles) return;

    unsigned boff[C::NI];
#pragma unroll
    for (int j = 0; j < C::NI; ++j) boff[j] = slot_source_offset(64u * j + lane, C::CHUNKS);

    auto stage = [&](int t) __attribute__((always_inline)) { wide_stage_cf32<true, 0>(img, in, hist, last_chunk, n_odd, lane, boff, t); };

    if (b == a.hist_wave) carry_history<8, C::HIST>(lane, in, hist, a.hist_out + 2 * a.hist_stride * ch, a.n_in);

    // the mixer's phases, 32 bits: the lane's offset into a tile and the first tile's phase (the only divisions of the kernel)
    const unsigned den = ma.mix.den, s = ma.mix.s;
    const unsigned lane_ph = (unsigned)lane * ma.lane_step % den;                              // (63 * 65535 < 2^32)
    unsigned tile_ph = ma.mix.phase + ((unsigned)tile % den) * ma.tile_step % den;            // (65535^2 < 2^32)
    if (tile_ph >= den) tile_ph -= den;

    const f32x4 *win = img + 17 * lane;
    const int swz_w = (lane & 1) ^ ((lane >> 1) & 3), swz_r = ((lane >> 2) & 1) ^ ((lane >> 3) & 3);   // the output transposition's swizzles
    for (; tile < a.n_tiles; tile += G) {
        stage(tile);
        SXFIR_WAIT_VMCNT(0);

        f32x2 a1a[8], a1b[8], a0a[8], a0b[8];
        {
            f32x2 hs[32], hv[32];
            unsigned long long tp = (unsigned long long)a.taps;
            asm volatile("" : "+s"(tp));
            load_cx_taps(tp, 1, hs, hv);
            fir_cx_pass<DecimCx::NB>(std::make_integer_sequence<int, DecimCx::PCH>{}, win, hs, hv, a1a, a1b);
        }
        // the lane's eight table entries, read behind pass 1 (its tap registers are dead) and in front of pass 0's FMAs
        f32x2 wv[8];
        {
            unsigned long long wp = (unsigned long long)ma.mix.w;
            asm volatile("" : "+s"(wp) : "v"(a1a[0]), "v"(a1a[7]), "v"(a1b[0]), "v"(a1b[7]));
            const __attribute__((address_space(1))) f32x2 *wt = (const __attribute__((address_space(1))) f32x2 *)wp;      // (global, not flat, loads)
            unsigned idx = tile_ph + lane_ph;
            if (idx >= den) idx -= den;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                wv[i] = wt[idx];
                idx += s;
                if (idx >= den) idx -= den;
            }
        }
        {
            f32x2 hs[32], hv[32];
            unsigned long long tp = (unsigned long long)a.taps;
            // (after pass 1: the second tap sets are loaded when the first are dead)
            asm volatile("" : "+s"(tp) : "v"(a1a[0]), "v"(a1a[7]), "v"(a1b[0]), "v"(a1b[7]));
            load_cx_taps(tp, 0, hs, hv);
            fir_cx_pass<DecimCx::NB>(std::make_integer_sequence<int, DecimCx::PCH>{}, win + (DecimCx::P0FROM + DecimCx::P0FROM / 16), hs, hv, a0a, a0b);
        }
        f32x4 y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // decim4_cx_kernel's combine (z = A + j B, one rounding each), then the rotation
            f32x2 yy[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i = 2 * k + e;
                const float are = __fadd_rn(a0a[i].x, a1a[i].x), aim = __fadd_rn(a0a[i].y, a1a[i].y);
                const float bre = __fadd_rn(a0b[i].x, a1b[i].x), bim = __fadd_rn(a0b[i].y, a1b[i].y);
                const float2 r = mix_rotate(make_float2(__fsub_rn(are, bim), __fadd_rn(aim, bre)), make_float2(wv[i].x, wv[i].y));
                yy[e] = (f32x2){r.x, r.y};
            }
            y[k] = (f32x4){yy[0].x, yy[0].y, yy[1].x, yy[1].y};
        }

        const long long m0 = (long long)tile * C::TILE_OUT;
        if (m0 + C::TILE_OUT <= a.n_out) {
#pragma unroll
            for (int k = 0; k < 4; ++k) img[4 * lane + (k ^ swz_w)] = y[k];
            auto store_full = [&]() __attribute__((always_inline)) { wide_store_full<0>(img, out, m0, lane, swz_r); };
            store_full();
        } else {
            wide_store_ragged(out, m0, lane, a.n_out, y);
        }
        // the next tile's DMA overwrites the image only after these LDS reads have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        tile_ph += ma.stride_step;
        if (tile_ph >= den) tile_ph -= den;
    }
}

}  // namespace sxfir
