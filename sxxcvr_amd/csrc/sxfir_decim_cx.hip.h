// Decimate-by-4, 128 COMPLEX taps (h = a + j b), CF32: 8 outputs per lane, one wave per tile of 512 outputs (gfx950).
// The band-pass partner of decim4_wide_kernel (sxfir_decim_wide.hip.h): the same tile, the same staged image, the same
// stores -- that kernel's frame functions, called from here -- and two FMA chains per window read instead of one.
//
// Contract: A = a (*) x and B = b (*) x are the two REAL-tap results under the plan's real-tap contract
// ((jsplit, cw) = (2, 4), rotation 0: P1 = taps 127..64 and P0 = taps 63..0 of each output, both chains from +0, A = P0 + P1);
// then y.re = A.re - B.im and y.im = A.im + B.re, one rounding each.
//
//   * lane l -> outputs 8l..8l+7 of the tile, as in the wide kernel; window base chunk 16l (slot 17l: conflict free);
//   * 256 tap floats do not fit the scalar file, so a tile is walked in TWO PASSES by tap half, a split like the wide
//     kernel's ASYM form in each: pass 1 = the P1 chains (taps 127..64, window chunks [0, 47)), pass 0 = the P0 chains (taps
//     63..0, chunks [32, 79)).  In a pass the 64 taps of `a` sit in 32 SGPR pairs (the A chain: packed FMAs with a scalar tap
//     operand) and the 64 taps of `b` in 32 VGPR pairs (the B chain); both sets are re-loaded per pass with scalar loads (the b
//     set copied to vector registers: 64 v_mov per pass, 3 % of the pass's issue slots);
//   * every ds_read_b128 of the window feeds BOTH chains: chunk c of a pass yields up to 16 FMAs per sample and chain, A and
//     B back to back on the same sample pair;
//   * the combine (A = P0 + P1, B = P0 + P1, re = A.re - B.im, im = A.im + B.re) is in registers, in front of the output
//     transposition through the dead image;
//   * staging (19 LDS-DMA instructions, 16 of them non-temporal), XCD-blocked tile dealing, fused history carry-over and whole-line
//     non-temporal stores are the wide kernel's: the wide_* functions of sxfir_decim_wide.hip.h with the shipped parameters.
//
// Per tile of 512 outputs: 2048 v_pk_fma_f32 (2 chains x 8 outputs x 128 taps per lane; half of them with a scalar tap
// operand) = twice a real-tap tile's 1024; 94 window ds_read_b128 (47 per pass) + 4 of the output transposition: 23.5 window
// reads per 512 FMAs (the wide kernel: 39.5).  LDS 18 496 B per wave -> 8 waves per CU (2 per SIMD, 256 VGPRs each).
// Registers and spills of the shipped instances: DESIGN.md 5.5, 5.12 (tools/shipped_isa.py decim4_cx).
//
// One kernel, two instances by argument struct: the complex-tap decimators' (DecimTileArgs) and the translating decimators'
// (MixTileArgs: the same tile with every output turned by a table entry, sxfir_mixer.hip.h); what the mixer adds sits under
// `if constexpr (MIX)`, and the plain instance's text is what it was before the mixer came.
//
// New code: the reference decimates inside the SX1255, whose base-band decimator is fixed and low-pass (SoapySX.cpp:180-208
// only programs the divider); a band other than the one around 0 Hz has no counterpart there.
#pragma once

#include <type_traits>
#include <utility>

#include "sxfir_decim_wide.hip.h"       // DecimWide and the wide tile's frame: schedule, staging, carry-over, stores
#include "sxfir_mixer.hip.h"            // Mixer, mix_rotate: the translating decimators' instance

namespace sxfir {

struct DecimCx {
    static constexpr int PCH = 47;                        // window chunks per pass
    static constexpr int P0FROM = 32;                     // pass 0 starts at window chunk 32 (slot 34)
    static constexpr int NB = 16;                         // LDS read-ahead in chunks
};

// One window chunk CL of a pass (pass base: window chunk 0 for P1, 32 for P0).  Sample w = 2 CL + s meets output i at tap
// kl = 4i + 64 - w of the pass's tap half; hs[m] = {a[2m], a[2m+1]} (SGPR pairs), hv[m] = {b[2m], b[2m+1]} (VGPR pairs) of that
// half.  A function template per chunk: every tap index is a compile-time constant.  kl == 63 is a chain's first tap: from +0.
template <int CL, int NB>
__device__ __forceinline__ void fir_cx_step(const f32x4 *win, f32x4 (&buf)[NB], const f32x2 (&hs)[32], const f32x2 (&hv)[32],
                                            f32x2 (&aa)[8], f32x2 (&ab)[8])
{
    const f32x4 v = buf[CL % NB];
    if constexpr (CL + NB < DecimCx::PCH) buf[CL % NB] = win[(CL + NB) + ((CL + NB) >> 4)];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const f32x2 x = s ? __builtin_shufflevector(v, v, 2, 3) : __builtin_shufflevector(v, v, 0, 1);
        const int w = 2 * CL + s;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kl = 4 * i + 64 - w;
            if (kl >= 0 && kl < 64) {
                if (kl == 63) {
                    pk_fma_s_hi_first(aa[i], hs[kl >> 1], x);
                    pk_fma_hi_first(ab[i], hv[kl >> 1], x);
                } else if (kl & 1) {
                    pk_fma_s_hi(aa[i], hs[kl >> 1], x);
                    pk_fma_hi(ab[i], hv[kl >> 1], x);
                } else {
                    pk_fma_s_lo(aa[i], hs[kl >> 1], x);
                    pk_fma_lo(ab[i], hv[kl >> 1], x);
                }
            }
        }
    }
}

template <int NB, int... Cs>
__device__ __forceinline__ void fir_cx_pass(std::integer_sequence<int, Cs...>, const f32x4 *win, const f32x2 (&hs)[32],
                                            const f32x2 (&hv)[32], f32x2 (&aa)[8], f32x2 (&ab)[8])
{
    f32x4 buf[NB];
    fill_read_ahead<0>(win, buf);
    (fir_cx_step<Cs, NB>(win, buf, hs, hv, aa, ab), ...);
}

// taps: 256 floats, planar -- a[0..127] then b[0..127].  `half` = 1: taps 64..127 of both, 0: taps 0..63.  tp is an opaque
// scalar (the caller launders it per pass) so that the loads stay inside the tile loop: hoisted, the four sets would need 128
// SGPRs at once.
__device__ __forceinline__ void load_cx_taps(unsigned long long tp, int half, f32x2 (&hs)[32], f32x2 (&hv)[32])
{
    const __attribute__((address_space(4))) f32x2 *tq = (const __attribute__((address_space(4))) f32x2 *)tp;
#pragma unroll
    for (int m = 0; m < 32; ++m) {
        f32x2 t = tq[64 + 32 * half + m];                 // b: the same value in every lane ...
        asm volatile("" : "+v"(t));                        // ... kept as a vector register pair
        hv[m] = t;
    }
#pragma unroll
    for (int m = 0; m < 32; ++m) hs[m] = tq[32 * half + m];
}

// The argument struct of the translating decimators' instance (include/sxfir_translate.h): the plain struct plus the mixer and
// the three steps of the tile walk, worked out by the host (mix_tile_args, sxfir_launch.hip.h) so that the tile loop holds no division
struct MixTileArgs : DecimTileArgs {
    Mixer mix;
    unsigned lane_step;     // (8 s) mod den: between the first outputs of two lanes
    unsigned tile_step;     // (512 s) mod den: between two tiles
    unsigned stride_step;   // (n_waves * 512 s) mod den: between two tiles of one wave
};

// Args = DecimTileArgs: the complex-tap decimators' kernel.  Args = MixTileArgs: the translating decimators' (the launch geometry
// calls that instance decim4_mix_kernel) -- the same tile with output m turned by w[(m s) mod den], m the ABSOLUTE output index.
// Lane l owns outputs 8l..8l+7 of the tile: its first table index is (tile's phase + l (8 s mod den)) mod den, the next seven follow
// by adding s and taking den off on overflow, all in 32 bits.  The tile's phase starts at (call's phase + (tile mod den)(512 s mod
// den)) mod den and moves by (n_waves 512 s) mod den per stride of the tile loop.  The eight table reads (8 bytes each, a table of
// at most 512 KiB that lives in L2) are issued between the two passes, behind the 1024 packed FMAs of pass 0; the rotation sits
// between the combine and the transposition writes, so the full and the ragged store path both see rotated values.
template <typename Args>
__global__ __launch_bounds__(64) void decim4_cx_kernel(const Args ka)
{
    using C = DecimWide;
    constexpr bool MIX = std::is_same_v<Args, MixTileArgs>;
    static_assert(C::CHUNKS % 16 == 0, "whole 16-chunk rows");
    static_assert(DecimCx::P0FROM + DecimCx::PCH == C::WCH, "the two passes cover the window");
    __shared__ __attribute__((aligned(16))) f32x4 img[C::SLOTS];

    const DecimTileArgs &a = ka;
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
    // (through a lambda: called straight from the tile loop the function leaves the kernel's text another)
    auto stage = [&](int t) __attribute__((always_inline)) { wide_stage_cf32<true, 0>(img, in, hist, last_chunk, n_odd, lane, boff, t); };

    if (b == a.hist_wave) carry_history<8, C::HIST>(lane, in, hist, a.hist_out + 2 * a.hist_stride * ch, a.n_in);

    // the mixer's phases, 32 bits: the lane's offset into a tile and the first tile's phase (the only divisions of the kernel)
    unsigned den = 0, s = 0, lane_ph = 0, tile_ph = 0;
    if constexpr (MIX) {
        den = ka.mix.den, s = ka.mix.step;
        lane_ph = (unsigned)lane * ka.lane_step % den;                                          // (63 * 65535 < 2^32)
        tile_ph = ka.mix.phase + ((unsigned)tile % den) * ka.tile_step % den;                  // (65535^2 < 2^32)
        if (tile_ph >= den) tile_ph -= den;
    }

    // lane l: outputs 8l..8l+7 of the tile; window from chunk 16l (lane stride 17 slots: conflict free)
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
        f32x2 wv[MIX ? 8 : 1];
        if constexpr (MIX) {
            unsigned long long wp = (unsigned long long)ka.mix.w;
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
            // A = P0 + P1 and B = P0 + P1 (the real-tap contract's last addition), then y = A + j B: one rounding each; then the
            // mixer's rotation
            f32x2 yy[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i = 2 * k + e;
                const float are = __fadd_rn(a0a[i].x, a1a[i].x), aim = __fadd_rn(a0a[i].y, a1a[i].y);
                const float bre = __fadd_rn(a0b[i].x, a1b[i].x), bim = __fadd_rn(a0b[i].y, a1b[i].y);
                if constexpr (MIX) {
                    const float2 r = mix_rotate(make_float2(__fsub_rn(are, bim), __fadd_rn(aim, bre)), make_float2(wv[i].x, wv[i].y));
                    yy[e] = (f32x2){r.x, r.y};
                } else {
                    yy[e] = (f32x2){__fsub_rn(are, bim), __fadd_rn(aim, bre)};
                }
            }
            y[k] = (f32x4){yy[0].x, yy[0].y, yy[1].x, yy[1].y};
        }

        const long long m0 = (long long)tile * C::TILE_OUT;
        if (m0 + C::TILE_OUT <= a.n_out) {
            // transposed through the dead image (the wide kernel's swizzled layout), then whole-line non-temporal stores
#pragma unroll
            for (int k = 0; k < 4; ++k) img[4 * lane + (k ^ swz_w)] = y[k];
            auto store_full = [&]() __attribute__((always_inline)) { wide_store_full<0>(img, out, m0, lane, swz_r); };
            store_full();
        } else {
            wide_store_ragged(out, m0, lane, a.n_out, y);
        }
        // the next tile's DMA overwrites the image only after these LDS reads have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (MIX) {
            tile_ph += ka.stride_step;
            if (tile_ph >= den) tile_ph -= den;
        }
    }
}

}  // namespace sxfir
