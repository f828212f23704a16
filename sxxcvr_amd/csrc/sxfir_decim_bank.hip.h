// The kernels of the tuner bank (include/sxfir_bank.h), gfx950: K translating decimators over one stream in one pass.
//
// decim_bank_generic_kernel: every shape and format -- decim_cx_generic_kernel's mixer instance (sxfir_kernels.hip.h) with the
// band in the grid's third dimension; a thread's band selects its taps, table and step.
//
// decim4_bank_kernel: /4 x 128 complex taps on CF32, decim4_cx_kernel's frame (sxfir_decim_cx.hip.h) with a band loop INSIDE the tile
// loop.  A tile of 2048 inputs is staged once (wide_stage_cf32, the shipped policy) and the history carried over once; then, band
// after band, the two fir_cx_pass passes over the SAME image with the band's tap halves (planar a|b at taps + 256 k floats), eight
// table reads between the passes, the combine, mix_rotate, and the stores to the band's row.  Per band and tile the arithmetic is
// the single-band kernel's, chain for chain: 2048 v_pk_fma_f32, 94 window ds_read_b128.
//
//   * The output transposition.  decim4_cx_kernel transposes its 512 outputs through the dead image; here the image lives until the
//     last band.  The bank transposes through a scratch of ONE KILOBYTE behind the image, a quarter tile at a time: lanes 16 q ..
//     16 q + 15 hold outputs 128 q .. 128 q + 127 of the tile (64 chunks); they write their four chunks each in the wide kernel's
//     swizzled layout (restricted to 64 chunks it stays a permutation of 64 slots: the swizzle only touches a chunk's two low
//     bits), every lane reads chunk l back and the wave stores 1 KiB of consecutive addresses, as the single-band kernel does: the
//     same four reads and four stores per band and tile, sixteen quarter-masked ds_write_b128 in the place of four full ones.
//     LDS 18 496 + 1024 + 64 = 19 584 B per wave: 8 waves per CU, the single-band kernel's figure (a 4 KiB scratch: 22 592 B, 7 waves).
//     LDS operations of one wave complete in order, so a quarter's writes need no wait for the quarter before; every band ends in
//     s_waitcnt lgkmcnt(0) -- what the tile loop had against the next tile's DMA, which follows the last band.
//   * The per-band arguments: a fixed array of sixteen BankBand in the argument struct, read with scalar loads at the loop's (scalar)
//     band index.  The band's tile phase -- the one value a band carries from one of a wave's tiles to the next -- lives in sixteen
//     words of LDS behind the scratch: written in the prologue (the kernel's only integer divisions, uniform), read, advanced by
//     stride_step and written back once per band and tile.  The lane's offset into the tile, (l lane_step) mod den, would be a
//     register per band; it is recomputed per band and tile without a division (bank_reduce: the float quotient of a sum below
//     64 den, one off at most, then two unsigned minimums).  Sums stay below 2^22, products below 2^32.
//   * The band loop is a runtime loop (no unrolling into a register budget that spills); no scratch memory (tools/shipped_isa.py).
//
// New code: the reference has neither a mixer nor a second band behind its decimator (the SX1255's filters are fixed and low-pass,
// SoapySX.cpp:180-208).
#pragma once

#include "sxfir_decim_cx.hip.h"         // the complex-tap tile: fir_cx_pass, load_cx_taps, and the wide tile's frame
#include "sxfir_kernels.hip.h"          // GenericArgs, decim_generic_output

namespace sxfir {

static constexpr int BANK_MAX = 16;     // SXFIR_BANK_MAX_BANDS

// One band's mixer and its steps through the table (the host: bank_bands, sxfir_launch.hip.h).  The generic kernel reads w, den, step.
struct BankBand {
    const float *w;         // den (re, im) pairs: w[i] = exp(-j 2 pi i / den) (sxfir_design_rotator)
    unsigned den;           // 1 .. 65536
    unsigned step;          // s = (num ratio) mod den: table entries per output
    unsigned phase;         // table index of the call's first output
    unsigned lane_step;     // (8 s) mod den: between the first outputs of two lanes
    unsigned tile_step;     // (512 s) mod den: between two tiles
    unsigned stride_step;   // (n_waves * 512 s) mod den: between two tiles of one wave
    float rden;             // 1.0f / den, rounded once (bank_reduce)
    unsigned pad;
};

struct BankGenericArgs : GenericArgs {
    BankBand band[BANK_MAX];
};

struct BankTileArgs : DecimTileArgs {
    long long band_stride;  // outputs between the bands of a channel
    int nbands;
    BankBand band[BANK_MAX];
};

// x mod den for x < 64 den, den <= 2^16 (so x < 2^22: exact in float), without a division: rden = fl(1 / den) and the product carry
// a relative error below 2^-23 together and the quotient is below 64, so the truncated float quotient is the true one or one off
// either way; r = x - q den then lies in (-den, 2 den) as a wrapped unsigned, and one unsigned minimum each puts it right (a wrapped
// negative plus den is small; a value in [0, den) less den wraps to a large one).
__device__ __forceinline__ unsigned bank_reduce(unsigned x, unsigned den, float rden)
{
    const unsigned q = (unsigned)(__fmul_rn((float)x, rden));
    unsigned r = x - q * den;
    r = min(r, r + den);
    r = min(r, r - den);
    return r;
}

// One output per thread and band (blockIdx.z), any ntaps / ratio / alignment: decim_cx_generic_kernel's mixer instance, the band's
// taps at taps + 2 ntaps k (planar a | b), its table, its step.  Output m_first + m is turned by the table entry of
// ((m_first + m) mod den) s mod den, reduced exactly, in integers.
template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void decim_bank_generic_kernel(const BankGenericArgs ka)
{
    const GenericArgs &a = ka;
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_out) return;
    const int ch = blockIdx.y, k = blockIdx.z;
    const BankBand &bd = ka.band[k];
    const char *in = (const char *)a.in + sizeof(typename F::storage) * a.in_stride * ch;
    const char *hist = (const char *)a.hist + sizeof(typename F::storage) * a.hist_stride * ch;
    char *out = (char *)a.out + sizeof(typename FO::storage) * (a.out_stride * ch + a.band_stride * k);
    const float *taps = a.taps + (size_t)2 * a.ntaps * k;
    float2 ab[2] = {make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)};
#pragma nounroll
    for (int part = 0; part < 2; ++part) {
        const float2 v = decim_generic_output<F>(a, taps + (size_t)part * a.ntaps, in, hist, a.first + m * a.ratio);
        if (part == 0) ab[0] = v;
        else ab[1] = v;
    }
    const float2 z = make_float2(__fsub_rn(ab[0].x, ab[1].y), __fadd_rn(ab[0].y, ab[1].x));
    const unsigned r = (unsigned)((unsigned long long)(a.m_first + m) % bd.den);       // < 2^16
    const unsigned idx = r * bd.step % bd.den;                                         // (65535^2 < 2^32)
    const float2 w = reinterpret_cast<const float2 *>(bd.w)[idx];
    FO::store(out, m, mix_rotate(z, w), a.thr2);
}

// The tiled bank: decim4_cx_kernel<MixTileArgs>'s tile for every band of ka.band[0 .. nbands), the image staged once.
__global__ __launch_bounds__(64) void decim4_bank_kernel(const BankTileArgs ka)
{
    using C = DecimWide;
    static_assert(C::CHUNKS % 16 == 0, "whole 16-chunk rows");
    static_assert(DecimCx::P0FROM + DecimCx::PCH == C::WCH, "the two passes cover the window");
    constexpr int SCR = 64;                                  // slots of the transposition scratch: a quarter tile's 64 output chunks
    __shared__ __attribute__((aligned(16))) f32x4 img[C::SLOTS + SCR];
    __shared__ unsigned band_ph[BANK_MAX];                   // every band's phase at the wave's current tile

    const DecimTileArgs &a = ka;
    const int lane = threadIdx.x;
    const int ch = blockIdx.y;
    const float *in = a.in + 2 * a.in_stride * ch;
    const float *hist = a.hist + 2 * a.hist_stride * ch;
    float *out = a.out + 2 * a.out_stride * ch;
    const long long last_chunk = (a.n_in - 1) >> 1;
    const int n_odd = (int)(a.n_in & 1);
    const int K = ka.nbands;

    // the wide kernel's tile schedule, always XCD-blocked
    const int G = a.n_waves;
    const int b = blockIdx.x;
    int tile = wide_first_tile(b, 0, a.w8);
    if (tile >= a.n_tiles) return;

    unsigned boff[C::NI];
#pragma unroll
    for (int j = 0; j < C::NI; ++j) boff[j] = slot_source_offset(64u * j + lane, C::CHUNKS);

    auto stage = [&](int t) __attribute__((always_inline)) { wide_stage_cf32<true, 0>(img, in, hist, last_chunk, n_odd, lane, boff, t); };

    if (b == a.hist_wave) carry_history<8, C::HIST>(lane, in, hist, a.hist_out + 2 * a.hist_stride * ch, a.n_in);

    // every band's phase at the wave's first tile (the only divisions of the kernel; uniform)
#pragma nounroll
    for (int k = 0; k < K; ++k) {
        const unsigned den = ka.band[k].den;
        unsigned ph = ka.band[k].phase + ((unsigned)tile % den) * ka.band[k].tile_step % den;          // (65535^2 < 2^32)
        if (ph >= den) ph -= den;
        band_ph[k] = ph;                                     // (every lane the same word)
    }

    const f32x4 *win = img + 17 * lane;
    f32x4 *scr = img + C::SLOTS;
    const int swz_w = (lane & 1) ^ ((lane >> 1) & 3), swz_r = ((lane >> 2) & 1) ^ ((lane >> 3) & 3);   // the output transposition's swizzles
    for (; tile < a.n_tiles; tile += G) {
        stage(tile);
        SXFIR_WAIT_VMCNT(0);
        const long long m0 = (long long)tile * C::TILE_OUT;

#pragma nounroll
        for (int k = 0; k < K; ++k) {
            const BankBand &bd = ka.band[k];
            f32x2 a1a[8], a1b[8], a0a[8], a0b[8];
            {
                f32x2 hs[32], hv[32];
                unsigned long long tp = (unsigned long long)(a.taps + 256 * k);
                asm volatile("" : "+s"(tp));
                load_cx_taps(tp, 1, hs, hv);
                fir_cx_pass<DecimCx::NB>(std::make_integer_sequence<int, DecimCx::PCH>{}, win, hs, hv, a1a, a1b);
            }
            // the lane's eight table entries of this band, read behind pass 1 and in front of pass 0's FMAs
            const unsigned den = bd.den, s = bd.step;
            const unsigned tile_ph = band_ph[k];
            f32x2 wv[8];
            {
                unsigned long long wp = (unsigned long long)bd.w;
                asm volatile("" : "+s"(wp) : "v"(a1a[0]), "v"(a1a[7]), "v"(a1b[0]), "v"(a1b[7]));
                const __attribute__((address_space(1))) f32x2 *wt = (const __attribute__((address_space(1))) f32x2 *)wp;          // (global, not flat, loads)
                unsigned idx = bank_reduce(tile_ph + (unsigned)lane * bd.lane_step, den, bd.rden);      // (< den + 63 den)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    wv[i] = wt[idx];
                    idx += s;
                    if (idx >= den) idx -= den;
                }
            }
            {
                f32x2 hs[32], hv[32];
                unsigned long long tp = (unsigned long long)(a.taps + 256 * k);
                asm volatile("" : "+s"(tp) : "v"(a1a[0]), "v"(a1a[7]), "v"(a1b[0]), "v"(a1b[7]));
                load_cx_taps(tp, 0, hs, hv);
                fir_cx_pass<DecimCx::NB>(std::make_integer_sequence<int, DecimCx::PCH>{}, win + (DecimCx::P0FROM + DecimCx::P0FROM / 16), hs, hv, a0a, a0b);
            }
            f32x4 y[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                // A = P0 + P1 and B = P0 + P1, then y = A + j B: one rounding each; then the band's rotation
                f32x2 yy[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int i = 2 * kk + e;
                    const float are = __fadd_rn(a0a[i].x, a1a[i].x), aim = __fadd_rn(a0a[i].y, a1a[i].y);
                    const float bre = __fadd_rn(a0b[i].x, a1b[i].x), bim = __fadd_rn(a0b[i].y, a1b[i].y);
                    const float2 r = mix_rotate(make_float2(__fsub_rn(are, bim), __fadd_rn(aim, bre)), make_float2(wv[i].x, wv[i].y));
                    yy[e] = (f32x2){r.x, r.y};
                }
                y[kk] = (f32x4){yy[0].x, yy[0].y, yy[1].x, yy[1].y};
            }

            float *row = out + 2 * ka.band_stride * k;
            if (m0 + C::TILE_OUT <= a.n_out) {
                // a quarter tile at a time through the scratch behind the (live) image, then whole-line non-temporal stores
                f32x4 *dst = reinterpret_cast<f32x4 *>(row + 2 * m0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if ((lane >> 4) == q) {
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) scr[4 * (lane & 15) + (kk ^ swz_w)] = y[kk];
                    }
                    // (other lanes' writes: the compiler must read the scratch again in every quarter, and after the writes)
                    asm volatile("" ::: "memory");
                    const f32x4 v = scr[lane ^ swz_r];
                    asm volatile("" ::: "memory");
                    store16_policy<0>(v, dst + 64 * q + lane);
                }
            } else {
                wide_store_ragged(row, m0, lane, a.n_out, y);
            }
            // the band's phase at the wave's next tile
            unsigned next_ph = tile_ph + bd.stride_step;
            if (next_ph >= den) next_ph -= den;
            band_ph[k] = next_ph;
            // the next band's scratch writes, and behind the last band the next tile's DMA, come after these LDS reads have returned
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
}

}  // namespace sxfir
