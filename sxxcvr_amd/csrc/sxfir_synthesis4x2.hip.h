// The 2x oversampled 4-band synthesizer (include/sxfir_synthesizer_os.h): four sub-bands at fs/2 each into one wideband stream in
// one pass (gfx950).  The oversampled channelizer of sxfir_chan4x2.hip.h, transposed; written beside synthesis4_kernel
// (sxfir_synthesis4.hip.h), whose pieces are called here and not edited.
//
// Band k is interpolated by 2 and placed at k/4 cycles per output sample: w[n] = sum_k (j)^(k n) (h * up2 x_k)[n].  With n the
// ABSOLUTE output index and m = n >> 1 the absolute input index
//   w[n] = sum_i h[2i + (n & 1)] v_(n & 3)[(n >> 1) - i],     v_r[m] = sum_k (j)^(k r) x_k[m]:
// the synthesizer's 4-point DFT across the bands (additions only), then ONE real-tap x2 interpolation in which output n reads the
// stream v_(n mod 4).  The (-1)^(k m) of the channelizer's odd times is that choice of stream by the absolute index: nothing is
// multiplied.  64 packed FMAs per output: what a x2 interpolator of these taps spends on one band.
//
// Contract: chan4_butterfly, one rounding per real operation; then the real-tap x2 interpolator's contract on
// v_(n & 3): jsplit contiguous ranges of i, one fmaf chain from +0 over i descending in each, P0 + P1.  x_k[<0] = 0, hence v_r[<0] = +0.
//
// synthesis4x2_kernel -- CF32, 4 bands x 128 taps -- keeps synthesis4_kernel's frame (one wave per workgroup, the XCD-blocked deal,
// four band images staged by LDS-DMA, the butterflies once per sample in place over LDS, the transposition buffer and its eight
// 1 KiB stores, the next tile's DMAs behind a counted wait) on a tile twice as long:
//   * a tile is 512 inputs per band -> 1024 outputs; lane l owns inputs 8l..8l+7 and their sixteen outputs, one 128-byte line;
//   * the history is 64 samples per band: an image is 576 samples = 288 chunks, five DMA instructions per band and twenty per tile
//     (the fifth on 32 lanes), the middle three -- rows no other tile reads -- non-temporal; a band's five are issued as soon as
//     no later pass reads its image, two to three passes ahead of their use;
//   * the four passes are by output RESIDUE r = n mod 4 inside the tile, in the order 0, 2, 1, 3 (a tap set serves two passes): pass r holds the 64 taps h[2i + (r & 1)] in 32 SGPR pairs
//     (the phase-major table at ratio 2: by output parity; behind a laundered pointer), reads the lane's window -- 36 chunks -- of the image v_(r ^ 2 par) and runs
//     the two row-half chains of its four outputs 16l + r + 4q: 256 packed FMAs, every one with a scalar tap; P0 + P1; residues
//     2c, 2c + 1 of q are one 16-byte chunk of the lane's line in the transposition buffer;
//   * `par` is the parity of the call's absolute per-band start index, a uniform argument: it only selects which image a pass
//     reads, so a call that starts at an odd index runs the same code.
//
// Per tile of 1024 outputs: 1024 v_pk_fma_f32, 20 LDS-DMA instructions, 8 global_store_dwordx4.  LDS 4 x 4.5 KiB + 8 KiB = 26 624 B per
// wave -> 6 waves per CU.  Registers of the shipped instance: DESIGN.md 5.9 (tools/shipped_isa.py synthesis4x2).
//
// synthesis_os_generic_kernel -- every other tap count, CF16 storage, S32 wire words out, misaligned output -- is one thread per
// input index: outputs 2m and 2m + 1, the two DFT outputs their residues name, two chains in named registers.
//
// New code: the reference interpolates inside the SX1255, which takes the one band around 0 Hz (SoapySX.cpp:1093 hands it the
// samples); placing four oversampled bands on the /4 raster has no counterpart there.
#pragma once

#include <utility>

#include "sxfir_synthesis4.hip.h"       // SynTileArgs, syn_step, synthesis_history_kernel; through it chan4_butterfly, glds16, the packed FMAs

namespace sxfir {

// The tiled kernel's arguments: synthesis4_kernel's (hist: 64 samples of band k at 64 k; taps: parity-major, h[2i + p] at 64 p + i;
// outputs = 2 n_in) and the parity of the call's absolute per-band start index.
struct SynOsTileArgs {
    SynTileArgs s;
    int par;
};

struct Syn4x2 {
    static constexpr int NBANDS = 4;
    static constexpr int QI = 8;                          // inputs per lane and band (layout A of DESIGN.md 5.9; 4: layout B, synthesis4_kernel's tile)
    static constexpr int NQ = QI / 2;                     // outputs of a lane per pass
    static constexpr int TILE_IN = 64 * QI;               // inputs per band and tile
    static constexpr int HIST = 64;
    static constexpr int CHUNKS = (TILE_IN + HIST) / 2;   // staged chunks per band: samples [q0 - 64, q0 + TILE_IN)
    static constexpr int NLOAD = (CHUNKS + 63) / 64;      // DMA instructions per band
    static constexpr int IMG = CHUNKS;                    // slots of a band image: no more than the chunks (the last DMA instruction runs on the
                                                          // lanes below CHUNKS % 64 alone), so that six waves fit a CU's LDS
    static constexpr int CPL = QI;                        // output chunks per lane: QI inputs x 2 outputs x 8 bytes / 16
    static constexpr int OBUF = 64 * CPL;
    static constexpr int NW = (QI + HIST) / 2;            // window chunks of a pass: image samples QI l .. QI l + QI + 63
    static constexpr int NBFLY = (CHUNKS + 63) / 64;      // butterfly chunks per lane (the last one on the lanes below CHUNKS % 64)
};

__global__ __launch_bounds__(64) void synthesis4x2_kernel(const SynOsTileArgs ao)
{
    using C = Syn4x2;
    const SynTileArgs &a = ao.s;
    static_assert(C::TILE_IN >= C::HIST && (C::TILE_IN & (C::TILE_IN - 1)) == 0, "tile 0 is the only one that reaches into the history");
    static_assert(C::NQ * 63 + C::NW <= C::CHUNKS, "the last lane's window ends inside the image");
    static_assert(C::CPL == 8 || C::CPL == 4, "the counted wait below names the stores of a tile");
    static_assert(C::NBANDS * C::NLOAD < 64 - C::CPL, "the DMAs of a tile and its stores fit the 6-bit vmcnt");
    static_assert(C::HIST == 64, "one lane per history sample");
    // four band images (x, then v in place), then the 1024-output (8 KiB) transposition buffer
    __shared__ __attribute__((aligned(16))) f32x4 lds[C::NBANDS * C::IMG + C::OBUF];
    f32x4 *obuf = lds + C::NBANDS * C::IMG;

    const int lane = threadIdx.x;
    const int ch = blockIdx.y;
    const float *in = a.in + 2 * a.in_stride * ch;
    const float *hist = a.hist + 2 * a.hist_stride * ch;
    float *out = a.out + 2 * a.out_stride * ch;

    const int G = a.n_groups;
    const int first_tile = syn_first_tile(blockIdx.x, G);
    if (first_tile >= a.n_tiles) return;
    if (first_tile == (a.n_tiles - 1) % G) {
        float *ho = a.hist_out + 2 * a.hist_stride * ch;
        const long long s = a.n_in - C::HIST + lane;
#pragma unroll
        for (int k = 0; k < C::NBANDS; ++k) {
            const float2 v = s >= 0 ? reinterpret_cast<const float2 *>(in + 2 * a.band_stride * k)[s]
                                    : reinterpret_cast<const float2 *>(hist + 2 * C::HIST * k)[s + C::HIST];
            reinterpret_cast<float2 *>(ho + 2 * C::HIST * k)[lane] = v;
        }
    }

    // HBM -> LDS for one band of one tile: samples [q0 - 64, q0 + 512) of band k into image k.  Tiles below n_full have all their
    // inputs (and store all their outputs); of those all but tile 0 have their history inside this call's input.
    const int n_full = (int)(a.n_in / C::TILE_IN);
    auto stage_band = [&](int tile, int k) __attribute__((always_inline)) {
        const long long q0 = (long long)tile * C::TILE_IN;
        const bool interior = tile >= 1 && tile < n_full;
        unsigned el = lane;                                     // (opaque: the chunk offsets are worked out here, not kept in registers
        asm volatile("" : "+v"(el));                            // across the passes)
        if (interior) {
            const char *band = reinterpret_cast<const char *>(in + 2 * (a.band_stride * k + q0 - C::HIST));
#pragma unroll
            for (int i = 0; i < C::NLOAD; ++i) {
                const unsigned cc = 64 * i + el;
                // chunks 32 .. CHUNKS - 33 are this tile's alone: all of the middle instructions (non-temporal); the last
                // instruction's lanes behind the image's end stay out of it (their slots are the next image's)
                if (i >= 1 && i < C::NLOAD - 1) glds16<2>(band + 16u * cc, lds + C::IMG * k + 64 * i);
                else if (i < C::NLOAD - 1 || C::CHUNKS % 64 == 0) glds16(band + 16u * cc, lds + C::IMG * k + 64 * i);
                else if (cc < (unsigned)C::CHUNKS) glds16(band + 16u * cc, lds + C::IMG * k + 64 * i);
            }
        } else {
            // edge tiles (first / last of a call): through registers and plain LDS writes; stage_band() then returns false and the
            // caller waits with vmcnt(0) instead of the counted form, which presumes the DMA instructions
            const long long last = a.n_in - 1;
            const float2 *ik = reinterpret_cast<const float2 *>(in + 2 * a.band_stride * k);
            const float2 *hk = reinterpret_cast<const float2 *>(hist + 2 * C::HIST * k);
#pragma unroll
            for (int i = 0; i < C::NLOAD; ++i) {
                const unsigned cc = 64 * i + el;
                if (cc >= (unsigned)C::CHUNKS) continue;
                const long long s = q0 - C::HIST + 2 * (long long)cc;
                float2 v0, v1;
                if (s >= 0) v0 = ik[s <= last ? s : last];
                else v0 = hk[s + C::HIST];
                if (s + 1 >= 0) v1 = ik[s + 1 <= last ? s + 1 : last];
                else v1 = hk[s + 1 + C::HIST];
                lds[C::IMG * k + cc] = (f32x4){v0.x, v0.y, v1.x, v1.y};
            }
        }
        return interior;
    };

    const __attribute__((address_space(4))) f32x2 *tq0 = (const __attribute__((address_space(4))) f32x2 *)a.taps;
    // pass r reads the image of v_((r + 2 par) mod 4) = v_(r ^ 2 par): residues are counted from the stream's start
    const int flip = ao.par ? 2 : 0;

    int tile = first_tile;
#pragma unroll 1
    for (int k = 0; k < C::NBANDS; ++k) stage_band(tile, k);
    bool counted = false;                                       // (the first tile's DMAs have no stores behind them)
    while (true) {
        // s_waitcnt vmcnt counts loads and stores together, in issue order: with the next tile's twenty DMAs issued BEFORE this
        // tile's eight stores (a band's five as soon as its image is free), "at most 8 outstanding" means the DMAs have landed
        if (!counted) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if constexpr (C::CPL == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        const long long q0 = (long long)tile * C::TILE_IN;

        // ---- x -> v in place, once per sample: chunks lane, 64 + lane, .. and (lanes 0..31) 256 + lane of the four images
#pragma unroll
        for (int i = 0; i < C::NBFLY - 1; ++i) syn_butterfly_chunk<C::IMG>(lds, 64 * i + lane);
        if (lane < C::CHUNKS - 64 * (C::NBFLY - 1)) syn_butterfly_chunk<C::IMG>(lds, 64 * (C::NBFLY - 1) + lane);

        const int next = tile + G;
        counted = false;
        f32x2 ylo[2][C::NQ];                                    // residues 0 and 2 of the lane's outputs, until residues 1 and 3 join them
        f32x2 prev;                                             // a result of the pass before: what the next tap set's loads wait for
        f32x2 hs[32];                                           // the taps of a parity: loaded for the first pass of each pair
        // the passes in the order 0, 2, 1, 3 of their residues: two passes per tap set
#pragma unroll
        for (int pi = 0; pi < C::NBANDS; ++pi) {
            const int r = 2 * (pi & 1) + (pi >> 1);
            if ((pi & 1) == 0) syn_load_tap_set(hs, tq0, r & 1, pi == 0, prev);      // (a set per pair of passes)
            // the lane's window of v_(r ^ flip): image samples 8l .. 8l + 71 -> chunks 4l .. 4l + 35
            f32x4 win[C::NW];
            {
                const f32x4 *wp = lds + C::IMG * (r ^ flip) + C::NQ * lane;
#pragma unroll
                for (int t = 0; t < C::NW; ++t) win[t] = wp[t];
            }
            if (pi == C::NBANDS - 1) {
                // the last image is free once this window is in registers: its band of the next tile behind the arithmetic of
                // this pass and the stores
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (next < a.n_tiles) counted = stage_band(next, r ^ flip);
            }
            f32x2 acc[2][C::NQ];                                  // every chain's first FMA (rows 63 and 31) writes it
            // syn_step (sxfir_synthesis4.hip.h): window sample w meets output q (input 2q + (r >> 1) of the lane's eight) at tap row
            // i = 64 + 2q + (r >> 1) - w of the parity's 64
            if (r < 2) syn_steps<64, 2, 0, C::NQ>(std::make_integer_sequence<int, C::NW>{}, win, hs, acc);
            else syn_steps<64, 2, 1, C::NQ>(std::make_integer_sequence<int, C::NW>{}, win, hs, acc);
            f32x2 y[C::NQ];
#pragma unroll
            for (int q = 0; q < C::NQ; ++q) y[q] = (f32x2){__fadd_rn(acc[0][q].x, acc[1][q].x), __fadd_rn(acc[0][q].y, acc[1][q].y)};
            prev = y[0];
            if ((r & 1) == 0) {
#pragma unroll
                for (int q = 0; q < C::NQ; ++q) ylo[r >> 1][q] = y[q];
            } else {
                // outputs r - 1 + 4q, r + 4q of the lane's sixteen: chunk k = 2q + r / 2 of its eight
#pragma unroll
                for (int q = 0; q < C::NQ; ++q) {
                    const int k = 2 * q + (r >> 1);
                    obuf[C::CPL * lane + (k ^ (lane & (C::CPL - 1)))] = (f32x4){ylo[r >> 1][q].x, ylo[r >> 1][q].y, y[q].x, y[q].y};
                }
            }
            if (pi < C::NBANDS - 1) {
                // no later pass reads image r ^ flip: the next tile's band goes there now, two to three passes ahead of its use
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (next < a.n_tiles) stage_band(next, r ^ flip);
            }
        }

        // ---- store: instruction i moves slots 64i .. 64i+63 = the lines of lanes 8i .. 8i+7, each lane the chunk its slot holds:
        // eight whole lines per instruction.  Always eight store instructions per full tile: the counted wait relies on it.
        const long long o0 = q0 * 2;
        if (tile < n_full) {
            f32x4 v[C::CPL];
#pragma unroll
            for (int i = 0; i < C::CPL; ++i) v[i] = obuf[64 * i + lane];
#pragma unroll
            for (int i = 0; i < C::CPL; ++i) {
                const int slot = 64 * i + lane;
                const int g2 = slot / C::CPL, k2 = (slot & (C::CPL - 1)) ^ (g2 & (C::CPL - 1));
                __builtin_nontemporal_store(v[i], reinterpret_cast<f32x4 *>(out + 2 * (o0 + 2 * (C::CPL * g2 + k2))));
            }
        } else {
            // the call's last tile (no counted wait follows it: the wave ends here)
            const long long o_end = a.n_in * 2;
#pragma unroll
            for (int i = 0; i < C::CPL; ++i) {
                const int slot = 64 * i + lane;
                const int g2 = slot / C::CPL, k2 = (slot & (C::CPL - 1)) ^ (g2 & (C::CPL - 1));
                const f32x4 v = obuf[slot];
                const long long o = o0 + 2 * (C::CPL * g2 + k2);       // two output samples per chunk
                if (o + 2 <= o_end) __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(out + 2 * o));
            }
        }
        // the next tile's output writes reuse the buffer only after these reads have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (next >= a.n_tiles) break;
        tile = next;
    }
}

// ---- every other shape: one thread per input index, two chains in registers

// Outputs 2m and 2m + 1 (residues 2 (M & 1) and 2 (M & 1) + 1 for the absolute per-band input index M = a.m_first + m): per tap row i (descending inside each
// of the jsplit ranges) the four bands' samples at m - i, the two DFT outputs these residues name -- each the butterflies' own
// expression of it -- and one FMA of each chain; the chains by name, no per-thread array that an index could send to scratch.
template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void synthesis_os_generic_kernel(const GenericArgs a)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_in) return;
    const int ch = blockIdx.y;
    const long long sb = (long long)sizeof(typename F::storage);
    const char *in = (const char *)a.in + sb * a.in_stride * ch;
    const char *hist = (const char *)a.hist + sb * a.hist_stride * ch;
    const long long bs = sb * a.band_stride, hs = sb * a.hist_len;
    const bool odd = ((a.m_first + m) & 1) != 0;           // outputs of residues 2, 3: v_2 and v_3; else v_0 and v_1
    const int jl = a.ntaps / 2 / a.jsplit;
    f32x2 y0 = {0.0f, 0.0f}, y1 = y0;
    for (int p = 0; p < a.jsplit; ++p) {
        f32x2 u0 = {0.0f, 0.0f}, u1 = u0;
        for (int i = (p + 1) * jl - 1; i >= p * jl; --i) {
            const float2 x0 = sample_at<F>(a, in, hist, m - i), x1 = sample_at<F>(a, in + bs, hist + hs, m - i);
            const float2 x2 = sample_at<F>(a, in + 2 * bs, hist + 2 * hs, m - i), x3 = sample_at<F>(a, in + 3 * bs, hist + 3 * hs, m - i);
            // chan4_butterfly's lines for v_0 / v_2 (from a0, b0) and v_1 / v_3 (from a1, b1)
            const f32x2 a0 = {__fadd_rn(x0.x, x2.x), __fadd_rn(x0.y, x2.y)}, b0 = {__fadd_rn(x1.x, x3.x), __fadd_rn(x1.y, x3.y)};
            const f32x2 a1 = {__fsub_rn(x0.x, x2.x), __fsub_rn(x0.y, x2.y)}, b1 = {__fsub_rn(x1.x, x3.x), __fsub_rn(x1.y, x3.y)};
            f32x2 va, vb;
            if (odd) {
                va = (f32x2){__fsub_rn(a0.x, b0.x), __fsub_rn(a0.y, b0.y)};         // v_2
                vb = (f32x2){__fadd_rn(a1.x, b1.y), __fsub_rn(a1.y, b1.x)};         // v_3
            } else {
                va = (f32x2){__fadd_rn(a0.x, b0.x), __fadd_rn(a0.y, b0.y)};         // v_0
                vb = (f32x2){__fsub_rn(a1.x, b1.y), __fadd_rn(a1.y, b1.x)};         // v_1
            }
            const float *t = a.taps + 2 * i;
            u0 = (f32x2){__builtin_fmaf(t[0], va.x, u0.x), __builtin_fmaf(t[0], va.y, u0.y)};
            u1 = (f32x2){__builtin_fmaf(t[1], vb.x, u1.x), __builtin_fmaf(t[1], vb.y, u1.y)};
        }
        if (p == 0) {
            y0 = u0; y1 = u1;
        } else {
            // (jsplit <= 2: the adjacent-pair tree is P0 + P1)
            y0 = (f32x2){__fadd_rn(y0.x, u0.x), __fadd_rn(y0.y, u0.y)};
            y1 = (f32x2){__fadd_rn(y1.x, u1.x), __fadd_rn(y1.y, u1.y)};
        }
    }
    // FO::store rounds to half once for CF16 and makes the wire words for S32
    char *out = (char *)a.out + sizeof(typename FO::storage) * a.out_stride * ch;
    FO::store(out, 2 * m, make_float2(y0.x, y0.y), a.thr2);
    FO::store(out, 2 * m + 1, make_float2(y1.x, y1.y), a.thr2);
}

}  // namespace sxfir
