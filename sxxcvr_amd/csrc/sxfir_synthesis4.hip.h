// The 4-band synthesizer (include/sxfir_synthesizer.h): four sub-bands into one x4 wideband stream in one pass (gfx950).  The
// channelizer of sxfir_chan4.hip.h, transposed.
//
// Band k is placed at k/4 cycles per output sample by h[n] (j)^(k n); with n = 4m + r the sum over the bands is
//   w[4m + r] = sum_j h[4j + r] v_r[m - j],     v_r[m] = sum_k (j)^(k r) x_k[m]:
// a 4-point DFT across the bands (twiddles +-1, +-j: additions only), then ONE real-tap x4 interpolation in which output phase r
// reads the stream v_r instead of x.  32 packed FMAs per output: what interp8_pass_kernel<4, ..., 4> spends on one band.
//
// Contract: the radix-2 butterflies, one rounding per real operation (chan4_butterfly, the same four lines):
//   a0 = x0 + x2, a1 = x0 - x2, b0 = x1 + x3, b1 = x1 - x3;  v0 = a0 + b0, v2 = a0 - b0,
//   v1 = (a1.re - b1.im, a1.im + b1.re), v3 = (a1.re + b1.im, a1.im - b1.re);
// then the real-tap interpolator's contract on v_r: jsplit contiguous ranges of j, one fmaf chain from +0 over j descending in each,
// P0 + P1.  x_k[<0] = 0, hence v_r[<0] = +0.
//
// synthesis4_kernel -- CF32, 4 bands x 128 taps -- is the x4 pass kernel's frame (sxfir_interp_pass.hip.h: one wave per workgroup, a
// tile of 256 inputs per band -> 1024 outputs, lane l owns inputs 4l..4l+3 and their sixteen outputs, one 128-byte line; the same
// transposition buffer, store path, XCD-blocked deal and counted wait) with this changed:
//   * four band images are staged per tile, 4 x (256 + 32) samples, three LDS-DMA instructions per band, the middle one -- rows no
//     other tile reads -- non-temporal;
//   * the butterflies run ONCE per sample, by the wave over LDS, in place: a lane reads chunk c of the four band images and writes
//     v_0..v_3 to the same four slots (2.25 chunks per lane and tile, 16 packed additions per chunk).  One wave: no barrier, LDS
//     operations of a wave complete in order.  The 32-sample history is kept in the x domain (a band's own last samples, as every
//     plan keeps them) and takes part in the butterflies of the next tile: 12.5 % more additions, no second kind of history;
//   * the four passes are by PHASE r: pass r holds the 32 taps h[4j + r] in 16 SGPR pairs (phase-major table, behind a laundered
//     pointer so that the four sets are not loaded at once), reads the lane's window of v_r -- 36 samples, 18 ds_read_b128 -- and
//     runs the two row-half chains of the lane's four inputs: 128 packed FMAs, every one with a scalar tap; P0 + P1; phases 2c,
//     2c + 1 of an input are one 16-byte chunk of the lane's line in the transposition buffer;
//   * the image is free once pass 3's window is in registers: the next tile's twelve DMA instructions are issued there, in front of
//     pass 3's arithmetic and the tile's eight stores, and awaited by s_waitcnt vmcnt(8) at the loop head.
//
// Per tile of 1024 outputs: 512 v_pk_fma_f32, 72 window ds_read_b128 + 12 of the butterflies + 8 of the transposition, 12 LDS-DMA
// instructions, 8 global_store_dwordx4 (1 KiB of consecutive addresses each).  LDS 4 x 3 KiB + 8 KiB = 20 480 B per wave -> 8 waves
// per CU.  Registers of the shipped instance: DESIGN.md 5.7 (tools/shipped_isa.py synthesis).
//
// synthesis_generic_kernel -- every other tap count, CF16 storage, S32 wire words out, misaligned output -- is one thread per input
// index: the butterflies once per (m - j) in named registers, four chains, four stores.
//
// New code: the reference interpolates inside the SX1255, which takes the one band around 0 Hz (SoapySX.cpp:1093 hands it the
// samples); placing four bands on the x4 raster has no counterpart there.
#pragma once

#include <utility>

#include "sxfir_chan4.hip.h"            // chan4_butterfly: the radix-2 4-point DFT, one rounding per real operation
#include "sxfir_interp_tile.hip.h"      // (through it sxfir_common.hip.h: glds16, the packed FMAs with scalar taps)
#include "sxfir_kernels.hip.h"          // GenericArgs, sample_at, the storage formats

namespace sxfir {

// The tiled kernel's arguments: InterpTileArgs' stream fields and the band stride of the input.
struct SynTileArgs {
    const float *in;        // channel 0, band 0, sample 0 of this call (8-byte aligned)
    const float *hist;      // channel 0: the 32 samples preceding `in` of band k at 32 k
    float *hist_out;
    float *out;             // 16-byte aligned
    const float *taps;      // phase-major: h[4j + r] at 32 r + j
    long long n_in;         // input samples per channel AND BAND (outputs = 4 n_in)
    long long in_stride;    // samples between channels
    long long band_stride;  // samples between the bands of a channel
    long long out_stride;   // outputs between channels (even)
    long long hist_stride;  // 4 x 32
    int n_tiles, n_groups;
};

struct Syn4 {
    static constexpr int NBANDS = 4;
    static constexpr int TILE_IN = 256;                   // inputs per band and tile
    static constexpr int HIST = 32;
    static constexpr int CHUNKS = (TILE_IN + HIST) / 2;   // staged chunks per band: samples [q0 - 32, q0 + 256)
    static constexpr int NLOAD = (CHUNKS + 63) / 64;      // DMA instructions per band
    static constexpr int IMG = NLOAD * 64;                // slots of a band image (the last instruction's clamped lanes land behind the chunks)
    static constexpr int CPL = 8;                         // output chunks per lane: 4 inputs x 4 outputs x 8 bytes / 16
    static constexpr int OBUF = 64 * CPL;
    static constexpr int NW = 18;                         // window chunks of a pass: image samples 4l .. 4l + 35
};

// One window chunk T of a pass of either synthesizer kernel: samples w = 2T, 2T + 1 of the lane's window meet the lane's q-th
// output of the pass (NQ of them) at tap row j = ROWS + STEP q + OFF - w (when 0 <= j < ROWS); hs[j >> 1] holds the pass's ROWS taps
// pairwise; each row half j / (ROWS / 2) has its own chain, whose first tap is its last row.  synthesis4_kernel: <32, 1, 0, 4>
// (pass = phase r, q = the lane's input qi); synthesis4x2_kernel: <64, 2, r >> 1, NQ> (pass = output residue r, q = output r + 4q
// of the lane's sixteen).
template <int T, int ROWS, int STEP, int OFF, int NQ>
__device__ __forceinline__ void syn_step(const f32x4 &v, const f32x2 (&hs)[ROWS / 2], f32x2 (&acc)[2][NQ])
{
    constexpr int HALF = ROWS / 2;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int w = 2 * T + s;
        const f32x2 x = s ? __builtin_shufflevector(v, v, 2, 3) : __builtin_shufflevector(v, v, 0, 1);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int j = ROWS + STEP * q + OFF - w;
            if (j >= 0 && j < ROWS) {
                // (w ascends, j descends: the last row of a half is its chain's first, from an inline +0)
                if ((j & (HALF - 1)) == HALF - 1) pk_fma_s_hi_first(acc[j / HALF][q], hs[j >> 1], x);
                else if (j & 1) pk_fma_s_hi(acc[j / HALF][q], hs[j >> 1], x);
                else pk_fma_s_lo(acc[j / HALF][q], hs[j >> 1], x);
            }
        }
    }
}

template <int ROWS, int STEP, int OFF, int NQ, int NW, int... Ts>
__device__ __forceinline__ void syn_steps(std::integer_sequence<int, Ts...>, const f32x4 (&win)[NW], const f32x2 (&hs)[ROWS / 2], f32x2 (&acc)[2][NQ])
{
    (syn_step<Ts, ROWS, STEP, OFF, NQ>(win[Ts], hs, acc), ...);
}

// The butterflies of one chunk (two samples) of the four band images of PITCH slots each, in place.
template <int PITCH>
__device__ __forceinline__ void syn_butterfly_chunk(f32x4 *img, int c)
{
    const f32x4 x0 = img[c], x1 = img[PITCH + c], x2 = img[2 * PITCH + c], x3 = img[3 * PITCH + c];
    f32x2 e[4], o[4];
    chan4_butterfly(__builtin_shufflevector(x0, x0, 0, 1), __builtin_shufflevector(x1, x1, 0, 1), __builtin_shufflevector(x2, x2, 0, 1),
                    __builtin_shufflevector(x3, x3, 0, 1), e);
    chan4_butterfly(__builtin_shufflevector(x0, x0, 2, 3), __builtin_shufflevector(x1, x1, 2, 3), __builtin_shufflevector(x2, x2, 2, 3),
                    __builtin_shufflevector(x3, x3, 2, 3), o);
#pragma unroll
    for (int r = 0; r < 4; ++r) img[PITCH * r + c] = (f32x4){e[r].x, e[r].y, o[r].x, o[r].y};
}

// The pass kernel's tile schedule: in pass i the G workgroups cover tiles [iG, (i+1)G), the workgroups of one XCD a contiguous block
// of them (a tile's history is its neighbour's tail: found in that XCD's L2).  Workgroup `b`'s first tile.  (Unsigned % 8, / 8:
// xcd_blocked's signed form is other code.)
__device__ __forceinline__ int syn_first_tile(unsigned b, int G)
{
    return (G % 8 == 0) ? (int)(b % 8) * (G / 8) + (int)(b / 8) : (int)b;
}

// A tap set of N SGPR pairs, set `index` of the table at `tq0`, behind an opaque pointer (hoisted, a tile's sets would need 128 SGPRs
// at once): the first set of a tile waits for nothing, a later one for `prev`, a result of the pass before.
template <int N>
__device__ __forceinline__ void syn_load_tap_set(f32x2 (&hs)[N], const __attribute__((address_space(4))) f32x2 *tq0, int index, bool first, const f32x2 &prev)
{
    unsigned long long tp = (unsigned long long)tq0;
    if (first) asm volatile("" : "+s"(tp));
    else asm volatile("" : "+s"(tp) : "v"(prev));
    const __attribute__((address_space(4))) f32x2 *tq = (const __attribute__((address_space(4))) f32x2 *)tp;
#pragma unroll
    for (int m = 0; m < N; ++m) hs[m] = tq[N * index + m];
}

__global__ __launch_bounds__(64) void synthesis4_kernel(const SynTileArgs a)
{
    using C = Syn4;
    static_assert(C::TILE_IN >= C::HIST && (C::TILE_IN & (C::TILE_IN - 1)) == 0, "tile 0 is the only one that reaches into the history");
    static_assert(2 * 63 + C::NW <= C::CHUNKS, "the last lane's window ends inside the image");
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
    if (first_tile == (a.n_tiles - 1) % G && lane < C::HIST) {
        float *ho = a.hist_out + 2 * a.hist_stride * ch;
        const long long s = a.n_in - C::HIST + lane;
#pragma unroll
        for (int k = 0; k < C::NBANDS; ++k) {
            const float2 v = s >= 0 ? reinterpret_cast<const float2 *>(in + 2 * a.band_stride * k)[s]
                                    : reinterpret_cast<const float2 *>(hist + 2 * C::HIST * k)[s + C::HIST];
            reinterpret_cast<float2 *>(ho + 2 * C::HIST * k)[lane] = v;
        }
    }

    // HBM -> LDS for one tile: samples [q0 - 32, q0 + 256) of every band.  Tiles below n_full have all their inputs (and store all
    // their outputs); of those all but tile 0 have their history inside this call's input.
    const int n_full = (int)(a.n_in / C::TILE_IN);
    auto stage = [&](int tile) __attribute__((always_inline)) {
        const long long q0 = (long long)tile * C::TILE_IN;
        const bool interior = tile >= 1 && tile < n_full;
        if (interior) {
#pragma unroll
            for (int i = 0; i < C::NLOAD; ++i) {
                unsigned cc = 64 * i + lane;
                cc = cc < (unsigned)C::CHUNKS ? cc : (unsigned)C::CHUNKS - 1u;
                asm volatile("" : "+v"(cc));
#pragma unroll
                for (int k = 0; k < C::NBANDS; ++k) {
                    const char *src = reinterpret_cast<const char *>(in + 2 * (a.band_stride * k + q0 - 32)) + 16u * cc;
                    // chunks 16 .. CHUNKS - 17 are this tile's alone: all of instruction 1 (non-temporal)
                    if (i == 1) glds16<2>(src, lds + C::IMG * k + 64 * i);
                    else glds16(src, lds + C::IMG * k + 64 * i);
                }
            }
        } else {
            // edge tiles (first / last of a call): through registers and plain LDS writes; stage() then returns false and the
            // caller waits with vmcnt(0) instead of the counted form, which presumes the DMA instructions
            const long long last = a.n_in - 1;
#pragma unroll 1
            for (int k = 0; k < C::NBANDS; ++k) {
                const float2 *ik = reinterpret_cast<const float2 *>(in + 2 * a.band_stride * k);
                const float2 *hk = reinterpret_cast<const float2 *>(hist + 2 * C::HIST * k);
#pragma unroll
                for (int i = 0; i < C::NLOAD; ++i) {
                    unsigned cc = 64 * i + lane;
                    cc = cc < (unsigned)C::CHUNKS ? cc : (unsigned)C::CHUNKS - 1u;
                    const long long s = q0 - 32 + 2 * (long long)cc;
                    float2 v0, v1;
                    if (s >= 0) v0 = ik[s <= last ? s : last];
                    else v0 = hk[s + C::HIST];
                    if (s + 1 >= 0) v1 = ik[s + 1 <= last ? s + 1 : last];
                    else v1 = hk[s + 1 + C::HIST];
                    lds[C::IMG * k + 64 * i + lane] = (f32x4){v0.x, v0.y, v1.x, v1.y};
                }
            }
        }
        return interior;
    };

    const __attribute__((address_space(4))) f32x2 *tq0 = (const __attribute__((address_space(4))) f32x2 *)a.taps;

    int tile = first_tile;
    bool counted = stage(tile);
    counted = false;                                            // (the first tile's DMAs have no stores behind them)
    while (true) {
        // s_waitcnt vmcnt counts loads and stores together, in issue order: with the next tile's twelve DMAs issued BEFORE this
        // tile's eight stores, "at most 8 outstanding" means the DMAs have landed
        if (counted) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const long long q0 = (long long)tile * C::TILE_IN;

        // ---- x -> v in place, once per sample: chunks lane, 64 + lane and (lanes 0..15) 128 + lane of the four images
        syn_butterfly_chunk<C::IMG>(lds, lane);
        syn_butterfly_chunk<C::IMG>(lds, 64 + lane);
        if (lane < C::CHUNKS - 128) syn_butterfly_chunk<C::IMG>(lds, 128 + lane);

        const int next = tile + G;
        counted = false;
        f32x2 ylo[4];                                           // phase 2c of the lane's four inputs, until phase 2c + 1 joins it
        f32x2 prev;                                             // a result of the pass before: what the next tap set's loads wait for
#pragma unroll
        for (int r = 0; r < C::NBANDS; ++r) {
            // the lane's window of v_r: image samples 4l .. 4l + 35 -> chunks 2l .. 2l + 17
            f32x4 win[C::NW];
            {
                const f32x4 *wp = lds + C::IMG * r + 2 * lane;
#pragma unroll
                for (int t = 0; t < C::NW; ++t) win[t] = wp[t];
            }
            if (r == C::NBANDS - 1) {
                // the images are free: fetch the next tile behind the arithmetic of this pass and the stores
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (next < a.n_tiles) counted = stage(next);
            }
            f32x2 hs[16];
            syn_load_tap_set(hs, tq0, r, r == 0, prev);      // (a set per pass)
            f32x2 acc[2][4];                                    // every chain's first FMA (rows 31 and 15) writes it
            syn_steps<32, 1, 0, 4>(std::make_integer_sequence<int, C::NW>{}, win, hs, acc);
            f32x2 y[4];
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) y[qi] = (f32x2){__fadd_rn(acc[0][qi].x, acc[1][qi].x), __fadd_rn(acc[0][qi].y, acc[1][qi].y)};
            prev = y[0];
            if ((r & 1) == 0) {
#pragma unroll
                for (int qi = 0; qi < 4; ++qi) ylo[qi] = y[qi];
            } else {
                // phases r - 1, r of input qi: chunk k = 2 qi + r / 2 of the lane's eight
#pragma unroll
                for (int qi = 0; qi < 4; ++qi) {
                    const int k = 2 * qi + (r >> 1);
                    obuf[C::CPL * lane + (k ^ (lane & (C::CPL - 1)))] = (f32x4){ylo[qi].x, ylo[qi].y, y[qi].x, y[qi].y};
                }
            }
        }

        // ---- store: instruction i moves slots 64i .. 64i+63 = the lines of lanes 8i .. 8i+7, each lane the chunk its slot holds:
        // eight whole lines per instruction.  Always eight store instructions per full tile: the counted wait relies on it.
        const long long o0 = q0 * 4;
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
            const long long o_end = a.n_in * 4;
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

// ---- every other shape: one thread per input index, the butterflies once per (m - j), four chains in registers

// Both synthesizer generic kernels read GenericArgs with ratio = 4 (2: oversampled), n_in = inputs per band, hist_len = a BAND's
// history (band k of a channel at k * hist_len of its hist_stride = 4 * hist_len samples) and band_stride = samples between the
// bands of a channel.

// Outputs 4m .. 4m + 3: per tap row j (descending inside each of the jsplit ranges) the four bands' samples at m - j, their
// butterflies, one FMA of each phase chain -- phases 0..3 by name, no per-thread array that an index could send to scratch.
template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void synthesis_generic_kernel(const GenericArgs a)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_in) return;
    const int ch = blockIdx.y;
    const long long sb = (long long)sizeof(typename F::storage);
    const char *in = (const char *)a.in + sb * a.in_stride * ch;
    const char *hist = (const char *)a.hist + sb * a.hist_stride * ch;
    const long long bs = sb * a.band_stride, hs = sb * a.hist_len;
    const int jl = a.ntaps / 4 / a.jsplit;
    f32x2 y0 = {0.0f, 0.0f}, y1 = y0, y2 = y0, y3 = y0;
    for (int p = 0; p < a.jsplit; ++p) {
        f32x2 u0 = {0.0f, 0.0f}, u1 = u0, u2 = u0, u3 = u0;
        for (int j = (p + 1) * jl - 1; j >= p * jl; --j) {
            const float2 x0 = sample_at<F>(a, in, hist, m - j), x1 = sample_at<F>(a, in + bs, hist + hs, m - j);
            const float2 x2 = sample_at<F>(a, in + 2 * bs, hist + 2 * hs, m - j), x3 = sample_at<F>(a, in + 3 * bs, hist + 3 * hs, m - j);
            f32x2 v[4];
            chan4_butterfly((f32x2){x0.x, x0.y}, (f32x2){x1.x, x1.y}, (f32x2){x2.x, x2.y}, (f32x2){x3.x, x3.y}, v);
            const float *t = a.taps + 4 * j;
            u0 = (f32x2){__builtin_fmaf(t[0], v[0].x, u0.x), __builtin_fmaf(t[0], v[0].y, u0.y)};
            u1 = (f32x2){__builtin_fmaf(t[1], v[1].x, u1.x), __builtin_fmaf(t[1], v[1].y, u1.y)};
            u2 = (f32x2){__builtin_fmaf(t[2], v[2].x, u2.x), __builtin_fmaf(t[2], v[2].y, u2.y)};
            u3 = (f32x2){__builtin_fmaf(t[3], v[3].x, u3.x), __builtin_fmaf(t[3], v[3].y, u3.y)};
        }
        if (p == 0) {
            y0 = u0; y1 = u1; y2 = u2; y3 = u3;
        } else {
            // (jsplit <= 2: the adjacent-pair tree is P0 + P1)
            y0 = (f32x2){__fadd_rn(y0.x, u0.x), __fadd_rn(y0.y, u0.y)};
            y1 = (f32x2){__fadd_rn(y1.x, u1.x), __fadd_rn(y1.y, u1.y)};
            y2 = (f32x2){__fadd_rn(y2.x, u2.x), __fadd_rn(y2.y, u2.y)};
            y3 = (f32x2){__fadd_rn(y3.x, u3.x), __fadd_rn(y3.y, u3.y)};
        }
    }
    // FO::store rounds to half once for CF16 and makes the wire words for S32
    char *out = (char *)a.out + sizeof(typename FO::storage) * a.out_stride * ch;
    FO::store(out, 4 * m, make_float2(y0.x, y0.y), a.thr2);
    FO::store(out, 4 * m + 1, make_float2(y1.x, y1.y), a.thr2);
    FO::store(out, 4 * m + 2, make_float2(y2.x, y2.y), a.thr2);
    FO::store(out, 4 * m + 3, make_float2(y3.x, y3.y), a.thr2);
}

// History carry-over of the generic path: band k's last hist_len samples of (hist_k ++ in_k), out of place as history_kernel.
template <typename S>
__global__ __launch_bounds__(256) void synthesis_history_kernel(S *hist_out, const S *hist, const S *in, long long n_in, long long in_stride,
                                                                long long band_stride, int hist_len)
{
    const int ch = blockIdx.y, k = blockIdx.z;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= hist_len) return;
    const long long s = n_in - hist_len + j;
    const long long h = ((long long)4 * ch + k) * hist_len;
    hist_out[h + j] = s >= 0 ? in[in_stride * ch + band_stride * k + s] : hist[h + s + hist_len];
}

}  // namespace sxfir
