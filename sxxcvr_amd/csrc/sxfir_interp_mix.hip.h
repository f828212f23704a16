// Translating interpolators (include/sxfir_translate_tx.h), gfx950: a complex-tap interpolator whose input sample m is turned by
// exp(+j 2 pi m s / den) = w[(den - (m s mod den)) mod den] in front of the filter, w[i] = exp(-j 2 pi i / den) the translating
// decimators' table (sxfir_design_rotator) in device memory, m the ABSOLUTE input index, s = (num ratio) mod den.  With
// t = (den - s) mod den the table index of sample m is (m t) mod den: the kernels step FORWARD through the table by t per input
// sample, an add and a conditional subtraction, and never form a negative value.  Two kernels:
//
//   * interp_mix_generic_kernel<F, FO>: one output per thread, any shape, format, stride and start -- the two chains of
//     interp_cx_generic_kernel (sxfir_kernels.hip.h) over window samples that are rotated as they are read.  One 64-bit modulo per
//     thread (the input index of the output), one 32-bit product and modulo per chain (its oldest sample), then the index moves by
//     t per sample along the descending j;
//   * interp_mix_pass_kernel<QI, LL>: x4 x 128 and x8 x 256 complex taps on CF32, interp_cx_pass_kernel's frame
//     (sxfir_interp_cx.hip.h: its staging, window read, two-chain passes, combine, transposition and stores, restated here because
//     that kernel is not edited).  Between the staged image landing and the window read the wave rotates the image IN PLACE in
//     LDS: all TILE_IN + 32 samples, the halo included, lane l the chunks l, 64 + l (and 128 + l) below CHUNKS -- 2.25 chunks of two
//     samples per lane at x4, 1.25 at x8 -- so the passes read rotated samples and what is carried to the next call's history,
//     read from HBM, stays raw.  The table entries of a tile (two 8-byte reads per chunk, a table of at most 512 KiB that lives in
//     L2) are fetched one tile ahead, in front of that tile's DMAs, and held in 2 NLOAD register pairs through the arithmetic.
//
// The counted wait.  s_waitcnt vmcnt(8) at the loop head presumes that at least eight VMEM instructions were issued behind the next
// tile's DMAs (the tile's eight stores: vmcnt counts loads and stores together, in issue order) -- "at most 8 outstanding" then
// means the DMAs have landed.  The table reads are issued in FRONT of the DMAs, so the sequence behind the DMAs is
// interp_cx_pass_kernel's, eight stores and nothing else, and the same wait covers the table reads.  They are written as inline
// instructions (an ordinary load's result, used while an LDS-DMA is in flight, makes the compiler wait with vmcnt(0) and drain the
// stores); behind the wait their registers pass through an empty statement, so no use of them can be placed in front of it.
//
// The wave's prologue holds the only divisions (the lane's offset, the first tile's phase); the steps per chunk, per DMA
// instruction, per tile and per stride of the tile loop come from the host, worked out in 64 bits (imix_tile_args,
// sxfir_launch.hip.h).  den <= 65536: every sum stays below 2^17, every product below 2^32.
//
// New code: the reference has no mixer in front of its interpolator (the SX1255 interpolates the one band around 0 Hz,
// SoapySX.cpp:1093).
#pragma once

#include "sxfir_decim_mix.hip.h"        // mix_rotate
#include "sxfir_interp_cx.hip.h"        // the pass kernel's frame: InterpPass8, interp_pass_steps, syn_first_tile, syn_load_tap_set

namespace sxfir {

struct TxMixer {
    const float *w;         // den (re, im) pairs: w[i] = exp(-j 2 pi i / den) (sxfir_design_rotator)
    unsigned den;           // 1 .. 65536
    unsigned t;             // (den - (num * ratio) mod den) mod den: table entries per INPUT sample
    unsigned phase;         // table index of the generic kernel's input 0 of the call; of the tiled kernel's sample -32 of the call
};

struct InterpMixGenericArgs {
    GenericArgs g;
    TxMixer mix;
};

struct InterpMixTileArgs {
    InterpTileArgs t;
    TxMixer mix;
    unsigned lane_step;     // (2 t) mod den: between the chunks of two lanes
    unsigned instr_step;    // (128 t) mod den: between a lane's chunks (64 chunks apart)
    unsigned tile_step;     // (TILE_IN t) mod den: between two tiles
    unsigned stride_step;   // (n_groups TILE_IN t) mod den: between two tiles of one wave
};

// interp_cx_generic_kernel's output over rotated samples: one output per thread.  Both chains (the a taps, the b taps) in one loop
// over the window, so a sample is rotated once; each chain is the real-tap interpolator's (interp_generic_output), bit for bit.
template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void interp_mix_generic_kernel(const InterpMixGenericArgs ma)
{
    const GenericArgs &a = ma.g;
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.n_out) return;
    const int ch = blockIdx.y;
    const char *in = (const char *)a.in + sizeof(typename F::storage) * a.in_stride * ch;
    const char *hist = (const char *)a.hist + sizeof(typename F::storage) * a.hist_stride * ch;
    char *out = (char *)a.out + sizeof(typename FO::storage) * a.out_stride * ch;
    const int L = a.ratio;
    const long long q = n / L;
    const int r = (int)(n - q * L);
    const int jl = a.ntaps / L / a.jsplit;
    const float *ta = a.taps, *tb = a.taps + a.ntaps;

    // the table index of input q: (phase + (q mod den) t) mod den                           ((65535^2 < 2^32))
    const unsigned den = ma.mix.den, t = ma.mix.t;
    unsigned iq = ma.mix.phase + (unsigned)((unsigned long long)q % den) * t % den;
    if (iq >= den) iq -= den;
    const float2 *w = reinterpret_cast<const float2 *>(ma.mix.w);

    float2 A = make_float2(0.0f, 0.0f), B = make_float2(0.0f, 0.0f);
    for (int p = 0; p < a.jsplit; ++p) {
        const int j0 = (p + 1) * jl - 1;                                // the chain's oldest sample: q - j0
        unsigned idx = iq + den - (unsigned)j0 * t % den;              // (j0 < 65536)
        if (idx >= den) idx -= den;
        float ai = 0.0f, aq = 0.0f, bi = 0.0f, bq = 0.0f;
        for (int j = j0; j >= p * jl; --j) {
            const float2 x = mix_rotate(sample_at<F>(a, in, hist, q - j), w[idx]);
            const float ha = ta[j * L + r], hb = tb[j * L + r];
            ai = __builtin_fmaf(ha, x.x, ai);
            aq = __builtin_fmaf(ha, x.y, aq);
            bi = __builtin_fmaf(hb, x.x, bi);
            bq = __builtin_fmaf(hb, x.y, bq);
            idx += t;
            if (idx >= den) idx -= den;
        }
        A = p == 0 ? make_float2(ai, aq) : make_float2(__fadd_rn(A.x, ai), __fadd_rn(A.y, aq));
        B = p == 0 ? make_float2(bi, bq) : make_float2(__fadd_rn(B.x, bi), __fadd_rn(B.y, bq));
    }
    FO::store(out, n, make_float2(__fsub_rn(A.x, B.y), __fadd_rn(A.y, B.x)), a.thr2);
}

template <int QI, int LL>
__global__ __launch_bounds__(64) void interp_mix_pass_kernel(const InterpMixTileArgs ma)
{
    using C = InterpPass8<QI, LL>;
    static_assert((QI == 4 && LL == 4) || (QI == 2 && LL == 8), "x4 with four inputs per lane, x8 with two");
    static_assert(C::CPL == 8, "eight stores per tile behind the next tile's DMAs");
    static_assert(C::TILE_IN >= C::HIST && (C::TILE_IN & (C::TILE_IN - 1)) == 0, "tile 0 is the only one that reaches into the history");
    static_assert((QI / 2) * 63 + C::NWU <= C::CHUNKS, "the last lane's window ends inside the image");
    static_assert(C::CHUNKS <= C::IMG, "slot = chunk: the rotation reads every slot of the image, writes those below CHUNKS");
    constexpr int NSETS = C::L / 2;               // tap sets (passes) of one table: (c, p) at 2c + p; b's follow a's
    __shared__ __attribute__((aligned(16))) f32x4 lds[C::IMG + C::OBUF];
    f32x4 *obuf = lds + C::IMG;

    const InterpTileArgs &a = ma.t;
    const int lane = threadIdx.x;
    const int ch = blockIdx.y;
    const float *in = a.in + 2 * a.in_stride * ch;
    const float *hist = a.hist + 2 * a.hist_stride * ch;
    float *out = a.out + 2 * a.out_stride * ch;
    const __attribute__((address_space(4))) f32x2 *tq0 = (const __attribute__((address_space(4))) f32x2 *)a.taps;

    // the pass kernel's tile schedule: in pass i the G workgroups cover tiles [iG, (i+1)G), those of one XCD a contiguous block
    const int G = a.n_groups;
    const int first_tile = syn_first_tile(blockIdx.x, G);
    if (first_tile >= a.n_tiles) return;
    // the next call's history: raw samples, from HBM
    if (first_tile == (a.n_tiles - 1) % G && lane < C::HIST) {
        const long long s = a.n_in - C::HIST + lane;
        const float2 v = s >= 0 ? reinterpret_cast<const float2 *>(in)[s] : reinterpret_cast<const float2 *>(hist)[s + C::HIST];
        reinterpret_cast<float2 *>(a.hist_out + 2 * a.hist_stride * ch)[lane] = v;
    }

    // the mixer's phases, 32 bits: the lane's chunks in a tile's image and the first tile's phase (the only divisions of the kernel)
    const unsigned den = ma.mix.den, tstep = ma.mix.t;
    unsigned lane_ph[C::NLOAD];
    lane_ph[0] = (unsigned)lane * ma.lane_step % den;                                          // (63 * 65535 < 2^32)
#pragma unroll
    for (int i = 1; i < C::NLOAD; ++i) {
        lane_ph[i] = lane_ph[i - 1] + ma.instr_step;
        if (lane_ph[i] >= den) lane_ph[i] -= den;
    }
    unsigned tile_ph = ma.mix.phase + ((unsigned)first_tile % den) * ma.tile_step % den;       // (65535^2 < 2^32)
    if (tile_ph >= den) tile_ph -= den;

    // a tile's table entries: the two samples of the lane's chunk 64 i + lane.  Every index is below den, so the lanes whose chunk
    // lies past the image's end read an entry too (and use it for nothing)
    // The reads are written out as instructions of their own: beside an LDS-DMA in flight the compiler waits with vmcnt(0) for
    // an ordinary load's result, which would drain the tile's stores at every loop head.  So nothing the compiler knows of is
    // pending on these registers; wait_image at the loop head makes them usable.
    f32x2 wt[C::NLOAD][2];
    const unsigned long long wbase = (unsigned long long)ma.mix.w;
    auto fetch = [&](unsigned ph) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < C::NLOAD; ++i) {
            unsigned i0 = ph + lane_ph[i];
            if (i0 >= den) i0 -= den;
            unsigned i1 = i0 + tstep;
            if (i1 >= den) i1 -= den;
            asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(wt[i][0]) : "v"(8u * i0), "s"(wbase) : "memory");      // (8 * 65535 < 2^20)
            asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(wt[i][1]) : "v"(8u * i1), "s"(wbase) : "memory");
        }
    };
    // the wait for a staged tile: its table entries and its image.  Counted (at most 8 outstanding: the eight stores issued behind
    // both) or, for a tile staged through registers and for a wave's first tile, everything.  BEHIND the wait the table registers
    // pass through an empty statement: every use of them follows it, and a copy the compiler makes for it follows the wait too
    auto wait_image = [&](bool counted) __attribute__((always_inline)) {
        static_assert(C::NLOAD == 2 || C::NLOAD == 3, "the operand lists below");
        if (counted) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (C::NLOAD == 3) asm volatile("" : "+v"(wt[0][0]), "+v"(wt[0][1]), "+v"(wt[1][0]), "+v"(wt[1][1]), "+v"(wt[2][0]), "+v"(wt[2][1]) :: "memory");
        else asm volatile("" : "+v"(wt[0][0]), "+v"(wt[0][1]), "+v"(wt[1][0]), "+v"(wt[1][1]) :: "memory");
    };

    // HBM -> LDS for one tile: interp_cx_pass_kernel's staging (samples [q0 - 32, q0 + TILE_IN), slot = chunk)
    const int n_full = (int)(a.n_in / C::TILE_IN);
    auto stage = [&](int tile) __attribute__((always_inline)) {
        const long long q0 = (long long)tile * C::TILE_IN;
        const bool interior = tile >= 1 && tile < n_full;
        if (interior) {
            if constexpr (QI == 4) {
#pragma unroll
                for (int i = 0; i < C::NLOAD; ++i) {
                    unsigned cc = 64 * i + lane;
                    cc = cc < (unsigned)C::CHUNKS ? cc : (unsigned)C::CHUNKS - 1u;
                    asm volatile("" : "+v"(cc));
                    const char *src = reinterpret_cast<const char *>(in + 2 * (q0 - 32)) + 16u * cc;
                    // chunks 16 .. CHUNKS - 17 are this tile's alone: all of instruction 1
                    if (i == 1) glds16<2>(src, lds + 64 * i);
                    else glds16(src, lds + 64 * i);
                }
            } else {
                // 80 chunks: 0 .. 15 (lanes 0 .. 15), 16 .. 63 (lanes 0 .. 47, this tile's alone), 64 .. 79 (lanes 0 .. 15); a lane
                // that sits an instruction out writes nothing (slot = the instruction's base + lane)
                static_assert(C::CHUNKS == 80 && C::IMG >= 80, "the x8 image");
                unsigned off = 16u * (unsigned)lane;
                asm volatile("" : "+v"(off));
                const char *src = reinterpret_cast<const char *>(in + 2 * (q0 - 32)) + off;
                if (lane < 16) glds16(src, lds);
                if (lane < 48) glds16<2>(src + 16 * 16, lds + 16);
                if (lane < 16) glds16(src + 16 * 64, lds + 64);
            }
        } else {
            // edge tiles (first / last of a call): through registers and plain LDS writes; stage() then returns false and the
            // caller waits with vmcnt(0) instead of the counted form, which presumes the DMA instructions
#pragma unroll
            for (int i = 0; i < C::NLOAD; ++i) {
                unsigned cc = 64 * i + lane;
                cc = cc < (unsigned)C::CHUNKS ? cc : (unsigned)C::CHUNKS - 1u;
                asm volatile("" : "+v"(cc));
                const long long s = q0 - 32 + 2 * (long long)cc;
                float2 v0, v1;
                const long long last = a.n_in - 1;
                if (s >= 0) v0 = reinterpret_cast<const float2 *>(in)[s <= last ? s : last];
                else v0 = reinterpret_cast<const float2 *>(hist)[s + C::HIST];
                if (s + 1 >= 0) v1 = reinterpret_cast<const float2 *>(in)[s + 1 <= last ? s + 1 : last];
                else v1 = reinterpret_cast<const float2 *>(hist)[s + 1 + C::HIST];
                lds[64 * i + lane] = (f32x4){v0.x, v0.y, v1.x, v1.y};
            }
        }
        return interior;
    };

    int tile = first_tile;
    fetch(tile_ph);
    stage(tile);
    bool counted = false;                                       // the staged tile's DMAs sit in front of CPL stores
    while (true) {
        // s_waitcnt vmcnt counts loads and stores together, in issue order: with the next tile's table reads and DMAs issued BEFORE
        // this tile's eight stores, "at most 8 outstanding" means both have landed
        wait_image(counted);
        const long long q0 = (long long)tile * C::TILE_IN;

        // ---- the rotation, in place: chunk 64 i + lane holds samples q0 - 32 + 2 (64 i + lane) and the one behind it.  (A slot
        // past CHUNKS belongs to no sample: it is read, since every lane runs the instruction anyway, and not written.)
#pragma unroll
        for (int i = 0; i < C::NLOAD; ++i) {
            const int slot = 64 * i + lane;
            const f32x4 v = lds[slot];
            const float2 r0 = mix_rotate(make_float2(v.x, v.y), make_float2(wt[i][0].x, wt[i][0].y));
            const float2 r1 = mix_rotate(make_float2(v.z, v.w), make_float2(wt[i][1].x, wt[i][1].y));
            if (64 * i + 63 < C::CHUNKS || slot < C::CHUNKS) lds[slot] = (f32x4){r0.x, r0.y, r1.x, r1.y};
        }
        // one wave: its LDS instructions complete in order; the window reads below follow the rotated writes
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

        // ---- the lane's window, once: samples q0 + QI g - 32 .. q0 + QI g + QI - 1  ->  image chunks (QI/2) g .. + NWU - 1
        // (row half p uses chunks 8 - 8p + t, t = 0 .. NW - 1, of these; both tap tables use the same)
        f32x4 win[C::NWU];
        {
            const f32x4 *wp = lds + (QI / 2) * lane;
#pragma unroll
            for (int t = 0; t < C::NWU; ++t) win[t] = wp[t];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // the image is free: fetch the next tile -- its table entries, then its image -- behind the arithmetic of this one
        const int next = tile + G;
        counted = false;
        // (the table reads are issued on the wave's last tile too -- every index is a valid one --, so that the registers have one
        // definition inside the loop and the compiler no reason to copy them while they are in flight)
        tile_ph += ma.stride_step;
        if (tile_ph >= den) tile_ph -= den;
        fetch(tile_ph);
        if (next < a.n_tiles) counted = stage(next);

        // what the next tap set's loads wait for: a result of the pass before (the tile's first set: a window register)
        f32x2 prev = __builtin_shufflevector(win[0], win[0], 0, 1);
#pragma unroll 1
        for (int c = 0; c < C::L / 4; ++c) {
            f32x2 y[QI][4];                                     // A, then the combined output
#pragma unroll
            for (int part = 0; part < 2; ++part) {              // the a table, then the b table
                f32x2 u[QI][4];                                 // P0, then P0 + P1
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    f32x2 hs[32];
                    syn_load_tap_set(hs, tq0, NSETS * part + 2 * c + p, false, prev);
                    f32x4 wv[C::NW];
#pragma unroll
                    for (int t = 0; t < C::NW; ++t) wv[t] = win[8 - 8 * p + t];
                    f32x2 acc[QI][4];                           // every chain's first FMA (tap row 15) writes it
                    interp_pass_steps<QI>(std::make_integer_sequence<int, C::NW>{}, wv, hs, acc);
#pragma unroll
                    for (int qi = 0; qi < QI; ++qi)
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {
                            if (p == 0) u[qi][rr] = acc[qi][rr];
                            else u[qi][rr] = (f32x2){__fadd_rn(u[qi][rr].x, acc[qi][rr].x), __fadd_rn(u[qi][rr].y, acc[qi][rr].y)};
                        }
                    prev = u[0][0];
                }
#pragma unroll
                for (int qi = 0; qi < QI; ++qi)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        if (part == 0) y[qi][rr] = u[qi][rr];
                        else y[qi][rr] = (f32x2){__fsub_rn(y[qi][rr].x, u[qi][rr].y), __fadd_rn(y[qi][rr].y, u[qi][rr].x)};
                    }
            }
            // phases 4c..4c+3 of the lane's inputs: chunks k = (L / 2) qi + 2c + {0, 1} of its CPL
#pragma unroll
            for (int qi = 0; qi < QI; ++qi) {
                const int k = (C::L / 2) * qi + 2 * c;
                obuf[C::CPL * lane + (k ^ (lane & (C::CPL - 1)))] = (f32x4){y[qi][0].x, y[qi][0].y, y[qi][1].x, y[qi][1].y};
                obuf[C::CPL * lane + ((k + 1) ^ (lane & (C::CPL - 1)))] = (f32x4){y[qi][2].x, y[qi][2].y, y[qi][3].x, y[qi][3].y};
            }
        }

        // ---- store: instruction i moves slots 64i .. 64i+63 = the rows of lanes 8i .. 8i+7, each lane the chunk its slot holds (a
        // permutation inside the 128-byte row): eight whole rows per instruction.  Always eight store instructions per full tile:
        // the counted wait relies on it.
        const long long o0 = q0 * C::L;
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
            const long long o_end = a.n_in * C::L;
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

}  // namespace sxfir
