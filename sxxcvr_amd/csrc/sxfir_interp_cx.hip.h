// Complex-tap interpolators (include/sxfir_complex_tx.h): one band onto the x L raster in one pass (gfx950).  The decimator of
// sxfir_decim_cx.hip.h, transposed.
//
//   y[n] = sum_j h[j L + n mod L] x[n / L - j],   h = a + j b
//
// Contract: A = a (*) x and B = b (*) x are the two real-tap interpolator results -- per output two fmaf chains
// from +0.0f over j descending in [16p, 16p + 16), P0 + P1 -- then y.re = A.re - B.im, y.im = A.im + B.re, one rounding each.
//
// interp_cx_pass_kernel<QI, LL> -- CF32, x4 x 128 taps (QI = 4) and x8 x 256 taps (QI = 2) -- is the pass kernel's frame
// (sxfir_interp_pass.hip.h: one wave per workgroup, lane g owns QI consecutive inputs of a tile of 64 QI and all their L QI outputs,
// the same image and LDS-DMA staging, XCD-blocked deal, transposition buffer, whole-line non-temporal stores, counted wait and fused
// history carry-over) with this changed:
//   * two chains per window read: the lane's window -- 18 (x4) / 17 (x8) ds_read_b128 -- is read ONCE per tile and serves the passes
//     of BOTH tap tables: per (phase group c, row half p) a pass with the 64 `a` taps in 32 SGPR pairs and a pass with the 64 `b`
//     taps (TAPS_PASS8_CX: the pass-major table of a, then that of b), each set loaded behind a laundered pointer so that no two
//     are live together.  2 x 512 (x4) / 2 x 256 (x8) v_pk_fma_f32 per tile, every one with a scalar tap: half the LDS reads, half
//     the staging and half the input bytes per FMA of two real-tap passes;
//   * the combine in registers: A = P0 + P1 and B = P0 + P1 per chain as the real kernel takes them, re = A.re - B.im and
//     im = A.im + B.re in front of the transposition writes;
//   * x8 stages its image with three DMA instructions instead of two, so that the rows no other tile reads (chunks 16 .. 63) are an
//     instruction of their own and non-temporal, as the x4 image's middle instruction is;
//   * no keyed and no wire-word instance: the keying count depends on the input alone and runs as count_keyed_kernel
//     (launch_interp_tiled), S32 words and CF16 storage run interp_cx_generic_kernel (sxfir_kernels.hip.h).
// The output path keeps the compiler's addressing at both ratios (the real x8 instance's hand-written store offsets are not
// carried over).  Eight stores per tile at both ratios (CPL = QI L / 2 = 8): the counted wait is s_waitcnt vmcnt(8).
//
// One kernel, two instances per ratio by argument struct: the complex-tap interpolators' (InterpTileArgs) and the translating
// interpolators' (InterpMixTileArgs, sxfir_mixer.hip.h); what the mixer adds sits under `if constexpr (MIX)`.  Between the staged
// image landing and the window read the wave rotates the image IN PLACE in LDS: all TILE_IN + 32 samples, the halo included, lane l
// the chunks l, 64 + l (and 128 + l) below CHUNKS -- 2.25 chunks of two samples per lane at x4, 1.25 at x8 -- so the passes read
// rotated samples and what is carried to the next call's history, read from HBM, stays raw.  The table entries of a tile (two 8-byte
// reads per chunk, a table of at most 512 KiB that lives in L2) are fetched one tile ahead, in front of that tile's DMAs, and held in
// 2 NLOAD register pairs through the arithmetic.  The wave's prologue holds the only divisions (the lane's offset, the first tile's
// phase); the steps per chunk, per DMA instruction, per tile and per stride of the tile loop come from the host.
//
// The counted wait.  s_waitcnt vmcnt(8) at the loop head presumes that at least eight VMEM instructions were issued behind the next
// tile's DMAs (the tile's eight stores: vmcnt counts loads and stores together, in issue order) -- "at most 8 outstanding" then
// means the DMAs have landed.  The mixer's table reads are issued in FRONT of the DMAs, so the sequence behind the DMAs is eight
// stores and nothing else in both instances, and the same wait covers the table reads.  They are written as inline instructions
// (an ordinary load's result, used while an LDS-DMA is in flight, makes the compiler wait with vmcnt(0) and drain the stores);
// behind the wait their registers pass through an empty statement, so no use of them can be placed in front of it.
//
// New code: in the reference the SX1255 interpolates what snd_pcm_writei hands it (SoapySX.cpp:1093), the one band around 0 Hz.
#pragma once

#include <type_traits>
#include <utility>

#include "sxfir_interp_pass.hip.h"      // InterpPass8, interp_pass_steps, InterpTileArgs
#include "sxfir_mixer.hip.h"            // Mixer, mix_rotate: the translating interpolators' instances
#include "sxfir_synthesis4.hip.h"       // syn_first_tile, syn_load_tap_set

namespace sxfir {

// The argument struct of the translating interpolators' instances (include/sxfir_translate_tx.h): the plain struct plus the mixer and
// the steps of the image walk, worked out by the host in 64 bits (imix_tile_args, sxfir_launch.hip.h)
struct InterpMixTileArgs : InterpTileArgs {
    Mixer mix;
    unsigned lane_step;     // (2 t) mod den: between the chunks of two lanes
    unsigned instr_step;    // (128 t) mod den: between a lane's chunks (64 chunks apart)
    unsigned tile_step;     // (TILE_IN t) mod den: between two tiles
    unsigned stride_step;   // (n_groups TILE_IN t) mod den: between two tiles of one wave
};

template <int QI, int LL, typename Args>
__global__ __launch_bounds__(64) void interp_cx_pass_kernel(const Args ka)
{
    using C = InterpPass8<QI, LL>;
    constexpr bool MIX = std::is_same_v<Args, InterpMixTileArgs>;
    static_assert((QI == 4 && LL == 4) || (QI == 2 && LL == 8), "x4 with four inputs per lane, x8 with two");
    static_assert(C::CPL == 8, "eight stores per tile behind the next tile's DMAs");
    static_assert(C::TILE_IN >= C::HIST && (C::TILE_IN & (C::TILE_IN - 1)) == 0, "tile 0 is the only one that reaches into the history");
    static_assert((QI / 2) * 63 + C::NWU <= C::CHUNKS, "the last lane's window ends inside the image");
    static_assert(!MIX || C::CHUNKS <= C::IMG, "slot = chunk: the rotation reads every slot of the image, writes those below CHUNKS");
    constexpr int NSETS = C::L / 2;               // tap sets (passes) of one table: (c, p) at 2c + p; b's follow a's
    __shared__ __attribute__((aligned(16))) f32x4 lds[C::IMG + C::OBUF];
    f32x4 *obuf = lds + C::IMG;

    const InterpTileArgs &a = ka;
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
    unsigned den = 0, tstep = 0, tile_ph = 0;
    unsigned lane_ph[C::NLOAD] = {};
    unsigned long long wbase = 0;
    if constexpr (MIX) {
        den = ka.mix.den, tstep = ka.mix.step;
        lane_ph[0] = (unsigned)lane * ka.lane_step % den;                                          // (63 * 65535 < 2^32)
#pragma unroll
        for (int i = 1; i < C::NLOAD; ++i) {
            lane_ph[i] = lane_ph[i - 1] + ka.instr_step;
            if (lane_ph[i] >= den) lane_ph[i] -= den;
        }
        tile_ph = ka.mix.phase + ((unsigned)first_tile % den) * ka.tile_step % den;                // (65535^2 < 2^32)
        if (tile_ph >= den) tile_ph -= den;
        wbase = (unsigned long long)ka.mix.w;
    }

    // a tile's table entries: the two samples of the lane's chunk 64 i + lane.  Every index is below den, so the lanes whose chunk
    // lies past the image's end read an entry too (and use it for nothing)
    // The reads are written out as instructions of their own: beside an LDS-DMA in flight the compiler waits with vmcnt(0) for
    // an ordinary load's result, which would drain the tile's stores at every loop head.  So nothing the compiler knows of is
    // pending on these registers; wait_image at the loop head makes them usable.
    f32x2 wt[MIX ? C::NLOAD : 1][2];
    auto fetch = [&](unsigned ph) __attribute__((always_inline)) {
        if constexpr (MIX) {
#pragma unroll
            for (int i = 0; i < C::NLOAD; ++i) {
                unsigned i0 = ph + lane_ph[i];
                if (i0 >= den) i0 -= den;
                unsigned i1 = i0 + tstep;
                if (i1 >= den) i1 -= den;
                asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(wt[i][0]) : "v"(8u * i0), "s"(wbase) : "memory");      // (8 * 65535 < 2^20)
                asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(wt[i][1]) : "v"(8u * i1), "s"(wbase) : "memory");
            }
        }
    };
    // the wait for a staged tile: its image and, with a mixer, its table entries.  s_waitcnt vmcnt counts loads and stores together,
    // in issue order: with the next tile's table reads and DMAs issued BEFORE this tile's eight stores, "at most 8 outstanding" means
    // both have landed; a tile staged through registers and a wave's first tile wait for everything.  BEHIND the wait the table
    // registers pass through an empty statement: every use of them follows it, and a copy the compiler makes for it follows the
    // wait too
    auto wait_image = [&](bool counted) __attribute__((always_inline)) {
        if (counted) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (MIX) {
            static_assert(C::NLOAD == 2 || C::NLOAD == 3, "the operand lists below");
            if constexpr (C::NLOAD == 3) asm volatile("" : "+v"(wt[0][0]), "+v"(wt[0][1]), "+v"(wt[1][0]), "+v"(wt[1][1]), "+v"(wt[2][0]), "+v"(wt[2][1]) :: "memory");
            else asm volatile("" : "+v"(wt[0][0]), "+v"(wt[0][1]), "+v"(wt[1][0]), "+v"(wt[1][1]) :: "memory");
        }
    };

    // HBM -> LDS for one tile: samples [q0 - 32, q0 + TILE_IN).  The first and the last 16 chunks are shared with the neighbouring
    // tiles (plain loads), those in between are this tile's alone (non-temporal).  Tiles below n_full have all their inputs (and
    // store all their outputs); of those all but tile 0 have their history inside this call's input.
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
        wait_image(counted);
        const long long q0 = (long long)tile * C::TILE_IN;

        // ---- the mixer's rotation, in place: chunk 64 i + lane holds samples q0 - 32 + 2 (64 i + lane) and the one behind it.  (A
        // slot past CHUNKS belongs to no sample: it is read, since every lane runs the instruction anyway, and not written.)
        if constexpr (MIX) {
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
        }

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
        if constexpr (MIX) {
            tile_ph += ka.stride_step;
            if (tile_ph >= den) tile_ph -= den;
            fetch(tile_ph);
        }
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
