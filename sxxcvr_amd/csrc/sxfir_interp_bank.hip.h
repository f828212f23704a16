// The kernels of the combiner bank (include/sxfir_bank_tx.h), gfx950: K translating interpolators whose results are summed into one
// wideband stream in one pass.  The tuner bank of sxfir_decim_bank.hip.h, transposed.
//
//   y[n] = y_0[n] + y_1[n] + .. + y_{K-1}[n]   (float32 adds in this order),   y_k the translating interpolator of band k
//
// interp_bank_generic_kernel: every shape and format -- interp_mix_generic_kernel's chain loop (sxfir_kernels.hip.h) inside a band
// loop in the thread.  The band cannot be a grid plane as it is in the tuner bank's generic kernel: the bands meet in one output word.
//
// interp4_bank_kernel: x4 x 128 complex taps on CF32, on the frame of interp_cx_pass_kernel<4, 4, InterpMixTileArgs>
// (sxfir_interp_cx.hip.h: one wave per workgroup, 256 inputs per band and 1024 outputs per tile, the LDS-DMA image with its 32-sample
// halo, the rotation of the image in place, 18 window reads that serve both tap tables, 1024 v_pk_fma_f32 with scalar taps per band,
// the transposition buffer, eight whole-line non-temporal stores), walked in STEPS: step (tile, k) is band k of a tile, the steps of a
// tile follow each other k = 0 .. K - 1 (a runtime count), and the tile is stored ONCE, behind its last step.
//
//   * Where the sum lives between the bands of a tile: in the transposition buffer, in the LANE-OWNER layout -- the slots lane g writes
//     in front of the transposition are the slots of its own sixteen outputs.  Band 0 writes them, band k > 0 reads them back, adds
//     (old + new: the order of the definition) and writes them again: a lane touches its own slots alone, so no lane waits for
//     another between bands.  Only behind the last band's writes does the wave read the buffer across lanes (the transposed read of
//     the store), and LDS instructions of one wave complete in order.  No accumulator registers: the register count stays near the
//     single-band instance's (DESIGN.md 5.16 has the figures), two waves per SIMD, no scratch memory.
//   * Staging: ONE image buffer.  The frame reads a lane's window into registers and then owns no part of the image, so the next
//     step's table reads and DMAs are issued right behind the window read and fly under this step's 1024 FMAs -- whether the next
//     step is the next band of this tile or band 0 of the wave's next tile.  A second image buffer would buy nothing.
//   * Per-band state: one word per band and LANE in LDS (4 KiB): the table index of the first sample of the lane's chunk `lane` in
//     the band's image of the wave's current tile -- the tile's phase and the lane's offset in one value.  The prologue writes it
//     (the kernel's only divisions); the step that fetches a band's table entries reads it, and writes it back advanced by the band's
//     stride_step (an add and a conditional subtraction).  A lane reads and writes its own words alone.  The sixteen per-band
//     argument entries are read with scalar loads at the step's (uniform) band index.
//
// The wait rule.  s_waitcnt vmcnt counts loads and stores together, in issue order.  Behind a step's window read the wave issues,
// for the NEXT step, six table reads (inline instructions, in FRONT of the DMAs, for the reason given in sxfir_interp_cx.hip.h) and
// then the three DMAs of the image (or, for an edge tile, ordinary loads the compiler waits for itself).
//   - The next step is band 0 of another tile and its image came by DMA: this tile's EIGHT stores are issued behind the DMAs.  At the
//     next step's head the outstanding sequence is [6 table reads][3 DMAs][8 stores]: s_waitcnt vmcnt(8) -- the frame's counted wait.
//   - The next step is band k > 0 of the SAME tile: there are no stores between the two steps.  Outstanding at the next step's head:
//     [the eight stores of the wave's previous tile, if any][6 table reads][3 DMAs] and NOTHING behind them: vmcnt(8) would let the
//     image be read before it has landed.  The wait is s_waitcnt vmcnt(0).  The stores it also waits for are a whole band's arithmetic
//     old.
//   - An image staged through registers (a call's first and last tile) and a wave's first step: vmcnt(0).
//
// New code: the reference interpolates one band around 0 Hz (SoapySX.cpp:1093).
#pragma once

#include "sxfir_decim_bank.hip.h"       // BANK_MAX
#include "sxfir_interp_cx.hip.h"        // the frame: InterpPass8, interp_pass_steps, syn_first_tile, syn_load_tap_set, mix_rotate

namespace sxfir {

// One band's mixer and its steps through the table (the host: bank_tx_bands, sxfir_launch.hip.h): mixer_of's rule for the translating
// interpolator at the call's first input.  The generic kernel reads w, den, step and phase.
struct BankTxBand {
    const float *w;         // den (re, im) pairs: w[i] = exp(-j 2 pi i / den) (sxfir_design_rotator)
    unsigned den;           // 1 .. 65536
    unsigned step;          // t = (den - s) mod den: table entries per input sample
    unsigned phase;         // table index of the call's first input (the tiled kernel: of sample -32 of the call, its halo's first)
    unsigned lane_step;     // (2 t) mod den: between the chunks of two lanes
    unsigned instr_step;    // (128 t) mod den: between a lane's chunks (64 chunks apart)
    unsigned tile_step;     // (256 t) mod den: between two tiles
    unsigned stride_step;   // (n_groups 256 t) mod den: between two tiles of one wave
    unsigned pad;
};

struct BankTxGenericArgs : GenericArgs {    // (hist_len: a band's history; band_stride: input samples between the bands of a channel)
    int nbands;
    BankTxBand band[BANK_MAX];
};

struct BankTxTileArgs : InterpTileArgs {    // (hist_stride: a channel's K histories of 32 samples, band k's at 32 k)
    long long band_stride;  // input samples between the bands of a channel
    int nbands;
    BankTxBand band[BANK_MAX];
};

// One output per thread, any ntaps / ratio / format: for every band interp_mix_generic_kernel's two chains over the band's rotated
// window (bit for bit), the combine, then the sum in band order.  Band k: its input row at band_stride k, its history at hist_len k of
// the channel's, its planar taps (a | b) at 2 ntaps k, its table and step.
template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void interp_bank_generic_kernel(const BankTxGenericArgs ka)
{
    const GenericArgs &a = ka;
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.n_out) return;
    const int ch = blockIdx.y;
    char *out = (char *)a.out + sizeof(typename FO::storage) * a.out_stride * ch;
    const int L = a.ratio;
    const long long q = n / L;
    const int r = (int)(n - q * L);
    const int jl = a.ntaps / L / a.jsplit;

    float2 acc = make_float2(0.0f, 0.0f);
#pragma nounroll
    for (int k = 0; k < ka.nbands; ++k) {
        const BankTxBand &bd = ka.band[k];
        const char *in = (const char *)a.in + sizeof(typename F::storage) * (a.in_stride * ch + a.band_stride * k);
        const char *hist = (const char *)a.hist + sizeof(typename F::storage) * (a.hist_stride * ch + (long long)a.hist_len * k);
        const float *ta = a.taps + (size_t)2 * a.ntaps * k, *tb = ta + a.ntaps;

        // the table index of input q: (phase + (q mod den) t) mod den                       ((65535^2 < 2^32))
        const unsigned den = bd.den, t = bd.step;
        unsigned iq = bd.phase + (unsigned)((unsigned long long)q % den) * t % den;
        if (iq >= den) iq -= den;
        const float2 *w = reinterpret_cast<const float2 *>(bd.w);

        float2 A = make_float2(0.0f, 0.0f), B = make_float2(0.0f, 0.0f);
        for (int p = 0; p < a.jsplit; ++p) {
            const int j0 = (p + 1) * jl - 1;                            // the chain's oldest sample: q - j0
            unsigned idx = iq + den - (unsigned)j0 * t % den;          // (j0 < 65536)
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
        const float2 y = make_float2(__fsub_rn(A.x, B.y), __fadd_rn(A.y, B.x));
        // acc = y_0, then acc + y_k: band 0 is taken as it is (its signed zeros stay)
        acc = k == 0 ? y : make_float2(__fadd_rn(acc.x, y.x), __fadd_rn(acc.y, y.y));
    }
    FO::store(out, n, acc, a.thr2);
}

// History carry-over of the generic path: band k's last hist_len samples of (hist_k ++ in_k), out of place as history_kernel; a
// channel's histories band after band (grid: x over hist_len, y channels, z bands).
template <typename S>
__global__ __launch_bounds__(256) void bank_tx_history_kernel(S *hist_out, const S *hist, const S *in, long long n_in, long long in_stride,
                                                              long long band_stride, int hist_len)
{
    const int ch = blockIdx.y, k = blockIdx.z;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= hist_len) return;
    const long long s = n_in - hist_len + j;
    const long long h = ((long long)gridDim.z * ch + k) * hist_len;
    hist_out[h + j] = s >= 0 ? in[in_stride * ch + band_stride * k + s] : hist[h + s + hist_len];
}

// The tiled combiner: the steps (tile, band) of the head comment.
__global__ __launch_bounds__(64) void interp4_bank_kernel(const BankTxTileArgs ka)
{
    using C = InterpPass8<4, 4>;
    constexpr int QI = 4;
    static_assert(C::CPL == 8, "eight stores per tile behind the next tile's DMAs");
    static_assert(C::TILE_IN >= C::HIST && (C::TILE_IN & (C::TILE_IN - 1)) == 0, "tile 0 is the only one that reaches into the history");
    static_assert((QI / 2) * 63 + C::NWU <= C::CHUNKS, "the last lane's window ends inside the image");
    static_assert(C::CHUNKS <= C::IMG && C::NLOAD == 3 && C::L == 4, "slot = chunk; three DMAs per image; one phase group");
    constexpr int NSETS = C::L / 2;               // tap sets (passes) of one table: row half p at p; b's follow a's
    __shared__ __attribute__((aligned(16))) f32x4 lds[C::IMG + C::OBUF];
    __shared__ unsigned band_ph[BANK_MAX][64];    // [band][lane]: table index of the first sample of chunk `lane` of the band's image
    f32x4 *obuf = lds + C::IMG;

    const InterpTileArgs &a = ka;
    const int lane = threadIdx.x;
    const int ch = blockIdx.y;
    const int K = ka.nbands;
    const float *in = a.in + 2 * a.in_stride * ch;
    const float *hist = a.hist + 2 * a.hist_stride * ch;
    float *out = a.out + 2 * a.out_stride * ch;
    const __attribute__((address_space(4))) f32x2 *tq0 = (const __attribute__((address_space(4))) f32x2 *)a.taps;

    // the pass kernel's tile schedule: in pass i the G workgroups cover tiles [iG, (i+1)G), those of one XCD a contiguous block
    const int G = a.n_groups;
    const int first_tile = syn_first_tile(blockIdx.x, G);
    if (first_tile >= a.n_tiles) return;
    // the next call's histories: raw samples, from HBM, band after band, by one wave
    if (first_tile == (a.n_tiles - 1) % G && lane < C::HIST) {
        float2 *ho = reinterpret_cast<float2 *>(a.hist_out + 2 * a.hist_stride * ch);
#pragma nounroll
        for (int k = 0; k < K; ++k) {
            const long long s = a.n_in - C::HIST + lane;
            const float2 v = s >= 0 ? reinterpret_cast<const float2 *>(in + 2 * ka.band_stride * k)[s]
                                    : reinterpret_cast<const float2 *>(hist)[C::HIST * k + s + C::HIST];
            ho[C::HIST * k + lane] = v;
        }
    }

    // every band's index of the lane's chunk `lane` at the wave's first tile (the only divisions of the kernel)
#pragma nounroll
    for (int k = 0; k < K; ++k) {
        const BankTxBand &bd = ka.band[k];
        const unsigned den = bd.den;
        unsigned ph = bd.phase + ((unsigned)first_tile % den) * bd.tile_step % den;                // (65535^2 < 2^32)
        if (ph >= den) ph -= den;
        ph += (unsigned)lane * bd.lane_step % den;                                                 // (63 * 65535 < 2^32)
        if (ph >= den) ph -= den;
        band_ph[k][lane] = ph;
    }

    // a step's table entries: the two samples of the lane's chunks 64 i + lane of band kb's image; the band's word moves on to the
    // wave's next tile.  Every index is below den, so the lanes whose chunk lies past the image's end read an entry too (and use it
    // for nothing), and so does the fetch behind a wave's last step.  Inline instructions: nothing the compiler knows of is pending on
    // these registers (sxfir_interp_cx.hip.h); wait_image makes them usable.
    f32x2 wt[C::NLOAD][2];
    auto fetch = [&](int kb) __attribute__((always_inline)) {
        const BankTxBand &bd = ka.band[kb];
        const unsigned den = bd.den, tstep = bd.step;
        const unsigned long long wbase = (unsigned long long)bd.w;
        unsigned ph = band_ph[kb][lane];
        unsigned nx = ph + bd.stride_step;
        if (nx >= den) nx -= den;
        band_ph[kb][lane] = nx;
#pragma unroll
        for (int i = 0; i < C::NLOAD; ++i) {
            const unsigned i0 = ph;
            unsigned i1 = i0 + tstep;
            if (i1 >= den) i1 -= den;
            asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(wt[i][0]) : "v"(8u * i0), "s"(wbase) : "memory");      // (8 * 65535 < 2^20)
            asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(wt[i][1]) : "v"(8u * i1), "s"(wbase) : "memory");
            ph += bd.instr_step;
            if (ph >= den) ph -= den;
        }
    };
    // the wait for a staged step (the rule: the head comment).  BEHIND the wait the table registers pass through an empty statement:
    // every use of them follows it, and a copy the compiler makes for it follows the wait too
    auto wait_image = [&](bool counted) __attribute__((always_inline)) {
        if (counted) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" : "+v"(wt[0][0]), "+v"(wt[0][1]), "+v"(wt[1][0]), "+v"(wt[1][1]), "+v"(wt[2][0]), "+v"(wt[2][1]) :: "memory");
    };

    // HBM -> LDS for one step: samples [q0 - 32, q0 + 256) of band kb.  The first and the last 16 chunks are shared with the
    // neighbouring tiles (plain loads), those in between are this tile's alone (non-temporal).  Tiles below n_full have all their
    // inputs; of those all but tile 0 have their history inside this call's input.  An edge tile reads no sample past the band's n_in.
    const int n_full = (int)(a.n_in / C::TILE_IN);
    auto stage = [&](int tile, int kb) __attribute__((always_inline)) {
        const long long q0 = (long long)tile * C::TILE_IN;
        const bool interior = tile >= 1 && tile < n_full;
        const float *inb = in + 2 * ka.band_stride * kb;
        if (interior) {
#pragma unroll
            for (int i = 0; i < C::NLOAD; ++i) {
                unsigned cc = 64 * i + lane;
                cc = cc < (unsigned)C::CHUNKS ? cc : (unsigned)C::CHUNKS - 1u;
                asm volatile("" : "+v"(cc));
                const char *src = reinterpret_cast<const char *>(inb + 2 * (q0 - 32)) + 16u * cc;
                if (i == 1) glds16<2>(src, lds + 64 * i);
                else glds16(src, lds + 64 * i);
            }
        } else {
            const float *histb = hist + 2 * C::HIST * kb;
#pragma unroll
            for (int i = 0; i < C::NLOAD; ++i) {
                unsigned cc = 64 * i + lane;
                cc = cc < (unsigned)C::CHUNKS ? cc : (unsigned)C::CHUNKS - 1u;
                asm volatile("" : "+v"(cc));
                const long long s = q0 - 32 + 2 * (long long)cc;
                float2 v0, v1;
                const long long last = a.n_in - 1;
                if (s >= 0) v0 = reinterpret_cast<const float2 *>(inb)[s <= last ? s : last];
                else v0 = reinterpret_cast<const float2 *>(histb)[s + C::HIST];
                if (s + 1 >= 0) v1 = reinterpret_cast<const float2 *>(inb)[s + 1 <= last ? s + 1 : last];
                else v1 = reinterpret_cast<const float2 *>(histb)[s + 1 + C::HIST];
                lds[64 * i + lane] = (f32x4){v0.x, v0.y, v1.x, v1.y};
            }
        }
        return interior;
    };

    int tile = first_tile, k = 0;
    fetch(0);
    stage(tile, 0);
    bool counted = false;
    while (true) {
        wait_image(counted);
        const long long q0 = (long long)tile * C::TILE_IN;

        // ---- the band's rotation, in place: chunk 64 i + lane holds samples q0 - 32 + 2 (64 i + lane) and the one behind it.  (A slot
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

        // ---- the lane's window, once: samples q0 + 4 g - 32 .. q0 + 4 g + 3  ->  image chunks 2 g .. + NWU - 1
        f32x4 win[C::NWU];
        {
            const f32x4 *wp = lds + (QI / 2) * lane;
#pragma unroll
            for (int t = 0; t < C::NWU; ++t) win[t] = wp[t];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // the image is free: fetch the next step -- its table entries, then its image -- behind the arithmetic of this one.  (The
        // table reads are issued behind the wave's last step too -- every index is a valid one --, so that the registers have one
        // definition inside the loop and the compiler no reason to copy them while they are in flight.)
        const bool last_band = k + 1 == K;
        const int nk = last_band ? 0 : k + 1;
        const int ntile = last_band ? tile + G : tile;
        counted = false;
        fetch(nk);
        // counted: the eight stores of THIS tile follow the DMAs; between two bands of one tile nothing does
        if (ntile < a.n_tiles) counted = stage(ntile, nk) && last_band;

        // band k's tap tables: the pass-major a table then the b table, 256 floats per band
        const __attribute__((address_space(4))) f32x2 *tqk = tq0 + 128 * k;
        // what the next tap set's loads wait for: a result of the pass before (the step's first set: a window register)
        f32x2 prev = __builtin_shufflevector(win[0], win[0], 0, 1);
        f32x2 y[QI][4];                                         // A, then the band's combined output
#pragma unroll
        for (int part = 0; part < 2; ++part) {                  // the a table, then the b table
            f32x2 u[QI][4];                                     // P0, then P0 + P1
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                f32x2 hs[32];
                syn_load_tap_set(hs, tqk, NSETS * part + p, false, prev);
                f32x4 wv[C::NW];
#pragma unroll
                for (int t = 0; t < C::NW; ++t) wv[t] = win[8 - 8 * p + t];
                f32x2 acc[QI][4];                               // every chain's first FMA (tap row 15) writes it
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
        // ---- the sum, in the lane's own slots of the transposition buffer: chunks 2 qi, 2 qi + 1 of its eight.  Band 0 writes y_0
        // as it is; band k adds itself to what the bands before it left: acc = fadd_rn(acc, y_k)
#pragma unroll
        for (int qi = 0; qi < QI; ++qi) {
            f32x4 *s0 = obuf + C::CPL * lane + ((2 * qi) ^ (lane & (C::CPL - 1)));
            f32x4 *s1 = obuf + C::CPL * lane + ((2 * qi + 1) ^ (lane & (C::CPL - 1)));
            f32x4 v0 = (f32x4){y[qi][0].x, y[qi][0].y, y[qi][1].x, y[qi][1].y};
            f32x4 v1 = (f32x4){y[qi][2].x, y[qi][2].y, y[qi][3].x, y[qi][3].y};
            if (k != 0) {
                const f32x4 o0 = *s0, o1 = *s1;
                v0 = (f32x4){__fadd_rn(o0.x, v0.x), __fadd_rn(o0.y, v0.y), __fadd_rn(o0.z, v0.z), __fadd_rn(o0.w, v0.w)};
                v1 = (f32x4){__fadd_rn(o1.x, v1.x), __fadd_rn(o1.y, v1.y), __fadd_rn(o1.z, v1.z), __fadd_rn(o1.w, v1.w)};
            }
            *s0 = v0;
            *s1 = v1;
        }

        if (last_band) {
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
        }
        // the next step's buffer writes come only after this step's reads of it have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (ntile >= a.n_tiles) break;
        tile = ntile;
        k = nk;
    }
}

}  // namespace sxfir
