// The 2x oversampled 4-band channelizer (include/sxfir_channelizer_os.h): the four bands of the /4 raster, each at fs/2, in one
// pass (gfx950).
//
// With the tap index written n = 4j + r and m counting outputs at fs/2,
//   u_r[m] = sum_j h[4j + r] x[2m - 4j - r],     y_k[m] = (-1)^(k m) sum_r (j)^(k r) u_r[m].
// The even-time outputs are the critically sampled channelizer's (sxfir_chan4.hip.h); the odd-time outputs are that channelizer's
// on the stream advanced by two samples -- ONE 16-byte chunk of the wide tile's window -- and the factor (-1)^(k m) is a circular
// shift of the branch sums by two in front of the same butterflies: chan4_butterfly(u2, u3, u0, u1).  Nothing is multiplied.
//
// Contract: u_r is ONE fmaf chain from +0 over j descending, I and Q each ((jsplit, cw) = (1, 1), rotation 0, on the
// taps of phase r alone); then chan4_butterfly, one rounding per real operation, on (u0, u1, u2, u3) for even m and on
// (u2, u3, u0, u1) for odd m.
//
// chan4x2_kernel -- CF32, 4 bands x 128 taps -- stands on the wide tile as it is (sxfir_decim_wide.hip.h: 2048 inputs + 128-sample
// halo), that kernel's frame functions called from here, and on chan4_kernel's lane map:
//   * a tile is 2048 inputs -> 1024 outputs PER BAND; lane l owns outputs 16l..16l+15 of each band (one 128-byte line per band),
//     window base chunk 16l.  Its even-time output 2i (i = 0..7) is chan4_kernel's output i: window sample w meets it at tap
//     4i + 128 - w.  Its odd-time output 2i + 1 meets w at tap 4i + 130 - w: the same walk one chunk further on.  The lane's window
//     is 80 chunks, one more than the wide kernel's 79, still inside the image: lane 63 reads up to sample 2175 of 2176;
//   * TWO SWEEPS over the window, even times then odd times (chan4_sweep<0>, chan4_sweep<1> of sxfir_chan4.hip.h: that kernel's
//     own walk, the window one chunk further on for the odd times), each chan4_kernel's two passes by tap half (pass 1 = taps 127..64,
//     pass 0 = taps 63..0, the 64 taps of a pass in 32 SGPR pairs re-loaded per pass behind a laundered pointer): 4 x 47 window
//     ds_read_b128 and 2048 v_pk_fma_f32 per tile, every one with a scalar tap operand.  The even sweep's 32 butterfly results
//     (64 VGPRs) are held while the odd sweep accumulates.  (The other layout -- ONE sweep in which a window sample feeds sixteen
//     accumulators, half the window reads per FMA -- needs 64 accumulator pairs + the read-ahead buffer + the tile constants
//     beside each other: not built, LABBOOK.md 19);
//   * a tile's output is 32 KiB and the dead image holds 18 496 B: the bands leave in TWO TRIPS of two bands, 512 slots each.
//     Output chunk c of a band (512 per tile; lane l owns 8l..8l+7) sits at slot c ^ ((c >> 3) & 7): the 8 lanes a ds_write_b128
//     is served with hit 8 different slots mod 16, and the read-back of chunk 64k + l is slot 64k + (l ^ (l >> 3)) -- the wide
//     kernel's read-back form with the swizzle l >> 3, 16 different slots mod 16 per service group -- so each half of a band is
//     stored by wide_store_full<0>: every store instruction writes 1 KiB of consecutive addresses, non-temporal.  The ragged last
//     tile goes straight from the registers, band by band.
//
// Per tile of 1024 outputs per band: 2048 v_pk_fma_f32, 188 window ds_read_b128 + 32 of the output transposition, 19 LDS-DMA
// instructions, 32 global_store_dwordx4.  LDS 18 496 B per wave.  Registers of the shipped instance: DESIGN.md 5.8
// (tools/shipped_isa.py chan4x2).  No parity flag: the host sends a call that starts at an odd output index to the generic kernel.
//
// chan4x2_generic_kernel -- every other tap count, CF16 storage, S32 wire words, off-position or misaligned calls -- is one
// thread per output index: four chains in named registers, the butterflies with their operands chosen by the parity of the
// ABSOLUTE output index, four stores: chan_generic_output of sxfir_chan4.hip.h, the critically sampled plan's body with the shift.
//
// New code: the reference decimates inside the SX1255, whose base-band decimator takes the one band around 0 Hz
// (SoapySX.cpp:180-208 only programs the divider); an oversampled raster has no counterpart there.
#pragma once

#include <utility>

#include "sxfir_chan4.hip.h"            // ChanTileArgs, Chan4, chan4_sweep, chan4_butterfly, chan_generic_output; through it the wide tile's frame

namespace sxfir {

struct Chan4x2 {
    static constexpr int TILE_OUT = 2 * DecimWide::TILE_OUT;      // 1024 outputs per band and tile
    static constexpr int WCH = DecimWide::WCH + 1;                // 80 window chunks per lane
    static constexpr int BAND_SLOTS = 512;                        // a band's 1024 outputs in the dead image
    static constexpr int TRIP_BANDS = 2;                          // bands per trip through the image
};

// a.n_out: outputs per channel and band at fs/2; the call starts at an EVEN output index (the host's business)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void chan4x2_kernel(const ChanTileArgs a)
{
    using C = DecimWide;
    static_assert(C::CHUNKS % 16 == 0, "whole 16-chunk rows");
    static_assert(16 * 63 + Chan4x2::WCH <= C::CHUNKS, "lane 63's window ends inside the image");
    static_assert(Chan4x2::TRIP_BANDS * Chan4x2::BAND_SLOTS <= C::SLOTS, "two bands fit the dead image");
    static_assert(2 * Chan4x2::BAND_SLOTS == Chan4x2::TILE_OUT && Chan4x2::TILE_OUT * 2 == C::TILE_IN, "a band's tile at fs/2");
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

    // the wide kernel's staging with the shipped policy: instructions 1..16 non-temporal.  Its 19 tile-invariant source offsets are
    // worked out again per tile (some 80 VALU instructions beside 2048 packed FMAs) behind a laundered lane index: held over the
    // sweeps they are 19 of the registers that two waves per SIMD do not leave
    auto stage = [&](int t) __attribute__((always_inline)) {
        unsigned l = (unsigned)lane;
        asm volatile("" : "+v"(l));
        unsigned boff[C::NI];
#pragma unroll
        for (int j = 0; j < C::NI; ++j) boff[j] = slot_source_offset(64u * j + l, C::CHUNKS);
        wide_stage_cf32<true, 0>(img, in, hist, last_chunk, n_odd, lane, boff, t);
    };

    if (b == a.hist_wave) carry_history<8, C::HIST>(lane, in, hist, a.hist_out + 2 * a.hist_stride * ch, a.n_in);

    // lane l: outputs 16l..16l+15 of the tile; window from chunk 16l (lane stride 17 slots: conflict free)
    const f32x4 *win = img + 17 * lane;
    const int swz_w = lane & 7, swz_r = lane >> 3;         // the output transposition's swizzles
    for (; tile < a.n_tiles; tile += G) {
        stage(tile);
        SXFIR_WAIT_VMCNT(0);

        f32x4 y[Chan4::NBANDS][8];                         // y[k][q]: outputs 2q (even time), 2q + 1 (odd time) of band k
        {
            f32x2 e[8][4];                                 // the even times' butterflies, held over the odd sweep
            {
                f32x2 u[4][8];                             // u[r][i]: branch sum r of even-time output i
                chan4_sweep<0>(win, a.taps, u);
#pragma unroll
                for (int i = 0; i < 8; ++i) chan4_butterfly(u[0][i], u[1][i], u[2][i], u[3][i], e[i]);
            }
            f32x2 u[4][8];                                 // ... of odd-time output i
            chan4_sweep<1>(win, a.taps, u);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                f32x2 o[4];
                chan4_butterfly(u[2][i], u[3][i], u[0][i], u[1][i], o);       // (-1)^(k m): the branches shifted by two
#pragma unroll
                for (int k = 0; k < Chan4::NBANDS; ++k) y[k][i] = (f32x4){e[i][k].x, e[i][k].y, o[k].x, o[k].y};
            }
        }

        const long long m0 = (long long)tile * Chan4x2::TILE_OUT;
        if (m0 + Chan4x2::TILE_OUT <= a.n_out) {
            // two bands at a time through the dead image (512 swizzled slots each), then whole-line non-temporal stores; a trip's
            // writes follow the previous trip's reads in this wave's LDS queue
            auto store_half = [&](int kk, int k, int half) __attribute__((always_inline)) {
                wide_store_full<0>(img + Chan4x2::BAND_SLOTS * kk + 256 * half, out + 2 * a.band_stride * k, m0 + C::TILE_OUT * half, lane, swz_r);
            };
#pragma unroll
            for (int trip = 0; trip < Chan4::NBANDS / Chan4x2::TRIP_BANDS; ++trip) {
#pragma unroll
                for (int kk = 0; kk < Chan4x2::TRIP_BANDS; ++kk)
#pragma unroll
                    for (int q = 0; q < 8; ++q) img[Chan4x2::BAND_SLOTS * kk + 8 * lane + (q ^ swz_w)] = y[Chan4x2::TRIP_BANDS * trip + kk][q];
#pragma unroll
                for (int kk = 0; kk < Chan4x2::TRIP_BANDS; ++kk) {
                    store_half(kk, Chan4x2::TRIP_BANDS * trip + kk, 0);
                    store_half(kk, Chan4x2::TRIP_BANDS * trip + kk, 1);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < Chan4::NBANDS; ++k) wide_store_ragged(out + 2 * a.band_stride * k, m0, lane, a.n_out, y[k]);
        }
        // the next tile's DMA overwrites the image only after these LDS reads have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// ---- every other shape: one thread per output index, four chains in registers

// chan_generic_output (sxfir_chan4.hip.h) at the stream's ratio 2, the butterflies' operands by the parity of a.m_first + m
template <typename F, typename FO = F>
__global__ __launch_bounds__(256) void chan4x2_generic_kernel(const GenericArgs a) { chan_generic_output<F, FO, true>(a); }

}  // namespace sxfir
