// The base of the device code: what every kernel header builds on, and no kernel.  Vector types, the LDS-DMA front ends (untyped
// global_load_lds_dwordx4 and the typed buffer_load_format_x ... lds of the CF16 storage path), lane swaps, the packed FMAs with the
// tap in a VGPR pair or in an SGPR pair, half <-> float, the conflict-free lane maps' tables, the argument block of the multi-row
// decimators, and the pieces the tiled kernels repeat: the XCD-blocked deal of tiles, the tap set of a pass by tap half, the
// read-ahead prologue of a pass over the padded image, the edge chunk of an odd-length call and the fused history carry-over.  Includes no kernel header; every kernel header includes this one.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace sxfir {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef int v4i32 __attribute__((ext_vector_type(4)));      // a buffer resource descriptor in four SGPRs

// Argument block of the multi-row decimators (decim_dense_kernel, decim_blocks_kernel; profiling: decim_multi_kernel)
struct DecimMultiArgs {
    const void *in;         // channel 0, sample 0 of this call (aligned to one complex sample)
    const void *hist;       // NT samples preceding `in`
    void *hist_out;
    void *out;              // 16-byte aligned
    const float *taps;
    long long n_in, n_out;
    long long in_stride, out_stride, hist_stride;
    int n_tiles;            // workgroup tiles per channel
    int n_groups;           // workgroups per channel (strided passes over the tiles)
    unsigned long long *stamps;   // diagnostic builds only (ABL 3): 5 counters per wave
};

#define SXFIR_WAIT_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// LDS-DMA: 16 bytes per lane from HBM to LDS, no VGPR round trip.
// AUX = cache policy bits of the load (0 = default, 2 = nt: streaming, 1 = sc0, 16 = sc1)
template <int AUX = 0>
__device__ __forceinline__ void glds16(const void *gsrc, void *ldst)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)ldst, 16, 0, AUX);
}

// ---- typed LDS-DMA: the CF16 storage front end.  gfx950's LDS-DMA exists for one typed load, buffer_load_format_x; with a buffer
// descriptor of format {16, FLOAT} it fetches one half per lane and writes one float per lane to LDS address M0 + 4 * lane, so one
// instruction turns 128 consecutive source bytes (32 samples of half pairs) into 16 slots of a CF32 image: the texture path
// converts on the way in, bit for bit the conversion v_cvt_f32_f16 makes for every non-NaN half (tools/typed_dma_probe.hip).
// The descriptor {DATA_FORMAT 16, NUM_FORMAT FLOAT, X <- R}, stride 0, `size` bytes addressable from a 64-bit base that the
// caller rebuilds per tile from scalars: every offset is then a small constant and a call may be as long as it likes.
__device__ __forceinline__ v4i32 typed_dma_descriptor(unsigned long long base, int size)
{
    v4i32 rs;
    rs.x = __builtin_amdgcn_readfirstlane((int)(unsigned)base);
    rs.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32)) & 0xffff;
    rs.z = size;
    rs.w = 4 | (7 << 12) | (2 << 15);
    return rs;
}
// One instruction: lane l fetches the half at byte soff + voff of the descriptor's range, its float lands at LDS byte m0v + 4 l.
// This is the one place where the source writes M0 behind the compiler's back.  M0 is a reserved register to the compiler -- it
// sets it right before each of its own uses and keeps nothing in it across an asm statement -- so writing it here needs, and
// admits, no clobber entry.  What the caller owes: an instance that calls this holds no compiler-managed LDS-DMA (glds16) at all
// -- structurally, by `if constexpr`, not left to the optimizer: LLVM may hoist or merge ITS M0 set-up across an asm statement it
// cannot see into (tests/test_abi.py::test_shipped_code_object counts the M0 writes of every instance).
template <bool NT>
__device__ __forceinline__ void typed_dma_x(unsigned m0v, unsigned voff, const v4i32 &rs, unsigned soff)
{
    if constexpr (NT)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_format_x %1, %2, %3 offen nt lds"
                     :: "s"(m0v), "v"(voff), "s"(rs), "s"(soff) : "memory");
    else
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_format_x %1, %2, %3 offen lds"
                     :: "s"(m0v), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

// v_permlane32_swap_b32 vdst, src (gfx950): lanes 32-63 of vdst <-> lanes 0-31
// of src.  Inline asm on purpose: with two DIFFERENT operands hipcc 7.2's
// __builtin_amdgcn_permlane32_swap returns the first result register for both
// elements of its result pair (seen in the .s: "v_permlane32_swap v1, v2" then
// v1 used for r[0] and r[1]).  "s_nop 1" = the 2 wait states the ISA requires
// between a VALU write of an operand and the swap.
__device__ __forceinline__ void permlane32_swap(float &vdst, float &src)
{
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(vdst), "+v"(src));
}
__device__ __forceinline__ void permlane16_swap(float &vdst, float &src)
{
    // odd 16-lane rows of vdst <-> even rows of src (inline asm for the same reason as permlane32_swap)
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(vdst), "+v"(src));
}

// ---- packed FMAs: acc += tap * x for two floats (I, Q) at once -- two independent IEEE fused multiply-adds per v_pk_fma_f32,
// so the results are bit-identical to the scalar loop.  The tap is broadcast to both halves by op_sel: taps live in 64-bit
// register pairs {h[2k], h[2k+1]} and op_sel / op_sel_hi pick the low or the high dword for both lanes of the packed operation.
// Inline asm keeps the register picture of the scalar loop (the compiler's own packing of the /4 loop needs 178 VGPRs).
// The tap pair in VGPRs:
__device__ __forceinline__ void pk_fma_lo(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(hpair), "v"(x));
}
__device__ __forceinline__ void pk_fma_hi(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(hpair), "v"(x));
}
// a chain's first FMA: acc = fmaf(tap, x, +0.0f), the zero as an inline constant (no register cleared first)
__device__ __forceinline__ void pk_fma_hi_first(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm("v_pk_fma_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "=v"(acc) : "v"(hpair), "v"(x));
}
__device__ __forceinline__ void pk_fma_lo_first(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm("v_pk_fma_f32 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "=v"(acc) : "v"(hpair), "v"(x));
}

// the same packed FMAs with the tap pair in SGPRs
__device__ __forceinline__ void pk_fma_s_lo(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "s"(hpair), "v"(x));
}
__device__ __forceinline__ void pk_fma_s_hi(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "s"(hpair), "v"(x));
}
// the first FMA of a chain: acc = fmaf(tap, x, +0.0f) with the zero as an inline constant, so no register is cleared first
// (a cleared register costs a v_mov_b64 per chain and tile: 0.6 of a packed FMA's energy each, profiles/round4z9_price_list.txt)
__device__ __forceinline__ void pk_fma_s_lo_first(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm("v_pk_fma_f32 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "=v"(acc) : "s"(hpair), "v"(x));
}
__device__ __forceinline__ void pk_fma_s_hi_first(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm("v_pk_fma_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "=v"(acc) : "s"(hpair), "v"(x));
}

// ... as volatile asm (issue order = source order)
__device__ __forceinline__ void pk_fma_sv_lo(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "s"(hpair), "v"(x));
}
__device__ __forceinline__ void pk_fma_sv_hi(f32x2 &acc, const f32x2 &hpair, const f32x2 &x)
{
    asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "s"(hpair), "v"(x));
}


// byte offset (from the tile's first staged chunk) of the chunk that lands in slot q of the image
__device__ __forceinline__ unsigned slot_source_offset(unsigned q, unsigned chunks)
{
    unsigned off = q - (((q + 1u) * 3856u) >> 16);                        // (q+1)/17, exact for q < 4096
    off = off < chunks ? off : chunks - 1u;
    return 16u * off;
}

// output group r of lanes 8k..8k+7 of a half-wave, 5 bits each (see the kernel: conflict-free ds_read_b128 groups)
constexpr unsigned long long rgrp_word(int k)
{
    unsigned long long w = 0;
    for (int i = 0; i < 8; ++i) {
        const int l5 = 8 * k + i;
        const bool first = l5 < 4 || (l5 >= 12 && l5 < 16) || (l5 >= 20 && l5 < 28);
        const int idx = first ? (l5 < 4 ? l5 : (l5 < 16 ? l5 - 8 : l5 - 12)) : (l5 < 12 ? l5 - 4 : (l5 < 20 ? l5 - 8 : l5 - 16));
        w |= (unsigned long long)(2 * idx + (first ? 0 : 1)) << (5 * i);
    }
    return w;
}
__device__ __forceinline__ unsigned long long rgrp_table(int k)
{
    constexpr unsigned long long W0 = rgrp_word(0), W1 = rgrp_word(1), W2 = rgrp_word(2), W3 = rgrp_word(3);
    return k == 0 ? W0 : (k == 1 ? W1 : (k == 2 ? W2 : W3));
}

__device__ __forceinline__ float half_bits_to_float(unsigned bits16)
{
    return __half2float(__ushort_as_half((unsigned short)bits16));
}
__device__ __forceinline__ float half_lo_to_float(unsigned w) { return half_bits_to_float(w & 0xffffu); }
__device__ __forceinline__ float half_hi_to_float(unsigned w) { return half_bits_to_float(w >> 16); }

__device__ __forceinline__ unsigned pack_half2(float i, float q)
{
    const __half2 h = __floats2half2_rn(i, q);
    return *reinterpret_cast<const unsigned *>(&h);
}

// ---- the pieces every tiled kernel repeats

// The XCD-blocked deal: in a pass the 8 * w8 workgroups of a channel cover that many consecutive tiles; workgroup b takes the
// tile with this number, so that the workgroups of one XCD (blockIdx % 8 shares an XCD and its L2; speed only) hold a contiguous
// block of the pass and a tile's halo -- its neighbour's tail -- is found in that XCD's L2.
__device__ __forceinline__ int xcd_blocked(int b, int w8)
{
    return (b & 7) * w8 + (b >> 3);
}

// Taps 64 `half` .. 64 `half` + 63 of a 128-tap table as 32 SGPR pairs: the tap set of one pass of the kernels that walk a tile in
// two passes by tap half (chan4_kernel, chan4x2_kernel, resample45_kernel).  tp is an opaque scalar (the caller launders it per
// pass) so that the loads stay inside the tile loop: hoisted, the two sets would need 128 SGPRs at once.
__device__ __forceinline__ void load_tap_half(unsigned long long tp, int half, f32x2 (&hs)[32])
{
    const __attribute__((address_space(4))) f32x2 *tq = (const __attribute__((address_space(4))) f32x2 *)tp;
#pragma unroll
    for (int m = 0; m < 32; ++m) hs[m] = tq[32 * half + m];
}

// The read-ahead prologue of a pass over a lane's window of the padded image: chunks BASE .. BASE + NB - 1 (a pad slot after every 16)
template <int BASE, int NB>
__device__ __forceinline__ void fill_read_ahead(const f32x4 *win, f32x4 (&buf)[NB])
{
#pragma unroll
    for (int c = 0; c < NB; ++c) buf[c] = win[(BASE + c) + ((BASE + c) >> 4)];
}

// One 16-byte chunk of an edge tile's image: `slot0` is lane 0's slot of the DMA instruction.  With an odd n_in the call's last
// chunk holds ONE valid sample (`one_sample`): its second half lies beyond the caller's buffer (possibly beyond the allocation)
// and is never touched; that lane fetches 8 bytes through a register instead of taking part in the DMA.
__device__ __forceinline__ void stage_edge_chunk(bool one_sample, int lane, const f32x4 *src, f32x4 *slot0)
{
    if (one_sample) {
        const float2 v = *reinterpret_cast<const float2 *>(src);
        slot0[lane] = (f32x4){v.x, v.y, 0.0f, 0.0f};
    } else {
        glds16(src, slot0);
    }
}

// History carry-over fused into the launch (no second kernel): the wave that owns the call's last tile copies the last HIST
// samples of (hist ++ in) into the plan's OTHER history buffer (the current one is still being read by the wave of tile 0).
// SB = bytes per complex sample in HBM: 8 (CF32, S32 wire words) or 4 (CF16 half pairs); the pointers are the channel's.
template <int SB, int HIST>
__device__ __forceinline__ void carry_history(int lane, const void *in, const void *hist, void *hist_out, long long n_in)
{
    static_assert(SB == 4 || SB == 8, "half pairs or float pairs");
    for (int j = lane; j < HIST; j += 64) {
        const long long s = n_in - HIST + j;
        if constexpr (SB == 4) {
            reinterpret_cast<unsigned *>(hist_out)[j] = s >= 0 ? reinterpret_cast<const unsigned *>(in)[s]
                                                               : reinterpret_cast<const unsigned *>(hist)[s + HIST];
        } else {
            const float2 v = s >= 0 ? reinterpret_cast<const float2 *>(in)[s] : reinterpret_cast<const float2 *>(hist)[s + HIST];
            reinterpret_cast<float2 *>(hist_out)[j] = v;
        }
    }
}

}  // namespace sxfir
