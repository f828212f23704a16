// Plan bookkeeping of the C ABI (include/sxfir.h): what a plan holds and which of the four kinds it is, the kernel table (which
// instance a shape launches: the one statement of it, for the occupancy queries and the launches), the creation frame every
// sxfir_create* goes through (argument checks, the device, the plan's common fields, the real-tap contract, the plan's device
// memory and the one list of what to free), how sxfir_create settles a real-tap plan's flags and lays out its tap tables, the
// one creation path of the four band plans (create_band_plan), and the small state entry points (reset, history, position, contract).
// Included by sxfir.hip after the kernel headers; not a stand-alone translation unit.
#pragma once

// What created the plan: sxfir_create, sxfir_create_complex (sxfir_complex.hip.h), sxfir_create_channelizer
// (sxfir_channelizer.hip.h), sxfir_create_synthesizer (sxfir_synthesizer.hip.h), sxfir_create_channelizer_os
// (sxfir_channelizer_os.hip.h: KIND_CHANNELIZER with ratio = bands / oversample), sxfir_create_synthesizer_os
// (sxfir_synthesizer_os.hip.h: KIND_SYNTHESIZER with ratio = bands / oversample).  A complex-tap plan is a decimator whose taps_dev
// holds a[0, ntaps) then b[0, ntaps); the band kinds are a /ratio decimator and a x ratio interpolator in everything about the stream.
enum PlanKind { KIND_REAL = 0, KIND_COMPLEX = 1, KIND_CHANNELIZER = 2, KIND_SYNTHESIZER = 3 };
enum TapTable { TAPS_SCALED = 0, TAPS_SUBSET8 = 1, TAPS_PASS8 = 2, TAPS_BLOCKS16 = 3, TAPS_PHASED = 4 };

// Which kernel family a call launches (LaunchGeom::kind, sxfir_launch.hip.h)
enum { GEOM_GENERIC = 0, GEOM_MULTI = 1, GEOM_WIDE = 2, GEOM_TILE = 3, GEOM_IPASS = 4, GEOM_ITILE = 5, GEOM_CX = 6, GEOM_CHAN4 = 7, GEOM_SYN4 = 8, GEOM_CHAN4X2 = 9, GEOM_SYN4X2 = 10 };

// One typed kernel pointer per launch-argument family, and a plan's kernels: resolved once by the plan's creator
// (resolve_kernels below), read by the occupancy queries there and by the launches (sxfir_launch.hip.h).
typedef void (*GenericFn)(sxfir::GenericArgs);
typedef void (*DecimMultiFn)(sxfir::DecimMultiArgs);
typedef void (*DecimBlocksFn)(sxfir::DecimMultiArgs, sxfir::DecimBlocksJoin);
typedef void (*DecimTileFn)(sxfir::DecimTileArgs);
typedef void (*InterpTileFn)(sxfir::InterpTileArgs);
typedef void (*ChanTileFn)(sxfir::ChanTileArgs);
typedef void (*ChanGenericFn)(sxfir::ChanGenericArgs);
typedef void (*ChanOsGenericFn)(sxfir::ChanOsGenericArgs);
typedef void (*SynTileFn)(sxfir::SynTileArgs);
typedef void (*SynGenericFn)(sxfir::SynGenericArgs);
typedef void (*SynOsTileFn)(sxfir::SynOsTileArgs);
typedef void (*SynOsGenericFn)(sxfir::SynOsGenericArgs);
struct KernelTable {
    GenericFn generic;           // decim_generic_kernel / decim_cx_generic_kernel / interp_generic_kernel: every plan has one
    DecimMultiFn dense;          // decim_dense_kernel (/8, /16, /32)
    DecimBlocksFn blocks[2];     // decim_blocks_kernel (/48, /96): [0] the walking form, [1] SPLIT, (tile, block) items
    DecimTileFn tile, wide, cx;  // /4: decim4_tile_kernel, decim4_wide_kernel, decim4_cx_kernel (complex taps)
    InterpTileFn interp[2][2];   // [keyed][split]: interp8_pass_kernel; interp_tile_kernel on CF16 storage ([0][0] alone)
    ChanTileFn chan4;            // channelizer plans (include/sxfir_channelizer.h): chan4_kernel (4 bands x 128 taps, CF32) ...
    ChanGenericFn chan_generic;  // ... and chan_generic_kernel, which every channelizer plan has INSTEAD of `generic`
    ChanTileFn chan4x2;          // 2x oversampled channelizer plans (include/sxfir_channelizer_os.h): chan4x2_kernel (4 bands x 128 taps, CF32) ...
    ChanOsGenericFn chan4x2_generic;   // ... and chan4x2_generic_kernel, which every such plan has INSTEAD of `generic` and `chan_generic`
    SynTileFn syn4;              // synthesizer plans (include/sxfir_synthesizer.h): synthesis4_kernel (4 bands x 128 taps, CF32) ...
    SynGenericFn syn_generic;    // ... and synthesis_generic_kernel, which every synthesizer plan has INSTEAD of `generic`
    SynOsTileFn syn4x2;          // 2x oversampled synthesizer plans (include/sxfir_synthesizer_os.h): synthesis4x2_kernel (4 bands x 128 taps, CF32) ...
    SynOsGenericFn syn4x2_generic;     // ... and synthesis_os_generic_kernel, which every such plan has INSTEAD of `generic` and `syn_generic`
};

// What the geometry and launch code needs to know of a band plan's pair of kernels (BAND_FORMS below; resolve_kernels picks one)
struct BandForm {
    const char *tiled, *generic;   // the kernels' names, as sxfir_launch_geometry reports them
    int geom;                      // GEOM_* of the tiled kernel: also names the form where the typed pointers and argument structs differ
    int tile;                      // the tiled kernel's tile PER BAND: outputs of a channelizer, inputs of a synthesizer
    int start_multiple;            // the tiled kernel takes a call that starts at a stream position that is a multiple of this (1: any)
};

struct sxfir_plan {
    int kind;              // PlanKind
    int mode, ntaps, ratio, nchan, fmt, device;
    int bands;             // the band kinds: 4 (= ratio, but for the oversampled plans); else 0.  A synthesizer's hist_dev holds
                           // bands x hist_len / bands samples per channel, band k's at k * hist_len / bands
    int oversample;        // channelizer plans: bands / ratio -- 1 critically sampled (sxfir_create_channelizer), 2 each band at fs/2
                           // (sxfir_create_channelizer_os: ratio 2, bands 4); synthesizer plans likewise: 1 each band at fs/4
                           // (sxfir_create_synthesizer), 2 each band at fs/2 (sxfir_create_synthesizer_os: ratio 2, bands 4); else 0
    int kernel;            // SXFIR_KERNEL_*
    int hist_len;          // samples of history kept per channel
    int blocks;            // /48, /96: sixteen-column blocks of decim_blocks_kernel (3, 6), else 0
    int jsplit, cw;        // numeric contract
    int rot;               // ... and its rotation (0; 1 for /48, /96: sxfir_contract_rotation)
    void *join_partials;   // /48, /96: scratch of decim_blocks_kernel<..., SPLIT>: join_tiles x blocks block values of 4 KiB
    unsigned *join_arrived;   // ... and one arrival counter per (channel, tile); zero between launches: each tile's last item
                              // zeroes its own, sxfir_reset and a failed launch zero them all
    long long join_tiles;  // tiles (over all channels) the scratch holds = the largest call the SPLIT form takes
    bool blocks_split;     // (profiling: SXFIR_BLOCKS_SPLIT=0 switches the (tile, block) dealing off)
#ifdef SXFIR_PROFILING
    int join_drop;         // SXFIR_BLOCKS_JOIN_DROP=<b> (test hook): the items of block b store their block value to join_shadow instead
    void *join_shadow;     // of the scratch, where it is copied behind the launch (join_tiles x 4 KiB, allocated with the knob); -1 = off
#endif
    bool ipass_split;      // x32, x48, x96: (tile, phase block) items for small calls (profiling: SXFIR_IPASS_SPLIT=0 switches it off)
    bool tile_capable;     // decim4_tile_kernel (ratio 4, 128 or 64 taps, CF32)
    bool multi_capable;    // decim_multi_kernel (ratio 8/16/32, 32 taps per phase, CF32)
    bool itile_capable;    // interp_tile_kernel (ratio 4/8/16/32, 32 taps per phase, CF32)
    int dense_nt;          // profiling build, SXFIR_DENSE_NT = 1 / 0: decim_dense_kernel with nt / plain staging loads at every ratio
    int dense_nt_set;      // ... and whether the knob was given at all
    bool dense_hc;         // (profiling) SXFIR_DENSE_HC=1: decim_dense_kernel with halo carry (/32, /16)
    bool dense_subset;     // /8, CF32 or S32 words: the scalar-tap form of decim_dense_kernel (tap subsets on the four waves)
    bool dense32;          // decim_dense_kernel (ratio 8 / 16 / 32, 32 taps per phase, CF32 / S32): the linear-image form
    int multi_waves;       // waves per workgroup of the multi kernel
    int multi_ps;          // lanes that share the 32 tap rows of one output (2 or 4) in the multi kernel
    int occ_multi;         // resident workgroups per CU of the multi kernel
    bool tile_dbuf;        // double-buffered LDS-DMA variant of the tile kernel
    int occ_sb, occ_db;    // resident waves per CU of the two tile-kernel variants
    int oversub;           // waves launched = CUs * occupancy * oversub
    void *stamps_dev;      // diagnostic clock stamps (ABLATE 11/12 only)
    size_t stamps_n;
    float thr2;            // S32 interpolator: transmitter-keying threshold (squared magnitude)
    int sgpr_r;            // experiment: SGPR-tap variant with R outputs per lane (0 = off)
    int sched;             // tile schedule of the tile kernel (0 strided passes, 1 contiguous runs)
    int ablate;            // profiling only: 1 = memory side alone, 2 = compute side alone
    int lds_pad;           // profiling only: extra dynamic LDS bytes per workgroup of a tile2 variant (caps the waves per CU)
    int t2_wpg, t2_opt;    // profiling only: decim4_tile2_kernel variant (waves per workgroup, T2_* bits); wpg 0 = off
    bool pair;             // decim4_pair_kernel: the two tap halves on the two waves of a workgroup
    bool pair_xsep;        // ... with a separate exchange buffer (two barriers per tile instead of four)
    int occ_pair;          // its resident workgroups per CU
    bool wide8;            // product: /4 with 128 symmetric taps runs decim4_wide_kernel (8 outputs per lane, 512-output tiles)
    bool wide;             // (profiling) a non-default build of decim4_wide_kernel was asked for ("wide<nb>", "wident<nb>")
    int wide_nb;           // (profiling) its LDS read-ahead depth: 0 = default
    bool wide_nt;          // (profiling) "wident...": with non-temporal staging loads
    bool wide_pin;         // (profiling) "widentp...": and the FMA issue order pinned (volatile asm)
    int wide_pol;          // (profiling) SXFIR_WIDE_POL: cache policy of its nt loads (low byte) and stores (next byte)
    int occ_wide;
    int compute_units;
    float *taps_dev;
    float *taps_scaled_dev;   // the second tap table; its layout is one of TapTable, chosen from dense_subset / ipass in sxfir_create
    int tap_table;            // TAPS_SCALED: taps * 2^-31 (exact) in tap order, for the /4 scalar-tap kernels on S32 wire words;
                              // TAPS_SUBSET8: the subset-major table of decim_dense_kernel<8, ..., SUBSET> (times 2^-31 for S32 plans);
                              // TAPS_PASS8: the pass-major table of interp8_pass_kernel (pass (c, p) at 64 (2c + p), (jj, rr) at 4 jj + rr).
                              // TAPS_PHASED: the phase-major table of synthesis4_kernel and synthesis4x2_kernel (h[ratio j + r] at
                              // (ntaps / ratio) r + j: four phases, or the two output parities of the oversampled plan).
                              // Every launch that hands taps_scaled_dev to a kernel checks this first (need_tap_table).
    bool ipass;               // x8, 256 taps, CF32: interp8_pass_kernel (scalar taps, four passes per tile)
    int occ_ipass;
    int ipass_qi;             // inputs per lane of that kernel (2; profiling: 4)
    bool ipass_wait0;         // (profiling) SXFIR_IPASS_WAIT0=1: its vmcnt(0) form (A/B partner of the counted wait)
    float taps_k[64];         // the first 64 taps (times 2^-31 for S32 plans) for kernels that take them by value
    bool symmetric;           // taps[k] == taps[ntaps-1-k] bit for bit (every linear-phase design)
    bool ext_tiled;           // the other kinds: the shape their tiled kernel takes (decim4_cx_kernel: /4, 128 taps, CF32; chan4_kernel,
                              // chan4x2_kernel, synthesis4_kernel and synthesis4x2_kernel: 4 bands x 128 taps, CF32)
    int occ_ext;              // its resident waves per CU
    void *hist_dev;        // current history: nchan * hist_len samples
    void *hist_alt;        // the tile kernel writes the next history here, then the two swap
    KernelTable k;         // the instances this plan launches (null: none in this build for that family)
    const BandForm *form;  // the band kinds: what decim_geom / interp_geom and the launches read of the plan's two kernels; else null
    long long consumed, produced;
};

// ---- The kernel table: for each family ONE function from a shape (mode, ratio, ntaps, fmt, symmetric, cx; for the
// interpolators also the two run-time selectors, keyed and split) to the instance that ships.  This is the only place where
// the product's template argument lists are written.  nullptr: no instance for that shape in the production library (its A/B
// partners are launched by the profiling build's hooks, sxfir_prof_dispatch.inc); launch() refuses a null entry.
//
// Occupancy (sxfir_create) is queried on the entry of a plan's BASE form, which is not always the instance a call launches:
// the walking, non-SPLIT form for /48 and /96; interp_kernel(16, CF32, unkeyed, walking) for every x16 .. x96 plan whatever its
// ratio, format or keying, (8, CF32, ...) for x8 and (4, CF32, ...) for x4; decim4_tile_kernel's CF32 instance for S32 words too.
// The launch geometry of every plan was measured with these figures.
static GenericFn generic_kernel(int mode, int fmt, bool cx)
{
    using namespace sxfir;
    if (cx) {
        if (fmt == SXFIR_CF32) return decim_cx_generic_kernel<CF32>;
        if (fmt == SXFIR_CF16) return decim_cx_generic_kernel<CF16>;
        return decim_cx_generic_kernel<S32, CF32>;
    }
    if (mode == SXFIR_DECIMATE) {
        if (fmt == SXFIR_CF32) return decim_generic_kernel<CF32>;
        if (fmt == SXFIR_CF16) return decim_generic_kernel<CF16>;
        return decim_generic_kernel<S32, CF32>;
    }
    if (fmt == SXFIR_CF32) return interp_generic_kernel<CF32>;
    if (fmt == SXFIR_CF16) return interp_generic_kernel<CF16>;
    return interp_generic_kernel<CF32, S32>;
}

// channelizer plans: four chains and the butterflies per thread
static ChanGenericFn chan_generic_kernel_for(int fmt)
{
    using namespace sxfir;
    if (fmt == SXFIR_CF32) return chan_generic_kernel<CF32>;
    if (fmt == SXFIR_CF16) return chan_generic_kernel<CF16>;
    return chan_generic_kernel<S32, CF32>;
}

// /8, /16, /32 with 32 taps per phase: decim_dense_kernel, non-temporal staging loads for the image rows no other tile reads
// (NTLD = 2: both halos stay plain loads; round 4, profiles/round4h_kbench_both_halos_plain.txt: whole kernel -0.9 % at /32,
// -2.8 % at /8 and /16 against plain loads).  /8 is the scalar-tap SUBSET form; CF16 storage: the typed LDS-DMA front end (HALFIN).
template <int D, bool SUBSET>
static DecimMultiFn dense_kernel_for(int fmt)
{
    if (fmt == SXFIR_CF16) return sxfir::decim_dense_kernel<D, 0, false, 2, SUBSET, false, true>;
    if (fmt == SXFIR_S32) return sxfir::decim_dense_kernel<D, 0, true, 2, SUBSET>;
    return sxfir::decim_dense_kernel<D, 0, false, 2, SUBSET>;
}
static DecimMultiFn dense_kernel(int ratio, int fmt)
{
    return ratio == 8 ? dense_kernel_for<8, true>(fmt) : ratio == 16 ? dense_kernel_for<16, false>(fmt) : ratio == 32 ? dense_kernel_for<32, false>(fmt) : nullptr;
}

// /48, /96: decim_blocks_kernel<NB, S32IN, NTLD, HALFIN, SPLIT, RP>, the lines no other tile reads as non-temporal loads (2-3 %
// less time, profiles/round5_rates.txt), waves by column group (RP, round 6)
template <int NB, bool SPLIT>
static DecimBlocksFn blocks_kernel_for(int fmt)
{
    if (fmt == SXFIR_CF16) return sxfir::decim_blocks_kernel<NB, false, true, true, SPLIT, true>;
    if (fmt == SXFIR_S32) return sxfir::decim_blocks_kernel<NB, true, true, false, SPLIT, true>;
    return sxfir::decim_blocks_kernel<NB, false, true, false, SPLIT, true>;
}
static DecimBlocksFn blocks_kernel(int blocks, int fmt, bool split)
{
    if (blocks == 3) return split ? blocks_kernel_for<3, true>(fmt) : blocks_kernel_for<3, false>(fmt);
    if (blocks == 6) return split ? blocks_kernel_for<6, true>(fmt) : blocks_kernel_for<6, false>(fmt);
    return nullptr;
}

// /4, four outputs per lane: the VGPR-tap form for any 128 or 64 taps
static DecimTileFn tile_kernel(int ntaps, int fmt)
{
    if (fmt == SXFIR_S32) return sxfir::decim4_tile_kernel<128, false, 0, true>;
    if (ntaps == 128) return sxfir::decim4_tile_kernel<128, false>;
    return sxfir::decim4_tile_kernel<64, false>;
}

// /4, 128 taps, eight outputs per lane (sxfir_decim_wide.hip.h): all 64 distinct taps of a bit-symmetric filter (every linear-phase
// design) in SGPR pairs; 18.5 KB of LDS per wave -> 8 waves per CU.  Its ASYM form (round 5: taps 127..64 in SGPR pairs, taps 63..0 in
// VGPR pairs) ships for CF16 storage only, where it beats the multi-column kernel by 3 %; on CF32 and S32 words it measured 1.4 %
// slower / 0.7 % faster than decim4_tile_kernel<128> (profiles/round5_kbench_asym.txt), which therefore keeps the non-symmetric
// 128-tap plans (the instances exist in the profiling build: SXFIR_WIDE_ASYM=1)
static DecimTileFn wide_kernel(int fmt, bool symmetric)
{
    if (!symmetric) return fmt == SXFIR_CF16 ? sxfir::decim4_wide_kernel<0, false, 24, true, false, 0, true, true> : nullptr;
    if (fmt == SXFIR_S32) return sxfir::decim4_wide_kernel<0, true>;
    if (fmt == SXFIR_CF16) return sxfir::decim4_wide_kernel<0, false, 24, true, false, 0, true>;
    return sxfir::decim4_wide_kernel<0, false>;
}

// Interpolators with 32 taps per phase.  CF32 / S32 words: interp8_pass_kernel<QI, KEYED, S32OUT, COUNTED, LL, LT, PBSPLIT> -- x4
// with four inputs per lane and two passes, x8 with two inputs per lane and four passes, x16 .. x96 over ratio / 16 phase blocks of
// sixteen per tile, walked or (x32, x48, x96: split) dealt.  CF16 storage: interp_tile_kernel with the typed LDS-DMA front end and
// half stores, x48 / x96 as three phase blocks of its x16 / x32 form; the keying count is defined on CF32 input.
template <bool KEYED, bool S32OUT>
static InterpTileFn interp_pass_kernel_for(int ratio, bool split)
{
    using namespace sxfir;
    switch (ratio + (split ? 1000 : 0)) {
    case 4: return interp8_pass_kernel<4, KEYED, S32OUT, true, 4>;
    case 8: return interp8_pass_kernel<2, KEYED, S32OUT>;
    case 16: return interp8_pass_kernel<2, KEYED, S32OUT, true, 16, 16>;
    case 32: return interp8_pass_kernel<2, KEYED, S32OUT, true, 16, 32>;
    case 48: return interp8_pass_kernel<2, KEYED, S32OUT, true, 16, 48>;
    case 96: return interp8_pass_kernel<2, KEYED, S32OUT, true, 16, 96>;
    case 1032: return interp8_pass_kernel<2, KEYED, S32OUT, true, 16, 32, true>;
    case 1048: return interp8_pass_kernel<2, KEYED, S32OUT, true, 16, 48, true>;
    case 1096: return interp8_pass_kernel<2, KEYED, S32OUT, true, 16, 96, true>;
    }
    return nullptr;
}
static InterpTileFn interp_kernel(int ratio, int fmt, bool keyed, bool split)
{
    using namespace sxfir;
    if (fmt == SXFIR_S32) return keyed ? interp_pass_kernel_for<true, true>(ratio, split) : interp_pass_kernel_for<false, true>(ratio, split);
    if (fmt == SXFIR_CF32) return keyed ? interp_pass_kernel_for<true, false>(ratio, split) : interp_pass_kernel_for<false, false>(ratio, split);
    if (keyed || split) return nullptr;
    switch (ratio) {
    case 4: return interp_tile_kernel<4, false, false, 4, true>;
    case 8: return interp_tile_kernel<8, false, false, 8, true>;
    case 16: return interp_tile_kernel<16, false, false, 16, true>;
    case 32: return interp_tile_kernel<32, false, false, 32, true>;
    case 48: return interp_tile_kernel<16, false, false, 48, true>;
    case 96: return interp_tile_kernel<32, false, false, 96, true>;
    }
    return nullptr;
}

// 2x oversampled channelizer plans: four chains and the butterflies of the output's parity per thread
static ChanOsGenericFn chan4x2_generic_kernel_for(int fmt)
{
    using namespace sxfir;
    if (fmt == SXFIR_CF32) return chan4x2_generic_kernel<CF32>;
    if (fmt == SXFIR_CF16) return chan4x2_generic_kernel<CF16>;
    return chan4x2_generic_kernel<S32, CF32>;
}

// synthesizer plans: the butterflies once per input index, four phase chains per thread
static SynGenericFn synthesis_generic_kernel_for(int fmt)
{
    using namespace sxfir;
    if (fmt == SXFIR_CF32) return synthesis_generic_kernel<CF32>;
    if (fmt == SXFIR_CF16) return synthesis_generic_kernel<CF16>;
    return synthesis_generic_kernel<CF32, S32>;
}

// 2x oversampled synthesizer plans: the two DFT outputs an input index needs, two chains per thread
static SynOsGenericFn synthesis_os_generic_kernel_for(int fmt)
{
    using namespace sxfir;
    if (fmt == SXFIR_CF32) return synthesis_os_generic_kernel<CF32>;
    if (fmt == SXFIR_CF16) return synthesis_os_generic_kernel<CF16>;
    return synthesis_os_generic_kernel<CF32, S32>;
}

// The four band forms, [synthesizer][oversampled].  chan4_kernel: tiles of 512 outputs per band.  chan4x2_kernel (ratio 2): 1024
// outputs per band = 2048 inputs; its lane map needs the call's first output to have an EVEN index, i.e. a stream position that is
// a multiple of 4 (every position of the /2 raster starts on an output).  synthesis4_kernel: 256 inputs per band on the x4 pass
// kernel's frame.  synthesis4x2_kernel: any per-band start index -- the start's parity is its argument.
static const BandForm BAND_FORMS[2][2] = {
    {{"chan4_kernel", "chan_generic_kernel", GEOM_CHAN4, 512, 1}, {"chan4x2_kernel", "chan4x2_generic_kernel", GEOM_CHAN4X2, 1024, 4}},
    {{"synthesis4_kernel", "synthesis_generic_kernel", GEOM_SYN4, 256, 1},
     {"synthesis4x2_kernel", "synthesis_os_generic_kernel", GEOM_SYN4X2, sxfir::Syn4x2::TILE_IN, 1}}};

// The plan's kernels, from its kind and the capability flags its creator has settled (the profiling knobs included)
static void resolve_kernels(sxfir_plan *p)
{
    KernelTable &k = p->k;
    k = KernelTable{};
    p->form = nullptr;
    if (p->kind == KIND_CHANNELIZER || p->kind == KIND_SYNTHESIZER) {
        p->form = &BAND_FORMS[p->kind == KIND_SYNTHESIZER][p->oversample == 2];
        switch (p->form->geom) {            // every band plan has its form's generic kernel INSTEAD of `generic`
        case GEOM_CHAN4:
            k.chan_generic = chan_generic_kernel_for(p->fmt);
            if (p->ext_tiled) k.chan4 = sxfir::chan4_kernel;
            break;
        case GEOM_CHAN4X2:
            k.chan4x2_generic = chan4x2_generic_kernel_for(p->fmt);
            if (p->ext_tiled) k.chan4x2 = sxfir::chan4x2_kernel;
            break;
        case GEOM_SYN4:
            k.syn_generic = synthesis_generic_kernel_for(p->fmt);
            if (p->ext_tiled) k.syn4 = sxfir::synthesis4_kernel;
            break;
        case GEOM_SYN4X2:
            k.syn4x2_generic = synthesis_os_generic_kernel_for(p->fmt);
            if (p->ext_tiled) k.syn4x2 = sxfir::synthesis4x2_kernel;
            break;
        }
        return;
    }
    k.generic = generic_kernel(p->mode, p->fmt, p->kind == KIND_COMPLEX);
    if (p->ext_tiled) k.cx = sxfir::decim4_cx_kernel;
    if (p->dense32) k.dense = dense_kernel(p->ratio, p->fmt);
    for (int split = 0; split < 2; ++split) k.blocks[split] = blocks_kernel(p->blocks, p->fmt, split != 0);
    if (p->tile_capable) k.tile = tile_kernel(p->ntaps, p->fmt);
    if (p->tile_capable && p->ntaps == 128) k.wide = wide_kernel(p->fmt, p->symmetric);
    if (p->itile_capable)
        for (int keyed = 0; keyed < 2; ++keyed)
            for (int split = 0; split < 2; ++split) k.interp[keyed][split] = interp_kernel(p->ratio, p->fmt, keyed != 0, split != 0);
}

// resident workgroups per CU of a kernel; *occ keeps its default where the runtime has no answer
template <typename Fn>
static void query_occupancy(int *occ, Fn kernel, int threads, size_t dynamic_lds = 0)
{
    int nb = 0;
    if (kernel && hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kernel, threads, dynamic_lds) == hipSuccess && nb > 0) *occ = nb;
}

// ---- The creation frame.  A creator is: check_create_args, its own refusals, new_plan, its own fields and tap layout,
// resolve_kernels and the occupancy of its tiled kernel, plan_to_device.  Every argument error comes before the device is looked at.

// `ratio_name`: what the caller calls it ("ratio", "nbands")
static int check_create_args(sxfir_plan **out, const float *taps, int mode, int ntaps, const char *ratio_name, int ratio, int nchan, int fmt)
{
    if (!out || !taps) return fail(SXFIR_EINVAL, "NULL argument");
    *out = nullptr;
    if (mode != SXFIR_DECIMATE && mode != SXFIR_INTERPOLATE) return fail(SXFIR_EINVAL, "bad mode %d", mode);
    if (ntaps < 1 || ntaps > 65536) return fail(SXFIR_EINVAL, "ntaps %d out of range", ntaps);
    if (ratio < 1 || ratio > 4096) return fail(SXFIR_EINVAL, "%s %d out of range", ratio_name, ratio);
    if (nchan < 1 || nchan > 65535) return fail(SXFIR_EINVAL, "nchan %d out of range", nchan);
    if (fmt != SXFIR_CF32 && fmt != SXFIR_CF16 && fmt != SXFIR_S32) return fail(SXFIR_EINVAL, "bad format %d", fmt);
    return SXFIR_OK;
}

// *device < 0: the current one.  Makes it current and hands back its properties; only gfx950 passes.
static int open_device(int *device, hipDeviceProp_t *prop)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(SXFIR_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (*device < 0) HIPCHECK(hipGetDevice(device));
    if (*device >= ndev) return fail(SXFIR_EINVAL, "device %d of %d", *device, ndev);
    HIPCHECK(hipSetDevice(*device));
    HIPCHECK(hipGetDeviceProperties(prop, *device));
    if (strncmp(prop->gcnArchName, "gfx950", 6) != 0)
        return fail(SXFIR_ENODEVICE, "device %d is %s; kernels are built for gfx950 only", *device, prop->gcnArchName);
    return SXFIR_OK;
}

// A plan on `device` with what every kind sets; everything else is zero (value-initialised: no kernel family is enabled, no
// pointer, counter or knob is set)
static int new_plan(sxfir_plan **pp, int kind, int mode, int ntaps, int ratio, int nchan, int fmt, int device)
{
    hipDeviceProp_t prop;
    if (int rc = open_device(&device, &prop)) return rc;
    sxfir_plan *p = new (std::nothrow) sxfir_plan();
    if (!p) return fail(SXFIR_ENOMEM, "out of host memory");
    p->kind = kind;
    p->mode = mode;
    p->ntaps = ntaps;
    p->ratio = ratio;
    p->nchan = nchan;
    p->fmt = fmt;
    p->device = device;
    p->bands = kind == KIND_CHANNELIZER || kind == KIND_SYNTHESIZER ? ratio : 0;
    p->oversample = kind == KIND_CHANNELIZER || kind == KIND_SYNTHESIZER ? 1 : 0;
    p->kernel = SXFIR_KERNEL_AUTO;
    p->compute_units = prop.multiProcessorCount;
    p->thr2 = 1.0e-3f * 1.0e-3f;
    p->oversub = 16;
    p->occ_ext = 8;
#ifdef SXFIR_PROFILING
    p->join_drop = -1;
#endif
    *pp = p;
    return SXFIR_OK;
}

// The numeric contract of a real-tap plan of (mode, ntaps, ratio).  Decimators: two row halves and column groups of 4
// when the shape allows the adjacent-pair trees, i.e. whole, even rows and a power-of-two number (<= 32) of column groups;
// otherwise one chain over all taps.  /48 and /96 with 32 taps per phase (the reference's rates master clock / 768 and / 1536,
// SoapySX.cpp:180-208) run decim_blocks_kernel, sixteen-column blocks of whole input lines under the ROTATED contract (slot k'
// holds tap (k' + 1) mod ntaps: sxfir_contract_rotation); 12 / 24 column groups meet in the adjacent-pair tree whose odd element
// at the end of a level moves up unchanged (oracle B and the generic kernel state the same tree and rotation).  Interpolators:
// a phase's taps in two halves when their count is even.
static void real_tap_contract(sxfir_plan *p)
{
    const int ntaps = p->ntaps, ratio = p->ratio;
    p->rot = 0;
    if (p->mode == SXFIR_INTERPOLATE) {
        p->jsplit = ((ntaps / ratio) % 2 == 0) ? 2 : 1;
        p->cw = 1;
        return;
    }
    const int jt = (ntaps + ratio - 1) / ratio;
    const int ncol4 = ratio / 4;
    const bool pow2_cols = ratio % 4 == 0 && (ncol4 & (ncol4 - 1)) == 0 && ncol4 <= 32;
    const bool blocks = ntaps == 32 * ratio && (ratio == 48 || ratio == 96);
    p->rot = blocks ? 1 : 0;
    if (ntaps % ratio == 0 && (pow2_cols || blocks) && jt % 2 == 0) {
        p->jsplit = 2;
        p->cw = 4;
    } else {
        p->jsplit = 1;
        p->cw = ratio;
    }
}

// The one list of what a plan owns
static void free_plan(sxfir_plan *p)
{
    (void)hipFree(p->taps_dev);
    (void)hipFree(p->taps_scaled_dev);
    (void)hipFree(p->hist_dev);
    (void)hipFree(p->hist_alt);
    (void)hipFree(p->join_partials);
    (void)hipFree(p->join_arrived);
#ifdef SXFIR_PROFILING
    (void)hipFree(p->join_shadow);
#endif
    (void)hipFree(p->stamps_dev);          // the profiling build's clock stamps; null in the product
    delete p;
}

static hipError_t upload(float **dev, const float *host, size_t n)
{
    const hipError_t e = hipMalloc((void **)dev, sizeof(float) * n);
    return e != hipSuccess ? e : hipMemcpy(*dev, host, sizeof(float) * n, hipMemcpyHostToDevice);
}

// The plan's device memory: the tap table (`taps`: ntaps floats; `second`: p->ntaps floats for taps_scaled_dev too, in the layout
// p->tap_table names), the two history buffers, the current one zeroed, and for /48 and /96 the join scratch.  The last step of
// every creator: *out is the plan, or the plan is freed.
static int plan_to_device(sxfir_plan **out, sxfir_plan *p, const float *taps, size_t ntaps, const float *second)
{
    const size_t hist_bytes = sample_bytes(p->fmt) * (size_t)p->hist_len * (size_t)p->nchan;
    hipError_t e = upload(&p->taps_dev, taps, ntaps);
    if (e == hipSuccess && second) e = upload(&p->taps_scaled_dev, second, (size_t)p->ntaps);
    if (e == hipSuccess) e = hipMalloc(&p->hist_dev, hist_bytes);
    if (e == hipSuccess) e = hipMalloc(&p->hist_alt, hist_bytes);
    if (e == hipSuccess) e = hipMemset(p->hist_dev, 0, hist_bytes);
    if (e == hipSuccess && p->blocks) {
        e = hipMalloc(&p->join_partials, (size_t)p->join_tiles * (size_t)p->blocks * 4096);
        if (e == hipSuccess) e = hipMalloc((void **)&p->join_arrived, sizeof(unsigned) * (size_t)p->join_tiles);
        if (e == hipSuccess) e = hipMemset(p->join_arrived, 0, sizeof(unsigned) * (size_t)p->join_tiles);
#ifdef SXFIR_PROFILING
        if (e == hipSuccess && p->join_drop >= 0) e = hipMalloc(&p->join_shadow, (size_t)p->join_tiles * 4096);
#endif
    }
    if (e != hipSuccess) {
        free_plan(p);
        return fail(SXFIR_EHIP, "plan allocation failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return SXFIR_OK;
}

// The one creation path of the four band plans (sxfir_create_channelizer, sxfir_create_synthesizer and their _os forms, in
// their own headers): `kind` KIND_CHANNELIZER or KIND_SYNTHESIZER, `what` the creator's name for its plan in the refusals
// ("channelizer", "oversampled channelizer", ...), `oversample` 1 or 2 once an _os creator's own checks are through.  The plan is a
// /ratio decimator or a x ratio interpolator, ratio = nbands / oversample, in everything about the stream.
static int create_band_plan(sxfir_plan **out, int kind, const char *what, const float *taps, int ntaps, int nbands, int oversample,
                            int nchan, int fmt, int device)
{
    const bool syn = kind == KIND_SYNTHESIZER;
    const char *word = syn ? "synthesizer" : "channelizer";
    const int mode = syn ? SXFIR_INTERPOLATE : SXFIR_DECIMATE;
    if (int rc = check_create_args(out, taps, mode, ntaps, "nbands", nbands, nchan, fmt)) return rc;
    if (nbands != 4)
        return fail(SXFIR_EUNSUPPORTED, "%s: 4 bands only (the twiddles of %d bands are not exact: no rounding rule for them)", what, nbands);
    if (ntaps % nbands) return fail(SXFIR_EINVAL, "%s needs ntaps %% nbands == 0 (%d, %d)", word, ntaps, nbands);
    const int ratio = nbands / oversample;
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, kind, mode, ntaps, ratio, nchan, fmt, device)) return rc;
    p->bands = nbands;
    p->oversample = oversample;
    p->ext_tiled = fmt == SXFIR_CF32 && ntaps == 128;
    const int jt = ntaps / ratio;                           // a synthesizer's taps per phase (oversampled: per output parity)
    std::vector<float> phased(syn ? (size_t)ntaps : 0);     // a synthesizer's second tap table
    if (syn) {
        p->hist_len = nbands * ((jt + 1) & ~1);             // per channel: a x ratio interpolator's history for every band, band k's at k * hist_len / 4
        real_tap_contract(p);                               // a phase's sum: the real-tap interpolator's
        // the phase-major table of the tiled kernels: h[ratio j + r] at jt r + j
        p->tap_table = TAPS_PHASED;
        for (int r = 0; r < ratio; ++r)
            for (int j = 0; j < jt; ++j) phased[(size_t)(jt * r + j)] = taps[ratio * j + r];
    } else {
        p->hist_len = ntaps;                                // (a multiple of 4)
        // the numeric contract of a branch sum: one chain per phase, no tree, no rotation
        p->jsplit = 1;
        p->cw = 1;
    }
    resolve_kernels(p);
    if (p->form->geom == GEOM_SYN4X2) p->occ_ext = 5;       // (where the runtime has no answer; its answer replaces it)
    const KernelTable &k = p->k;                            // the form's tiled kernel: at most one of the four is set
    query_occupancy(&p->occ_ext, k.chan4 ? (const void *)k.chan4 : k.chan4x2 ? (const void *)k.chan4x2 : k.syn4 ? (const void *)k.syn4 : (const void *)k.syn4x2, 64);
    return plan_to_device(out, p, taps, (size_t)ntaps, syn ? phased.data() : nullptr);
}

// The _os creators' own argument, checked behind check_create_args and in front of create_band_plan: its range, and the two values
// version 1 does not take (`word`: "channelizer" / "synthesizer").  A band count that create_band_plan refuses is left to it: that
// refusal has always come in front of the two here.
static int check_oversample(const char *word, int nbands, int oversample)
{
    if (oversample < 1 || oversample > 4096) return fail(SXFIR_EINVAL, "oversample %d out of range", oversample);
    if (nbands != 4) return SXFIR_OK;
    if (oversample == 1)
        return fail(SXFIR_EUNSUPPORTED, "oversample 1 is the critically sampled %s: sxfir_create_%s (include/sxfir_%s.h)", word, word, word);
    if (oversample != 2) return fail(SXFIR_EUNSUPPORTED, "oversampled %s: oversample 2 only (%d asked for)", word, oversample);
    return SXFIR_OK;
}

extern "C" {

int sxfir_abi_version(void) { return SXFIR_ABI_VERSION; }

const char *sxfir_last_error(void) { return g_err; }

int sxfir_device_count(int *count)
{
    if (!count) return fail(SXFIR_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(SXFIR_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return SXFIR_OK;
}

int sxfir_device_info(int device, char *name, char *arch, int *compute_units, size_t *hbm_bytes)
{
    hipDeviceProp_t p;
    HIPCHECK(hipGetDeviceProperties(&p, device));
    if (name) snprintf(name, 64, "%s", p.name);
    if (arch) {
        snprintf(arch, 32, "%s", p.gcnArchName);
        char *colon = strchr(arch, ':');
        if (colon) *colon = 0;
    }
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
    return SXFIR_OK;
}

int sxfir_device_pci_bus_id(int device, char *bdf, size_t bdf_bytes)
{
    if (!bdf || bdf_bytes < 16) return fail(SXFIR_EINVAL, "bdf needs at least 16 bytes");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(SXFIR_ENODEVICE, "no GPU visible");
    if (device < 0) HIPCHECK(hipGetDevice(&device));
    if (device >= n) return fail(SXFIR_EINVAL, "device %d of %d", device, n);
    HIPCHECK(hipDeviceGetPCIBusId(bdf, (int)bdf_bytes, device));
    return SXFIR_OK;
}

int sxfir_create(sxfir_plan **out, int mode, const float *taps, int ntaps, int ratio, int nchan, int fmt,
                 int device)
{
    if (int rc = check_create_args(out, taps, mode, ntaps, "ratio", ratio, nchan, fmt)) return rc;
    if (mode == SXFIR_INTERPOLATE && ntaps % ratio)
        return fail(SXFIR_EINVAL, "interpolator needs ntaps %% ratio == 0 (%d, %d)", ntaps, ratio);
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, KIND_REAL, mode, ntaps, ratio, nchan, fmt, device)) return rc;
    p->occ_ipass = 16;
    p->ipass_qi = 2;
    p->symmetric = true;
    for (int k = 0; k < ntaps / 2; ++k)
        if (memcmp(&taps[k], &taps[ntaps - 1 - k], sizeof(float)) != 0) p->symmetric = false;
    p->blocks_split = true;
    p->ipass_split = true;
    real_tap_contract(p);

    if (mode == SXFIR_DECIMATE) {
        p->hist_len = (ntaps + 1) & ~1;
        // CF16 storage at /4 with 128 taps: the wide kernel with the typed-DMA front end (round 5)
        const bool half4_wide = fmt == SXFIR_CF16 && ratio == 4 && ntaps == 128;
        p->tile_capable = ((fmt == SXFIR_CF32 && ratio == 4 && (ntaps == 128 || ntaps == 64)) ||
                           (fmt == SXFIR_S32 && ratio == 4 && ntaps == 128) || half4_wide);
        // multi-column kernel: 32 taps per phase; CF32 at ratio 8/16/32, CF16 at ratio 4/8/16/32
        p->multi_capable = (ntaps == 32 * ratio) && !half4_wide &&
                           (((fmt == SXFIR_CF32 || fmt == SXFIR_S32) && (ratio == 8 || ratio == 16 || ratio == 32)) ||
                            (fmt == SXFIR_CF16 && (ratio == 4 || ratio == 8 || ratio == 16 || ratio == 32)));
        // /48 and /96 with 32 taps per phase (the rotated contract): decim_blocks_kernel on CF32, S32 words and CF16 storage
        p->blocks = p->rot ? ratio / 16 : 0;
#ifdef SXFIR_PROFILING
        // experiment (round 6): /16 and /32 CF32 through the sixteen-column-block form too (one / two blocks per row, scalar taps,
        // the ROTATED contract, or with SXFIR_BLOCKS_SMALL=2 the unrotated one): would config 5's shape gain what /48 and /96
        // gained over the VGPR-tap dense kernel?
        if (getenv("SXFIR_BLOCKS_SMALL") && atoi(getenv("SXFIR_BLOCKS_SMALL")) && fmt == SXFIR_CF32 && ntaps == 32 * ratio &&
            (ratio == 16 || ratio == 32)) {
            p->blocks = ratio / 16;
            p->blocks_split = false;
            p->rot = atoi(getenv("SXFIR_BLOCKS_SMALL")) == 2 ? 0 : 1;
        }
#endif
        if (p->blocks) p->multi_capable = true;
    } else {
        p->hist_len = (ntaps / ratio + 1) & ~1;
        // (x48, x96 -- the reference's rates master clock / 768 and / 1536 -- as three / six phase blocks of the x16 kernel)
        // (CF16 storage, round 5: interp_tile_kernel<.., HALF> at every one of these ratios)
        p->itile_capable = ((fmt == SXFIR_CF32 || fmt == SXFIR_S32 || fmt == SXFIR_CF16) && ntaps == 32 * ratio &&
                            (ratio == 4 || ratio == 8 || ratio == 16 || ratio == 32 || ratio == 48 || ratio == 96));
    }

    // measured on MI355X (tools/kbench.py): single-buffered LDS-DMA at 16 waves/CU, 16 generations
    // of short-lived waves (4 tiles each at 2^28 samples), strided XCD-blocked passes; the
    // double-buffered variant at 8 waves/CU and long contiguous runs are slower
    p->occ_sb = p->occ_db = 8;
    // waves per workgroup of the multi-column kernel, measured (tools/kbench.py, KB_D, specs "w1".."w8"):
    // the choice that brings the LDS image down to 10 KiB per wave (16 waves per CU) while the 31-row
    // halo stays a small part of the staging
    p->multi_waves = ratio <= 4 ? 1 : 4;
    p->multi_ps = 2;
    // CF32 / S32 words at ratio 8, 16, 32: the linear-image form (sxfir_decim_dense.hip.h); CF16 and ratio 4 keep
    // the multi-column kernel
    // ... and, since round 5, CF16 storage at /32 (BASELINE config 5's fp16 leg): the dense kernel with the typed LDS-DMA front end
    // (HALFIN: the texture path converts half -> float on the way into the same CF32 image; no conversions in the FIR)
    p->dense32 = p->multi_capable && !p->blocks && (ratio == 8 || ratio == 16 || ratio == 32);
    // /8 CF32: the scalar-tap form of the dense kernel (tap subsets on the four waves, round 4: 4.4-5 % less time)
    p->dense_subset = p->dense32 && ratio == 8;      // (CF16 storage too, round 5: the typed-DMA front end under the same scalar-tap FIR)
    p->occ_pair = 8;
    p->occ_wide = 8;
    p->occ_multi = 2;
    // generations of workgroups per launch, measured (tools/kbench.py): the multi-column kernel's prologue
    // (64 taps and the DMA offset table per lane) is heavier than the tile kernel's, 8 beats 16; the
    // interpolator is flat between 2 and 16 (tools/ibench.py)
    if (p->multi_capable) p->oversub = 8;
    if (p->itile_capable) p->oversub = ratio > 32 ? 2 : 4;     // (x48, x96: 2 measured 1-2 % ahead of 4 .. 32, profiles/round5_rates.txt)
    // CF32 / S32 words: the scalar-tap pass kernel (interp8_pass_kernel) at every ratio -- x8 (two inputs per lane, four passes per
    // tile; 4 / 8 / 16 generations measured within 0.3 %, tools/ibench2.py), x4 (round 5: four inputs per lane, two passes) and
    // x16 .. x96 (round 5: ratio / 16 phase blocks of sixteen per tile, a lane's sixteen outputs per input and block are one line:
    // 8-9 % less time than interp_tile_kernel, which keeps CF16 storage, profiles/round5_rates.txt)
    if (p->itile_capable && fmt != SXFIR_CF16) {
        p->ipass = true;
        p->ipass_qi = ratio == 4 ? 4 : 2;
        p->oversub = 8;
        query_occupancy(&p->occ_ipass, interp_kernel(ratio < 16 ? ratio : 16, SXFIR_CF32, false, false), 64);
    }
#ifdef SXFIR_PROFILING
    // A/B knobs of the profiling build.  The production library never looks at the environment.
    if (const char *v = getenv("SXFIR_TILE_VARIANT")) {
        if (strcmp(v, "mu") == 0 && mode == SXFIR_DECIMATE && fmt == SXFIR_CF32 && ratio == 4 && ntaps == 128) {
            p->multi_capable = true;        // the multi-column kernel at D = 4 instead of decim4_tile_kernel
            p->tile_capable = false;
            p->oversub = 8;
        }
    }
    if (const char *v = getenv("SXFIR_DENSE")) p->dense32 = p->dense32 && atoi(v) != 0;
    if (const char *v = getenv("SXFIR_IPASS")) {     // 0: interp_tile_kernel at x8 too (A/B); 4: four inputs per lane
        p->ipass = p->ipass && atoi(v) != 0;
        if (p->ipass && atoi(v) == 4 && ratio == 8) {
            p->ipass_qi = 4;
            query_occupancy(&p->occ_ipass, sxfir::interp8_pass_kernel<4>, 64);
        }
    }
    if (const char *v = getenv("SXFIR_IPASS_WAIT0")) p->ipass_wait0 = atoi(v) != 0;
    if (const char *v = getenv("SXFIR_IPASS_SPLIT")) p->ipass_split = atoi(v) != 0;
    if (const char *v = getenv("SXFIR_DENSE_NT")) { p->dense_nt = atoi(v); p->dense_nt_set = 1; }
    if (const char *v = getenv("SXFIR_DENSE_HC")) p->dense_hc = atoi(v) != 0;
    if (const char *v = getenv("SXFIR_DENSE_SUBSET")) p->dense_subset = p->dense_subset && atoi(v) != 0;     // 0: the VGPR-tap form (A/B)
    if (!p->dense32) p->dense_subset = false;
    if (getenv("SXFIR_MULTI_PS") || getenv("SXFIR_MULTI_W")) p->dense32 = false;   // those knobs belong to the multi-column kernel
    if (p->multi_capable && fmt != SXFIR_S32 && !p->dense32) {
        if (const char *v = getenv("SXFIR_MULTI_PS")) p->multi_ps = atoi(v) == 4 ? 4 : 2;
        if (p->multi_ps == 4) p->multi_waves = ratio <= 4 ? 2 : (ratio == 8 ? 4 : 8);
        if (const char *v = getenv("SXFIR_MULTI_W")) p->multi_waves = atoi(v);
        p->jsplit = p->multi_ps;
    }
    if (p->multi_capable || p->itile_capable || p->tile_capable) {
        if (const char *v = getenv("SXFIR_OVERSUB")) p->oversub = atoi(v) > 0 ? atoi(v) : 1;
    }
    if (p->multi_capable || p->tile_capable) {
        if (const char *v = getenv("SXFIR_ABLATE")) p->ablate = atoi(v);
    }
#endif
    resolve_kernels(p);
    if (p->multi_capable) {
        // resident workgroups per CU: LDS is the limiter (checked against the occupancy API below)
        const int W = p->multi_waves;
        const void *k = p->blocks ? (const void *)p->k.blocks[0] : (const void *)p->k.dense;
#ifdef SXFIR_PROFILING
        if (p->blocks && p->blocks < 3) {       // (the unrotated instances have the same resources)
            k = p->blocks == 1 ? (const void *)sxfir::decim_blocks_kernel<1, false, true, false, false, true> : (const void *)sxfir::decim_blocks_kernel<2, false, true, false, false, true>;
        } else if (!p->blocks && !p->dense32 && fmt == SXFIR_S32) {   // wire-word input: one instantiation per ratio (4 waves, 2-way row split)
            k = ratio == 8    ? (const void *)sxfir::decim_multi_kernel<8, 4, false, 0, 2, true>
                : ratio == 16 ? (const void *)sxfir::decim_multi_kernel<16, 4, false, 0, 2, true>
                              : (const void *)sxfir::decim_multi_kernel<32, 4, false, 0, 2, true>;
        } else if (!p->blocks && !p->dense32) {
            switch (SXFIR_MULTI_KEY(ratio, W, fmt == SXFIR_CF16, p->multi_ps)) {
#define SXFIR_X(DD, WW, HH, PP) \
            case SXFIR_MULTI_KEY(DD, WW, HH, PP): k = (const void *)sxfir::decim_multi_kernel<DD, WW, HH, 0, PP>; break;
                SXFIR_MULTI_VARIANTS(SXFIR_X)
#undef SXFIR_X
            }
        }
#endif
        if (!k) {
            free_plan(p);
            return fail(SXFIR_EUNSUPPORTED, "no multi-column kernel for ratio %d with %d waves per workgroup", ratio, W);
        }
        query_occupancy(&p->occ_multi, k, 64 * W);
    }
    if (p->blocks) {
        // calls of at most eight times as many tiles as the chip has workgroup slots are dealt as (tile, block) items (SPLIT).
        // Measured (tools/split_ab.sh, profiles/round6_split_ab.txt): against the walking form the dealt form takes 2.9 x less time at
        // 2^22 samples (/96), -39 % at 2^24, -15 % at 2^26 (2731 / 1366 tiles), -6 % at 5.3 x slots and +2 .. +5 % at 10.7 x slots
        // (2^28 samples at /96: the walking form keeps a tile's halo in one XCD's L2 and pays one prologue per eight tiles).
        // Scratch: 4096 tiles x blocks x 4 KiB = 48 / 96 MiB per plan.
        p->join_tiles = 8LL * p->compute_units * p->occ_multi;
#ifdef SXFIR_PROFILING
        if (const char *v = getenv("SXFIR_BLOCKS_SPLIT")) {     // 0: off; n >= 1: dealt while a call has at most n x slots tiles
            p->blocks_split = atoi(v) != 0;
            if (atoi(v) > 1) p->join_tiles = (long long)atoi(v) * p->compute_units * p->occ_multi;
        }
        // test hook: a hand-off that never arrives (tests/test_gpu_join.py proves with it that its checker sees one)
        if (const char *v = getenv("SXFIR_BLOCKS_JOIN_DROP")) p->join_drop = (atoi(v) >= 0 && atoi(v) < p->blocks) ? atoi(v) : -1;
#endif
    }
    if (p->tile_capable) {
        // the 4-outputs-per-lane kernels (the CF32 instance's figure: see the kernel table) -- and, in the profiling build, round 3's
        // scalar-tap form for 128 symmetric taps ("t2s"), the A/B partner of the wide kernel that replaced it
        const void *ksb = (const void *)tile_kernel(ntaps, SXFIR_CF32);
#ifdef SXFIR_PROFILING
        if (ntaps == 128 && p->symmetric)
            ksb = fmt == SXFIR_S32 ? (const void *)sxfir::decim4_tile2_kernel<128, 1, sxfir::T2_SHIPPED, 0, true>
                                   : (const void *)sxfir::decim4_tile2_kernel<128, 1, sxfir::T2_SHIPPED>;
#endif
        query_occupancy(&p->occ_sb, ksb, 64);
        // 128 taps: the wide kernel, for bit-symmetric taps and (its ASYM form) for CF16 storage
        p->wide8 = p->k.wide != nullptr;
        query_occupancy(&p->occ_wide, p->k.wide, 64);
#ifdef SXFIR_PROFILING
        if (!p->k.wide && ntaps == 128 && getenv("SXFIR_WIDE_ASYM") && atoi(getenv("SXFIR_WIDE_ASYM"))) {
            p->wide8 = true;                                   // A/B: the wide kernel's ASYM form on CF32 / S32 words
            p->k.wide = fmt == SXFIR_S32 ? sxfir::decim4_wide_kernel<0, true, 24, true, false, 0, false, true>
                                         : sxfir::decim4_wide_kernel<0, false, 24, true, false, 0, false, true>;
            query_occupancy(&p->occ_wide, p->k.wide, 64);
        }
        if (ntaps == 128) {
            const void *kp = fmt == SXFIR_S32 ? (const void *)sxfir::decim4_pair_kernel<0, true> : (const void *)sxfir::decim4_pair_kernel<0, false>;
            query_occupancy(&p->occ_pair, kp, 128);
        }
        const void *kdb = ntaps == 128 ? (const void *)sxfir::decim4_tile_kernel<128, true>
                                       : (const void *)sxfir::decim4_tile_kernel<64, true>;
        query_occupancy(&p->occ_db, kdb, 64);
        if (const char *v = getenv("SXFIR_TILE_VARIANT")) {
            p->tile_dbuf = (strcmp(v, "db") == 0);
            // "sb", "db", "sg": the first-generation tile kernel (taps in VGPR pairs) also for symmetric taps
            if (strcmp(v, "sb") == 0 || strcmp(v, "db") == 0 || strncmp(v, "sg", 2) == 0) { p->symmetric = false; p->wide8 = false; }
            // "t2s": round 3's shipped form (decim4_tile2_kernel, T2_SHIPPED) as the A/B partner of the wide kernel
            if (strcmp(v, "t2s") == 0) p->wide8 = false;
            p->sgpr_r = strcmp(v, "sg") == 0 ? 8 : (strcmp(v, "sg4") == 0 ? 4 : 0);
            if (p->sgpr_r && ntaps == 128) {
                const void *k = p->sgpr_r == 8 ? (const void *)sxfir::decim4_sgpr_kernel<8>
                                               : (const void *)sxfir::decim4_sgpr_kernel<4>;
                query_occupancy(&p->occ_sb, k, 64);
            }
            // "wide": decim4_wide_kernel (sxfir_decim_wide.hip.h), symmetric taps only
            if (strncmp(v, "wide", 4) == 0 && ntaps == 128 && p->symmetric) {
                p->wide = true;
                p->wide_nt = strncmp(v, "wident", 6) == 0;
                p->wide_pin = strncmp(v, "widentp", 7) == 0;
                p->wide_nb = atoi(v + (p->wide_pin ? 7 : (p->wide_nt ? 6 : 4)));
                // "widepol<hex>": the shipped build (wident24) with another cache policy (sxfir_decim_wide.hip.h, POL)
                if (strncmp(v, "widepol", 7) == 0) {
                    p->wide_nt = true;
                    p->wide_nb = 24;
                    p->wide_pol = (int)strtol(v + 7, nullptr, 16);
                }
                // SXFIR_LDS_PAD: dynamic LDS bytes on top of the kernel's own image: fewer waves fit a CU (a probe: what would a
                // form with a larger tile per wave -- 16 outputs per lane, 34 KB -- have left of the latency hiding?)
                if (const char *lp = getenv("SXFIR_LDS_PAD")) {
                    p->lds_pad = atoi(lp) > 0 ? atoi(lp) : 0;
                    if (p->lds_pad) query_occupancy(&p->occ_wide, sxfir::decim4_wide_kernel<0, false, 24, true>, 64, (size_t)p->lds_pad);
                }
            }
            // "pair": decim4_pair_kernel (sxfir_decim_pair.hip.h)
            if (strncmp(v, "pair", 4) == 0 && ntaps == 128) {
                p->pair = true;
                p->pair_xsep = strcmp(v, "pairx") == 0;
                if (p->pair_xsep) p->occ_pair = 7;
            }
            // "t2:<waves per workgroup>:<option bits>": decim4_tile2_kernel (sxfir_decim_tile2.hip.h)
            if (strncmp(v, "t2:", 3) == 0 && ntaps == 128 && fmt == SXFIR_CF32) {
                int wpg = 0, opt = 0;
                if (sscanf(v + 3, "%d:%d", &wpg, &opt) == 2) {
                    const void *k = nullptr;
                    switch (wpg * 100 + opt) {
#define SXFIR_X(WW, OO) case WW * 100 + OO: k = (const void *)sxfir::decim4_tile2_kernel<128, WW, OO>; break;
                        SXFIR_TILE2_VARIANTS(SXFIR_X)
#undef SXFIR_X
                    }
                    if (!k || ((opt & sxfir::T2_SCALAR) && !p->symmetric)) {
                        free_plan(p);
                        return fail(SXFIR_EUNSUPPORTED, "no tile2 variant %d:%d for these taps", wpg, opt);
                    }
                    p->t2_wpg = wpg;
                    p->t2_opt = opt;
                    // SXFIR_LDS_PAD: dynamic LDS bytes on top of the kernel's own image: fewer waves fit a CU
                    if (const char *lp = getenv("SXFIR_LDS_PAD")) p->lds_pad = atoi(lp) > 0 ? atoi(lp) : 0;
                    // occ_sb = resident WAVES per CU of this variant
                    int nb = 0;
                    query_occupancy(&nb, k, 64 * wpg, (size_t)p->lds_pad);
                    if (nb > 0) p->occ_sb = nb * wpg;
                }
            }
        }
        if (const char *v = getenv("SXFIR_SCHED")) p->sched = atoi(v);
        if (const char *v = getenv("SXFIR_OCC")) {
            if (atoi(v) > 0) p->occ_sb = p->occ_db = atoi(v);
        }
#endif
    }

    std::vector<float> scaled(taps, taps + ntaps);
    for (int k = 0; k < 64; ++k) p->taps_k[k] = k < ntaps ? (fmt == SXFIR_S32 ? taps[k] * 4.656612873077393e-10f : taps[k]) : 0.0f;
    // the layout follows the kernel the plan will launch (the same flags launch_decim / launch_interp branch on),
    // not the shape: a plan whose /8 scalar-tap form was switched off (profiling knobs) keeps the plain table
    p->tap_table = p->blocks ? TAPS_BLOCKS16 : p->dense_subset ? TAPS_SUBSET8 : (mode == SXFIR_INTERPOLATE && p->ipass) ? TAPS_PASS8 : TAPS_SCALED;
    if (p->tap_table == TAPS_SUBSET8) {
        // /8 scalar-tap form (decim_dense_kernel<8, ..., SUBSET>): subset s = 2c + p at 64 s, (jj, rr) at 4 jj + rr
        for (int c = 0; c < 2; ++c)
            for (int ph = 0; ph < 2; ++ph)
                for (int jj = 0; jj < 16; ++jj)
                    for (int rr = 0; rr < 4; ++rr)
                        scaled[(size_t)(64 * (2 * c + ph) + 4 * jj + rr)] =
                            taps[8 * (16 * ph + jj) + 4 * c + rr] * (fmt == SXFIR_S32 ? 4.656612873077393e-10f : 1.0f);   // 2^-31: exact
    } else if (p->tap_table == TAPS_BLOCKS16) {
        // decim_blocks_kernel: the ROTATED taps (slot k' holds tap (k' + 1) mod ntaps); block b (columns 16 b .. 16 b + 15)
        // at 512 b, subset s = 2c + p at 64 s inside it, (jj, rr) at 4 jj + rr
        for (int b = 0; b < p->blocks; ++b)
            for (int c = 0; c < 4; ++c)
                for (int ph = 0; ph < 2; ++ph)
                    for (int jj = 0; jj < 16; ++jj)
                        for (int rr = 0; rr < 4; ++rr) {
                            const int slot = ratio * (16 * ph + jj) + 16 * b + 4 * c + rr;
                            scaled[(size_t)(512 * b + 64 * (2 * c + ph) + 4 * jj + rr)] =
                                taps[(slot + p->rot) % ntaps] * (fmt == SXFIR_S32 ? 4.656612873077393e-10f : 1.0f);
                        }
    } else if (p->tap_table == TAPS_PASS8) {
        const int ll = ratio >= 16 ? 16 : ratio;            // phases per (block of the) pass kernel
        for (int b = 0; b < ratio / ll; ++b)
        for (int c = 0; c < ll / 4; ++c)                    // x8: two phase groups; x4: one; x16 blocks: four
            for (int ph = 0; ph < 2; ++ph)
                for (int jj = 0; jj < 16; ++jj)
                    for (int rr = 0; rr < 4; ++rr)
                        scaled[(size_t)(32 * ll * b + 64 * (2 * c + ph) + 4 * jj + rr)] = taps[(16 * ph + jj) * ratio + ll * b + 4 * c + rr];
    } else {
        for (float &t : scaled) t *= 4.656612873077393e-10f;      // 2^-31: exact
    }
    return plan_to_device(out, p, taps, (size_t)ntaps, scaled.data());
}

int sxfir_destroy(sxfir_plan *p)
{
    if (p) free_plan(p);
    return SXFIR_OK;
}

int sxfir_reset(sxfir_plan *p, void *stream)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    HIPCHECK(hipMemsetAsync(p->hist_dev, 0, sample_bytes(p->fmt) * (size_t)p->hist_len * (size_t)p->nchan,
                            S(stream)));
    // /48, /96: the arrival counters of the (tile, block) join too (16 KiB at 256 CUs) -- a launch that was abandoned, or a plan
    // that was misused on two streams, must not make the next stream's tiles join early or never
    if (p->join_arrived) HIPCHECK(hipMemsetAsync(p->join_arrived, 0, sizeof(unsigned) * (size_t)p->join_tiles, S(stream)));
    p->consumed = p->produced = 0;
    return SXFIR_OK;
}

int sxfir_set_history(sxfir_plan *p, const void *src_dev, size_t n, size_t stride, void *stream)
{
    if (!p || !src_dev) return fail(SXFIR_EINVAL, "NULL argument");
    if (p->kind == KIND_SYNTHESIZER)
        return fail(SXFIR_EUNSUPPORTED, "sxfir_set_history has one stride: it cannot name the bands and the channels of a synthesizer plan's input");
    if (n < (size_t)p->hist_len) return fail(SXFIR_EINVAL, "history needs %d samples per channel, %zu given", p->hist_len, n);
    if (p->nchan > 1 && stride < n) return fail(SXFIR_EINVAL, "channel stride %zu shorter than the block (%zu)", stride, n);
    const size_t sb = sample_bytes(p->fmt);
    // the LAST hist_len samples of the block, channel by channel
    const char *src = static_cast<const char *>(src_dev) + sb * (n - (size_t)p->hist_len);
    HIPCHECK(hipMemcpy2DAsync(p->hist_dev, sb * (size_t)p->hist_len, src, sb * stride, sb * (size_t)p->hist_len, (size_t)p->nchan,
                              hipMemcpyDeviceToDevice, S(stream)));
    return SXFIR_OK;
}

int sxfir_set_position(sxfir_plan *p, int64_t consumed)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (consumed < 0) return fail(SXFIR_EINVAL, "negative stream position");
    p->consumed = (long long)consumed;
    p->produced = p->mode == SXFIR_DECIMATE ? ((long long)consumed + p->ratio - 1) / p->ratio
                                            : (long long)consumed * p->ratio;
    return SXFIR_OK;
}

int sxfir_set_kernel(sxfir_plan *p, int kernel)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (kernel < SXFIR_KERNEL_AUTO || kernel > SXFIR_KERNEL_GENERIC) return fail(SXFIR_EINVAL, "bad kernel id");
    if (kernel == SXFIR_KERNEL_TILED && !p->tile_capable && !p->multi_capable && !p->itile_capable && !p->ext_tiled)
        return fail(SXFIR_EUNSUPPORTED, "no tiled kernel for ntaps=%d ratio=%d fmt=%d mode=%d", p->ntaps,
                    p->ratio, p->fmt, p->mode);
    p->kernel = kernel;
    return SXFIR_OK;
}

int sxfir_set_tx_threshold(sxfir_plan *p, float tx_threshold2)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    p->thr2 = tx_threshold2;
    return SXFIR_OK;
}

#ifdef SXFIR_PROFILING
// Diagnostic (SXFIR_ABLATE=11/12 builds): median in-kernel shader clock in MHz of the last launch.
int sxfir_debug_clock(sxfir_plan *p, double *mhz)
{
    if (!p || !mhz || !p->stamps_dev) return fail(SXFIR_EINVAL, "no stamps recorded");
    std::vector<unsigned long long> h(2 * p->stamps_n);
    HIPCHECK(hipMemcpy(h.data(), p->stamps_dev, 16 * p->stamps_n, hipMemcpyDeviceToHost));
    std::vector<double> f;
    for (size_t i = 0; i < p->stamps_n; ++i)
        if (h[2 * i + 1] > 0) f.push_back(100.0 * (double)h[2 * i] / (double)h[2 * i + 1]);
    if (f.empty()) return fail(SXFIR_EINVAL, "no stamps recorded");
    std::sort(f.begin(), f.end());
    *mhz = f[f.size() / 2];
    return SXFIR_OK;
}

int sxfir_debug_stamps(sxfir_plan *p, unsigned long long *host, size_t capacity_records, size_t *n_records)
{
    if (!p || !host || !n_records || !p->stamps_dev || (p->ablate != 3 && p->ablate != 5)) return fail(SXFIR_EINVAL, "no stamps recorded");
    const size_t n = p->stamps_n < capacity_records ? p->stamps_n : capacity_records;
    // records: 5 x uint64 (multi-column kernel, ablate 3) or 8 x uint64 (tile2 kernel, ablate 5)
    HIPCHECK(hipMemcpy(host, p->stamps_dev, (p->ablate == 5 ? 64 : 40) * n, hipMemcpyDeviceToHost));
    *n_records = n;
    return SXFIR_OK;
}

// Test hooks of the (tile, block) join of decim_blocks_kernel<..., SPLIT> (tests/gpu_util.py, tools/soak_split.py).
int sxfir_debug_join_poison(sxfir_plan *p, uint32_t word, void *stream)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (!p->join_partials) return fail(SXFIR_EUNSUPPORTED, "this plan has no join scratch");
    HIPCHECK(hipMemsetD32Async((hipDeviceptr_t)p->join_partials, (int)word, (size_t)p->join_tiles * (size_t)p->blocks * 1024, S(stream)));
    return SXFIR_OK;
}

int sxfir_debug_join_counters(sxfir_plan *p, long long *nonzero, void *stream)
{
    if (!p || !nonzero) return fail(SXFIR_EINVAL, "NULL argument");
    if (!p->join_arrived) return fail(SXFIR_EUNSUPPORTED, "this plan has no join scratch");
    std::vector<unsigned> h((size_t)p->join_tiles);
    HIPCHECK(hipMemcpyAsync(h.data(), p->join_arrived, sizeof(unsigned) * h.size(), hipMemcpyDeviceToHost, S(stream)));
    HIPCHECK(hipStreamSynchronize(S(stream)));
    long long n = 0;
    for (unsigned v : h) n += v != 0;
    *nonzero = n;
    return SXFIR_OK;
}

int sxfir_debug_join_set_counter(sxfir_plan *p, long long tile_index, unsigned value, void *stream)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (!p->join_arrived) return fail(SXFIR_EUNSUPPORTED, "this plan has no join scratch");
    if (tile_index < 0 || tile_index >= p->join_tiles) return fail(SXFIR_EINVAL, "tile %lld of %lld", tile_index, p->join_tiles);
    HIPCHECK(hipMemsetD32Async((hipDeviceptr_t)(p->join_arrived + tile_index), (int)value, 1, S(stream)));
    return SXFIR_OK;
}

#endif  // SXFIR_PROFILING

int sxfir_contract(const sxfir_plan *p, int *jsplit, int *cw)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (jsplit) *jsplit = p->jsplit;
    if (cw) *cw = p->cw;
    return SXFIR_OK;
}

int sxfir_contract_rotation(const sxfir_plan *p, int *rot)
{
    if (!p || !rot) return fail(SXFIR_EINVAL, "NULL argument");
    *rot = p->rot;
    return SXFIR_OK;
}

int sxfir_position(const sxfir_plan *p, int64_t *consumed, int64_t *produced)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (consumed) *consumed = p->consumed;
    if (produced) *produced = p->produced;
    return SXFIR_OK;
}

static long long outputs_for(const sxfir_plan *p, long long n_in)
{
    if (p->mode == SXFIR_INTERPOLATE) return n_in * p->ratio;
    const long long D = p->ratio;
    const long long before = (p->consumed + D - 1) / D;
    const long long after = (p->consumed + n_in + D - 1) / D;
    return after - before;
}

int sxfir_outputs_for(const sxfir_plan *p, size_t n_in, size_t *n_out)
{
    if (!p || !n_out) return fail(SXFIR_EINVAL, "NULL argument");
    *n_out = (size_t)outputs_for(p, (long long)n_in);
    return SXFIR_OK;
}

}  // extern "C"
