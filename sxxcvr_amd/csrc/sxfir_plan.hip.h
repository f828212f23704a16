// Plan bookkeeping of the C ABI (include/sxfir.h): what a plan holds and which of the five kinds it is, the kernel table (which
// instance a shape launches: the one statement of it, for the occupancy query and the launches), the form rows (what the geometry
// and launch code needs to know of a tiled kernel family: one row per family, one pointer per plan), settle_form (which row a
// real-tap shape gets: the one statement of the product's shape-to-family rules), the tap-table layouts, the creation frame every
// sxfir_create* goes through (argument checks, the device, the plan's common fields, the real-tap contract, the form, its kernels
// and occupancy, the plan's device memory and the one list of what to free), sxfir_create, the one creation path of the four band
// plans (create_band_plan), and the small state entry points (reset, history, position, contract).  The product never looks at the
// environment: what the profiling build's knobs change sits behind the prof_* hooks of sxfir_prof_create.inc.
// Included by sxfir.hip after the kernel headers; not a stand-alone translation unit.
#pragma once

// What created the plan: sxfir_create, sxfir_create_complex (sxfir_complex.hip.h), sxfir_create_channelizer
// (sxfir_channelizer.hip.h), sxfir_create_synthesizer (sxfir_synthesizer.hip.h), sxfir_create_channelizer_os
// (sxfir_channelizer_os.hip.h: KIND_CHANNELIZER with ratio = bands / oversample), sxfir_create_synthesizer_os
// (sxfir_synthesizer_os.hip.h: KIND_SYNTHESIZER with ratio = bands / oversample).  A complex-tap plan is a decimator whose taps_dev
// holds a[0, ntaps) then b[0, ntaps) -- sxfir_create_translating (sxfir_translate.hip.h) makes one that carries a mixer (mix_dev,
// mix_den, mix_s: its outputs turned by a table entry each, the mixer instances of the complex-tap kernels on argument structs of
// their own); the band kinds are a /ratio decimator and a x ratio interpolator in everything about the stream.
// sxfir_create_rational (sxfir_rational.hip.h): KIND_RATIONAL, a x ratio interpolator (ratio = up) of which every down-th output is
// computed -- an interpolator's history and contract, positions and output counts of its own (rational_produced).
// sxfir_create_arbitrary (sxfir_arbitrary.hip.h): KIND_ARBITRARY, a x ratio interpolator (ratio = nphases) between whose outputs the
// plan's own are blended, at a fixed-point time that advances by arb_step per output -- an interpolator's history and contract, a
// time and output counts of its own (arb_outputs, sxfir_arb_index.h).
// sxfir_create_bank (sxfir_bank.hip.h): KIND_BANK, a /ratio decimator with bank_n sets of complex taps (taps_dev: band k's planar a | b at
// 2 ntaps k) and a mixer per band (bank_num, bank_den, bank_s, bank_w) -- one history, one position, K output rows.
// sxfir_create_bank_interpolator (sxfir_bank_tx.hip.h): KIND_BANK_TX, a x ratio interpolator with the bank's fields (bank_n tap sets, a mixer per
// band) whose K results are summed -- one position, a history per band (hist_dev: bank_n x hist_len / bank_n samples per channel), one output row.
enum PlanKind { KIND_REAL = 0, KIND_COMPLEX = 1, KIND_CHANNELIZER = 2, KIND_SYNTHESIZER = 3, KIND_RATIONAL = 4, KIND_ARBITRARY = 5, KIND_BANK = 6, KIND_BANK_TX = 7 };

// The layout of a plan's second tap table (taps_scaled_dev); one function per layout below (second_tap_table).
// TAPS_SCALED: taps * 2^-31 (exact) in tap order, for the /4 scalar-tap kernels on S32 wire words;
// TAPS_SUBSET8: the subset-major table of decim_dense_kernel<8, ..., SUBSET> (times 2^-31 for S32 plans);
// TAPS_PASS8: the pass-major table of interp8_pass_kernel (pass (c, p) at 64 (2c + p), (jj, rr) at 4 jj + rr);
// TAPS_BLOCKS16: the block-major table of decim_blocks_kernel, of the ROTATED taps (times 2^-31 for S32 plans);
// TAPS_PHASED: the phase-major table of synthesis4_kernel and synthesis4x2_kernel (h[ratio j + r] at (ntaps / ratio) r + j: four
// phases, or the two output parities of the oversampled plan); TAPS_NONE: the plan's kernels read taps_dev alone;
// TAPS_PASS8_CX: interp_cx_pass_kernel's, 2 x ntaps floats -- the TAPS_PASS8 table of a, then that of b;
// TAPS_ARB: resample_arb_kernel's, (P + 1) rows of T + 4 floats -- row p holds h[(T - 1 - i) P + p] at i (j descending), row P repeats row 0.
// Every launch that hands taps_scaled_dev to a kernel checks the plan's layout first (need_tap_table).
enum TapTable { TAPS_SCALED = 0, TAPS_SUBSET8 = 1, TAPS_PASS8 = 2, TAPS_BLOCKS16 = 3, TAPS_PHASED = 4, TAPS_NONE = 5, TAPS_PASS8_CX = 6, TAPS_ARB = 7 };

// Which kernel family a call launches (LaunchGeom::kind, sxfir_launch.hip.h)
enum { GEOM_GENERIC = 0, GEOM_MULTI = 1, GEOM_WIDE = 2, GEOM_TILE = 3, GEOM_IPASS = 4, GEOM_ITILE = 5, GEOM_CX = 6, GEOM_CHAN4 = 7, GEOM_SYN4 = 8, GEOM_CHAN4X2 = 9, GEOM_SYN4X2 = 10, GEOM_ICX = 11, GEOM_RAT45 = 12, GEOM_MIX = 13, GEOM_IMIX = 14, GEOM_ARB = 15, GEOM_BANK = 16, GEOM_BANK_TX = 17 };

// One typed kernel pointer per launch-argument family, and a plan's kernels: resolved once by the plan's creator
// (resolve_kernels below), read by the occupancy query there and by the launches (sxfir_launch.hip.h).
typedef void (*GenericFn)(sxfir::GenericArgs);
typedef void (*DecimMultiFn)(sxfir::DecimMultiArgs);
typedef void (*DecimBlocksFn)(sxfir::DecimMultiArgs, sxfir::DecimBlocksJoin);
typedef void (*DecimTileFn)(sxfir::DecimTileArgs);
typedef void (*InterpTileFn)(sxfir::InterpTileArgs);
typedef void (*ChanTileFn)(sxfir::ChanTileArgs);
typedef void (*SynTileFn)(sxfir::SynTileArgs);
typedef void (*SynOsTileFn)(sxfir::SynOsTileArgs);
typedef void (*MixGenericFn)(sxfir::MixGenericArgs);
typedef void (*MixTileFn)(sxfir::MixTileArgs);
typedef void (*InterpMixTileFn)(sxfir::InterpMixTileArgs);
typedef void (*ArbTileFn)(sxfir::ArbTileArgs);
typedef void (*BankGenericFn)(sxfir::BankGenericArgs);
typedef void (*BankTileFn)(sxfir::BankTileArgs);
typedef void (*BankTxGenericFn)(sxfir::BankTxGenericArgs);
typedef void (*BankTxTileFn)(sxfir::BankTxTileArgs);
struct KernelTable {
    const char *generic_name;    // the plan's generic kernel, as sxfir_launch_geometry reports it, and the instance: every plan of every
    GenericFn generic;           // kind has exactly one (generic_kernel below), the kernel of every call its form does not take
    DecimMultiFn dense;          // decim_dense_kernel (/8, /16, /32)
    DecimBlocksFn blocks[2];     // decim_blocks_kernel (/48, /96): [0] the walking form, [1] SPLIT, (tile, block) items
    DecimTileFn tile, wide, cx;  // /4: decim4_tile_kernel, decim4_wide_kernel, decim4_cx_kernel<DecimTileArgs> (complex taps)
    InterpTileFn interp[2][2];   // [keyed][split]: interp8_pass_kernel; interp_tile_kernel on CF16 storage ([0][0] alone)
    InterpTileFn interp_cx;      // complex-tap interpolators (include/sxfir_complex_tx.h): interp_cx_pass_kernel<.., InterpTileArgs> (x4 x 128, x8 x 256, CF32)
    ChanTileFn chan4;            // channelizer plans (include/sxfir_channelizer.h): chan4_kernel (4 bands x 128 taps, CF32)
    ChanTileFn chan4x2;          // 2x oversampled channelizer plans (include/sxfir_channelizer_os.h): chan4x2_kernel (4 bands x 128 taps, CF32)
    SynTileFn syn4;              // synthesizer plans (include/sxfir_synthesizer.h): synthesis4_kernel (4 bands x 128 taps, CF32)
    SynOsTileFn syn4x2;          // 2x oversampled synthesizer plans (include/sxfir_synthesizer_os.h): synthesis4x2_kernel (4 bands x 128 taps, CF32)
    DecimTileFn rat45;           // rational plans (include/sxfir_rational.h): resample45_kernel (4/5 x 128 taps, CF32)
    MixGenericFn mix_generic;    // translating plans (include/sxfir_translate.h, include/sxfir_translate_tx.h), in the place of `generic`:
                                 // decim_cx_generic_kernel<.., MixGenericArgs> or interp_mix_generic_kernel
    MixTileFn mix;               // translating decimators: decim4_cx_kernel<MixTileArgs> (/4 x 128 complex taps, CF32)
    InterpMixTileFn imix;        // translating interpolators: interp_cx_pass_kernel<.., InterpMixTileArgs> (x4 x 128, x8 x 256 complex taps, CF32)
    ArbTileFn arb;               // arbitrary-rate plans (include/sxfir_arbitrary.h): resample_arb_kernel (128 phases x 32 taps, CF32)
    BankGenericFn bank_generic;  // bank plans (include/sxfir_bank.h), in the place of `generic`: decim_bank_generic_kernel
    BankTileFn bank;             // ... and decim4_bank_kernel (/4 x 128 complex taps per band, CF32)
    BankTxGenericFn bank_tx_generic;   // combiner plans (include/sxfir_bank_tx.h), in the place of `generic`: interp_bank_generic_kernel
    BankTxTileFn bank_tx;        // ... and interp4_bank_kernel (x4 x 128 complex taps per band, CF32)
};

// What the geometry and launch code needs to know of a tiled kernel family (FORM_* below).  A plan has at most one, settled at
// creation (settle_form; the band and complex-tap creators' one line each); a call only chooses between it and the plan's generic
// kernel.  A plan without a row runs its generic kernel alone.
enum { TILE_DENSE = -1, TILE_IPASS = -2, TILE_ITILE = -3 };    // PlanForm::tile where one family serves several ratios (form_tile)
struct PlanForm {
    const char *tiled;             // the kernel's name, as sxfir_launch_geometry reports it
    int geom;                      // GEOM_*: also names the family where the typed pointers and argument structs differ
    int tile;                      // outputs per tile of a decimator, inputs of an interpolator (band plans: PER BAND), or a TILE_* rule
    int threads;                   // per workgroup
    int start_multiple;            // the kernel takes a call that starts at a stream position that is a multiple of this (1: any)
    int cf16_stride;               // on CF16 storage its 16-byte stores need a channel stride that is a multiple of this (else: of 2)
    bool heavy_prologue;           // generations(): a workgroup of a small call keeps at least four tiles
    int generations;               // generations of resident workgroups per launch, measured (the comments at the rows)
    int occ;                       // resident workgroups per CU where the runtime has no answer
    int taps;                      // the TapTable layout its kernel reads
};

#include "sxfir_prof_knobs.inc"    // struct ProfKnobs: what the profiling build's knobs set; empty in the production library

struct sxfir_plan {
    int kind;              // PlanKind
    int mode, ntaps, ratio, nchan, fmt, device;
    int down;              // rational plans: `down` of up / down (up is `ratio`); else 0
    uint64_t arb_step;     // arbitrary-rate plans (nphases is `ratio`): input samples per output, Q32.32; else 0
    long long arb_t_index; // ... the time of the next output: whole input samples
    uint32_t arb_t_frac;   // ... and its fraction, Q0.32
    int bands;             // the band kinds: 4 (= ratio, but for the oversampled plans); bank and combiner plans: bank_n; else 0.  A synthesizer's hist_dev holds
                           // bands x hist_len / bands samples per channel, band k's at k * hist_len / bands
    int oversample;        // channelizer plans: bands / ratio -- 1 critically sampled (sxfir_create_channelizer), 2 each band at fs/2
                           // (sxfir_create_channelizer_os: ratio 2, bands 4); synthesizer plans likewise: 1 each band at fs/4
                           // (sxfir_create_synthesizer), 2 each band at fs/2 (sxfir_create_synthesizer_os: ratio 2, bands 4); else 0
    int kernel;            // SXFIR_KERNEL_*
    int hist_len;          // samples of history kept per channel
    int jsplit, cw;        // numeric contract
    int rot;               // ... and its rotation (0; 1 for /48, /96: sxfir_contract_rotation)
    bool symmetric;        // real taps: taps[k] == taps[ntaps-1-k] bit for bit (every linear-phase design)
    const PlanForm *form;  // the plan's tiled kernel family; null: generic only
    int tile;              // ... its tile for this ratio (form_tile),
    int oversub;           // ... its generations per launch: workgroups launched = CUs * occ * oversub,
    int occ;               // ... and its resident workgroups per CU, asked of the runtime for the form's base instance (occupancy_instance)
    int blocks;            // the block form: sixteen-column blocks per row (/48: 3, /96: 6), else 0
    void *join_partials;   // ... scratch of decim_blocks_kernel<..., SPLIT>: join_tiles x blocks block values of 4 KiB
    unsigned *join_arrived;   // ... and one arrival counter per (channel, tile); zero between launches: each tile's last item
                              // zeroes its own, sxfir_reset and a failed launch zero them all
    long long join_tiles;  // tiles (over all channels) the scratch holds = the largest call the SPLIT form takes
    bool blocks_split;     // (tile, block) items for calls the scratch holds (profiling: SXFIR_BLOCKS_SPLIT=0 switches the dealing off)
    bool ipass_split;      // the pass form at x32, x48, x96: (tile, phase block) items for small calls (profiling: SXFIR_IPASS_SPLIT=0 switches it off)
    float thr2;            // S32 interpolator: transmitter-keying threshold (squared magnitude)
    int compute_units;
    float *taps_dev;
    float *taps_scaled_dev;   // the second tap table, in the layout tap_table names (the form's; TAPS_SCALED for a real-tap plan without a form)
    int tap_table;
    float taps_k[64];         // the first 64 taps (times 2^-31 for S32 plans) for kernels that take them by value
    void *hist_dev;        // current history: nchan * hist_len samples
    void *hist_alt;        // the tiled kernels write the next history here, then the two swap
    float *mix_dev;        // translating plans (include/sxfir_translate.h): the rotation table, mix_den (re, im) pairs; else null
    int mix_den, mix_num;  // ... its length (0: the plan has no mixer) and num mod den of the band centre num / den
    int mix_s;             // ... (num * ratio) mod den: table entries per output.  A translating INTERPOLATOR (include/sxfir_translate_tx.h:
                           // mode SXFIR_INTERPOLATE tells the two apart) carries the same three: its inputs are turned, by den - mix_s entries each
    int bank_n;            // bank and combiner plans (include/sxfir_bank.h, include/sxfir_bank_tx.h): the band count (0: neither); per band num mod den, den,
    int bank_num[sxfir::BANK_MAX], bank_den[sxfir::BANK_MAX], bank_s[sxfir::BANK_MAX];   // ... (num * ratio) mod den,
    float *bank_w[sxfir::BANK_MAX];   // ... and the rotation table: bands of one den share one (free_plan frees each once)
    KernelTable k;         // the instances this plan launches (null: none in this build for that family)
    ProfKnobs prof;        // written and read by the profiling build's hooks alone
    long long consumed, produced;
};

// ---- The kernel table: for each family ONE function from a shape (mode, ratio, ntaps, fmt, symmetric, cx; for the
// interpolators also the two run-time selectors, keyed and split) to the instance that ships.  This is the only place where
// the product's template argument lists are written.  nullptr: no instance for that shape in the production library (its A/B
// partners are launched by the profiling build's hooks, sxfir_prof_dispatch.inc); launch() refuses a null entry.
//
// Occupancy (occupancy_instance, resolve_form) is queried on the entry of a plan's BASE form, which is not always the instance a call launches:
// the walking, non-SPLIT form for /48 and /96; interp_kernel(16, CF32, unkeyed, walking) for every x16 .. x96 plan whatever its
// ratio, format or keying, (8, CF32, ...) for x8 and (4, CF32, ...) for x4; decim4_tile_kernel's CF32 instance for S32 words too.
// The launch geometry of every plan was measured with these figures.
//
// The generic kernels: one per plan kind (and, for the band kinds, per oversampling), one thread per item, all on GenericArgs.  A
// kernel's three instances by format: the RX kinds take S32 wire words in and give CF32 (<S32, CF32>), the TX kinds take CF32 and
// give wire words (<CF32, S32>); a rational plan has no wire-word form.
struct GenericKernel { const char *name; GenericFn fn; };
// (WI, WO: the storage formats of a wire-word plan's instance)
#define SXFIR_GENERIC(K, WI, WO) \
    return GenericKernel{#K, fmt == SXFIR_CF32 ? (GenericFn)K<CF32> : fmt == SXFIR_CF16 ? (GenericFn)K<CF16> : (GenericFn)K<WI, WO>}
static GenericKernel generic_kernel(int kind, int oversample, int mode, int fmt)
{
    using namespace sxfir;
    const bool os = oversample == 2, rx = mode == SXFIR_DECIMATE;
    switch (kind) {
    case KIND_CHANNELIZER:      // four chains and the butterflies per thread (oversampled: of the output's parity)
        if (os) SXFIR_GENERIC(chan4x2_generic_kernel, S32, CF32);
        SXFIR_GENERIC(chan_generic_kernel, S32, CF32);
    case KIND_SYNTHESIZER:      // the butterflies once per input index, four phase chains per thread (oversampled: the two DFT
        if (os) SXFIR_GENERIC(synthesis_os_generic_kernel, CF32, S32);      // outputs an input index needs, two chains)
        SXFIR_GENERIC(synthesis_generic_kernel, CF32, S32);
    case KIND_RATIONAL:
        return GenericKernel{"resample_generic_kernel", fmt == SXFIR_CF16 ? (GenericFn)resample_generic_kernel<CF16, CF16> : (GenericFn)resample_generic_kernel<CF32, CF32>};
    case KIND_ARBITRARY:
        return GenericKernel{"resample_arb_generic_kernel", fmt == SXFIR_CF16 ? (GenericFn)resample_arb_generic_kernel<CF16> : (GenericFn)resample_arb_generic_kernel<CF32>};
    case KIND_BANK:             // on an argument struct of its own (GenericArgs plus the bands): the instance is bank_generic_kernel's
        return GenericKernel{"decim_bank_generic_kernel", nullptr};
    case KIND_BANK_TX:          // likewise (GenericArgs plus the bands): bank_tx_generic_kernel's
        return GenericKernel{"interp_bank_generic_kernel", nullptr};
    case KIND_COMPLEX:
        if (rx) SXFIR_GENERIC(decim_cx_generic_kernel, S32, CF32);
        SXFIR_GENERIC(interp_cx_generic_kernel, CF32, S32);
    }
    if (rx) SXFIR_GENERIC(decim_generic_kernel, S32, CF32);
    SXFIR_GENERIC(interp_generic_kernel, CF32, S32);
}
#undef SXFIR_GENERIC

// Translating plans (include/sxfir_translate.h, include/sxfir_translate_tx.h), on MixGenericArgs: the complex-tap decimators'
// generic kernel with the mixer, the three instances of an RX kind (reported as decim_mix_generic_kernel); interp_mix_generic_kernel,
// the three of a TX kind
static MixGenericFn mix_generic_kernel(int mode, int fmt)
{
    using namespace sxfir;
    if (mode == SXFIR_DECIMATE)
        return fmt == SXFIR_CF32   ? decim_cx_generic_kernel<CF32, CF32, MixGenericArgs>
               : fmt == SXFIR_CF16 ? decim_cx_generic_kernel<CF16, CF16, MixGenericArgs>
                                   : decim_cx_generic_kernel<S32, CF32, MixGenericArgs>;
    return fmt == SXFIR_CF32 ? interp_mix_generic_kernel<CF32> : fmt == SXFIR_CF16 ? interp_mix_generic_kernel<CF16> : interp_mix_generic_kernel<CF32, S32>;
}

// Bank plans (include/sxfir_bank.h), on BankGenericArgs: the three instances of an RX kind
static BankGenericFn bank_generic_kernel(int fmt)
{
    using namespace sxfir;
    return fmt == SXFIR_CF32 ? decim_bank_generic_kernel<CF32, CF32> : fmt == SXFIR_CF16 ? decim_bank_generic_kernel<CF16, CF16> : decim_bank_generic_kernel<S32, CF32>;
}

// Combiner plans (include/sxfir_bank_tx.h), on BankTxGenericArgs: the three instances of a TX kind
static BankTxGenericFn bank_tx_generic_kernel(int fmt)
{
    using namespace sxfir;
    return fmt == SXFIR_CF32 ? interp_bank_generic_kernel<CF32> : fmt == SXFIR_CF16 ? interp_bank_generic_kernel<CF16> : interp_bank_generic_kernel<CF32, S32>;
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

// Complex-tap interpolators, 32 taps per phase on CF32: interp_cx_pass_kernel<QI, LL, Args> on the pass kernel's frame -- x4 with
// four inputs per lane, x8 with two (sxfir_interp_cx.hip.h); Args = InterpMixTileArgs: the translating interpolators' instances
template <typename Args>
static auto interp_cx_kernel(int ratio) -> void (*)(Args)
{
    if (ratio == 4) return sxfir::interp_cx_pass_kernel<4, 4, Args>;
    if (ratio == 8) return sxfir::interp_cx_pass_kernel<2, 8, Args>;
    return nullptr;
}

// The four band forms, [synthesizer][oversampled].  chan4_kernel: tiles of 512 outputs per band.  chan4x2_kernel (ratio 2): 1024
// outputs per band = 2048 inputs; its lane map needs the call's first output to have an EVEN index, i.e. a stream position that is
// a multiple of 4 (every position of the /2 raster starts on an output).  synthesis4_kernel: 256 inputs per band on the x4 pass
// kernel's frame.  synthesis4x2_kernel: any per-band start index -- the start's parity is its argument.
static const PlanForm BAND_FORMS[2][2] = {
    {{"chan4_kernel", GEOM_CHAN4, 512, 64, 1, 2, true, 16, 8, TAPS_NONE}, {"chan4x2_kernel", GEOM_CHAN4X2, 1024, 64, 4, 2, true, 16, 8, TAPS_NONE}},
    {{"synthesis4_kernel", GEOM_SYN4, 256, 64, 1, 2, true, 16, 8, TAPS_PHASED},
     {"synthesis4x2_kernel", GEOM_SYN4X2, sxfir::Syn4x2::TILE_IN, 64, 1, 2, true, 16, 5, TAPS_PHASED}}};

// ---- The form rows of the real-tap and complex-tap plans: {name, GEOM_*, tile, threads, start multiple, CF16 stride, heavy
// prologue, generations, occupancy where the runtime has no answer, tap layout}.
// Generations of workgroups per launch, measured on MI355X at 2^28 samples (tools/kbench.py): the /4 kernels, single-buffered LDS-DMA
// at their resident waves per CU, run 16 generations of short-lived waves (4 tiles each) in strided XCD-blocked passes (the
// double-buffered variant and long contiguous runs are slower); decim4_cx_kernel and the band kernels stand on the wide kernel's
// frame: its sixteen generations at the sizes they were measured at, fewer while that would leave a wave under four tiles.  The
// dense and block kernels' prologue (the taps and the DMA offset table per lane) is heavier than the /4 kernels': 8 beats 16, and
// where it is 64 taps into VGPRs (/16, /32) a small call keeps four tiles per workgroup.  The pass kernel: 4 / 8 / 16 measured within
// 0.3 % (tools/ibench2.py), 8; its x16 .. x96 form pays a window and lane constants per workgroup.  interp_tile_kernel is flat between
// 2 and 16 (tools/ibench.py): 4, and 2 for its three-phase-block form (x48, x96: 1-2 % ahead of 4 .. 32, profiles/round5_rates.txt).
// decim4_wide_kernel: /4, 128 taps, tiles of 512 outputs, one wave (= one workgroup) per tile and pass
static const PlanForm FORM_WIDE = {"decim4_wide_kernel", GEOM_WIDE, 512, 64, 1, 2, false, 16, 8, TAPS_SCALED};
// decim4_tile_kernel: /4, four outputs per lane, tiles of 256 outputs
static const PlanForm FORM_TILE4 = {"decim4_tile_kernel", GEOM_TILE, 256, 64, 1, 2, false, 16, 8, TAPS_SCALED};
// decim_dense_kernel: /16, /32, the linear-image form, 4096 / ratio outputs per tile of four waves (a 10 KiB LDS image per wave
// while the 31-row halo stays a small part of the staging); LDS is what limits the residents: 2
static const PlanForm FORM_DENSE = {"decim_dense_kernel", GEOM_MULTI, TILE_DENSE, 256, 1, 4, true, 8, 2, TAPS_SCALED};
// ... and /8: its scalar-tap form, the tap subsets on the four waves (round 4: 4.4-5 % less time)
static const PlanForm FORM_DENSE_SUBSET = {"decim_dense_kernel", GEOM_MULTI, TILE_DENSE, 256, 1, 4, false, 8, 2, TAPS_SUBSET8};
// decim_blocks_kernel: /48, /96, sixteen-column blocks of whole input lines under the rotated contract, tiles of 512 outputs
static const PlanForm FORM_BLOCKS = {"decim_blocks_kernel", GEOM_MULTI, 512, 256, 1, 4, false, 8, 2, TAPS_BLOCKS16};
// interp8_pass_kernel on CF32 / S32 words: 64 x inputs per lane -- x4 four inputs per lane and two passes, x8 two and four ...
static const PlanForm FORM_IPASS = {"interp8_pass_kernel", GEOM_IPASS, TILE_IPASS, 64, 1, 2, false, 8, 16, TAPS_PASS8};
// ... x16 .. x96 over ratio / 16 phase blocks of sixteen per tile, walked or (x32, x48, x96: ipass_split) dealt
static const PlanForm FORM_IPASS_BLOCKS = {"interp8_pass_kernel", GEOM_IPASS, TILE_IPASS, 64, 1, 2, true, 8, 16, TAPS_PASS8};
// interp_tile_kernel on CF16 storage: InterpTile<L>::TILE_IN inputs per tile; its 16 waves per CU are the measured figure, not asked
// of the runtime ...
static const PlanForm FORM_ITILE = {"interp_tile_kernel", GEOM_ITILE, TILE_ITILE, 64, 1, 2, false, 4, 16, TAPS_SCALED};
// ... x48 as three phase blocks of its x16 form, x96 of its x32 form (two whole lines per input and block)
static const PlanForm FORM_ITILE_BLOCKS = {"interp_tile_kernel", GEOM_ITILE, TILE_ITILE, 64, 1, 2, false, 2, 16, TAPS_SCALED};
// (FORM_MIX, FORM_IMIX: the label names the mixer INSTANCE of the shared kernel -- decim4_cx_kernel<MixTileArgs>,
// interp_cx_pass_kernel<QI, LL, InterpMixTileArgs> -- as sxfir_launch_geometry has reported it since the translating plans came)
// decim4_cx_kernel: complex taps, /4 x 128 on CF32, on the wide kernel's frame
static const PlanForm FORM_CX = {"decim4_cx_kernel", GEOM_CX, 512, 64, 1, 2, true, 16, 8, TAPS_NONE};
// decim4_cx_kernel<MixTileArgs>: translating plans, /4 x 128 complex taps on CF32: the complex-tap instance's tile, threads, start rule (an output
// boundary, which at /4 is a stream position that is a multiple of 4: decim_geom), store rule and generations
static const PlanForm FORM_MIX = {"decim4_mix_kernel", GEOM_MIX, 512, 64, 1, 2, true, 16, 8, TAPS_NONE};
// decim4_bank_kernel: bank plans, /4 x 128 complex taps per band on CF32: the translating instance's tile, threads, start rule, store rule
// (a band's row is stored like a channel's: stores_aligned) and generations; 19 584 B of LDS per wave leave its 8 waves per CU
static const PlanForm FORM_BANK = {"decim4_bank_kernel", GEOM_BANK, 512, 64, 1, 2, true, 16, 8, TAPS_NONE};
// interp_cx_pass_kernel: complex taps, x4 x 128 and x8 x 256 on CF32, on the pass kernel's frame and with its tiles and generations;
// a small call keeps four tiles per workgroup as the other complex-tap and band kernels' do (a tile is twice the pass kernel's work)
static const PlanForm FORM_ICX = {"interp_cx_pass_kernel", GEOM_ICX, TILE_IPASS, 64, 1, 2, true, 8, 8, TAPS_PASS8_CX};
// interp_cx_pass_kernel<.., InterpMixTileArgs>: translating interpolators, x4 x 128 and x8 x 256 complex taps on CF32: the complex-tap instances' tile, threads,
// start rule (any start), store rule, generations and tap tables
static const PlanForm FORM_IMIX = {"interp_mix_pass_kernel", GEOM_IMIX, TILE_IPASS, 64, 1, 2, true, 8, 8, TAPS_PASS8_CX};
// interp4_bank_kernel: combiner plans, x4 x 128 complex taps per band on CF32: the translating instance's tile, threads, start rule (any start),
// store rule and generations; every band's two pass-major tables, band after band
static const PlanForm FORM_BANK_TX = {"interp4_bank_kernel", GEOM_BANK_TX, TILE_IPASS, 64, 1, 2, true, 8, 8, TAPS_PASS8_CX};

// resample45_kernel: rational 4/5 x 128 on CF32, tiles of Resample45::TILE_IN = 1280 inputs (256 periods of five), one wave per tile; a
// call starts on a period (a stream position that is a multiple of 5).  Its prologue is light (the taps are re-loaded per tile), so a
// small call spreads over the chip; generations and occupancy: tools/ratbench.py, profiles/rational.txt
static const PlanForm FORM_RAT45 = {"resample45_kernel", GEOM_RAT45, sxfir::Resample45::TILE_IN, 64, 5, 2, false, 16, 8, TAPS_NONE};

// resample_arb_kernel: arbitrary-rate plans, 128 phases x 32 taps on CF32, tiles of 256 OUTPUTS, one wave per tile, four waves (one
// workgroup) around one tap table in LDS; any start.  Which calls it takes: arb_geom (sxfir_launch.hip.h).  Its prologue is heavy (18 KiB
// of taps into LDS per workgroup), so a small call keeps four workgroup-sized units per workgroup.  Four generations were not swept
// against other figures; occupancy 4 is what 36 KiB of LDS per workgroup leaves (tools/arbbench.py, profiles/arbitrary.txt)
static const PlanForm FORM_ARB = {"resample_arb_kernel", GEOM_ARB, sxfir::ArbTile::TILE, 256, 1, 2, true, 4, 4, TAPS_ARB};

// The ratio whose kernel a tile of interp_tile_kernel runs: x48 is three phase blocks of the x16 kernel, x96 three of the x32 kernel
static int itile_base(int ratio) { return ratio > 32 ? ratio / 3 : ratio; }

static int form_tile(const PlanForm *f, int ratio)
{
    switch (f->tile) {
    case TILE_DENSE: return 4096 / ratio;
    case TILE_IPASS: return 64 * (ratio == 4 ? 4 : 2);
    case TILE_ITILE: return 2048 / itile_base(ratio);          // InterpTile<L>::TILE_IN = 4 * 4 * (32 / (L / 4))
    }
    return f->tile;
}

// Which form a real-tap shape gets: DESIGN.md 5's table, row by row.  Everything it does not name -- any other ratio, any
// taps_per_phase but 32 -- runs the generic kernels (null).
static const PlanForm *settle_form(int mode, int ratio, int ntaps, int fmt, bool symmetric)
{
    const bool cf16 = fmt == SXFIR_CF16;
    if (mode == SXFIR_DECIMATE && ratio == 4 && ntaps == 64) return fmt == SXFIR_CF32 ? &FORM_TILE4 : nullptr;
    if (ntaps != 32 * ratio) return nullptr;
    if (mode == SXFIR_INTERPOLATE) {
        // CF32 / S32 words: the scalar-tap pass kernel at every ratio (x16 .. x96, round 5: 8-9 % less time than interp_tile_kernel,
        // which keeps CF16 storage: typed LDS-DMA in, half pairs out)
        switch (ratio) {
        case 4: case 8: return cf16 ? &FORM_ITILE : &FORM_IPASS;
        case 16: case 32: return cf16 ? &FORM_ITILE : &FORM_IPASS_BLOCKS;
        case 48: case 96: return cf16 ? &FORM_ITILE_BLOCKS : &FORM_IPASS_BLOCKS;
        }
        return nullptr;
    }
    switch (ratio) {
    // /4 x 128: the wide kernel for bit-symmetric taps and, its ASYM form, for CF16 storage whatever the taps (wide_kernel); else
    // the four-outputs-per-lane kernel
    case 4: return symmetric || cf16 ? &FORM_WIDE : &FORM_TILE4;
    case 8: return &FORM_DENSE_SUBSET;
    case 16: case 32: return &FORM_DENSE;
    case 48: case 96: return &FORM_BLOCKS;             // (the reference's rates master clock / 768 and / 1536)
    }
    return nullptr;
}

// The plan's form: its tile at the plan's ratio, its generations per launch and its default occupancy
static void set_form(sxfir_plan *p, const PlanForm *f)
{
    p->form = f;
    if (!f) return;
    p->tile = form_tile(f, p->ratio);
    p->oversub = f->generations;
    p->occ = f->occ;
}

// The plan's kernels, from its kind and its form: the generic kernel every plan has, and the form's tiled instance(s)
static void resolve_kernels(sxfir_plan *p)
{
    KernelTable &k = p->k;
    k = KernelTable{};
    const GenericKernel g = generic_kernel(p->kind, p->oversample, p->mode, p->fmt);
    k.generic_name = g.name;
    k.generic = g.fn;
    if (p->kind == KIND_BANK) k.bank_generic = bank_generic_kernel(p->fmt);
    if (p->kind == KIND_BANK_TX) k.bank_tx_generic = bank_tx_generic_kernel(p->fmt);
    if (p->mix_den) {           // a translating plan's generic kernel has an argument struct of its own
        // (RX: the label of decim_cx_generic_kernel's mixer instances)
        k.generic_name = p->mode == SXFIR_DECIMATE ? "decim_mix_generic_kernel" : "interp_mix_generic_kernel";
        k.generic = nullptr;
        k.mix_generic = mix_generic_kernel(p->mode, p->fmt);
    }
    switch (p->form ? p->form->geom : GEOM_GENERIC) {
    case GEOM_CHAN4: k.chan4 = sxfir::chan4_kernel; break;
    case GEOM_CHAN4X2: k.chan4x2 = sxfir::chan4x2_kernel; break;
    case GEOM_SYN4: k.syn4 = sxfir::synthesis4_kernel; break;
    case GEOM_SYN4X2: k.syn4x2 = sxfir::synthesis4x2_kernel; break;
    case GEOM_RAT45: k.rat45 = sxfir::resample45_kernel; break;
    case GEOM_ARB: k.arb = sxfir::resample_arb_kernel; break;
    case GEOM_CX: k.cx = sxfir::decim4_cx_kernel<sxfir::DecimTileArgs>; break;
    case GEOM_MIX: k.mix = sxfir::decim4_cx_kernel<sxfir::MixTileArgs>; break;
    case GEOM_BANK: k.bank = sxfir::decim4_bank_kernel; break;
    case GEOM_BANK_TX: k.bank_tx = sxfir::interp4_bank_kernel; break;
    case GEOM_ICX: k.interp_cx = interp_cx_kernel<sxfir::InterpTileArgs>(p->ratio); break;
    case GEOM_IMIX: k.imix = interp_cx_kernel<sxfir::InterpMixTileArgs>(p->ratio); break;
    case GEOM_MULTI:
        if (!p->blocks) k.dense = dense_kernel(p->ratio, p->fmt);
        for (int split = 0; split < 2; ++split) k.blocks[split] = blocks_kernel(p->blocks, p->fmt, split != 0);
        break;
    case GEOM_WIDE: k.wide = wide_kernel(p->fmt, p->symmetric); break;
    case GEOM_TILE: k.tile = tile_kernel(p->ntaps, p->fmt); break;
    case GEOM_IPASS:
    case GEOM_ITILE:
        for (int keyed = 0; keyed < 2; ++keyed)
            for (int split = 0; split < 2; ++split) k.interp[keyed][split] = interp_kernel(p->ratio, p->fmt, keyed != 0, split != 0);
        break;
    }
}

// The instance a form's occupancy is asked of: the plan's BASE form (the comment at the head of the kernel table), which is not
// always the instance a call launches.  Null: the form's own figure stands (interp_tile_kernel's 16 was never the runtime's).
static const void *occupancy_instance(const sxfir_plan *p)
{
    const KernelTable &k = p->k;
    switch (p->form ? p->form->geom : GEOM_GENERIC) {
    case GEOM_MULTI: return p->blocks ? (const void *)k.blocks[0] : (const void *)k.dense;
    case GEOM_WIDE: return (const void *)k.wide;
    case GEOM_TILE: return (const void *)tile_kernel(p->ntaps, SXFIR_CF32);
    case GEOM_IPASS: return (const void *)interp_kernel(p->ratio < 16 ? p->ratio : 16, SXFIR_CF32, false, false);
    case GEOM_CX: return (const void *)k.cx;
    case GEOM_MIX: return (const void *)k.mix;
    case GEOM_BANK: return (const void *)k.bank;
    case GEOM_BANK_TX: return (const void *)k.bank_tx;
    case GEOM_ICX: return (const void *)k.interp_cx;
    case GEOM_IMIX: return (const void *)k.imix;
    case GEOM_CHAN4: return (const void *)k.chan4;
    case GEOM_CHAN4X2: return (const void *)k.chan4x2;
    case GEOM_SYN4: return (const void *)k.syn4;
    case GEOM_SYN4X2: return (const void *)k.syn4x2;
    case GEOM_RAT45: return (const void *)k.rat45;
    case GEOM_ARB: return (const void *)k.arb;
    }
    return nullptr;
}

// resident workgroups per CU of a kernel; *occ keeps its default where the runtime has no answer
template <typename Fn>
static void query_occupancy(int *occ, Fn kernel, int threads, size_t dynamic_lds = 0)
{
    int nb = 0;
    if (kernel && hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kernel, threads, dynamic_lds) == hipSuccess && nb > 0) *occ = nb;
}

// What every creator does once its form is settled: the plan's kernels, then the form's occupancy on this device
static void resolve_form(sxfir_plan *p)
{
    resolve_kernels(p);
    if (p->form) query_occupancy(&p->occ, occupancy_instance(p), p->form->threads);
}

#include "sxfir_prof_create.inc"   // the creators' prof_* hooks and the sxfir_debug_* entry points; empty in the production library

// ---- The creation frame.  A creator is: check_create_args, its own refusals, new_plan, its own fields, set_form with the row of
// its shape (or null), resolve_form, plan_to_device.  Every argument error comes before the device is looked at.

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
    p->tap_table = TAPS_NONE;
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

// A rational plan's outputs after `consumed` inputs: ceil(consumed * up / down) -- output m needs input floor(m * down / up).
// (consumed < 2^63 / 4096: every stream position a caller can reach)
static long long rational_produced(const sxfir_plan *p, long long consumed)
{
    return (consumed * p->ratio + p->down - 1) / p->down;
}

// An arbitrary-rate plan's outputs for n_in more inputs, and its time after them: the count rule of include/sxfir_arbitrary.h, through
// the one function that states it
static long long arb_count(const sxfir_plan *p, long long n_in, int64_t *t_index_after, uint32_t *t_frac_after)
{
    uint64_t n_out = 0;
    sxfir::arb_outputs(p->arb_t_index, p->arb_t_frac, p->arb_step, p->consumed, (uint64_t)n_in, &n_out, t_index_after, t_frac_after);
    return (long long)n_out;
}

// The one list of what a plan owns
static void free_plan(sxfir_plan *p)
{
    (void)hipFree(p->taps_dev);
    (void)hipFree(p->taps_scaled_dev);
    (void)hipFree(p->hist_dev);
    (void)hipFree(p->hist_alt);
    (void)hipFree(p->mix_dev);
    for (int k = 0; k < p->bank_n; ++k)                 // (a table shared by several bands: once, at its first band)
        if (std::find(p->bank_w, p->bank_w + k, p->bank_w[k]) == p->bank_w + k) (void)hipFree(p->bank_w[k]);
    (void)hipFree(p->join_partials);
    (void)hipFree(p->join_arrived);
    prof_free(p);
    delete p;
}

static hipError_t upload(float **dev, const float *host, size_t n)
{
    const hipError_t e = hipMalloc((void **)dev, sizeof(float) * n);
    return e != hipSuccess ? e : hipMemcpy(*dev, host, sizeof(float) * n, hipMemcpyHostToDevice);
}

// ---- The second tap table: one function per layout.  S32-word plans fold the wire words' 2^-31 into the taps a scalar-tap kernel reads.
static const float TAPS_2_M31 = 4.656612873077393e-10f;       // 2^-31: exact
static float word_scale(int fmt) { return fmt == SXFIR_S32 ? TAPS_2_M31 : 1.0f; }

// the /4 scalar-tap kernels on S32 words (no other plan's kernel reads it): every tap times 2^-31, in tap order
static void taps_scaled(std::vector<float> &t, const float *taps)
{
    for (size_t k = 0; k < t.size(); ++k) t[k] = taps[k] * TAPS_2_M31;
}

// decim_dense_kernel<8, ..., SUBSET>: subset s = 2c + p at 64 s, (jj, rr) at 4 jj + rr
static void taps_subset8(std::vector<float> &t, const float *taps, int fmt)
{
    for (int c = 0; c < 2; ++c)
        for (int ph = 0; ph < 2; ++ph)
            for (int jj = 0; jj < 16; ++jj)
                for (int rr = 0; rr < 4; ++rr) t[(size_t)(64 * (2 * c + ph) + 4 * jj + rr)] = taps[8 * (16 * ph + jj) + 4 * c + rr] * word_scale(fmt);
}

// decim_blocks_kernel: the taps rotated by `rot` (slot k' holds tap (k' + rot) mod ntaps); block b (columns 16 b .. 16 b + 15) at
// 512 b, subset s = 2c + p at 64 s inside it, (jj, rr) at 4 jj + rr
static void taps_blocks16(std::vector<float> &t, const float *taps, int ratio, int rot, int fmt)
{
    const int ntaps = (int)t.size();
    for (int b = 0; b < ratio / 16; ++b)
        for (int c = 0; c < 4; ++c)
            for (int ph = 0; ph < 2; ++ph)
                for (int jj = 0; jj < 16; ++jj)
                    for (int rr = 0; rr < 4; ++rr) {
                        const int slot = ratio * (16 * ph + jj) + 16 * b + 4 * c + rr;
                        t[(size_t)(512 * b + 64 * (2 * c + ph) + 4 * jj + rr)] = taps[(slot + rot) % ntaps] * word_scale(fmt);
                    }
}

// interp8_pass_kernel: phase block b at 32 ll b, pass (c, p) at 64 (2c + p) inside it, (jj, rr) at 4 jj + rr
static void taps_pass8(std::vector<float> &t, const float *taps, int ratio)
{
    const int ll = ratio >= 16 ? 16 : ratio;            // phases per (block of the) pass kernel
    for (int b = 0; b < ratio / ll; ++b)
        for (int c = 0; c < ll / 4; ++c)                // x8: two phase groups; x4: one; x16 blocks: four
            for (int ph = 0; ph < 2; ++ph)
                for (int jj = 0; jj < 16; ++jj)
                    for (int rr = 0; rr < 4; ++rr) t[(size_t)(32 * ll * b + 64 * (2 * c + ph) + 4 * jj + rr)] = taps[(16 * ph + jj) * ratio + ll * b + 4 * c + rr];
}

// synthesis4_kernel, synthesis4x2_kernel: h[ratio j + r] at jt r + j, jt the taps per phase (oversampled: per output parity)
static void taps_phased(std::vector<float> &t, const float *taps, int ratio)
{
    const int jt = (int)t.size() / ratio;
    for (int r = 0; r < ratio; ++r)
        for (int j = 0; j < jt; ++j) t[(size_t)(jt * r + j)] = taps[ratio * j + r];
}

// interp_cx_pass_kernel: the planar taps a[0, ntaps) then b[0, ntaps), each as taps_pass8 lays it out, a's table then b's
static void taps_pass8_cx(std::vector<float> &t, const float *planar, int ntaps, int ratio)
{
    std::vector<float> half((size_t)ntaps);
    for (int part = 0; part < 2; ++part) {
        taps_pass8(half, planar + (size_t)part * ntaps, ratio);
        std::copy(half.begin(), half.end(), t.begin() + (size_t)part * ntaps);
    }
}

// resample_arb_kernel: row p at (T + 4) p, h[(T - 1 - i) P + p] at i (j descending: ascending window samples), the pad zero; row P
// repeats row 0 (the second chain of the last phase is phase 0, one sample on)
static void taps_arb(std::vector<float> &t, const float *taps, int ntaps, int P)
{
    const int T = ntaps / P, row = T + 4;
    t.assign((size_t)(P + 1) * row, 0.0f);
    for (int p = 0; p <= P; ++p)
        for (int i = 0; i < T; ++i) t[(size_t)p * row + i] = taps[(T - 1 - i) * P + p % P];
}

// p->ntaps floats in the layout p->tap_table names (TAPS_PASS8_CX: twice as many, from the planar complex taps; a combiner plan:
// that for every band, band k's two tables at 2 ntaps k)
static std::vector<float> second_tap_table(const sxfir_plan *p, const float *taps)
{
    const size_t sets = p->kind == KIND_BANK_TX ? (size_t)p->bank_n : 1;
    std::vector<float> t(taps, taps + (p->tap_table == TAPS_PASS8_CX ? 2 * sets : 1) * (size_t)p->ntaps);
    switch (p->tap_table) {
    case TAPS_PASS8_CX:
        for (size_t k = 0; k < sets; ++k) {
            std::vector<float> band(2 * (size_t)p->ntaps);
            taps_pass8_cx(band, taps + 2 * (size_t)p->ntaps * k, p->ntaps, p->ratio);
            std::copy(band.begin(), band.end(), t.begin() + 2 * (size_t)p->ntaps * k);
        }
        break;
    case TAPS_SCALED: taps_scaled(t, taps); break;
    case TAPS_SUBSET8: taps_subset8(t, taps, p->fmt); break;
    case TAPS_BLOCKS16: taps_blocks16(t, taps, p->ratio, p->rot, p->fmt); break;
    case TAPS_PASS8: taps_pass8(t, taps, p->ratio); break;
    case TAPS_PHASED: taps_phased(t, taps, p->ratio); break;
    case TAPS_ARB: taps_arb(t, taps, p->ntaps, p->ratio); break;
    }
    return t;
}

// The plan's device memory: the tap table (`taps`: n_taps floats) and, unless p->tap_table is TAPS_NONE, the second one in that
// layout (from the same `taps`: p->ntaps real taps), the two history buffers, the current one zeroed, and for the block form the
// join scratch -- for calls of at most eight times as many tiles as the chip has workgroup slots unless the creator set another
// figure.  Measured (tools/split_ab.sh, profiles/round6_split_ab.txt): against the walking form the dealt form takes 2.9 x less
// time at 2^22 samples (/96), -39 % at 2^24, -15 % at 2^26 (2731 / 1366 tiles), -6 % at 5.3 x slots and +2 .. +5 % at 10.7 x slots
// (2^28 samples at /96: the walking form keeps a tile's halo in one XCD's L2 and pays one prologue per eight tiles).  Scratch:
// 4096 tiles x blocks x 4 KiB = 48 / 96 MiB per plan.  The last step of every creator: *out is the plan, or the plan is freed.
static int plan_to_device(sxfir_plan **out, sxfir_plan *p, const float *taps, size_t n_taps)
{
    const size_t hist_bytes = sample_bytes(p->fmt) * (size_t)p->hist_len * (size_t)p->nchan;
    hipError_t e = upload(&p->taps_dev, taps, n_taps);
    if (e == hipSuccess && p->tap_table != TAPS_NONE) {
        const std::vector<float> second = second_tap_table(p, taps);
        e = upload(&p->taps_scaled_dev, second.data(), second.size());
    }
    if (e == hipSuccess) e = hipMalloc(&p->hist_dev, hist_bytes);
    if (e == hipSuccess) e = hipMalloc(&p->hist_alt, hist_bytes);
    if (e == hipSuccess) e = hipMemset(p->hist_dev, 0, hist_bytes);
    if (e == hipSuccess && p->mix_den) {                // a translating plan's rotation table
        std::vector<float> w(2 * (size_t)p->mix_den);
        (void)sxfir_design_rotator(p->mix_den, w.data());
        e = upload(&p->mix_dev, w.data(), w.size());
    }
    for (int k = 0; e == hipSuccess && k < p->bank_n; ++k) {      // a bank plan's rotation tables, one per distinct den
        const int *same = std::find(p->bank_den, p->bank_den + k, p->bank_den[k]);
        if (same != p->bank_den + k) {
            p->bank_w[k] = p->bank_w[same - p->bank_den];
            continue;
        }
        std::vector<float> w(2 * (size_t)p->bank_den[k]);
        (void)sxfir_design_rotator(p->bank_den[k], w.data());
        e = upload(&p->bank_w[k], w.data(), w.size());
    }
    if (e == hipSuccess && p->blocks) {
        if (!p->join_tiles) p->join_tiles = 8LL * p->compute_units * p->occ;
        e = hipMalloc(&p->join_partials, (size_t)p->join_tiles * (size_t)p->blocks * 4096);
        if (e == hipSuccess) e = hipMalloc((void **)&p->join_arrived, sizeof(unsigned) * (size_t)p->join_tiles);
        if (e == hipSuccess) e = hipMemset(p->join_arrived, 0, sizeof(unsigned) * (size_t)p->join_tiles);
        if (e == hipSuccess) e = prof_alloc(p);
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
    const PlanForm *form = &BAND_FORMS[syn][oversample == 2];
    p->tap_table = form->taps;                              // (a synthesizer's phase-major table, whether or not its tiled kernel takes the plan)
    if (syn) {
        const int jt = ntaps / ratio;                       // taps per phase (oversampled: per output parity)
        p->hist_len = nbands * ((jt + 1) & ~1);             // per channel: a x ratio interpolator's history for every band, band k's at k * hist_len / 4
        real_tap_contract(p);                               // a phase's sum: the real-tap interpolator's
    } else {
        p->hist_len = ntaps;                                // (a multiple of 4)
        // the numeric contract of a branch sum: one chain per phase, no tree, no rotation
        p->jsplit = 1;
        p->cw = 1;
    }
    set_form(p, fmt == SXFIR_CF32 && ntaps == 128 ? form : nullptr);       // the shape the tiled kernels take
    resolve_form(p);
    return plan_to_device(out, p, taps, (size_t)ntaps);
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
    p->symmetric = true;
    for (int k = 0; k < ntaps / 2; ++k)
        if (memcmp(&taps[k], &taps[ntaps - 1 - k], sizeof(float)) != 0) p->symmetric = false;
    real_tap_contract(p);
    p->hist_len = mode == SXFIR_DECIMATE ? (ntaps + 1) & ~1 : (ntaps / ratio + 1) & ~1;
    set_form(p, settle_form(mode, ratio, ntaps, fmt, p->symmetric));
    p->blocks_split = p->ipass_split = true;
    prof_settle(p);                     // (profiling: the knobs that ask for another form or contract)
    // the layout follows the form the plan will launch, not the shape: a plan whose /8 scalar-tap form was switched off
    // (profiling knobs) keeps the plain table
    p->tap_table = p->form ? p->form->taps : TAPS_SCALED;
    p->blocks = p->tap_table == TAPS_BLOCKS16 ? ratio / 16 : 0;
    resolve_form(p);
    if (int rc = prof_resolved(p)) {    // (profiling: the variants' instances, occupancies and schedules)
        free_plan(p);
        return rc;
    }
    for (int k = 0; k < 64; ++k) p->taps_k[k] = k < ntaps ? taps[k] * word_scale(fmt) : 0.0f;
    return plan_to_device(out, p, taps, (size_t)ntaps);
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
    if (p->kind == KIND_ARBITRARY) {    // t = 0
        p->arb_t_index = 0;
        p->arb_t_frac = 0;
    }
    return SXFIR_OK;
}

int sxfir_set_history(sxfir_plan *p, const void *src_dev, size_t n, size_t stride, void *stream)
{
    if (!p || !src_dev) return fail(SXFIR_EINVAL, "NULL argument");
    if (p->kind == KIND_SYNTHESIZER || p->kind == KIND_BANK_TX)
        return fail(SXFIR_EUNSUPPORTED, "sxfir_set_history has one stride: it cannot name the bands and the channels of a %s plan's input",
                    p->kind == KIND_SYNTHESIZER ? "synthesizer" : "combiner");
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
    if (p->kind == KIND_ARBITRARY && consumed >= (1ll << 62)) return fail(SXFIR_EINVAL, "stream position out of range");
    p->consumed = (long long)consumed;
    if (p->kind == KIND_ARBITRARY) {            // t = consumed * 2^32: the next output on the next input; outputs count from here
        p->arb_t_index = (long long)consumed;
        p->arb_t_frac = 0;
        p->produced = 0;                        // (nothing to count: the rule is arb_outputs', and it starts here)
    } else if (p->kind == KIND_RATIONAL) p->produced = rational_produced(p, p->consumed);
    else p->produced = p->mode == SXFIR_DECIMATE ? ((long long)consumed + p->ratio - 1) / p->ratio
                                                 : (long long)consumed * p->ratio;
    return SXFIR_OK;
}

int sxfir_set_kernel(sxfir_plan *p, int kernel)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (kernel < SXFIR_KERNEL_AUTO || kernel > SXFIR_KERNEL_GENERIC) return fail(SXFIR_EINVAL, "bad kernel id");
    if (kernel == SXFIR_KERNEL_TILED && !p->form)
        return p->kind == KIND_ARBITRARY
                   ? fail(SXFIR_EUNSUPPORTED, "no tiled kernel for ntaps=%d nphases=%d fmt=%d (128 phases x 32 taps on CF32 has one)", p->ntaps, p->ratio, p->fmt)
               : p->kind == KIND_RATIONAL
                   ? fail(SXFIR_EUNSUPPORTED, "no tiled kernel for ntaps=%d up=%d down=%d fmt=%d (4/5 x 128 on CF32 has one)", p->ntaps, p->ratio, p->down, p->fmt)
                   : fail(SXFIR_EUNSUPPORTED, "no tiled kernel for ntaps=%d ratio=%d fmt=%d mode=%d", p->ntaps, p->ratio, p->fmt, p->mode);
    p->kernel = kernel;
    return SXFIR_OK;
}

int sxfir_set_tx_threshold(sxfir_plan *p, float tx_threshold2)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    p->thr2 = tx_threshold2;
    return SXFIR_OK;
}

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
    if (p->kind == KIND_RATIONAL) return rational_produced(p, p->consumed + n_in) - rational_produced(p, p->consumed);
    if (p->kind == KIND_ARBITRARY) {
        int64_t ti;
        uint32_t tf;
        return arb_count(p, n_in, &ti, &tf);
    }
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
