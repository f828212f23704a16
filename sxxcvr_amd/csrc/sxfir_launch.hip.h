// Launches of the C ABI: the launch geometry of a call (which kernel family, which grid: call_geom), one builder per argument
// struct, launch_call (the frame of every launch: geometry and grid, the plan's generic kernel or the form's tiled one), and the
// call frame every streaming entry point ends in: stream_call (launch_call, history carry-over, keyed count, position commit)
// behind the entry point's own argument checks -- sxfir_decimate, sxfir_interpolate and sxfir_interpolate_keyed here,
// sxfir_channelize, sxfir_synthesize and sxfir_resample in their own headers.  WHICH instance a plan launches is not decided here:
// its creator resolved it from the kernel table (sxfir_plan.hip.h) into p->k.  The product path reads straight through; what the
// profiling build adds sits behind the prof_* hooks of sxfir_prof_dispatch.inc.  Included by sxfir.hip after sxfir_plan.hip.h.
#pragma once

// A launch that hands taps_scaled_dev to a kernel states which layout that kernel reads; the plan's creator took the layout
// from the plan's form row, so a mismatch means the two sides were changed apart: refuse instead of filtering with
// permuted taps.
static int need_tap_table(const sxfir_plan *p, int layout, const char *kernel)
{
    if (p->tap_table == layout) return SXFIR_OK;
    return fail(SXFIR_EUNSUPPORTED, "internal: %s reads tap table layout %d, the plan carries layout %d", kernel, layout, p->tap_table);
}

// One call's buffers, as the entry points received them
struct CallIO {
    const void *in;
    size_t n_in, in_stride;
    void *out;
    size_t out_stride;
    long long n_out;
    hipStream_t st;
    size_t band_stride;       // channelizer and bank plans (sxfir_channelize, sxfir_decimate_bank): outputs between the bands of a channel; synthesizer and
                              // combiner plans (sxfir_synthesize, sxfir_interpolate_bank): inputs between them; else 0
};

// What the tiled kernels' 16-byte stores need: an aligned output and, between channels, an even stride -- on CF16 storage the
// form's own quantum (whole 16-byte units of halves, a stride of 4, for the dense and block kernels); a channelizer's bands are
// stored like channels: an even band stride too (critically sampled or oversampled), and so are a bank's.  (LDS-DMA sources need no 16-byte alignment
// -- verified on MI355X, tools/probe_unaligned.hip -- and the edge loads go sample by sample: the input's alignment and strides are
// the entry point's business alone.)
static bool stores_aligned(const sxfir_plan *p, const CallIO &c)
{
    const size_t q = p->form && p->fmt == SXFIR_CF16 ? p->form->cf16_stride : 2;
    return (uintptr_t)c.out % 16 == 0 && (p->nchan == 1 || c.out_stride % q == 0) && ((p->kind != KIND_CHANNELIZER && p->kind != KIND_BANK) || c.band_stride % 2 == 0);
}

// Generic path: the next call's history goes to the plan's other buffer (stream_call swaps the two); a synthesizer's and a combiner's, band by band
template <typename T>
static void launch_history_of(sxfir_plan *p, const CallIO &c)
{
    T *next = (T *)p->hist_alt;
    const T *hist = (const T *)p->hist_dev, *in = (const T *)c.in;
    if (p->kind == KIND_SYNTHESIZER) {
        const int hb = p->hist_len / p->bands;
        hipLaunchKernelGGL(sxfir::synthesis_history_kernel<T>, dim3((unsigned)((hb + 255) / 256), (unsigned)p->nchan, (unsigned)p->bands), dim3(256), 0, c.st,
                           next, hist, in, (long long)c.n_in, (long long)c.in_stride, (long long)c.band_stride, hb);
    } else if (p->kind == KIND_BANK_TX) {
        const int hb = p->hist_len / p->bank_n;
        hipLaunchKernelGGL(sxfir::bank_tx_history_kernel<T>, dim3((unsigned)((hb + 255) / 256), (unsigned)p->nchan, (unsigned)p->bank_n), dim3(256), 0, c.st,
                           next, hist, in, (long long)c.n_in, (long long)c.in_stride, (long long)c.band_stride, hb);
    } else {
        hipLaunchKernelGGL(sxfir::history_kernel<T>, dim3((unsigned)((p->hist_len + 255) / 256), (unsigned)p->nchan), dim3(256), 0, c.st,
                           next, hist, in, (long long)c.n_in, (long long)c.in_stride, (long long)p->hist_len, p->hist_len);
    }
}
static int launch_history(sxfir_plan *p, const CallIO &c)
{
    if (p->fmt != SXFIR_CF16) launch_history_of<float2>(p, c);
    else launch_history_of<uint32_t>(p, c);
    HIPCHECK(hipGetLastError());
    return SXFIR_OK;
}
// key: count the input samples [lo, hi) of channel 0 that reach the plan's keying threshold into *counter
struct KeyedRange { unsigned long long *counter; long long lo, hi; };

// Launch an entry of the plan's kernel table.  A null entry is a shape the production library has no instance for (the
// profiling build's hooks launch its A/B partners before this is reached): no product plan gets here with one.
template <typename... P, typename... A>
static int launch(void (*kernel)(P...), dim3 grid, unsigned threads, hipStream_t st, const A &...args)
{
    if (!kernel) return fail(SXFIR_EUNSUPPORTED, "internal: the plan's kernel table has no instance for this launch");
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, st, args...);
    HIPCHECK(hipGetLastError());
    return SXFIR_OK;
}

// Launch geometry of a call: which kernel family, how many tiles, how many workgroups, how many of them the chip holds at
// once.  One statement of it (call_geom) for launch_call and for sxfir_launch_geometry (tools/sizebench.py, the Device's
// log line for plans that fall to the generic kernels).
struct LaunchGeom {
    int kind;                 // GEOM_* (sxfir_plan.hip.h)
    const char *kernel;
    long long tile_out;       // decimator: outputs per tile; interpolator: inputs per tile (generic kernels: 256 threads' items)
    long long tile_samples;   // ... in wideband samples: a decimator's inputs, an interpolator's outputs
    long long n_tiles;        // per channel
    long long groups;         // workgroups per channel (times phase_blocks)
    long long resident;       // workgroups the chip holds at once, all channels
    int split;                // work items per tile ((tile, block) dealing of decim_blocks_kernel), else 1
    int phase_blocks;         // CF16 interpolator tile kernel: workgroups that share a tile, one per phase block (x48, x96: 3), else 1
};

// The strided-pass constants of the /4 kernels: `groups` waves per channel over n_tiles tiles (sched 0: XCD-blocked strided passes,
// 1: one contiguous run per wave, else plain strided passes), worked out here so that a wave's prologue has no integer division
static void set_schedule(sxfir::DecimTileArgs &a, long long n_tiles, long long groups, int sched)
{
    const int W = (int)groups, last = (int)n_tiles - 1;
    a.n_tiles = (int)n_tiles;
    a.n_waves = W;
    a.w8 = (W % 8 == 0) ? W / 8 : 0;
    a.run_base = (int)(n_tiles / W);
    a.run_extra = (int)(n_tiles % W);
    if (sched == 1) {
        a.hist_wave = a.run_base >= 1 ? W - 1 : last;           // owner of the last contiguous run
    } else {
        const int t = last % W;                                  // first tile of the owner's sequence
        a.hist_wave = (sched == 0 && a.w8) ? (t % a.w8) * 8 + t / a.w8 : t;
    }
}

#include "sxfir_prof_dispatch.inc"   // the prof_* hooks: 0 = not mine, 1 = launched, < 0 = error; empty in the production library

// Generations of workgroups per launch.  The plan's figure (8) was measured at 2^28 samples; the calls the API issues are 2^17 ..
// 2^25, and there the kernels whose workgroups pay a heavy prologue per launch (64 taps into VGPRs: decim_dense_kernel<16 / 32>;
// the x16 .. x96 pass kernels' window and lane constants) run 2-3 % faster when a workgroup keeps at least four tiles
// (tools/split_ab.sh: /32 at 2^25 66.7 us with 2 generations, 69.0 with 8; at 2^28 the other way round, 514 against 508): as many
// generations as leave every workgroup four tiles, at least one, at most the plan's.
static long long generations(const sxfir_plan *p, long long n_tiles, long long resident)
{
    if (!p->form->heavy_prologue || prof_oversub_forced()) return p->oversub;
    long long g = n_tiles * p->nchan / (4 * resident);
    if (g < 1) g = 1;
    return g > p->oversub ? p->oversub : g;
}

static long long clamp_groups(long long g, long long n_tiles)
{
    if (g < 1) g = 1;
    return g > n_tiles ? n_tiles : g;
}

// The plan's generic kernel over n items, one per thread, each `samples_per_item` wideband samples: a decimator's outputs and a
// synthesizer's input indexes (ratio samples each), an interpolator's outputs (one)
static LaunchGeom generic_geom(const sxfir_plan *p, long long n, long long samples_per_item)
{
    return LaunchGeom{GEOM_GENERIC, p->k.generic_name, 256, 256 * samples_per_item, (n + 255) / 256, (n + 255) / 256, (long long)p->compute_units * 8, 1, 1};
}

// The plan's form over n outputs (interpolator: inputs) in tiles of `tile`, on the workgroup slots the chip has for it
static void set_tiles(LaunchGeom &g, const sxfir_plan *p, long long n, long long tile)
{
    g.kind = p->form->geom;
    g.kernel = p->form->tiled;
    g.tile_out = tile;
    g.tile_samples = tile * p->ratio;
    g.n_tiles = (n + tile - 1) / tile;
    g.resident = (long long)p->compute_units * p->occ;
}

// Workgroups per channel: the form's generations of resident workgroups (generations(): fewer for a small call of a form with a
// heavy prologue, whose tile is `work_per_tile` units of the rule), at most one per work item
static void set_groups(LaunchGeom &g, const sxfir_plan *p, long long work_per_tile)
{
    g.groups = clamp_groups(g.resident * generations(p, g.n_tiles * work_per_tile, g.resident) / p->nchan, g.n_tiles * g.split) * g.phase_blocks;
}

// samples of this call in front of the first one that completes an output (0: the call starts on an output boundary)
static long long first_offset(const sxfir_plan *p)
{
    const long long D = p->ratio;
    return ((p->consumed + D - 1) / D) * D - p->consumed;
}

// `aligned`: stores_aligned() of the call.  The plan's generic kernel, unless the plan has a form, the call wants it, is aligned,
// starts on an output boundary and at a position the form takes; then the form's tiles, its generations of workgroups, and for
// the block form, while the call's tiles over all channels fit the plan's scratch, (tile, block) items, one workgroup each
// (decim_blocks_kernel<..., SPLIT>).
static LaunchGeom decim_geom(const sxfir_plan *p, long long n_out, long long first, bool aligned)
{
    LaunchGeom g = generic_geom(p, n_out, p->ratio);
    const PlanForm *f = p->form;
    if (!(f && p->kernel != SXFIR_KERNEL_GENERIC && aligned && first == 0 && p->consumed % f->start_multiple == 0)) return g;
    set_tiles(g, p, n_out, p->tile);
    set_groups(g, p, 1);
    if (p->blocks && p->join_partials && p->blocks_split && g.n_tiles * p->nchan <= p->join_tiles) {
        g.split = p->blocks;
        g.groups = g.n_tiles * p->blocks;
    }
    return g;
}

// Interpolators and synthesizers: as decim_geom (every position starts a tile).  interp_tile_kernel's tile is shared by one
// workgroup per phase block (x48, x96: three; six blocks of the x16 kernel -- SXFIR_IBLOCK16=1 in the profiling build -- measured
// 5 % slower, profiles/round5_rates.txt).  The pass form's tile at x16 .. x96 is ratio / 16 phase blocks' work -- generations()
// counts blocks, dealt or walked -- and at x32, x48, x96, while a call has at most four times as many tiles as the chip holds
// waves, (tile, phase block) items are dealt (interp8_pass_kernel<..., PBSPLIT>: an interpolator's phases never meet, so nothing
// is joined).
static LaunchGeom interp_geom(const sxfir_plan *p, long long n_in, bool aligned, bool keyed)
{
    const bool syn = p->kind == KIND_SYNTHESIZER;       // one thread per input index of its generic kernels
    LaunchGeom g = generic_geom(p, syn ? n_in : n_in * p->ratio, syn ? p->ratio : 1);
    const PlanForm *f = p->form;
    if (!(f && p->kernel != SXFIR_KERNEL_GENERIC && aligned)) return g;
    long long tile = p->tile, blocks_per_tile = 1;
    if (f->geom == GEOM_ITILE) {
        const int base_l = prof_iblock16(p, keyed, itile_base(p->ratio));
        g.phase_blocks = p->ratio / base_l;
        tile = 2048 / base_l;
    }
    set_tiles(g, p, n_in, tile);
    if (f->geom == GEOM_IPASS && p->ratio >= 16) {
        blocks_per_tile = p->ratio / 16;
        if (p->ratio > 16 && p->ipass_split && g.n_tiles * p->nchan <= 4 * g.resident) g.split = p->ratio / 16;
    }
    set_groups(g, p, blocks_per_tile);
    return g;
}

// Rational plans: one thread per output of the generic kernel; the form's tiles (inputs, whole periods of `down`) for a call that
// wants it, is aligned and starts at a position the form takes -- as decim_geom
static LaunchGeom rational_geom(const sxfir_plan *p, long long n_in, long long n_out, bool aligned)
{
    LaunchGeom g = generic_geom(p, n_out, 1);
    const PlanForm *f = p->form;
    if (!(f && p->kernel != SXFIR_KERNEL_GENERIC && aligned && p->consumed % f->start_multiple == 0)) return g;
    set_tiles(g, p, n_in, p->tile);
    g.tile_samples = p->tile;                           // (the wideband side is the input)
    set_groups(g, p, 1);
    return g;
}

// Arbitrary-rate plans: one thread per output of the generic kernel; the form's tiles (256 OUTPUTS, one wave each, four waves per
// workgroup) for a call that wants it, is aligned and whose step lies in the range the tile's image is sized for.  Any start: the
// position is computed, not assumed.
static LaunchGeom arb_geom(const sxfir_plan *p, long long n_out, bool aligned)
{
    LaunchGeom g = generic_geom(p, n_out, 1);
    const PlanForm *f = p->form;
    const bool in_range = p->arb_step >= sxfir::ArbTile::STEP_MIN && p->arb_step <= sxfir::ArbTile::STEP_MAX;
    if (!(f && p->kernel != SXFIR_KERNEL_GENERIC && aligned && in_range)) return g;
    set_tiles(g, p, n_out, p->tile);
    g.tile_samples = p->tile;                           // (outputs: the input span of a tile depends on the step)
    // a workgroup's four waves take a tile each and pay for the tap table once: the generations rule counts workgroup-sized units
    const long long units = (g.n_tiles + sxfir::ArbTile::WAVES - 1) / sxfir::ArbTile::WAVES;
    g.groups = clamp_groups(g.resident * generations(p, units, g.resident) / p->nchan, units);
    return g;
}

// The geometry of a call of n_in samples (per band for a synthesizer), whatever the plan's kind
static LaunchGeom call_geom(const sxfir_plan *p, long long n_in, bool aligned, bool keyed)
{
    if (p->kind == KIND_ARBITRARY) return arb_geom(p, outputs_for(p, n_in), aligned);
    if (p->kind == KIND_RATIONAL) return rational_geom(p, n_in, outputs_for(p, n_in), aligned);
    if (p->mode == SXFIR_DECIMATE) return decim_geom(p, outputs_for(p, n_in), first_offset(p), aligned);
    return interp_geom(p, n_in, aligned, keyed);
}

// An arbitrary-rate plan's time relative to the call, Q32.32: t - (consumed - 1) * 2^32 >= 0 (the absolute 64.32 time stays on the
// host).  A call that yields an output has t below (consumed + n_in - 1) * 2^32, so the difference fits 64 bits for every call of
// fewer than 2^31 inputs -- the bound both entry points set in front of either kernel (check_arbitrary_io); a plan placed further
// ahead yields no output and launches nothing.
static unsigned long long arb_rel(const sxfir_plan *p)
{
    return ((unsigned long long)(p->arb_t_index - (p->consumed - 1)) << 32) | p->arb_t_frac;
}

// ---- one builder per argument struct (value-initialised: what a kernel does not read is zero)
// The one argument struct of every generic kernel.  `first`: a decimator's first_offset (the call's sample index of output 0's
// newest sample); 0 for every other plan.
static sxfir::GenericArgs generic_args(const sxfir_plan *p, const CallIO &c, long long first)
{
    sxfir::GenericArgs a{};
    a.in = c.in;
    a.hist = p->hist_dev;
    a.out = c.out;
    a.taps = p->taps_dev;                           // (complex taps: a[0, ntaps) then b[0, ntaps))
    a.n_in = (long long)c.n_in;
    a.n_out = c.n_out;
    a.in_stride = (long long)c.in_stride;
    a.out_stride = (long long)c.out_stride;
    a.hist_stride = p->hist_len;
    a.first = first;
    a.ntaps = p->ntaps;
    a.ratio = p->ratio;
    a.hist_len = p->hist_len;
    a.jsplit = p->jsplit;
    a.cw = p->cw;
    a.rot = p->rot;                                 // (0 for every interpolator)
    a.thr2 = p->thr2;
    a.band_stride = (long long)c.band_stride;
    a.consumed = p->consumed;
    a.down = p->down;
    // the absolute index of the call's first item
    if (p->kind == KIND_CHANNELIZER) a.m_first = (p->consumed + first) / p->ratio;     // `first` samples into the call lies that output
    if (p->kind == KIND_SYNTHESIZER) {
        a.m_first = p->consumed;                    // per-band input index
        a.hist_len = p->hist_len / p->bands;        // a band's history; hist_stride stays the channel's
    }
    if (p->kind == KIND_RATIONAL) a.m_first = p->produced;
    if (p->kind == KIND_ARBITRARY) {
        a.arb_rel = arb_rel(p);
        a.arb_step = p->arb_step;
    }
    return a;
}

// arbitrary-rate plans: the tiled kernel's argument struct of sxfir_arb.hip.h
static sxfir::ArbTileArgs arb_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::ArbTileArgs a{};
    a.in = c.in;
    a.hist = p->hist_dev;
    a.out = c.out;
    a.table = p->taps_scaled_dev;                   // the extended phase-major table
    a.n_in = (long long)c.n_in;
    a.n_out = c.n_out;
    a.in_stride = (long long)c.in_stride;
    a.out_stride = (long long)c.out_stride;
    a.hist_stride = p->hist_len;
    a.rel = arb_rel(p);
    a.step = p->arb_step;
    a.hist_len = p->hist_len;
    a.n_tiles = (int)geom.n_tiles;
    a.n_groups = (int)geom.groups;
    return a;
}

static sxfir::DecimMultiArgs decim_multi_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::DecimMultiArgs a{};
    a.in = c.in;
    a.hist = p->hist_dev;
    a.hist_out = p->hist_alt;
    a.out = c.out;
    a.taps = p->taps_dev;
    a.n_in = (long long)c.n_in;
    a.n_out = c.n_out;
    a.in_stride = (long long)c.in_stride;
    a.out_stride = (long long)c.out_stride;
    a.hist_stride = p->hist_len;
    a.n_tiles = (int)geom.n_tiles;
    a.n_groups = (int)geom.groups;
    return a;
}

static sxfir::DecimTileArgs decim_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::DecimTileArgs a{};
    a.in = (const float *)c.in;
    a.hist = (const float *)p->hist_dev;
    a.hist_out = (float *)p->hist_alt;
    a.out = (float *)c.out;
    a.taps = p->taps_dev;                           // (complex taps: a[0, 128) then b[0, 128))
    a.taps_scaled = p->taps_scaled_dev;             // only wire-word plans read it (S32IN ? a.taps_scaled : a.taps)
    memcpy(a.taps_k, p->taps_k, sizeof(a.taps_k));
    a.n_in = (long long)c.n_in;
    a.n_out = c.n_out;
    a.in_stride = (long long)c.in_stride;
    a.out_stride = (long long)c.out_stride;
    a.hist_stride = p->hist_len;
    a.sched = prof_sched(p);                        // (0: XCD-blocked strided passes)
    set_schedule(a, geom.n_tiles, geom.groups, a.sched);
    return a;
}

// channelizer plans, critically sampled and oversampled: the tiled kernels' argument struct of sxfir_chan4.hip.h
static sxfir::ChanTileArgs chan_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::DecimTileArgs s{};
    set_schedule(s, geom.n_tiles, geom.groups, 0);          // always XCD-blocked strided passes
    sxfir::ChanTileArgs a{};
    a.in = (const float *)c.in;
    a.hist = (const float *)p->hist_dev;
    a.hist_out = (float *)p->hist_alt;
    a.out = (float *)c.out;
    a.taps = p->taps_dev;
    a.n_in = (long long)c.n_in;
    a.n_out = c.n_out;
    a.in_stride = (long long)c.in_stride;
    a.out_stride = (long long)c.out_stride;
    a.band_stride = (long long)c.band_stride;
    a.hist_stride = p->hist_len;
    a.n_tiles = s.n_tiles;
    a.n_waves = s.n_waves;
    a.w8 = s.w8;
    a.hist_wave = s.hist_wave;
    return a;
}

// synthesizer plans: the tiled kernel's argument struct of sxfir_synthesis4.hip.h
static sxfir::SynTileArgs syn_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::SynTileArgs a{};
    a.in = (const float *)c.in;
    a.hist = (const float *)p->hist_dev;
    a.hist_out = (float *)p->hist_alt;
    a.out = (float *)c.out;
    a.taps = p->taps_scaled_dev;                    // the phase-major table (2x oversampled: its phases are the two parities)
    a.n_in = (long long)c.n_in;
    a.in_stride = (long long)c.in_stride;
    a.band_stride = (long long)c.band_stride;
    a.out_stride = (long long)c.out_stride;
    a.hist_stride = p->hist_len;
    a.n_tiles = (int)geom.n_tiles;
    a.n_groups = (int)geom.groups;
    return a;
}

// 2x oversampled synthesizer plans: the tiled kernel's argument struct of sxfir_synthesis4x2.hip.h -- the call's first input has
// the absolute per-band index `consumed`
static sxfir::SynOsTileArgs syn_os_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::SynOsTileArgs a{};
    a.s = syn_tile_args(p, c, geom);
    a.par = (int)(p->consumed & 1);
    return a;
}

static sxfir::InterpTileArgs interp_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom, const KeyedRange *key)
{
    sxfir::InterpTileArgs t{};
    t.in = (const float *)c.in;
    t.hist = (const float *)p->hist_dev;
    t.hist_out = (float *)p->hist_alt;
    t.out = (float *)c.out;
    t.taps = geom.kind == GEOM_IPASS || geom.kind == GEOM_ICX || geom.kind == GEOM_IMIX ? p->taps_scaled_dev : p->taps_dev;      // the pass-major table(s)
    t.n_in = (long long)c.n_in;
    t.in_stride = (long long)c.in_stride;
    t.out_stride = (long long)c.out_stride;
    t.hist_stride = p->hist_len;
    t.n_tiles = (int)(geom.n_tiles * geom.split);                              // (PBSPLIT: items)
    t.n_groups = (int)(geom.groups / geom.phase_blocks);
    t.thr2 = p->thr2;
    t.key_counter = key ? key->counter : nullptr;
    t.key_lo = key ? key->lo : 0;
    t.key_hi = key ? key->hi : 0;
    return t;
}

// translating plans (include/sxfir_translate.h, include/sxfir_translate_tx.h).  Item m of the stream -- a decimator's output, an
// interpolator's input -- is turned by table entry (m step) mod den, `step` entries per item: a decimator's mix_s, an interpolator's
// (den - mix_s) mod den.  The call's first item has the absolute index `first` (64 bits); `halo` items in front of it (the tiled
// interpolator's image) reach below 0 at the stream's start: the mathematical modulo.
static sxfir::Mixer mixer_of(const float *w, long long den, long long step, long long first, long long halo)
{
    sxfir::Mixer m{};
    m.w = w;
    m.den = (unsigned)den;
    m.step = (unsigned)step;
    m.phase = (unsigned)((((first - halo) % den + den) % den) * step % den);
    return m;
}
static sxfir::Mixer mixer_of(const sxfir_plan *p, long long step, long long first, long long halo)
{
    return mixer_of(p->mix_dev, p->mix_den, step, first, halo);
}

// the translating plans' generic kernels: a decimator's outputs count from `produced`, an interpolator's inputs from `consumed`
static sxfir::MixGenericArgs mix_generic_args(const sxfir_plan *p, const CallIO &c, long long first)
{
    sxfir::MixGenericArgs a{generic_args(p, c, first)};             // (the plain struct is its base)
    if (p->mode == SXFIR_DECIMATE) {
        a.m_first = p->produced;
        a.mix = mixer_of(p, p->mix_s, p->produced, 0);
    } else {
        a.mix = mixer_of(p, (p->mix_den - p->mix_s) % p->mix_den, p->consumed, 0);
    }
    return a;
}

// ... and for the tiled kernels the steps between lanes, tiles and a wave's tiles, so that their tile loops have no division
static sxfir::MixTileArgs mix_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::MixTileArgs a{decim_tile_args(p, c, geom)};
    a.mix = mixer_of(p, p->mix_s, p->produced, 0);
    const long long den = p->mix_den, s = p->mix_s;
    a.lane_step = (unsigned)(8 * s % den);
    a.tile_step = (unsigned)(p->tile * s % den);
    a.stride_step = (unsigned)((long long)a.n_waves % den * a.tile_step % den);
    return a;
}

// bank plans (include/sxfir_bank.h): every band's mixer by mixer_of's rule at the call's first output (`produced`), and for the tiled
// kernel mix_tile_args' three steps per band (n_waves 0: the generic kernel, which reads the mixer alone)
static void bank_bands(const sxfir_plan *p, sxfir::BankBand (&band)[sxfir::BANK_MAX], long long n_waves)
{
    for (int k = 0; k < p->bank_n; ++k) {
        const long long den = p->bank_den[k], s = p->bank_s[k];
        const sxfir::Mixer m = mixer_of(p->bank_w[k], den, s, p->produced, 0);
        sxfir::BankBand &b = band[k];
        b.w = m.w;
        b.den = m.den;
        b.step = m.step;
        b.phase = m.phase;
        b.lane_step = (unsigned)(8 * s % den);
        b.tile_step = (unsigned)(p->tile * s % den);
        b.stride_step = (unsigned)(n_waves % den * b.tile_step % den);
        b.rden = 1.0f / (float)den;
    }
}

static sxfir::BankGenericArgs bank_generic_args(const sxfir_plan *p, const CallIO &c, long long first)
{
    sxfir::BankGenericArgs a{generic_args(p, c, first)};            // (the plain struct is its base)
    a.m_first = p->produced;
    bank_bands(p, a.band, 0);
    return a;
}

static sxfir::BankTileArgs bank_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::BankTileArgs a{decim_tile_args(p, c, geom)};
    a.band_stride = (long long)c.band_stride;
    a.nbands = p->bank_n;
    bank_bands(p, a.band, a.n_waves);
    return a;
}

// combiner plans (include/sxfir_bank_tx.h): every band's mixer by mixer_of's rule for the translating interpolator at the call's first
// input (`consumed`), `halo` samples in front of it, and for the tiled kernel imix_tile_args' four steps per band (n_groups 0: the
// generic kernel, which reads the mixer alone).  64-bit arithmetic here; every value handed over is below den.
static void bank_tx_bands(const sxfir_plan *p, sxfir::BankTxBand (&band)[sxfir::BANK_MAX], long long halo, long long n_groups)
{
    for (int k = 0; k < p->bank_n; ++k) {
        const long long den = p->bank_den[k], t = (den - p->bank_s[k]) % den;
        const sxfir::Mixer m = mixer_of(p->bank_w[k], den, t, p->consumed, halo);
        sxfir::BankTxBand &b = band[k];
        b.w = m.w;
        b.den = m.den;
        b.step = m.step;
        b.phase = m.phase;
        b.lane_step = (unsigned)(2 * t % den);
        b.instr_step = (unsigned)(128 * t % den);
        b.tile_step = (unsigned)(256 * t % den);
        b.stride_step = (unsigned)(n_groups % den * b.tile_step % den);
    }
}

static sxfir::BankTxGenericArgs bank_tx_generic_args(const sxfir_plan *p, const CallIO &c)
{
    sxfir::BankTxGenericArgs a{generic_args(p, c, 0)};              // (the plain struct is its base)
    a.hist_len = p->hist_len / p->bank_n;                           // a band's history; hist_stride stays the channel's
    a.nbands = p->bank_n;
    bank_tx_bands(p, a.band, 0, 0);
    return a;
}

static sxfir::BankTxTileArgs bank_tx_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::BankTxTileArgs a{interp_tile_args(p, c, geom, nullptr)};
    a.taps = p->taps_scaled_dev;                                    // every band's pass-major tables
    a.band_stride = (long long)c.band_stride;
    a.nbands = p->bank_n;
    // (the image of tile 0 starts InterpPass8::HIST samples in front of the call)
    bank_tx_bands(p, a.band, 32, a.n_groups);
    return a;
}

// the tiled translating interpolators: the steps between the chunks of two lanes, a lane's chunks, tiles and a wave's tiles
static sxfir::InterpMixTileArgs imix_tile_args(const sxfir_plan *p, const CallIO &c, const LaunchGeom &geom)
{
    sxfir::InterpMixTileArgs a{interp_tile_args(p, c, geom, nullptr)};
    // (the image of tile 0 starts InterpPass8::HIST samples in front of the call)
    a.mix = mixer_of(p, (p->mix_den - p->mix_s) % p->mix_den, p->consumed, 32);
    const long long den = p->mix_den, t = a.mix.step;
    a.lane_step = (unsigned)(2 * t % den);
    a.instr_step = (unsigned)(128 * t % den);
    a.tile_step = (unsigned)(p->tile * t % den);
    a.stride_step = (unsigned)((long long)a.n_groups % den * a.tile_step % den);
    return a;
}

// ---- the tiled launches of the families that have checks of their own, called from launch_call's switch

// /8 .. /96 (GEOM_MULTI): decim_dense_kernel or decim_blocks_kernel
static int launch_decim_multi(sxfir_plan *p, const CallIO &c, const LaunchGeom &geom, dim3 grid)
{
    const unsigned threads = (unsigned)p->form->threads;
    sxfir::DecimMultiArgs a = decim_multi_args(p, c, geom);
    if (p->blocks) {
        // sixteen-column blocks, scalar taps from the block-major table of the rotated taps
        if (int rc = need_tap_table(p, TAPS_BLOCKS16, "decim_blocks_kernel")) return rc;
        a.taps = p->taps_scaled_dev;
        sxfir::DecimBlocksJoin jn{};
        jn.partials = (sxfir::f32x4 *)p->join_partials;
        jn.arrived = p->join_arrived;
        const int pr = prof_launch_blocks(p, geom, a, jn, grid, c.st);
        if (pr < 0) return pr;
        if (!pr)
            if (int rc = launch(p->k.blocks[geom.split > 1], grid, threads, c.st, a, jn)) return rc;
        return prof_join_drop_copy(p, geom, c.st);
    }
    // /8, /16, /32: decim_dense_kernel (profiling: its ablations, or the multi-column kernel it replaced)
    if (const int pr = prof_launch_dense(p, a, grid, c.st)) return pr < 0 ? pr : SXFIR_OK;
    if (p->form->taps == TAPS_SUBSET8) {
        if (int rc = need_tap_table(p, TAPS_SUBSET8, p->fmt == SXFIR_CF16 ? "decim_dense_kernel<8, SUBSET, HALFIN>" : "decim_dense_kernel<8, SUBSET>")) return rc;
        a.taps = p->taps_scaled_dev;                      // the subset-major tap table
    }
    return launch(p->k.dense, grid, threads, c.st, a);
}

// /4 (GEOM_CX, GEOM_WIDE, GEOM_TILE): one wave (= one workgroup) per tile and pass
static int launch_decim4(sxfir_plan *p, const CallIO &c, const LaunchGeom &geom, dim3 grid)
{
    const unsigned threads = (unsigned)p->form->threads;
    sxfir::DecimTileArgs a = decim_tile_args(p, c, geom);
    if (geom.kind == GEOM_CX) return launch(p->k.cx, grid, threads, c.st, a);
    if (p->fmt == SXFIR_S32)                               // only wire-word plans read taps_scaled
        if (int rc = need_tap_table(p, TAPS_SCALED, "the /4 scalar-tap kernels on S32 words")) return rc;
    if (p->fmt == SXFIR_CF16 && geom.kind != GEOM_WIDE)
        return fail(SXFIR_EUNSUPPORTED, "CF16 storage at /4 runs the wide kernel only (a profiling knob asked for another /4 variant)");
    if (const int pr = prof_launch_tile(p, geom, a, c.n_out, c.st)) return pr < 0 ? pr : SXFIR_OK;
    return launch(geom.kind == GEOM_WIDE ? p->k.wide : p->k.tile, grid, threads, c.st, a);
}

extern "C" {

// The interpolators (GEOM_IPASS, GEOM_ITILE, GEOM_ICX, GEOM_IMIX)
static int launch_interp_tiled(sxfir_plan *p, const CallIO &c, const LaunchGeom &geom, dim3 grid, const KeyedRange *key, bool *key_pending)
{
    const unsigned threads = (unsigned)p->form->threads;
    if (geom.kind == GEOM_IPASS)
        if (int rc = need_tap_table(p, TAPS_PASS8, "interp8_pass_kernel")) return rc;
    if (geom.n_tiles * geom.split > 0x7fffffffLL) return fail(SXFIR_EINVAL, "call too large");       // (PBSPLIT: items)
    if (geom.kind == GEOM_ICX || geom.kind == GEOM_IMIX) {
        // complex taps, with or without a mixer: no keyed instance -- the count depends on the raw input alone and runs as the
        // generic path's pass of its own
        if (int rc = need_tap_table(p, TAPS_PASS8_CX, p->form->tiled)) return rc;
        if (int rc = geom.kind == GEOM_ICX ? launch(p->k.interp_cx, grid, threads, c.st, interp_tile_args(p, c, geom, nullptr))
                                           : launch(p->k.imix, grid, threads, c.st, imix_tile_args(p, c, geom))) return rc;
        if (key && key->hi > key->lo && key_pending) *key_pending = true;
        return SXFIR_OK;
    }
    if (p->fmt == SXFIR_CF16 && key) return fail(SXFIR_EUNSUPPORTED, "the keying count is defined on CF32 input");
    const sxfir::InterpTileArgs t = interp_tile_args(p, c, geom, key);
    if (const int pr = prof_launch_interp(p, geom, t, grid, key != nullptr, c.st)) return pr < 0 ? pr : SXFIR_OK;
    return launch(p->k.interp[key != nullptr][geom.split > 1], grid, threads, c.st, t);
}

// SXFIR_KERNEL_TILED was asked for and the call falls to the generic kernel: the refusal, in the words of the plan's kind
static int refuse_tiled(const sxfir_plan *p)
{
    if (p->kind == KIND_SYNTHESIZER) return fail(SXFIR_EUNSUPPORTED, "tiled synthesizer needs a 16-byte aligned output and an even output stride");
    if (p->kind == KIND_BANK)
        return fail(SXFIR_EUNSUPPORTED, "tiled bank needs a 16-byte aligned output, an even output stride, an even band stride and a call that "
                                        "starts on an output boundary (a stream position that is a multiple of 4)");
    if (p->kind == KIND_BANK_TX) return fail(SXFIR_EUNSUPPORTED, "tiled combiner needs a 16-byte aligned output and an even output stride");
    if (p->kind == KIND_ARBITRARY)
        return fail(SXFIR_EUNSUPPORTED, "tiled arbitrary-rate resampler needs a 16-byte aligned output, an even output stride and a step in "
                                        "[2^31, 2^33] (step %llu)", (unsigned long long)p->arb_step);
    if (p->kind == KIND_RATIONAL)
        return fail(SXFIR_EUNSUPPORTED, "tiled resampler needs a 16-byte aligned output, an even output stride and a call that starts at a "
                                        "stream position that is a multiple of %d", p->form ? p->form->start_multiple : 1);
    if (p->mode == SXFIR_DECIMATE)
        return fail(SXFIR_EUNSUPPORTED,
                    "tiled kernel needs a 16-byte aligned output, an even output stride and a call that starts on "
                    "an output boundary%s", p->form && p->form->start_multiple == 4 ? " of even index (a stream position that is a multiple of 4)" : "");
    return fail(SXFIR_EUNSUPPORTED, "tiled interpolator needs a 16-byte aligned output and even strides");
}

// Shapes the tiled kernels do not take: the keying count as a pass of its own (same rule, same counter).  Queued by
// stream_call AFTER the history launch has succeeded, with the position commit: a call that fails half way has not
// touched the counter, so a caller that retries the block does not count it twice (on the tiled paths the count is part of
// the one kernel launch).
static int launch_keyed_count(sxfir_plan *p, const void *in_dev, const KeyedRange *key, hipStream_t st)
{
    const long long n = key->hi - key->lo;
    unsigned g = (unsigned)std::min<long long>((n + 255) / 256, 256);
    hipLaunchKernelGGL(sxfir::count_keyed_kernel, dim3(g), dim3(256), 0, st,
                       reinterpret_cast<const float2 *>(in_dev) + key->lo, n, p->thr2, key->counter);
    HIPCHECK(hipGetLastError());
    return SXFIR_OK;
}

// The resampling kernel of a call alone (no history pass, no position change): what stream_call launches and sxfir_time_* repeats.
// The frame of every plan kind: geometry and grid; the plan's generic kernel; else the form's tiled kernel.  *history_done: the
// kernel writes the next call's history to hist_alt (every tiled kernel does; the caller swaps hist_dev / hist_alt when it
// commits the call).  *key_pending: the keying count is still to be queued, as a pass of its own (launch_keyed_count).
static int launch_call(sxfir_plan *p, const CallIO &c, bool *history_done, const KeyedRange *key = nullptr, bool *key_pending = nullptr)
{
    *history_done = false;
    const LaunchGeom geom = call_geom(p, (long long)c.n_in, stores_aligned(p, c), key != nullptr);
    const dim3 grid((unsigned)geom.groups, (unsigned)p->nchan);
    if (geom.kind == GEOM_GENERIC) {
        if (p->kernel == SXFIR_KERNEL_TILED) return refuse_tiled(p);
        const long long first = p->mode == SXFIR_DECIMATE ? first_offset(p) : 0;        // (a rational plan is an interpolator)
        if (p->kind == KIND_BANK)       // a band per grid plane
            return launch(p->k.bank_generic, dim3(grid.x, grid.y, (unsigned)p->bank_n), 256, c.st, bank_generic_args(p, c, first));
        if (p->kind == KIND_BANK_TX)    // the bands inside the thread: they meet in one output word
            return launch(p->k.bank_tx_generic, grid, 256, c.st, bank_tx_generic_args(p, c));
        if (int rc = !p->mix_den ? launch(p->k.generic, grid, 256, c.st, generic_args(p, c, first))
                                 : launch(p->k.mix_generic, grid, 256, c.st, mix_generic_args(p, c, first))) return rc;
        if (key && key->hi > key->lo && key_pending) *key_pending = true;    // counted by the caller once the call is certain to commit
        return SXFIR_OK;
    }
    if (geom.n_tiles > 0x7fffffffLL) return fail(SXFIR_EINVAL, "call too large");
    *history_done = true;
    const unsigned threads = (unsigned)p->form->threads;
    switch (geom.kind) {
    case GEOM_CHAN4: return launch(p->k.chan4, grid, threads, c.st, chan_tile_args(p, c, geom));
    case GEOM_CHAN4X2: return launch(p->k.chan4x2, grid, threads, c.st, chan_tile_args(p, c, geom));
    case GEOM_SYN4:
    case GEOM_SYN4X2:
        if (int rc = need_tap_table(p, TAPS_PHASED, p->form->tiled)) return rc;
        if (geom.kind == GEOM_SYN4X2) return launch(p->k.syn4x2, grid, threads, c.st, syn_os_tile_args(p, c, geom));
        return launch(p->k.syn4, grid, threads, c.st, syn_tile_args(p, c, geom));
    // resample45_kernel stands on the /4 kernels' argument struct and schedule (decim_tile_args: XCD-blocked strided passes, the
    // last tile's wave carries the history over)
    case GEOM_RAT45: return launch(p->k.rat45, grid, threads, c.st, decim_tile_args(p, c, geom));
    case GEOM_MIX: return launch(p->k.mix, grid, threads, c.st, mix_tile_args(p, c, geom));
    case GEOM_BANK: return launch(p->k.bank, grid, threads, c.st, bank_tile_args(p, c, geom));
    case GEOM_BANK_TX:
        if (int rc = need_tap_table(p, TAPS_PASS8_CX, p->form->tiled)) return rc;
        return launch(p->k.bank_tx, grid, threads, c.st, bank_tx_tile_args(p, c, geom));
    // resample_arb_kernel leaves the history to the generic path's pass (history_kernel)
    case GEOM_ARB:
        *history_done = false;
        if (int rc = need_tap_table(p, TAPS_ARB, p->form->tiled)) return rc;
        return launch(p->k.arb, grid, threads, c.st, arb_tile_args(p, c, geom));
    case GEOM_IPASS:
    case GEOM_ITILE:
    case GEOM_ICX:
    case GEOM_IMIX: return launch_interp_tiled(p, c, geom, grid, key, key_pending);
    case GEOM_MULTI: return launch_decim_multi(p, c, geom, grid);
    }
    return launch_decim4(p, c, geom, grid);
}

// Everything behind an entry point's argument checks (which have set *n_out_p to 0).  A call that fails changes nothing: the
// history buffers are swapped and the positions advanced once every launch is queued.
static int stream_call(sxfir_plan *p, const CallIO &c, size_t *n_out_p, const KeyedRange *key = nullptr)
{
    if (c.n_in == 0) return SXFIR_OK;
    HIPCHECK(hipSetDevice(p->device));
    bool history_done = false, key_pending = false;
    if (c.n_out > 0) {                  // (a decimator call that completes no output only carries its samples into the history)
        const int rc = launch_call(p, c, &history_done, key, &key_pending);
        // a (tile, block) launch that failed may have left arrival counters half way: the next launch starts from zero again
        if (rc == SXFIR_EHIP && p->join_arrived)
            (void)hipMemsetAsync(p->join_arrived, 0, sizeof(unsigned) * (size_t)p->join_tiles, c.st);
        if (rc) return rc;
    }
    if (!history_done)
        if (int rc = launch_history(p, c)) return rc;
    if (key_pending)
        if (int rc = launch_keyed_count(p, c.in, key, c.st)) return rc;
    std::swap(p->hist_dev, p->hist_alt);
    if (p->kind == KIND_ARBITRARY) {                // the time after the call's outputs, by the rule that counted them
        int64_t ti;
        uint32_t tf;
        (void)arb_count(p, (long long)c.n_in, &ti, &tf);
        p->arb_t_index = ti;
        p->arb_t_frac = tf;
    }
    p->consumed += (long long)c.n_in;
    p->produced += c.n_out;
    if (n_out_p) *n_out_p = (size_t)c.n_out;
    return SXFIR_OK;
}

// Two strides name a band plan's bands and channels (`side`: "in" / "out", the side that has bands): a channel's bands in a row,
// channel after channel -- or a band's channels in a row, band after band
static int check_band_layout(const sxfir_plan *p, const char *side, size_t chan_stride, size_t band_stride, size_t n)
{
    const size_t nb = (size_t)p->bands, nc = (size_t)p->nchan;
    const bool bands_inside = chan_stride >= (nb - 1) * band_stride + n;
    const bool channels_inside = chan_stride >= n && band_stride >= (nc - 1) * chan_stride + n;
    if (nc == 1 || bands_inside || channels_inside) return SXFIR_OK;
    return fail(SXFIR_EINVAL, "bands and channels overlap (%s_stride %zu, band_stride %zu, %zu %sputs per band)", side, chan_stride, band_stride, n, side);
}

// One input and one output buffer per channel: real and complex taps, rational plans
static int check_buffers(const sxfir_plan *p, const CallIO &c)
{
    if ((c.n_in && !c.in) || (c.n_out > 0 && !c.out)) return fail(SXFIR_EINVAL, "NULL device buffer");
    if (p->nchan > 1 && (c.in_stride < c.n_in || c.out_stride < (size_t)c.n_out))
        return fail(SXFIR_EINVAL, "channel stride smaller than the block");
    if ((uintptr_t)c.in % sample_bytes(p->fmt) || (uintptr_t)c.out % sample_bytes(p->fmt))
        return fail(SXFIR_EINVAL, "buffers must be aligned to one complex sample");
    return SXFIR_OK;
}

static const char *const RATIONAL_TAKES = "a rational plan takes sxfir_resample (include/sxfir_rational.h)";
static const char *const BANK_TX_TAKES = "a combiner plan takes sxfir_interpolate_bank (include/sxfir_bank_tx.h)";
static const char *const ARBITRARY_TAKES = "an arbitrary-rate plan takes sxfir_resample_arbitrary (include/sxfir_arbitrary.h)";

// sxfir_decimate, sxfir_interpolate and sxfir_time_*: real and complex taps
static int check_io(const sxfir_plan *p, int mode, const CallIO &c)
{
    if (p->kind == KIND_RATIONAL) return fail(SXFIR_EINVAL, "%s", RATIONAL_TAKES);
    if (p->kind == KIND_ARBITRARY) return fail(SXFIR_EINVAL, "%s", ARBITRARY_TAKES);
    if (p->kind == KIND_SYNTHESIZER) return fail(SXFIR_EINVAL, "a synthesizer plan takes sxfir_synthesize (include/sxfir_synthesizer.h)");
    if (p->kind == KIND_BANK) return fail(SXFIR_EINVAL, "a bank plan takes sxfir_decimate_bank (include/sxfir_bank.h)");
    if (p->kind == KIND_BANK_TX) return fail(SXFIR_EINVAL, "%s", BANK_TX_TAKES);
    if (p->mode != mode) return fail(SXFIR_EINVAL, "plan was created for the other direction");
    if (p->kind == KIND_CHANNELIZER) return fail(SXFIR_EINVAL, "a channelizer plan takes sxfir_channelize (include/sxfir_channelizer.h)");
    return check_buffers(p, c);
}

static int resample(sxfir_plan *p, int mode, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                    size_t *n_out_p, void *stream, const KeyedRange *key)
{
    if (n_out_p) *n_out_p = 0;
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    const CallIO c{in_dev, n_in, in_stride, out_dev, out_stride, outputs_for(p, (long long)n_in), S(stream)};
    if (int rc = check_io(p, mode, c)) return rc;
    return stream_call(p, c, n_out_p, key);
}

int sxfir_decimate(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev,
                   size_t out_stride, size_t *n_out_p, void *stream)
{
    return resample(p, SXFIR_DECIMATE, in_dev, n_in, in_stride, out_dev, out_stride, n_out_p, stream, nullptr);
}

int sxfir_interpolate(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev,
                      size_t out_stride, size_t *n_out_p, void *stream)
{
    return resample(p, SXFIR_INTERPOLATE, in_dev, n_in, in_stride, out_dev, out_stride, n_out_p, stream, nullptr);
}

int sxfir_interpolate_keyed(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev,
                            size_t out_stride, size_t *n_out_p, size_t key_first, size_t key_count,
                            unsigned long long *counter, void *stream)
{
    if (n_out_p) *n_out_p = 0;
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (p->kind == KIND_RATIONAL) return fail(SXFIR_EINVAL, "%s", RATIONAL_TAKES);
    if (p->kind == KIND_ARBITRARY) return fail(SXFIR_EINVAL, "%s", ARBITRARY_TAKES);
    if (p->kind == KIND_SYNTHESIZER) return fail(SXFIR_EINVAL, "a synthesizer plan takes sxfir_synthesize (include/sxfir_synthesizer.h): no keying count in its version 1");
    if (p->kind == KIND_BANK_TX) return fail(SXFIR_EINVAL, "%s: no keying count in its version 1", BANK_TX_TAKES);
    if (p->mode != SXFIR_INTERPOLATE) return fail(SXFIR_EINVAL, "not an interpolator plan");
    if (p->fmt == SXFIR_CF16) return fail(SXFIR_EUNSUPPORTED, "the keying count is defined on CF32 input");
    if (!counter || ((uintptr_t)counter & 7)) return fail(SXFIR_EINVAL, "counter must be an 8-byte aligned device word");
    if (key_first > n_in || key_count > n_in - key_first) return fail(SXFIR_EINVAL, "keying range outside the block");
    const KeyedRange key{counter, (long long)key_first, (long long)(key_first + key_count)};
    return resample(p, SXFIR_INTERPOLATE, in_dev, n_in, in_stride, out_dev, out_stride, n_out_p, stream, key_count ? &key : nullptr);
}

int sxfir_launch_geometry(const sxfir_plan *p, size_t n_in, sxfir_geometry *out)
{
    if (!p || !out) return fail(SXFIR_EINVAL, "NULL argument");
    memset(out, 0, sizeof(*out));
    const LaunchGeom g = call_geom(p, (long long)n_in, true, false);
    snprintf(out->kernel, sizeof(out->kernel), "%s", g.kernel);
    out->tiled = g.kind != GEOM_GENERIC;
    out->split = g.split;
    out->tile_samples = g.tile_samples;
    out->n_tiles = g.n_tiles;
    out->workgroups = g.groups * p->nchan * (p->kind == KIND_BANK && g.kind == GEOM_GENERIC ? p->bank_n : 1);   // (the bank's generic kernel: a grid plane per band)
    out->resident = g.resident;
    return SXFIR_OK;
}

}  // extern "C"
