// Launch tables of the profiling build (libsxfir_prof.so, -DSXFIR_PROFILING): kernel A/B variants, ablation modes and
// phase stamps, selected by the SXFIR_* environment knobs (read at plan creation into the plan's ProfKnobs member:
// sxfir_prof_create.inc).  Included by sxfir_launch.hip.h in front of its geometry and launch functions, which call these
// hooks and otherwise read straight through; in libsxfir.so every hook is the empty inline function at the end of this file.
//
// Every prof_launch_* returns 0 when the plan asks for nothing of its kind (the product launch goes on), 1 when it
// has launched the kernel, and a negative SXFIR_E* code on an error.
#ifdef SXFIR_PROFILING

static int prof_oversub_forced() { return getenv("SXFIR_OVERSUB") != nullptr; }              // the knob means what it says

static int prof_sched(const sxfir_plan *p) { return p->prof.sched; }                          // SXFIR_SCHED

// SXFIR_IBLOCK16=1: x96 on CF32 as six phase blocks of the x16 tile kernel instead of three of the x32 one
static int prof_iblock16(const sxfir_plan *p, bool keyed, int base_l)
{
    return (p->ratio == 96 && getenv("SXFIR_IBLOCK16") && atoi(getenv("SXFIR_IBLOCK16")) && !keyed && p->fmt == SXFIR_CF32) ? 16 : base_l;
}

// stamp records for `need` waves of `bytes_per_record` bytes each (kept with the plan, regrown on demand)
static int prof_stamps(sxfir_plan *p, size_t need, size_t bytes_per_record, unsigned long long **out)
{
    if (p->prof.stamps_dev && p->prof.stamps_n < need) { (void)hipFree(p->prof.stamps_dev); p->prof.stamps_dev = nullptr; }
    if (!p->prof.stamps_dev) HIPCHECK(hipMalloc(&p->prof.stamps_dev, bytes_per_record * need));
    p->prof.stamps_n = need;
    *out = (unsigned long long *)p->prof.stamps_dev;
    return SXFIR_OK;
}

// decim_dense_kernel: SXFIR_ABLATE = 1 (memory side alone), 2 (arithmetic alone), 3 (phase stamps); SXFIR_DENSE_NT = 2 / 1 / 0:
// non-temporal loads for all but both halos / all but the next tile's halo / plain staging loads, at every ratio (the product ships 2 at all three ratios: dense_kernel, sxfir_plan.hip.h)
static int prof_launch_dense_ablations(sxfir_plan *p, sxfir::DecimMultiArgs &a, dim3 grid, hipStream_t st)
{
    if (p->fmt == SXFIR_CF16) return 0;                                                  // CF16 storage: the product dispatch (no ablations of it)
    if ((p->form->taps == TAPS_SUBSET8) && p->prof.ablate == 1 && p->fmt != SXFIR_S32) {                      // (ablate 0: the product dispatch launches it)
        sxfir::DecimMultiArgs b = a;
        if (int rc = need_tap_table(p, TAPS_SUBSET8, "decim_dense_kernel<8, SUBSET> (ablation 1)")) return rc;
        b.taps = p->taps_scaled_dev;                              // the subset-major tap table
        hipLaunchKernelGGL((sxfir::decim_dense_kernel<8, 1, false, 2, true>), grid, dim3(256), 0, st, b);
        HIPCHECK(hipGetLastError());
        return 1;
    }
    if (p->prof.dense_hc && p->fmt != SXFIR_S32 && (p->ratio == 32 || p->ratio == 16) && (p->prof.ablate == 0 || p->prof.ablate == 1)) {
        // SXFIR_DENSE_HC=1: halo carry (runs of consecutive tiles per workgroup, the next halo copied inside LDS)
        if (p->ratio == 32 && p->prof.ablate == 0) hipLaunchKernelGGL((sxfir::decim_dense_kernel<32, 0, false, 2, false, true>), grid, dim3(256), 0, st, a);
        else if (p->ratio == 32) hipLaunchKernelGGL((sxfir::decim_dense_kernel<32, 1, false, 2, false, true>), grid, dim3(256), 0, st, a);
        else if (p->prof.ablate == 0) hipLaunchKernelGGL((sxfir::decim_dense_kernel<16, 0, false, 2, false, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((sxfir::decim_dense_kernel<16, 1, false, 2, false, true>), grid, dim3(256), 0, st, a);
        HIPCHECK(hipGetLastError());
        return 1;
    }
    if ((p->form->taps == TAPS_SUBSET8) && p->prof.ablate == 0 && p->prof.dense_nt_set == 0) return 0;
    if (p->fmt == SXFIR_S32 || (p->prof.ablate == 0 && p->prof.dense_nt_set == 0) || p->prof.ablate > 3) return 0;
    if (p->prof.ablate == 3)
        if (int rc = prof_stamps(p, (size_t)grid.x * p->nchan * p->prof.multi_waves, 40, &a.stamps)) return rc;
#define SXFIR_PD(AA, NN) \
    do { \
        if (p->ratio == 8) hipLaunchKernelGGL((sxfir::decim_dense_kernel<8, AA, false, NN>), grid, dim3(256), 0, st, a); \
        else if (p->ratio == 16) hipLaunchKernelGGL((sxfir::decim_dense_kernel<16, AA, false, NN>), grid, dim3(256), 0, st, a); \
        else hipLaunchKernelGGL((sxfir::decim_dense_kernel<32, AA, false, NN>), grid, dim3(256), 0, st, a); \
    } while (0)
    if (p->prof.ablate == 0 && p->prof.dense_nt == 2) SXFIR_PD(0, 2);
    else if (p->prof.ablate == 0 && p->prof.dense_nt) SXFIR_PD(0, 1);
    else if (p->prof.ablate == 0) SXFIR_PD(0, 0);
    else if (p->prof.ablate == 1 && p->prof.dense_nt == 2) SXFIR_PD(1, 2);
    else if (p->prof.ablate == 1 && p->prof.dense_nt) SXFIR_PD(1, 1);
    else if (p->prof.ablate == 1) SXFIR_PD(1, 0);
    else if (p->prof.ablate == 2) SXFIR_PD(2, 0);
    else SXFIR_PD(3, 0);
#undef SXFIR_PD
    HIPCHECK(hipGetLastError());
    return 1;
}

static int prof_launch_multi(sxfir_plan *p, sxfir::DecimMultiArgs &a, dim3 grid, hipStream_t st);

// ... and SXFIR_DENSE_SUBSET=0: the VGPR-tap forms at /8, A/B partners of the scalar-tap form that ships; a plan of the
// multi-column form (FORM_MULTI) launches that kernel
static int prof_launch_dense(sxfir_plan *p, sxfir::DecimMultiArgs &a, dim3 grid, hipStream_t st)
{
    if (p->form == &FORM_MULTI) return prof_launch_multi(p, a, grid, st);
    if (const int pr = prof_launch_dense_ablations(p, a, grid, st)) return pr;
    if (p->ratio != 8 || (p->form->taps == TAPS_SUBSET8)) return 0;
    if (p->fmt == SXFIR_CF16) hipLaunchKernelGGL((sxfir::decim_dense_kernel<8, 0, false, 0, false, false, true>), grid, dim3(256), 0, st, a);
    else if (p->fmt == SXFIR_S32) hipLaunchKernelGGL((sxfir::decim_dense_kernel<8, 0, true, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((sxfir::decim_dense_kernel<8, 0, false, 2>), grid, dim3(256), 0, st, a);
    HIPCHECK(hipGetLastError());
    return 1;
}

// decim_multi_kernel (SXFIR_DENSE=0, SXFIR_MULTI_PS / _W, SXFIR_TILE_VARIANT=mu; no instance in the production library): S32 wire
// words (one instantiation per ratio), the (ratio, waves, CF16, row split) variants and their ablation / stamp builds
static int prof_launch_multi(sxfir_plan *p, sxfir::DecimMultiArgs &a, dim3 grid, hipStream_t st)
{
    const int W = p->prof.multi_waves;
    if (p->fmt == SXFIR_S32) {
        switch (p->ratio) {
        case 8: hipLaunchKernelGGL((sxfir::decim_multi_kernel<8, 4, false, 0, 2, true>), grid, dim3(256), 0, st, a); break;
        case 16: hipLaunchKernelGGL((sxfir::decim_multi_kernel<16, 4, false, 0, 2, true>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 4, false, 0, 2, true>), grid, dim3(256), 0, st, a); break;
        }
        HIPCHECK(hipGetLastError());
        return 1;
    }
    if (p->prof.ablate == 3)
        if (int rc = prof_stamps(p, (size_t)grid.x * p->nchan * W, 40, &a.stamps)) return rc;
    const int key = SXFIR_MULTI_KEY(p->ratio, W, p->fmt == SXFIR_CF16, p->prof.multi_ps) + 100000 * p->prof.ablate;
    switch (key) {
#define SXFIR_X(DD, WW, HH, PP) \
    case SXFIR_MULTI_KEY(DD, WW, HH, PP): hipLaunchKernelGGL((sxfir::decim_multi_kernel<DD, WW, HH, 0, PP>), grid, dim3(64 * WW), 0, st, a); break;
        SXFIR_MULTI_VARIANTS(SXFIR_X)
#undef SXFIR_X
    case 100801: hipLaunchKernelGGL((sxfir::decim_multi_kernel<8, 1, false, 1>), grid, dim3(64), 0, st, a); break;
    case 200801: hipLaunchKernelGGL((sxfir::decim_multi_kernel<8, 1, false, 2>), grid, dim3(64), 0, st, a); break;
    case 100804: hipLaunchKernelGGL((sxfir::decim_multi_kernel<8, 4, false, 1>), grid, dim3(256), 0, st, a); break;
    case 200804: hipLaunchKernelGGL((sxfir::decim_multi_kernel<8, 4, false, 2>), grid, dim3(256), 0, st, a); break;
    case 300804: hipLaunchKernelGGL((sxfir::decim_multi_kernel<8, 4, false, 3>), grid, dim3(256), 0, st, a); break;
    case 103204: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 4, false, 1>), grid, dim3(256), 0, st, a); break;
    case 203204: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 4, false, 2>), grid, dim3(256), 0, st, a); break;
    case 403204: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 4, false, 4>), grid, dim3(256), 0, st, a); break;
    case 503204: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 4, false, 5>), grid, dim3(256), 0, st, a); break;
    case 303204: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 4, false, 3>), grid, dim3(256), 0, st, a); break;
    case 303208: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 8, false, 3>), grid, dim3(512), 0, st, a); break;
    case 313204: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 4, true, 3>), grid, dim3(256), 0, st, a); break;
    case 313208: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 8, true, 3>), grid, dim3(512), 0, st, a); break;
    case 1303208: hipLaunchKernelGGL((sxfir::decim_multi_kernel<32, 8, false, 3, 4>), grid, dim3(512), 0, st, a); break;
    case 300802: hipLaunchKernelGGL((sxfir::decim_multi_kernel<8, 2, false, 3>), grid, dim3(128), 0, st, a); break;
    default: return fail(SXFIR_EUNSUPPORTED, "no multi kernel for ratio %d with %d waves (mode %d)", p->ratio, W, key);
    }
    HIPCHECK(hipGetLastError());
    return 1;
}

// decim_blocks_kernel: the join-drop test hook's two extra argument fields, and the experiments -- /16 and /32 through the block
// form (SXFIR_BLOCKS_SMALL=1, =2 unrotated), round 5's waves by row half (SXFIR_BLOCKS_RP=0), plain staging loads (SXFIR_BLOCKS_NT=0)
static int prof_launch_blocks(sxfir_plan *p, const LaunchGeom &geom, const sxfir::DecimMultiArgs &a, sxfir::DecimBlocksJoin &jn, dim3 grid, hipStream_t st)
{
    jn.shadow = (sxfir::f32x4 *)p->prof.join_shadow;
    jn.drop_blk = p->prof.join_drop;
#define SXFIR_B(...) hipLaunchKernelGGL((sxfir::decim_blocks_kernel<__VA_ARGS__>), grid, dim3(256), 0, st, a, jn)
    const bool cf32 = p->fmt == SXFIR_CF32, split = geom.split > 1;
    if (p->blocks < 3 && !p->rot) {
        if (p->blocks == 1) SXFIR_B(1, false, true, false, false, true, false);
        else SXFIR_B(2, false, true, false, false, true, false);
    } else if (p->blocks < 3) {
        if (p->blocks == 1) SXFIR_B(1, false, true, false, false, true);
        else SXFIR_B(2, false, true, false, false, true);
    } else if (getenv("SXFIR_BLOCKS_RP") && !atoi(getenv("SXFIR_BLOCKS_RP")) && cf32) {
        if (split && p->blocks == 3) SXFIR_B(3, false, true, false, true, false);
        else if (split) SXFIR_B(6, false, true, false, true, false);
        else if (p->blocks == 3) SXFIR_B(3, false, true, false, false, false);
        else SXFIR_B(6, false, true, false, false, false);
    } else if (getenv("SXFIR_BLOCKS_NT") && !atoi(getenv("SXFIR_BLOCKS_NT")) && cf32) {
        if (split && p->blocks == 3) SXFIR_B(3, false, false, false, true, true);
        else if (split) SXFIR_B(6, false, false, false, true, true);
        else if (p->blocks == 3) SXFIR_B(3, false, false, false, false, true);
        else SXFIR_B(6, false, false, false, false, true);
    } else {
        return 0;
    }
#undef SXFIR_B
    HIPCHECK(hipGetLastError());
    return 1;
}

// test hook: the dropped block's values reach the scratch only now, behind the launch that should have read them -- the
// NEXT launch's joiners find them there unless theirs arrive (what a stale hand-off looks like, deterministically)
static int prof_join_drop_copy(sxfir_plan *p, const LaunchGeom &geom, hipStream_t st)
{
    if (p->prof.join_drop >= 0 && geom.split > 1)
        HIPCHECK(hipMemcpy2DAsync((char *)p->join_partials + 4096 * (size_t)p->prof.join_drop, 4096 * (size_t)p->blocks, p->prof.join_shadow, 4096,
                                  4096, (size_t)(geom.n_tiles * p->nchan), hipMemcpyDeviceToDevice, st));
    return SXFIR_OK;
}

// /4: decim4_pair_kernel, decim4_wide_kernel (tiles of 512 outputs) and the (waves per workgroup, option bits) variants
// of decim4_tile2_kernel, each with its own grid
static int prof_launch_tile_variant(sxfir_plan *p, sxfir::DecimTileArgs &a, long long n_out, long long n_tiles, hipStream_t st)
{
    if ((p->prof.pair || p->prof.wide) && p->ntaps == 128) {
        // one workgroup (2 waves / 1 wave) per tile, strided XCD-blocked passes
        const long long n_tiles2 = (n_out + 511) / 512;
        long long G = ((long long)p->compute_units * (p->prof.wide ? p->prof.occ_wide : p->prof.occ_pair) * p->oversub) / p->nchan;
        if (G < 1) G = 1;
        if (G > n_tiles2) G = n_tiles2;
        set_schedule(a, n_tiles2, G, p->prof.sched == 1 ? 2 : p->prof.sched);          // (these kernels make strided passes only)
        dim3 grid((unsigned)G, (unsigned)p->nchan);
        const int abl = p->prof.ablate;
        if (abl == 5)
            if (int rc = prof_stamps(p, (size_t)G * p->nchan * (p->prof.wide ? 1 : 2), 64, &a.stamps)) return rc;
        if (p->prof.wide) {
            // <ABL, S32IN, NB (LDS read-ahead, chunks), NTL (nt staging loads)>; the product launches <0, *, 24, true>
#define SXFIR_W(AA, NB_, NT_) hipLaunchKernelGGL((sxfir::decim4_wide_kernel<AA, false, NB_, NT_>), grid, dim3(64), (size_t)p->prof.lds_pad, st, a)
            const int nbk = p->prof.wide_nb ? p->prof.wide_nb : 8;
            if (p->fmt == SXFIR_S32) hipLaunchKernelGGL((sxfir::decim4_wide_kernel<0, true, 8, false>), grid, dim3(64), 0, st, a);
            else if (abl == 1 && p->prof.wide_nt) SXFIR_W(1, 8, true);
            else if (abl == 1) SXFIR_W(1, 8, false);
            else if (abl == 5 && p->prof.wide_nt) SXFIR_W(5, 24, true);
            else if (abl == 5) SXFIR_W(5, 8, false);
#define SXFIR_WP(POL_) hipLaunchKernelGGL((sxfir::decim4_wide_kernel<0, false, 24, true, false, POL_>), grid, dim3(64), 0, st, a)
            else if (p->prof.wide_pol == 0x100 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x100);   // plain stores
            else if (p->prof.wide_pol == 0x200 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x200);   // sc0 sc1 stores
            else if (p->prof.wide_pol == 0x300 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x300);   // sc0 sc1 nt stores
            else if (p->prof.wide_pol == 0x400 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x400);   // sc1 stores
            else if (p->prof.wide_pol == 0x010 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x010);   // nt sc1 loads
            else if (p->prof.wide_pol == 0x011 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x011);   // nt sc0 sc1 loads
            else if (p->prof.wide_pol == 0x001 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x001);   // nt sc0 loads
            else if (p->prof.wide_pol == 0x310 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x310);
            else if (p->prof.wide_pol == 0x210 && nbk == 24 && p->prof.wide_nt) SXFIR_WP(0x210);
            else if (p->prof.wide_pol) return fail(SXFIR_EUNSUPPORTED, "no wide variant with cache policy 0x%x (wident24 only)", p->prof.wide_pol);
#undef SXFIR_WP
            else if (p->prof.wide_pin && nbk == 24) hipLaunchKernelGGL((sxfir::decim4_wide_kernel<0, false, 24, true, true>), grid, dim3(64), 0, st, a);
            else if (p->prof.wide_pin && nbk == 16) hipLaunchKernelGGL((sxfir::decim4_wide_kernel<0, false, 16, true, true>), grid, dim3(64), 0, st, a);
            else if (p->prof.wide_nt && nbk == 8) SXFIR_W(0, 8, true);
            else if (p->prof.wide_nt && nbk == 12) SXFIR_W(0, 12, true);
            else if (p->prof.wide_nt && nbk == 16) SXFIR_W(0, 16, true);
            else if (p->prof.wide_nt && nbk == 24) SXFIR_W(0, 24, true);
            else if (p->prof.wide_nt && nbk == 32) SXFIR_W(0, 32, true);
            else if (nbk == 2) SXFIR_W(0, 2, false);
            else if (nbk == 4) SXFIR_W(0, 4, false);
            else if (nbk == 12) SXFIR_W(0, 12, false);
            else if (nbk == 16) SXFIR_W(0, 16, false);
            else if (nbk == 24) SXFIR_W(0, 24, false);
            else if (nbk == 8 && !p->prof.wide_nt) SXFIR_W(0, 8, false);
            else return fail(SXFIR_EUNSUPPORTED, "no wide variant nb %d nt %d ablate %d", nbk, (int)p->prof.wide_nt, abl);
#undef SXFIR_W
        }
        else if (p->fmt == SXFIR_S32) hipLaunchKernelGGL((sxfir::decim4_pair_kernel<0, true>), grid, dim3(128), 0, st, a);
        else if (p->prof.pair_xsep && abl == 5) hipLaunchKernelGGL((sxfir::decim4_pair_kernel<5, false, true>), grid, dim3(128), 0, st, a);
        else if (p->prof.pair_xsep) hipLaunchKernelGGL((sxfir::decim4_pair_kernel<0, false, true>), grid, dim3(128), 0, st, a);
        else if (abl == 1) hipLaunchKernelGGL((sxfir::decim4_pair_kernel<1, false>), grid, dim3(128), 0, st, a);
        else if (abl == 5) hipLaunchKernelGGL((sxfir::decim4_pair_kernel<5, false>), grid, dim3(128), 0, st, a);
        else hipLaunchKernelGGL((sxfir::decim4_pair_kernel<0, false>), grid, dim3(128), 0, st, a);
        HIPCHECK(hipGetLastError());
        return 1;
    }
    if (!p->prof.t2_wpg) return 0;
    // decim4_tile2_kernel: G workgroups of t2_wpg waves per channel, wave ww of workgroup b takes tiles
    // (S(b) + i*G)*wpg + ww
    const int wpg = p->prof.t2_wpg;
    const long long n_super = (n_tiles + wpg - 1) / wpg;
    long long G = ((long long)p->compute_units * p->prof.occ_sb * p->oversub / wpg) / p->nchan;
    if (G < 1) G = 1;
    if (G > n_super) G = n_super;
    a.n_tiles = (int)n_tiles;
    a.w8 = (G % 8 == 0) ? (int)(G / 8) : 0;
    a.run_base = a.run_extra = 0;
    if (p->prof.t2_opt & sxfir::T2_HCARRY) {
        // contiguous runs of K tiles per wave, waves numbered in dispatch order
        const long long K = (n_tiles + G * wpg - 1) / (G * wpg);
        G = ((n_tiles + K - 1) / K + wpg - 1) / wpg;          // workgroups that have a tile
        a.run_base = (int)K;
        a.hist_wave = (int)((n_tiles - 1) / K);
    } else {
        const long long last = n_tiles - 1, sup = last / wpg;
        const int t = (int)(sup % G);
        const int bb = (p->prof.sched == 0 && a.w8) ? (t % a.w8) * 8 + t / a.w8 : t;
        a.hist_wave = bb * wpg + (int)(last % wpg);
    }
    const unsigned grid_y = (unsigned)p->nchan;
    a.n_waves = (int)G;
    dim3 grid((unsigned)G, grid_y);
    if (p->prof.ablate == 5)
        if (int rc = prof_stamps(p, (size_t)G * grid_y * wpg, 64, &a.stamps)) return rc;
    switch ((wpg * 100 + p->prof.t2_opt) * 10 + (p->prof.ablate == 1 || p->prof.ablate == 2 || p->prof.ablate == 5 ? p->prof.ablate : 0)) {
#define SXFIR_X(WW, OO) \
    case (WW * 100 + OO) * 10: hipLaunchKernelGGL((sxfir::decim4_tile2_kernel<128, WW, OO>), grid, dim3(64 * WW), p->prof.lds_pad, st, a); break; \
    case (WW * 100 + OO) * 10 + 1: hipLaunchKernelGGL((sxfir::decim4_tile2_kernel<128, WW, OO, 1>), grid, dim3(64 * WW), p->prof.lds_pad, st, a); break;
        SXFIR_TILE2_VARIANTS(SXFIR_X)
#undef SXFIR_X
#define SXFIR_X(WW, OO) \
    case (WW * 100 + OO) * 10 + 5: hipLaunchKernelGGL((sxfir::decim4_tile2_kernel<128, WW, OO, 5>), grid, dim3(64 * WW), p->prof.lds_pad, st, a); break;
        SXFIR_TILE2_STAMPED(SXFIR_X)
#undef SXFIR_X
    default: return fail(SXFIR_EUNSUPPORTED, "no tile2 variant %d:%d ablate %d", wpg, p->prof.t2_opt, p->prof.ablate);
    }
    HIPCHECK(hipGetLastError());
    return 1;
}

// SXFIR_SCHED=3, short tail: the last generation of long waves (one CU-filling set) is replaced by as many one-tile
// waves as it had tiles
static void prof_short_tail(sxfir_plan *p, sxfir::DecimTileArgs &a, long long n_tiles, long long *per_chan)
{
    if (!(p->prof.sched == 3 && p->ntaps == 128 && p->symmetric)) return;
    const long long W = *per_chan, passes = n_tiles / W;
    const long long resident = (long long)p->compute_units * p->prof.occ_sb / p->nchan;
    if (passes >= 2 && n_tiles % W == 0 && W > resident && resident % 8 == 0) {
        const long long glong = W - resident, gshort = resident * passes;
        a.long_waves = (int)glong;
        a.long_tiles = (int)(glong * passes);
        a.long_w8 = (glong % 8 == 0) ? (int)(glong / 8) : 0;
        a.short_w8 = (gshort % 8 == 0) ? (int)(gshort / 8) : 0;
        *per_chan = glong + gshort;
        a.n_waves = (int)*per_chan;
        const int t = (int)(gshort - 1);                       // the last tile's place among the short waves
        a.hist_wave = (int)glong + (a.short_w8 ? (t % a.short_w8) * 8 + t / a.short_w8 : t);
    }
}

// first-generation /4 kernel: its ablation modes (SXFIR_ABLATE, wrong results by design), the in-kernel clock
// diagnostic (11, 12), the double-buffered form and the decim4_sgpr_kernel experiments
static int prof_launch_tile_first_gen(sxfir_plan *p, sxfir::DecimTileArgs &a, dim3 grid, long long per_chan, bool dbuf, hipStream_t st)
{
    if (p->prof.ablate == 11 || p->prof.ablate == 12) {
        // one {cycles, ticks} pair per wave, printed by sxfir_debug_clock()
        if (!p->prof.stamps_dev) HIPCHECK(hipMalloc(&p->prof.stamps_dev, 16 * (size_t)per_chan * p->nchan));
        p->prof.stamps_n = (size_t)per_chan * p->nchan;
        a.stamps = (unsigned long long *)p->prof.stamps_dev;
    }
    if (p->fmt == SXFIR_CF32 && p->ntaps == 128 && (p->prof.sgpr_r || p->prof.ablate != 0 || dbuf)) {
        if (p->prof.sgpr_r == 8) {
            hipLaunchKernelGGL((sxfir::decim4_sgpr_kernel<8>), grid, dim3(64), 0, st, a);
        } else if (p->prof.sgpr_r == 4) {
            hipLaunchKernelGGL((sxfir::decim4_sgpr_kernel<4>), grid, dim3(64), 0, st, a);
        } else if (p->prof.ablate != 0) {
            switch (p->prof.ablate) {
#define SXFIR_X(N) \
            case N: hipLaunchKernelGGL((sxfir::decim4_tile_kernel<128, false, N>), grid, dim3(64), 0, st, a); break;
                SXFIR_TILE_ABLATIONS(SXFIR_X)
#undef SXFIR_X
            default: return fail(SXFIR_EINVAL, "SXFIR_ABLATE=%d is not a profiling mode of the tile kernel", p->prof.ablate);
            }
        } else {
            hipLaunchKernelGGL((sxfir::decim4_tile_kernel<128, true>), grid, dim3(64), 0, st, a);
        }
        HIPCHECK(hipGetLastError());
        return 1;
    }
    if (p->fmt == SXFIR_CF32 && p->ntaps == 64 && dbuf) {
        hipLaunchKernelGGL((sxfir::decim4_tile_kernel<64, true>), grid, dim3(64), 0, st, a);
        HIPCHECK(hipGetLastError());
        return 1;
    }
    return 0;
}

// The /4 hooks in launch order: the pair / wide / tile2 variants, then (4-outputs-per-lane plans only) the short tail, the
// first-generation kernel's modes and "t2s", round 3's shipped form (with one wave per workgroup both kernels take the same
// schedule constants)
static int prof_launch_tile(sxfir_plan *p, const LaunchGeom &geom, sxfir::DecimTileArgs &a, long long n_out, hipStream_t st)
{
    if (p->fmt != SXFIR_CF16)
        if (const int pr = prof_launch_tile_variant(p, a, n_out, (n_out + 255) / 256, st)) return pr;
    if (geom.kind != GEOM_TILE) return 0;
    long long per_chan = geom.groups;
    prof_short_tail(p, a, geom.n_tiles, &per_chan);                                    // SXFIR_SCHED=3
    const dim3 grid((unsigned)per_chan, (unsigned)p->nchan);
    if (const int pr = prof_launch_tile_first_gen(p, a, grid, per_chan, p->prof.tile_dbuf, st)) return pr;
    if (!(p->ntaps == 128 && p->symmetric && p->prof.sched != 1)) return 0;
    if (p->fmt == SXFIR_S32) hipLaunchKernelGGL((sxfir::decim4_tile2_kernel<128, 1, sxfir::T2_SHIPPED, 0, true>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((sxfir::decim4_tile2_kernel<128, 1, sxfir::T2_SHIPPED>), grid, dim3(64), 0, st, a);
    HIPCHECK(hipGetLastError());
    return 1;
}

// Interpolators: the x8 pass kernel with four inputs per lane (SXFIR_IPASS=4) and its vmcnt(0) form (SXFIR_IPASS_WAIT0=1), and
// interp_tile_kernel's CF32 / S32 instances (SXFIR_IPASS=0: the A/B partners of the pass kernels since round 5)
static int prof_launch_interp(sxfir_plan *p, const LaunchGeom &geom, const sxfir::InterpTileArgs &t, dim3 grid, bool key, hipStream_t st)
{
    const bool s32 = p->fmt == SXFIR_S32;
#define SXFIR_I(K_, ...) hipLaunchKernelGGL((sxfir::K_<__VA_ARGS__>), grid, dim3(64), 0, st, t)
    if (geom.kind == GEOM_IPASS) {
        if (p->ratio != 8) return 0;
        if (p->prof.ipass_qi == 4 && s32) return fail(SXFIR_EUNSUPPORTED, "four inputs per lane: CF32 only");
        else if (p->prof.ipass_qi == 4 && key) SXFIR_I(interp8_pass_kernel, 4, true);
        else if (p->prof.ipass_qi == 4) SXFIR_I(interp8_pass_kernel, 4);
        else if (!p->prof.ipass_wait0) return 0;
        else if (s32 && key) SXFIR_I(interp8_pass_kernel, 2, true, true, false);
        else if (s32) SXFIR_I(interp8_pass_kernel, 2, false, true, false);
        else if (key) SXFIR_I(interp8_pass_kernel, 2, true, false, false);
        else SXFIR_I(interp8_pass_kernel, 2, false, false, false);
    } else if (p->fmt == SXFIR_CF16) {
        return 0;
    } else if (geom.phase_blocks == 6) {
        SXFIR_I(interp_tile_kernel, 16, false, false, 96);                            // SXFIR_IBLOCK16=1
    } else {
#define SXFIR_IT(SS, KK) \
        switch (p->ratio) { \
        case 4: SXFIR_I(interp_tile_kernel, 4, SS, KK); break; \
        case 8: SXFIR_I(interp_tile_kernel, 8, SS, KK); break; \
        case 16: SXFIR_I(interp_tile_kernel, 16, SS, KK); break; \
        case 32: SXFIR_I(interp_tile_kernel, 32, SS, KK); break; \
        case 48: SXFIR_I(interp_tile_kernel, 16, SS, KK, 48); break; \
        default: SXFIR_I(interp_tile_kernel, 32, SS, KK, 96); break; \
        }
        if (key && s32) { SXFIR_IT(true, true) }
        else if (key) { SXFIR_IT(false, true) }
        else if (s32) { SXFIR_IT(true, false) }
        else { SXFIR_IT(false, false) }
#undef SXFIR_IT
    }
#undef SXFIR_I
    HIPCHECK(hipGetLastError());
    return 1;
}

#else  // the production library: no hook does anything

static inline int prof_iblock16(const sxfir_plan *, bool, int base_l) { return base_l; }
#define SXFIR_NO_HOOK(NAME) template <typename... A> static inline int NAME(const A &...) { return 0; }
SXFIR_NO_HOOK(prof_oversub_forced)
SXFIR_NO_HOOK(prof_sched)
SXFIR_NO_HOOK(prof_launch_blocks)
SXFIR_NO_HOOK(prof_join_drop_copy)
SXFIR_NO_HOOK(prof_launch_dense)
SXFIR_NO_HOOK(prof_launch_tile)
SXFIR_NO_HOOK(prof_launch_interp)
#undef SXFIR_NO_HOOK

#endif
