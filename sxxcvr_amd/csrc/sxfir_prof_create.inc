// Plan creation in the profiling build (libsxfir_prof.so, -DSXFIR_PROFILING): every SXFIR_* environment knob a creator reads,
// behind two hooks of sxfir_create (sxfir_plan.hip.h) -- prof_settle, behind the product's settle_form and in front of
// resolve_form: the knobs that ask for another form, tile or contract; prof_resolved, behind resolve_form: the variants' own
// instances, occupancies and schedules -- the two hooks of the plan's memory (prof_alloc, prof_free), and the sxfir_debug_* entry
// points (include/sxfir_prof.h).  What the knobs set lives in the plan's ProfKnobs member (sxfir_prof_knobs.inc).  In libsxfir.so
// every hook is the empty inline function at the end of this file: the production library never looks at the environment.
#ifdef SXFIR_PROFILING

// decim_multi_kernel (SXFIR_DENSE=0, SXFIR_MULTI_PS / _W, SXFIR_TILE_VARIANT=mu; no instance in the production library since
// round 5): tiles of waves x 8 x (64 / (row split x ratio / 4)) outputs, set with the knobs (prof_settle)
static const PlanForm FORM_MULTI = {"decim_multi_kernel", GEOM_MULTI, 0, 256, 1, 4, false, 8, 2, TAPS_SCALED};

static int prof_env(const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; }

static void prof_settle(sxfir_plan *p)
{
    ProfKnobs &K = p->prof;
    const int ratio = p->ratio, fmt = p->fmt;
    const char *variant = getenv("SXFIR_TILE_VARIANT");
    const bool dense = p->form == &FORM_DENSE || p->form == &FORM_DENSE_SUBSET;
    // experiment (round 6): /16 and /32 CF32 through the sixteen-column-block form too (one / two blocks per row, scalar taps,
    // the ROTATED contract, or with SXFIR_BLOCKS_SMALL=2 the unrotated one): would config 5's shape gain what /48 and /96
    // gained over the VGPR-tap dense kernel?
    if (prof_env("SXFIR_BLOCKS_SMALL", 0) && fmt == SXFIR_CF32 && dense && (ratio == 16 || ratio == 32)) {
        set_form(p, &FORM_BLOCKS);
        p->blocks_split = false;
        p->rot = prof_env("SXFIR_BLOCKS_SMALL", 0) == 2 ? 0 : 1;
    }
    // "mu": the multi-column kernel at D = 4 instead of the /4 kernels
    if (variant && strcmp(variant, "mu") == 0 && p->mode == SXFIR_DECIMATE && fmt == SXFIR_CF32 && ratio == 4 && p->ntaps == 128) set_form(p, &FORM_MULTI);
    // SXFIR_DENSE=0, and SXFIR_MULTI_PS / SXFIR_MULTI_W (those knobs belong to it): the multi-column kernel that decim_dense_kernel replaced
    if ((p->form == &FORM_DENSE || p->form == &FORM_DENSE_SUBSET) && (!prof_env("SXFIR_DENSE", 1) || getenv("SXFIR_MULTI_PS") || getenv("SXFIR_MULTI_W")))
        set_form(p, &FORM_MULTI);
    if (p->form == &FORM_DENSE_SUBSET && !prof_env("SXFIR_DENSE_SUBSET", 1)) set_form(p, &FORM_DENSE);     // 0: the VGPR-tap form at /8 (A/B)
    if (const char *v = getenv("SXFIR_DENSE_NT")) { K.dense_nt = atoi(v); K.dense_nt_set = 1; }
    K.dense_hc = prof_env("SXFIR_DENSE_HC", 0) != 0;
    // the multi-column kernel's waves per workgroup, measured (tools/kbench.py, KB_D, specs "w1".."w8"): the choice that brings the
    // LDS image down to 10 KiB per wave (16 waves per CU) while the 31-row halo stays a small part of the staging
    K.multi_waves = ratio <= 4 ? 1 : 4;
    K.multi_ps = 2;
    if (p->form && p->form->geom == GEOM_MULTI && fmt != SXFIR_S32 && p->form != &FORM_DENSE && p->form != &FORM_DENSE_SUBSET) {
        K.multi_ps = prof_env("SXFIR_MULTI_PS", 2) == 4 ? 4 : 2;
        if (K.multi_ps == 4) K.multi_waves = ratio <= 4 ? 2 : (ratio == 8 ? 4 : 8);
        K.multi_waves = prof_env("SXFIR_MULTI_W", K.multi_waves);
        p->jsplit = K.multi_ps;
    }
    if (p->form == &FORM_MULTI) p->tile = K.multi_waves * 8 * (64 / (K.multi_ps * (ratio / 4)));
    // SXFIR_IPASS=0: interp_tile_kernel on CF32 / S32 words too (A/B; the pass form's generations stay); 4: four inputs per lane at x8
    if (p->form && p->form->geom == GEOM_IPASS) {
        const int ipass = prof_env("SXFIR_IPASS", 1), generations = p->oversub;
        if (!ipass) {
            set_form(p, ratio > 32 ? &FORM_ITILE_BLOCKS : &FORM_ITILE);
            p->oversub = generations;
        } else if (ipass == 4 && ratio == 8) {
            K.ipass_qi = 4;
            p->tile = 64 * K.ipass_qi;
        }
    }
    K.ipass_wait0 = prof_env("SXFIR_IPASS_WAIT0", 0) != 0;
    p->ipass_split = prof_env("SXFIR_IPASS_SPLIT", 1) != 0;
    if (p->form) p->oversub = prof_env("SXFIR_OVERSUB", p->oversub) > 0 ? prof_env("SXFIR_OVERSUB", p->oversub) : 1;
    if (p->form && p->mode == SXFIR_DECIMATE) K.ablate = prof_env("SXFIR_ABLATE", 0);
}

// The /4 plans: the variants of SXFIR_TILE_VARIANT, SXFIR_WIDE_ASYM, SXFIR_SCHED, SXFIR_OCC -- and which of the two /4 forms the
// plan's calls then take (the variants launch their own grids: prof_launch_tile)
static int prof_resolved_div4(sxfir_plan *p)
{
    ProfKnobs &K = p->prof;
    const int ntaps = p->ntaps, fmt = p->fmt;
    bool wide_form = p->form == &FORM_WIDE;
    K.occ_sb = K.occ_db = K.occ_pair = 8;
    K.occ_wide = wide_form ? p->occ : 8;
    // the 4-outputs-per-lane kernels (the CF32 instance's figure: see the kernel table) -- and round 3's scalar-tap form for 128
    // symmetric taps ("t2s"), the A/B partner of the wide kernel that replaced it
    const void *ksb = (const void *)tile_kernel(ntaps, SXFIR_CF32);
    if (ntaps == 128 && p->symmetric)
        ksb = fmt == SXFIR_S32 ? (const void *)sxfir::decim4_tile2_kernel<128, 1, sxfir::T2_SHIPPED, 0, true>
                               : (const void *)sxfir::decim4_tile2_kernel<128, 1, sxfir::T2_SHIPPED>;
    query_occupancy(&K.occ_sb, ksb, 64);
    p->k.tile = tile_kernel(ntaps, fmt);
    if (!p->k.wide && ntaps == 128 && prof_env("SXFIR_WIDE_ASYM", 0)) {
        wide_form = true;                                      // A/B: the wide kernel's ASYM form on CF32 / S32 words
        p->k.wide = fmt == SXFIR_S32 ? sxfir::decim4_wide_kernel<0, true, 24, true, false, 0, false, true>
                                     : sxfir::decim4_wide_kernel<0, false, 24, true, false, 0, false, true>;
        query_occupancy(&K.occ_wide, p->k.wide, 64);
    }
    if (ntaps == 128) {
        const void *kp = fmt == SXFIR_S32 ? (const void *)sxfir::decim4_pair_kernel<0, true> : (const void *)sxfir::decim4_pair_kernel<0, false>;
        query_occupancy(&K.occ_pair, kp, 128);
    }
    const void *kdb = ntaps == 128 ? (const void *)sxfir::decim4_tile_kernel<128, true>
                                   : (const void *)sxfir::decim4_tile_kernel<64, true>;
    query_occupancy(&K.occ_db, kdb, 64);
    if (const char *v = getenv("SXFIR_TILE_VARIANT")) {
        K.tile_dbuf = (strcmp(v, "db") == 0);
        // "sb", "db", "sg": the first-generation tile kernel (taps in VGPR pairs) also for symmetric taps
        if (strcmp(v, "sb") == 0 || strcmp(v, "db") == 0 || strncmp(v, "sg", 2) == 0) { p->symmetric = false; wide_form = false; }
        // "t2s": round 3's shipped form (decim4_tile2_kernel, T2_SHIPPED) as the A/B partner of the wide kernel
        if (strcmp(v, "t2s") == 0) wide_form = false;
        K.sgpr_r = strcmp(v, "sg") == 0 ? 8 : (strcmp(v, "sg4") == 0 ? 4 : 0);
        if (K.sgpr_r && ntaps == 128) {
            const void *k = K.sgpr_r == 8 ? (const void *)sxfir::decim4_sgpr_kernel<8>
                                          : (const void *)sxfir::decim4_sgpr_kernel<4>;
            query_occupancy(&K.occ_sb, k, 64);
        }
        // "wide": decim4_wide_kernel (sxfir_decim_wide.hip.h), symmetric taps only
        if (strncmp(v, "wide", 4) == 0 && ntaps == 128 && p->symmetric) {
            K.wide = true;
            K.wide_nt = strncmp(v, "wident", 6) == 0;
            K.wide_pin = strncmp(v, "widentp", 7) == 0;
            K.wide_nb = atoi(v + (K.wide_pin ? 7 : (K.wide_nt ? 6 : 4)));
            // "widepol<hex>": the shipped build (wident24) with another cache policy (sxfir_decim_wide.hip.h, POL)
            if (strncmp(v, "widepol", 7) == 0) {
                K.wide_nt = true;
                K.wide_nb = 24;
                K.wide_pol = (int)strtol(v + 7, nullptr, 16);
            }
            // SXFIR_LDS_PAD: dynamic LDS bytes on top of the kernel's own image: fewer waves fit a CU (a probe: what would a
            // form with a larger tile per wave -- 16 outputs per lane, 34 KB -- have left of the latency hiding?)
            K.lds_pad = prof_env("SXFIR_LDS_PAD", 0) > 0 ? prof_env("SXFIR_LDS_PAD", 0) : 0;
            if (K.lds_pad) query_occupancy(&K.occ_wide, sxfir::decim4_wide_kernel<0, false, 24, true>, 64, (size_t)K.lds_pad);
        }
        // "pair": decim4_pair_kernel (sxfir_decim_pair.hip.h)
        if (strncmp(v, "pair", 4) == 0 && ntaps == 128) {
            K.pair = true;
            K.pair_xsep = strcmp(v, "pairx") == 0;
            if (K.pair_xsep) K.occ_pair = 7;
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
                if (!k || ((opt & sxfir::T2_SCALAR) && !p->symmetric)) return fail(SXFIR_EUNSUPPORTED, "no tile2 variant %d:%d for these taps", wpg, opt);
                K.t2_wpg = wpg;
                K.t2_opt = opt;
                // SXFIR_LDS_PAD: dynamic LDS bytes on top of the kernel's own image: fewer waves fit a CU
                K.lds_pad = prof_env("SXFIR_LDS_PAD", 0) > 0 ? prof_env("SXFIR_LDS_PAD", 0) : 0;
                // occ_sb = resident WAVES per CU of this variant
                int nb = 0;
                query_occupancy(&nb, k, 64 * wpg, (size_t)K.lds_pad);
                if (nb > 0) K.occ_sb = nb * wpg;
            }
        }
    }
    K.sched = prof_env("SXFIR_SCHED", 0);
    if (prof_env("SXFIR_OCC", 0) > 0) K.occ_sb = K.occ_db = prof_env("SXFIR_OCC", 0);
    // what geometry() reports and the plain launches take: the wide kernel (strided passes only), else the 4-outputs-per-lane kernels
    p->form = wide_form && K.sched != 1 ? &FORM_WIDE : &FORM_TILE4;
    p->tile = p->form == &FORM_WIDE ? 512 : (K.sgpr_r && ntaps == 128) ? 64 * K.sgpr_r : 256;         // (decim4_sgpr_kernel<R>: tiles of 64 R outputs)
    p->occ = p->form == &FORM_WIDE ? K.occ_wide : K.tile_dbuf ? K.occ_db : K.occ_sb;
    return SXFIR_OK;
}

static int prof_resolved(sxfir_plan *p)
{
    ProfKnobs &K = p->prof;
    const int ratio = p->ratio, fmt = p->fmt, geom = p->form ? p->form->geom : GEOM_GENERIC;
    if (geom == GEOM_MULTI && (p->form == &FORM_MULTI || (p->blocks && p->blocks < 3))) {
        // the instances the product's table does not have; LDS is what limits the residents
        const int W = K.multi_waves;
        const void *k = nullptr;
        if (p->blocks) {       // (the unrotated instances have the same resources)
            k = p->blocks == 1 ? (const void *)sxfir::decim_blocks_kernel<1, false, true, false, false, true> : (const void *)sxfir::decim_blocks_kernel<2, false, true, false, false, true>;
        } else if (fmt == SXFIR_S32) {   // wire-word input: one instantiation per ratio (4 waves, 2-way row split)
            k = ratio == 8    ? (const void *)sxfir::decim_multi_kernel<8, 4, false, 0, 2, true>
                : ratio == 16 ? (const void *)sxfir::decim_multi_kernel<16, 4, false, 0, 2, true>
                              : (const void *)sxfir::decim_multi_kernel<32, 4, false, 0, 2, true>;
        } else {
            switch (SXFIR_MULTI_KEY(ratio, W, fmt == SXFIR_CF16, K.multi_ps)) {
#define SXFIR_X(DD, WW, HH, PP) \
            case SXFIR_MULTI_KEY(DD, WW, HH, PP): k = (const void *)sxfir::decim_multi_kernel<DD, WW, HH, 0, PP>; break;
                SXFIR_MULTI_VARIANTS(SXFIR_X)
#undef SXFIR_X
            }
        }
        if (!k) return fail(SXFIR_EUNSUPPORTED, "no multi-column kernel for ratio %d with %d waves per workgroup", ratio, W);
        query_occupancy(&p->occ, k, 64 * W);
    }
    if (p->blocks) {
        if (const char *v = getenv("SXFIR_BLOCKS_SPLIT")) {     // 0: off; n >= 1: dealt while a call has at most n x slots tiles
            p->blocks_split = atoi(v) != 0;
            if (atoi(v) > 1) p->join_tiles = (long long)atoi(v) * p->compute_units * p->occ;
        }
        // test hook: a hand-off that never arrives (tests/test_gpu_join.py proves with it that its checker sees one)
        if (const char *v = getenv("SXFIR_BLOCKS_JOIN_DROP")) K.join_drop = (atoi(v) >= 0 && atoi(v) < p->blocks) ? atoi(v) : -1;
    }
    if (K.ipass_qi == 4) query_occupancy(&p->occ, sxfir::interp8_pass_kernel<4>, 64);
    if (geom == GEOM_WIDE || geom == GEOM_TILE) return prof_resolved_div4(p);
    return SXFIR_OK;
}

static hipError_t prof_alloc(sxfir_plan *p)
{
    return p->prof.join_drop >= 0 ? hipMalloc(&p->prof.join_shadow, (size_t)p->join_tiles * 4096) : hipSuccess;
}

static void prof_free(sxfir_plan *p)
{
    (void)hipFree(p->prof.join_shadow);
    (void)hipFree(p->prof.stamps_dev);
}

extern "C" {

// Diagnostic (SXFIR_ABLATE=11/12 builds): median in-kernel shader clock in MHz of the last launch.
int sxfir_debug_clock(sxfir_plan *p, double *mhz)
{
    if (!p || !mhz || !p->prof.stamps_dev) return fail(SXFIR_EINVAL, "no stamps recorded");
    std::vector<unsigned long long> h(2 * p->prof.stamps_n);
    HIPCHECK(hipMemcpy(h.data(), p->prof.stamps_dev, 16 * p->prof.stamps_n, hipMemcpyDeviceToHost));
    std::vector<double> f;
    for (size_t i = 0; i < p->prof.stamps_n; ++i)
        if (h[2 * i + 1] > 0) f.push_back(100.0 * (double)h[2 * i] / (double)h[2 * i + 1]);
    if (f.empty()) return fail(SXFIR_EINVAL, "no stamps recorded");
    std::sort(f.begin(), f.end());
    *mhz = f[f.size() / 2];
    return SXFIR_OK;
}

int sxfir_debug_stamps(sxfir_plan *p, unsigned long long *host, size_t capacity_records, size_t *n_records)
{
    if (!p || !host || !n_records || !p->prof.stamps_dev || (p->prof.ablate != 3 && p->prof.ablate != 5)) return fail(SXFIR_EINVAL, "no stamps recorded");
    const size_t n = p->prof.stamps_n < capacity_records ? p->prof.stamps_n : capacity_records;
    // records: 5 x uint64 (multi-column kernel, ablate 3) or 8 x uint64 (tile2 kernel, ablate 5)
    HIPCHECK(hipMemcpy(host, p->prof.stamps_dev, (p->prof.ablate == 5 ? 64 : 40) * n, hipMemcpyDeviceToHost));
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

}  // extern "C"

#else  // the production library: no hook does anything

static inline void prof_settle(sxfir_plan *) {}
static inline int prof_resolved(sxfir_plan *) { return SXFIR_OK; }
static inline hipError_t prof_alloc(sxfir_plan *) { return hipSuccess; }
static inline void prof_free(sxfir_plan *) {}

#endif
