// What the profiling build's SXFIR_* environment knobs set on a plan (libsxfir_prof.so, -DSXFIR_PROFILING).  One member of
// sxfir_plan (sxfir_plan.hip.h), value-initialised with the plan; written by the creators' hooks (sxfir_prof_create.inc) and
// read by them and by the launch hooks (sxfir_prof_dispatch.inc), nowhere else.  In libsxfir.so the member is empty.
#ifdef SXFIR_PROFILING
struct ProfKnobs {
    int ablate;            // SXFIR_ABLATE: 1 = memory side alone, 2 = compute side alone, 3 / 5 = phase stamps, 11 / 12 = clock stamps, ...
    void *stamps_dev;      // diagnostic clock / phase stamps of the last launch
    size_t stamps_n;
    int sched;             // SXFIR_SCHED: tile schedule of the /4 kernels (0 XCD-blocked strided passes, 1 contiguous runs, 3 short tail)
    bool tile_dbuf;        // "db": the double-buffered LDS-DMA variant of decim4_tile_kernel
    int occ_sb, occ_db;    // resident waves per CU of the 4-outputs-per-lane kernel in play and of its double-buffered variant
    int sgpr_r;            // "sg" / "sg4": decim4_sgpr_kernel with R outputs per lane (0 = off)
    int lds_pad;           // SXFIR_LDS_PAD: extra dynamic LDS bytes per workgroup of a wide / tile2 variant (caps the waves per CU)
    int t2_wpg, t2_opt;    // "t2:<w>:<bits>": decim4_tile2_kernel variant (waves per workgroup, T2_* bits); wpg 0 = off
    bool pair;             // "pair": decim4_pair_kernel, the two tap halves on the two waves of a workgroup
    bool pair_xsep;        // "pairx": ... with a separate exchange buffer (two barriers per tile instead of four)
    int occ_pair;          // its resident workgroups per CU
    bool wide;             // "wide<nb>", "wident<nb>", ...: a non-default build of decim4_wide_kernel
    int wide_nb;           // its LDS read-ahead depth: 0 = default
    bool wide_nt;          // "wident...": with non-temporal staging loads
    bool wide_pin;         // "widentp...": and the FMA issue order pinned (volatile asm)
    int wide_pol;          // "widepol<hex>": cache policy of its nt loads (low byte) and stores (next byte)
    int occ_wide;          // its resident workgroups per CU
    int dense_nt;          // SXFIR_DENSE_NT = 2 / 1 / 0: decim_dense_kernel's staging loads at every ratio
    int dense_nt_set;      // ... and whether the knob was given at all
    bool dense_hc;         // SXFIR_DENSE_HC=1: decim_dense_kernel with halo carry (/32, /16)
    int multi_waves;       // decim_multi_kernel: waves per workgroup
    int multi_ps;          // ... and lanes that share the 32 tap rows of one output (2 or 4)
    int ipass_qi;          // SXFIR_IPASS=4: inputs per lane of interp8_pass_kernel at x8 (else 0: the product's)
    bool ipass_wait0;      // SXFIR_IPASS_WAIT0=1: its vmcnt(0) form (A/B partner of the counted wait)
    int join_drop = -1;    // SXFIR_BLOCKS_JOIN_DROP=<b> (test hook): the items of block b store their block value to join_shadow instead
    void *join_shadow;     // of the scratch, where it is copied behind the launch (join_tiles x 4 KiB, allocated with the knob); -1 = off
};
#else
struct ProfKnobs {};
#endif
