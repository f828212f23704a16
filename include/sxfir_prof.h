/*
 * sxfir_prof.h -- extra entry points of the PROFILING build of the resampling
 * library (sxxcvr_amd/lib/libsxfir_prof.so, built with -DSXFIR_PROFILING).
 *
 * The profiling build carries the kernel A/B variants and ablation modes and
 * reads its knobs from the environment when a plan is created
 * (SXFIR_TILE_VARIANT, SXFIR_OVERSUB, SXFIR_OCC, SXFIR_SCHED, SXFIR_ABLATE,
 * SXFIR_MULTI_PS, SXFIR_MULTI_W; see tools/kbench.py).  Some ablation modes
 * produce wrong results on purpose.  It is used by tools/ and
 * tests/test_gpu_variants.py only; the production library libsxfir.so has none
 * of this and never looks at the environment.
 */
#ifndef SXFIR_PROF_H
#define SXFIR_PROF_H

#include "sxfir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SXFIR_ABLATE=11/12: median in-kernel shader clock (MHz) of the last launch. */
int sxfir_debug_clock(sxfir_plan *plan, double *mhz);

/* SXFIR_ABLATE=3 on the multi-column decimator: copies the raw per-wave stamp records of the last launch
 * (5 x uint64 each: tiles, cycles in reduction + store, waiting for data, arithmetic, barrier + issuing the
 * next tile's DMAs) to `host`; returns the number of records through *n_records. */
/* SXFIR_ABLATE=5 on the tile2 /4 kernel: records of 8 x uint64 {tiles, cycles issuing DMAs, waiting for data,
 * FIR arithmetic, output transposition + stores, whole-wave cycles, whole-wave 100 MHz ticks, 0}. */
int sxfir_debug_stamps(sxfir_plan *plan, unsigned long long *host, size_t capacity_records, size_t *n_records);

/* Test hooks of the (tile, block) join of the decimators by 48 and 96 (decim_blocks_kernel<..., SPLIT>: block values handed from
 * workgroup to workgroup through the plan's scratch, one arrival counter per tile).  SXFIR_EUNSUPPORTED for a plan without that
 * scratch.  With them goes the knob SXFIR_BLOCKS_JOIN_DROP=<b>, read when a plan is created: the items of block b count
 * themselves in without storing their block value where the joiner looks for it (it goes to a side buffer and is copied into
 * the scratch behind the launch): a hand-off that does not arrive -- the joiner adds what the slot held, the PREVIOUS launch's
 * value or the poison -- so wrong results on purpose (tests/test_gpu_join.py: the proof that its checker sees one).
 *   poison:      fills the whole block-value scratch with `word`, asynchronously on `stream` (0x7fc00000: a quiet NaN everywhere);
 *   counters:    waits for `stream` and returns how many of the plan's arrival counters are not zero (between launches: none);
 *   set_counter: writes one arrival counter, asynchronously on `stream` (index: channel * tiles of the call + tile).  Only
 *                sxfir_reset puts a plan right again after this. */
int sxfir_debug_join_poison(sxfir_plan *plan, uint32_t word, void *stream);
int sxfir_debug_join_counters(sxfir_plan *plan, long long *nonzero, void *stream);
int sxfir_debug_join_set_counter(sxfir_plan *plan, long long tile_index, unsigned value, void *stream);

#ifdef __cplusplus
}
#endif
#endif
