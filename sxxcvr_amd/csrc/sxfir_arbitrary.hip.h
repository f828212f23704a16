// Arbitrary-rate resamplers of the C ABI (include/sxfir_arbitrary.h): plan creation, the rate and time entry points, the two host-only
// pure functions and the streaming entry points.  The plan is of KIND_ARBITRARY: a x P interpolator (mode SXFIR_INTERPOLATE, ratio =
// nphases: its history, its contract) between whose outputs the plan's own are blended, created through the frame of
// sxfir_plan.hip.h -- the kernel table gives it resample_arb_generic_kernel and, at 128 x 32 on CF32, resample_arb_kernel; arb_geom /
// launch_call (sxfir_launch.hip.h) choose between the two per call; outputs_for and the commit of a call count with
// arb_outputs (sxfir_arb_index.h), sxfir_set_position and sxfir_reset set the time; sxfir_interpolate and its kin refuse it (check_io).  Included by sxfir.hip last; not a
// stand-alone translation unit.
#pragma once

static int check_arb_step(uint64_t step)
{
    if (step < sxfir::ARB_STEP_MIN || step > sxfir::ARB_STEP_MAX)
        return fail(SXFIR_EINVAL, "step %llu out of range (2^28 .. 2^36: 1/16 .. 16 input samples per output, Q32.32)", (unsigned long long)step);
    return SXFIR_OK;
}

extern "C" {

int sxfir_arbitrary_abi_version(void) { return SXFIR_ARBITRARY_ABI_VERSION; }

int sxfir_create_arbitrary(sxfir_plan **out, const float *taps, int ntaps, int nphases, uint64_t step, int nchan, int fmt, int device)
{
    if (!out || !taps) return fail(SXFIR_EINVAL, "NULL argument");
    *out = nullptr;
    if (ntaps < 1 || ntaps > 65536) return fail(SXFIR_EINVAL, "ntaps %d out of range", ntaps);
    if (nphases < 2 || nphases > 4096) return fail(SXFIR_EINVAL, "nphases %d out of range (2..4096)", nphases);
    if (ntaps % nphases) return fail(SXFIR_EINVAL, "arbitrary-rate resampler needs ntaps %% nphases == 0 (%d, %d)", ntaps, nphases);
    if (int rc = check_arb_step(step)) return rc;
    if (nchan < 1 || nchan > 65535) return fail(SXFIR_EINVAL, "nchan %d out of range", nchan);
    if (fmt != SXFIR_CF32 && fmt != SXFIR_CF16 && fmt != SXFIR_S32) return fail(SXFIR_EINVAL, "bad format %d", fmt);
    if (fmt == SXFIR_S32)
        return fail(SXFIR_EUNSUPPORTED, "a rational plan sits on neither wire side: SXFIR_CF32 or SXFIR_CF16 (the same storage in and out)");
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, KIND_ARBITRARY, SXFIR_INTERPOLATE, ntaps, nphases, nchan, fmt, device)) return rc;
    p->arb_step = step;
    p->hist_len = (ntaps / nphases + 1) & ~1;
    real_tap_contract(p);                                   // the x P interpolator's: a phase's taps in two halves when their count is even
    set_form(p, fmt == SXFIR_CF32 && nphases == sxfir::ArbTile::P && ntaps == sxfir::ArbTile::P * sxfir::ArbTile::T ? &FORM_ARB : nullptr);
    p->tap_table = p->form ? p->form->taps : TAPS_NONE;     // the extended phase-major table, built on the host
    resolve_form(p);
    return plan_to_device(out, p, taps, (size_t)ntaps);
}

int sxfir_set_rate(sxfir_plan *p, uint64_t step)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (p->kind != KIND_ARBITRARY) return fail(SXFIR_EINVAL, "sxfir_set_rate takes an arbitrary-rate plan (sxfir_create_arbitrary)");
    if (int rc = check_arb_step(step)) return rc;
    p->arb_step = step;
    return SXFIR_OK;
}

int sxfir_set_time(sxfir_plan *p, int64_t consumed, int64_t t_index, uint32_t t_frac)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (p->kind != KIND_ARBITRARY) return fail(SXFIR_EINVAL, "sxfir_set_time takes an arbitrary-rate plan (sxfir_create_arbitrary)");
    if (consumed < 0 || consumed >= (1ll << 62)) return fail(SXFIR_EINVAL, "stream position out of range");
    if (t_index < consumed - 1 || t_index >= (1ll << 62))
        return fail(SXFIR_EINVAL, "the next output's time %lld lies below consumed - 1 = %lld: its window would reach below the history",
                    (long long)t_index, (long long)consumed - 1);
    p->consumed = (long long)consumed;
    p->produced = 0;
    p->arb_t_index = t_index;
    p->arb_t_frac = t_frac;
    return SXFIR_OK;
}

int sxfir_plan_arbitrary(const sxfir_plan *p, int *nphases, uint64_t *step, int64_t *t_index, uint32_t *t_frac)
{
    if (!p || !nphases || !step || !t_index || !t_frac) return fail(SXFIR_EINVAL, "NULL argument");
    const bool arb = p->kind == KIND_ARBITRARY;
    *nphases = arb ? p->ratio : 0;
    *step = arb ? p->arb_step : 0;
    *t_index = arb ? p->arb_t_index : 0;
    *t_frac = arb ? p->arb_t_frac : 0;
    return SXFIR_OK;
}

int sxfir_arbitrary_outputs(int64_t t_index, uint32_t t_frac, uint64_t step, int64_t consumed, uint64_t n_in, uint64_t *n_out,
                            int64_t *t_index_after, uint32_t *t_frac_after)
{
    if (!n_out || !t_index_after || !t_frac_after) return fail(SXFIR_EINVAL, "NULL argument");
    *n_out = 0;
    *t_index_after = t_index;
    *t_frac_after = t_frac;
    if (int rc = check_arb_step(step)) return rc;
    if (t_index < -1 || t_index >= (1ll << 62) || consumed < 0 || consumed >= (1ll << 62) || n_in >= (1ull << 62))
        return fail(SXFIR_EINVAL, "time or stream position out of range");
    sxfir::arb_outputs(t_index, t_frac, step, consumed, n_in, n_out, t_index_after, t_frac_after);
    return SXFIR_OK;
}

int sxfir_arbitrary_locate(uint64_t rel_q32, uint64_t step, uint64_t m, int nphases, int64_t *n_rel, int *p, float *alpha)
{
    if (!n_rel || !p || !alpha) return fail(SXFIR_EINVAL, "NULL argument");
    if (nphases < 2 || nphases > 4096) return fail(SXFIR_EINVAL, "nphases %d out of range (2..4096)", nphases);
    if (int rc = check_arb_step(step)) return rc;
    long long n = 0;
    sxfir::arb_locate(rel_q32, step, m, nphases, &n, p, alpha);
    *n_rel = n;
    return SXFIR_OK;
}

// What sxfir_resample_arbitrary and sxfir_time_resample_arbitrary check of the plan and the buffers
static int check_arbitrary_io(const sxfir_plan *p, const CallIO &c)
{
    if (p->kind != KIND_ARBITRARY)
        return fail(SXFIR_EINVAL, "sxfir_resample_arbitrary takes an arbitrary-rate plan (sxfir_create_arbitrary); this plan takes %s",
                    p->kind == KIND_CHANNELIZER ? "sxfir_channelize" : p->kind == KIND_SYNTHESIZER ? "sxfir_synthesize" : p->kind == KIND_BANK ? "sxfir_decimate_bank" : p->kind == KIND_BANK_TX ? "sxfir_interpolate_bank"
                    : p->kind == KIND_RATIONAL ? "sxfir_resample" : p->mode == SXFIR_DECIMATE ? "sxfir_decimate" : "sxfir_interpolate");
    // both kernels take the call's first output's time relative to the call in 64 bits, Q32.32 (arb_rel): a call that yields an
    // output has that time below n_in * 2^32
    if (c.n_in >= ((size_t)1 << 31)) return fail(SXFIR_EINVAL, "call too large: an arbitrary-rate call takes fewer than 2^31 inputs per channel");
    return check_buffers(p, c);
}

int sxfir_resample_arbitrary(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                             size_t *n_out_p, void *stream)
{
    if (n_out_p) *n_out_p = 0;
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    const CallIO c{in_dev, n_in, in_stride, out_dev, out_stride, outputs_for(p, (long long)n_in), S(stream)};
    if (int rc = check_arbitrary_io(p, c)) return rc;
    return stream_call(p, c, n_out_p);
}

int sxfir_time_resample_arbitrary(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                                  int iters, void *stream, float *ms_per_pass)
{
    if (!p || !ms_per_pass || iters < 1) return fail(SXFIR_EINVAL, "bad argument");
    const CallIO c{in_dev, n_in, in_stride, out_dev, out_stride, outputs_for(p, (long long)n_in), S(stream)};
    if (int rc = check_arbitrary_io(p, c)) return rc;
    return time_call(p, c, iters, ms_per_pass);
}

}  // extern "C"
