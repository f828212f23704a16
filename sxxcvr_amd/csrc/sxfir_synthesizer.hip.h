// The 4-band synthesizer of the C ABI (include/sxfir_synthesizer.h): plan creation and the streaming entry point.  The plan is
// of KIND_SYNTHESIZER: a x4 interpolator in everything about the stream, created through the frame of sxfir_plan.hip.h -- the kernel
// table gives it synthesis4_kernel and synthesis_generic_kernel, interp_geom / launch_synth (sxfir_launch.hip.h) choose between the
// two per call, the state entry points take it as it is; sxfir_interpolate and its kin refuse it (check_io).  sxfir_synthesize is
// its own argument checks in front of stream_call.  Included by sxfir.hip last; not a stand-alone translation unit.
#pragma once

extern "C" {

int sxfir_synthesizer_abi_version(void) { return SXFIR_SYNTHESIZER_ABI_VERSION; }

int sxfir_create_synthesizer(sxfir_plan **out, const float *taps, int ntaps, int nbands, int nchan, int fmt, int device)
{
    if (int rc = check_create_args(out, taps, SXFIR_INTERPOLATE, ntaps, "nbands", nbands, nchan, fmt)) return rc;
    if (nbands != 4)
        return fail(SXFIR_EUNSUPPORTED, "synthesizer: 4 bands only (the twiddles of %d bands are not exact: no rounding rule for them)", nbands);
    if (ntaps % nbands) return fail(SXFIR_EINVAL, "synthesizer needs ntaps %% nbands == 0 (%d, %d)", ntaps, nbands);
    sxfir_plan *p = nullptr;      // critically sampled: everything about the stream is a x nbands interpolator's
    if (int rc = new_plan(&p, KIND_SYNTHESIZER, SXFIR_INTERPOLATE, ntaps, nbands, nchan, fmt, device)) return rc;
    const int jt = ntaps / nbands;                          // taps per phase
    p->hist_len = nbands * ((jt + 1) & ~1);                 // per channel: an interpolator's history for every band, band k's at k * hist_len / 4
    p->ext_tiled = fmt == SXFIR_CF32 && ntaps == 128;
    p->tap_table = TAPS_PHASE4;
    real_tap_contract(p);                                   // a phase's sum: the real-tap interpolator's
    resolve_kernels(p);
    query_occupancy(&p->occ_ext, p->k.syn4, 64);

    // the phase-major table of synthesis4_kernel: h[4j + r] at jt r + j
    std::vector<float> phased((size_t)ntaps);
    for (int r = 0; r < nbands; ++r)
        for (int j = 0; j < jt; ++j) phased[(size_t)(jt * r + j)] = taps[nbands * j + r];
    return plan_to_device(out, p, taps, (size_t)ntaps, phased.data());
}

int sxfir_plan_synthesis_bands(const sxfir_plan *p, int *nbands)
{
    if (!p || !nbands) return fail(SXFIR_EINVAL, "NULL argument");
    *nbands = p->kind == KIND_SYNTHESIZER ? p->bands : 0;
    return SXFIR_OK;
}

int sxfir_synthesize(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, size_t band_stride, void *out_dev,
                     size_t out_stride, size_t *n_out_p, void *stream)
{
    if (n_out_p) *n_out_p = 0;
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (p->kind != KIND_SYNTHESIZER) return fail(SXFIR_EINVAL, "not a synthesizer plan");
    const long long n_out = outputs_for(p, (long long)n_in);
    if ((n_in && !in_dev) || (n_out > 0 && !out_dev)) return fail(SXFIR_EINVAL, "NULL device buffer");
    if (band_stride < n_in) return fail(SXFIR_EINVAL, "band stride %zu smaller than the call's %zu inputs per band", band_stride, n_in);
    if (p->nchan > 1 && out_stride < (size_t)n_out) return fail(SXFIR_EINVAL, "channel stride smaller than the block");
    if (int rc = check_band_layout(p, "in", in_stride, band_stride, n_in)) return rc;
    if ((uintptr_t)in_dev % sample_bytes(p->fmt) || (uintptr_t)out_dev % sample_bytes(p->fmt))
        return fail(SXFIR_EINVAL, "buffers must be aligned to one complex sample");
    return stream_call(p, CallIO{in_dev, n_in, in_stride, out_dev, out_stride, n_out, S(stream), band_stride}, n_out_p);
}

}  // extern "C"
