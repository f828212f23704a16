// The 2x oversampled 4-band synthesizer of the C ABI (include/sxfir_synthesizer_os.h): plan creation.  The plan is of
// KIND_SYNTHESIZER with ratio = nbands / oversample = 2 and bands = 4: a x2 interpolator in everything about the stream, created
// through the frame of sxfir_plan.hip.h -- the kernel table gives it synthesis4x2_kernel and synthesis_os_generic_kernel,
// interp_geom / launch_synth (sxfir_launch.hip.h) choose between the two per call, the state entry points take it as it is, and
// its calls come through sxfir_synthesize (sxfir_synthesizer.hip.h) unchanged.  Included by sxfir.hip last; not a stand-alone
// translation unit.
#pragma once

extern "C" {

int sxfir_synthesizer_os_abi_version(void) { return SXFIR_SYNTHESIZER_OS_ABI_VERSION; }

int sxfir_create_synthesizer_os(sxfir_plan **out, const float *taps, int ntaps, int nbands, int oversample, int nchan, int fmt, int device)
{
    if (int rc = check_create_args(out, taps, SXFIR_INTERPOLATE, ntaps, "nbands", nbands, nchan, fmt)) return rc;
    if (oversample < 1 || oversample > 4096) return fail(SXFIR_EINVAL, "oversample %d out of range", oversample);
    if (nbands != 4)
        return fail(SXFIR_EUNSUPPORTED, "oversampled synthesizer: 4 bands only (the twiddles of %d bands are not exact: no rounding rule for them)", nbands);
    if (oversample == 1)
        return fail(SXFIR_EUNSUPPORTED, "oversample 1 is the critically sampled synthesizer: sxfir_create_synthesizer (include/sxfir_synthesizer.h)");
    if (oversample != 2)
        return fail(SXFIR_EUNSUPPORTED, "oversampled synthesizer: oversample 2 only (%d asked for)", oversample);
    if (ntaps % nbands) return fail(SXFIR_EINVAL, "synthesizer needs ntaps %% nbands == 0 (%d, %d)", ntaps, nbands);
    sxfir_plan *p = nullptr;      // everything about the stream is a x(nbands / oversample) interpolator's
    const int ratio = nbands / oversample;
    if (int rc = new_plan(&p, KIND_SYNTHESIZER, SXFIR_INTERPOLATE, ntaps, ratio, nchan, fmt, device)) return rc;
    p->bands = nbands;
    p->oversample = oversample;
    const int jt = ntaps / ratio;                           // taps per output parity (even: ntaps is a multiple of 4)
    p->hist_len = nbands * jt;                              // per channel: a x2 interpolator's history for every band, band k's at k * hist_len / 4
    p->ext_tiled = fmt == SXFIR_CF32 && ntaps == 128;
    p->tap_table = TAPS_PARITY2;
    real_tap_contract(p);                                   // a parity's sum: the real-tap x2 interpolator's
    resolve_kernels(p);
    p->occ_ext = 5;                                         // (28 KiB of LDS per wave; the runtime's answer replaces it)
    query_occupancy(&p->occ_ext, p->k.syn4x2, 64);

    // the parity-major table of synthesis4x2_kernel: h[2i + q] at jt q + i
    std::vector<float> by_parity((size_t)ntaps);
    for (int q = 0; q < ratio; ++q)
        for (int i = 0; i < jt; ++i) by_parity[(size_t)(jt * q + i)] = taps[ratio * i + q];
    return plan_to_device(out, p, taps, (size_t)ntaps, by_parity.data());
}

int sxfir_plan_synthesis_oversampling(const sxfir_plan *p, int *oversample)
{
    if (!p || !oversample) return fail(SXFIR_EINVAL, "NULL argument");
    *oversample = p->kind == KIND_SYNTHESIZER ? p->oversample : 0;
    return SXFIR_OK;
}

}  // extern "C"
