// The 2x oversampled 4-band channelizer of the C ABI (include/sxfir_channelizer_os.h): plan creation.  The plan is of
// KIND_CHANNELIZER with ratio = nbands / oversample = 2 and bands = 4: a /2 decimator in everything about the stream, created
// through the frame of sxfir_plan.hip.h -- the kernel table gives it chan4x2_kernel and chan4x2_generic_kernel, decim_geom /
// launch_decim (sxfir_launch.hip.h) choose between the two per call, the state entry points take it as it is, and its calls come
// through sxfir_channelize (sxfir_channelizer.hip.h) unchanged.  Included by sxfir.hip last; not a stand-alone translation unit.
#pragma once

extern "C" {

int sxfir_channelizer_os_abi_version(void) { return SXFIR_CHANNELIZER_OS_ABI_VERSION; }

int sxfir_create_channelizer_os(sxfir_plan **out, const float *taps, int ntaps, int nbands, int oversample, int nchan, int fmt, int device)
{
    if (int rc = check_create_args(out, taps, SXFIR_DECIMATE, ntaps, "nbands", nbands, nchan, fmt)) return rc;
    if (oversample < 1 || oversample > 4096) return fail(SXFIR_EINVAL, "oversample %d out of range", oversample);
    if (nbands != 4)
        return fail(SXFIR_EUNSUPPORTED, "oversampled channelizer: 4 bands only (the twiddles of %d bands are not exact: no rounding rule for them)", nbands);
    if (oversample == 1)
        return fail(SXFIR_EUNSUPPORTED, "oversample 1 is the critically sampled channelizer: sxfir_create_channelizer (include/sxfir_channelizer.h)");
    if (oversample != 2)
        return fail(SXFIR_EUNSUPPORTED, "oversampled channelizer: oversample 2 only (%d asked for)", oversample);
    if (ntaps % nbands) return fail(SXFIR_EINVAL, "channelizer needs ntaps %% nbands == 0 (%d, %d)", ntaps, nbands);
    sxfir_plan *p = nullptr;      // everything about the stream is a /(nbands / oversample) decimator's
    if (int rc = new_plan(&p, KIND_CHANNELIZER, SXFIR_DECIMATE, ntaps, nbands / oversample, nchan, fmt, device)) return rc;
    p->bands = nbands;
    p->oversample = oversample;
    p->hist_len = ntaps;                                    // (a multiple of 4)
    p->ext_tiled = fmt == SXFIR_CF32 && ntaps == 128;
    // the numeric contract of a branch sum: one chain per phase, no tree, no rotation
    p->jsplit = 1;
    p->cw = 1;
    resolve_kernels(p);
    query_occupancy(&p->occ_ext, p->k.chan4x2, 64);
    return plan_to_device(out, p, taps, (size_t)ntaps, nullptr);      // (no second tap table)
}

int sxfir_plan_oversampling(const sxfir_plan *p, int *oversample)
{
    if (!p || !oversample) return fail(SXFIR_EINVAL, "NULL argument");
    *oversample = p->kind == KIND_CHANNELIZER ? p->oversample : 0;
    return SXFIR_OK;
}

}  // extern "C"
