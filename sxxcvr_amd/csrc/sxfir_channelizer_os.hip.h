// The 2x oversampled 4-band channelizer of the C ABI (include/sxfir_channelizer_os.h): plan creation.  The plan is of
// KIND_CHANNELIZER with ratio = nbands / oversample = 2 and bands = 4: a /2 decimator in everything about the stream, created
// by create_band_plan (sxfir_plan.hip.h) -- the kernel table gives it chan4x2_kernel and chan4x2_generic_kernel, decim_geom /
// launch_call (sxfir_launch.hip.h) choose between the two per call, the state entry points take it as it is, and its calls come
// through sxfir_channelize (sxfir_channelizer.hip.h) unchanged.  Included by sxfir.hip last; not a stand-alone translation unit.
#pragma once

extern "C" {

int sxfir_channelizer_os_abi_version(void) { return SXFIR_CHANNELIZER_OS_ABI_VERSION; }

int sxfir_create_channelizer_os(sxfir_plan **out, const float *taps, int ntaps, int nbands, int oversample, int nchan, int fmt, int device)
{
    // (the shared range checks first, here too: the refusals of `oversample` keep their place behind them)
    if (int rc = check_create_args(out, taps, SXFIR_DECIMATE, ntaps, "nbands", nbands, nchan, fmt)) return rc;
    if (int rc = check_oversample("channelizer", nbands, oversample)) return rc;
    return create_band_plan(out, KIND_CHANNELIZER, "oversampled channelizer", taps, ntaps, nbands, oversample, nchan, fmt, device);
}

int sxfir_plan_oversampling(const sxfir_plan *p, int *oversample)
{
    if (!p || !oversample) return fail(SXFIR_EINVAL, "NULL argument");
    *oversample = p->kind == KIND_CHANNELIZER ? p->oversample : 0;
    return SXFIR_OK;
}

}  // extern "C"
