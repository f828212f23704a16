// The 4-band channelizer of the C ABI (include/sxfir_channelizer.h): plan creation and the streaming entry point.  The plan is
// of KIND_CHANNELIZER: a /4 decimator in everything about the stream, created by create_band_plan (sxfir_plan.hip.h) -- the kernel
// table gives it chan4_kernel and chan_generic_kernel, decim_geom / launch_call (sxfir_launch.hip.h) choose between the two per
// call, the state entry points take it as it is; sxfir_decimate and its kin refuse it (check_io).  sxfir_channelize is its own
// argument checks in front of stream_call.  Included by sxfir.hip last; not a stand-alone translation unit.
#pragma once

extern "C" {

int sxfir_channelizer_abi_version(void) { return SXFIR_CHANNELIZER_ABI_VERSION; }

int sxfir_create_channelizer(sxfir_plan **out, const float *taps, int ntaps, int nbands, int nchan, int fmt, int device)
{
    return create_band_plan(out, KIND_CHANNELIZER, "channelizer", taps, ntaps, nbands, 1, nchan, fmt, device);   // critically sampled
}

int sxfir_plan_bands(const sxfir_plan *p, int *nbands)
{
    if (!p || !nbands) return fail(SXFIR_EINVAL, "NULL argument");
    *nbands = p->kind == KIND_CHANNELIZER ? p->bands : 0;
    return SXFIR_OK;
}

int sxfir_channelize(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                     size_t band_stride, size_t *n_out_p, void *stream)
{
    if (n_out_p) *n_out_p = 0;
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (p->kind == KIND_SYNTHESIZER) return fail(SXFIR_EINVAL, "a synthesizer plan takes sxfir_synthesize (include/sxfir_synthesizer.h)");
    if (p->kind == KIND_RATIONAL) return fail(SXFIR_EINVAL, "%s", RATIONAL_TAKES);
    if (p->kind == KIND_ARBITRARY) return fail(SXFIR_EINVAL, "%s", ARBITRARY_TAKES);
    if (p->kind != KIND_CHANNELIZER) return fail(SXFIR_EINVAL, "not a channelizer plan");
    const long long n_out = outputs_for(p, (long long)n_in);
    if ((n_in && !in_dev) || (n_out > 0 && !out_dev)) return fail(SXFIR_EINVAL, "NULL device buffer");
    if (p->nchan > 1 && in_stride < n_in) return fail(SXFIR_EINVAL, "channel stride smaller than the block");
    if (band_stride < (size_t)n_out) return fail(SXFIR_EINVAL, "band stride %zu smaller than the call's %lld outputs per band", band_stride, n_out);
    if (int rc = check_band_layout(p, "out", out_stride, band_stride, (size_t)n_out)) return rc;
    if ((uintptr_t)in_dev % sample_bytes(p->fmt) || (uintptr_t)out_dev % sample_bytes(p->fmt == SXFIR_S32 ? SXFIR_CF32 : p->fmt))
        return fail(SXFIR_EINVAL, "buffers must be aligned to one complex sample");
    return stream_call(p, CallIO{in_dev, n_in, in_stride, out_dev, out_stride, n_out, S(stream), band_stride}, n_out_p);
}

}  // extern "C"
