// The 4-band synthesizer of the C ABI (include/sxfir_synthesizer.h): plan creation and the streaming entry point.  The plan is
// an ordinary x4 interpolator plan with `syn_bands` set -- the kernel table (sxfir_plan.hip.h) gives it synthesis4_kernel and
// synthesis_generic_kernel, interp_geom / launch_synth (sxfir_launch.hip.h) choose between the two per call, the state entry points
// take it as it is; sxfir_interpolate and its kin refuse it (check_io).  Included by sxfir.hip last; not a stand-alone translation unit.
#pragma once

extern "C" {

int sxfir_synthesizer_abi_version(void) { return SXFIR_SYNTHESIZER_ABI_VERSION; }

int sxfir_create_synthesizer(sxfir_plan **out, const float *taps, int ntaps, int nbands, int nchan, int fmt, int device)
{
    if (!out || !taps) return fail(SXFIR_EINVAL, "NULL argument");
    *out = nullptr;
    if (ntaps < 1 || ntaps > 65536) return fail(SXFIR_EINVAL, "ntaps %d out of range", ntaps);
    if (nbands < 1 || nbands > 4096) return fail(SXFIR_EINVAL, "nbands %d out of range", nbands);
    if (nchan < 1 || nchan > 65535) return fail(SXFIR_EINVAL, "nchan %d out of range", nchan);
    if (fmt != SXFIR_CF32 && fmt != SXFIR_CF16 && fmt != SXFIR_S32) return fail(SXFIR_EINVAL, "bad format %d", fmt);
    if (nbands != 4)
        return fail(SXFIR_EUNSUPPORTED, "synthesizer: 4 bands only (the twiddles of %d bands are not exact: no rounding rule for them)", nbands);
    if (ntaps % nbands) return fail(SXFIR_EINVAL, "synthesizer needs ntaps %% nbands == 0 (%d, %d)", ntaps, nbands);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(SXFIR_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (device < 0) HIPCHECK(hipGetDevice(&device));
    if (device >= ndev) return fail(SXFIR_EINVAL, "device %d of %d", device, ndev);
    HIPCHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SXFIR_ENODEVICE, "device %d is %s; kernels are built for gfx950 only", device, prop.gcnArchName);

    sxfir_plan *p = new (std::nothrow) sxfir_plan();       // value-initialised: no decimator or interpolator kernel family is enabled
    if (!p) return fail(SXFIR_ENOMEM, "out of host memory");
    const int jt = ntaps / nbands;                          // taps per phase
    p->mode = SXFIR_INTERPOLATE;
    p->ntaps = ntaps;
    p->ratio = nbands;                                      // critically sampled: everything about the stream is a x nbands interpolator's
    p->nchan = nchan;
    p->fmt = fmt;
    p->device = device;
    p->kernel = SXFIR_KERNEL_AUTO;
    p->compute_units = prop.multiProcessorCount;
    p->syn_bands = nbands;
    p->hist_len = nbands * ((jt + 1) & ~1);                 // per channel: an interpolator's history for every band, band k's at k * hist_len / 4
    p->syn_tiled = fmt == SXFIR_CF32 && ntaps == 128;
    p->tap_table = TAPS_PHASE4;
    p->thr2 = 1.0e-3f * 1.0e-3f;
    p->oversub = 16;
    p->occ_syn = 8;
#ifdef SXFIR_PROFILING
    p->join_drop = -1;
#endif
    // the numeric contract of a phase's sum: the real-tap interpolator's
    p->jsplit = (jt % 2 == 0) ? 2 : 1;
    p->cw = 1;
    p->rot = 0;
    resolve_kernels(p);
    query_occupancy(&p->occ_syn, p->k.syn4, 64);

    // the phase-major table of synthesis4_kernel: h[4j + r] at jt r + j
    std::vector<float> phased((size_t)ntaps);
    for (int r = 0; r < nbands; ++r)
        for (int j = 0; j < jt; ++j) phased[(size_t)(jt * r + j)] = taps[nbands * j + r];

    const size_t hist_bytes = sample_bytes(fmt) * (size_t)p->hist_len * (size_t)nchan;
    hipError_t e = hipMalloc((void **)&p->taps_dev, sizeof(float) * (size_t)ntaps);
    if (e == hipSuccess) e = hipMalloc((void **)&p->taps_scaled_dev, sizeof(float) * (size_t)ntaps);
    if (e == hipSuccess) e = hipMalloc(&p->hist_dev, hist_bytes);
    if (e == hipSuccess) e = hipMalloc(&p->hist_alt, hist_bytes);
    if (e == hipSuccess) e = hipMemcpy(p->taps_dev, taps, sizeof(float) * (size_t)ntaps, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->taps_scaled_dev, phased.data(), sizeof(float) * (size_t)ntaps, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(p->hist_dev, 0, hist_bytes);
    if (e != hipSuccess) {
        if (p->taps_dev) (void)hipFree(p->taps_dev);
        if (p->taps_scaled_dev) (void)hipFree(p->taps_scaled_dev);
        if (p->hist_dev) (void)hipFree(p->hist_dev);
        if (p->hist_alt) (void)hipFree(p->hist_alt);
        delete p;
        return fail(SXFIR_EHIP, "plan allocation failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return SXFIR_OK;
}

int sxfir_plan_synthesis_bands(const sxfir_plan *p, int *nbands)
{
    if (!p || !nbands) return fail(SXFIR_EINVAL, "NULL argument");
    *nbands = p->syn_bands;
    return SXFIR_OK;
}

int sxfir_synthesize(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, size_t band_stride, void *out_dev,
                     size_t out_stride, size_t *n_out_p, void *stream)
{
    if (n_out_p) *n_out_p = 0;
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (!p->syn_bands) return fail(SXFIR_EINVAL, "not a synthesizer plan");
    const long long n_out = outputs_for(p, (long long)n_in);
    if ((n_in && !in_dev) || (n_out > 0 && !out_dev)) return fail(SXFIR_EINVAL, "NULL device buffer");
    if (band_stride < n_in) return fail(SXFIR_EINVAL, "band stride %zu smaller than the call's %zu inputs per band", band_stride, n_in);
    if (p->nchan > 1) {
        if (out_stride < (size_t)n_out) return fail(SXFIR_EINVAL, "channel stride smaller than the block");
        // a channel's bands in a row, channel after channel -- or a band's channels in a row, band after band
        const size_t nb = (size_t)p->syn_bands, nc = (size_t)p->nchan;
        const bool bands_inside = in_stride >= (nb - 1) * band_stride + n_in;
        const bool channels_inside = in_stride >= n_in && band_stride >= (nc - 1) * in_stride + n_in;
        if (!bands_inside && !channels_inside)
            return fail(SXFIR_EINVAL, "bands and channels overlap (in_stride %zu, band_stride %zu, %zu inputs per band)", in_stride, band_stride, n_in);
    }
    if ((uintptr_t)in_dev % sample_bytes(p->fmt) || (uintptr_t)out_dev % sample_bytes(p->fmt))
        return fail(SXFIR_EINVAL, "buffers must be aligned to one complex sample");
    if (n_in == 0) return SXFIR_OK;
    HIPCHECK(hipSetDevice(p->device));
    const CallIO io{in_dev, n_in, in_stride, out_dev, out_stride, n_out, S(stream), band_stride};
    bool history_done = false;
    int rc = launch_synth(p, io, &history_done);
    if (rc) return rc;
    if (!history_done) {
        rc = launch_synth_history(p, io);
        if (rc) return rc;
    }
    std::swap(p->hist_dev, p->hist_alt);
    p->consumed += (long long)n_in;
    p->produced += n_out;
    if (n_out_p) *n_out_p = (size_t)n_out;
    return SXFIR_OK;
}

}  // extern "C"
