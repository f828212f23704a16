// Complex-tap (band-pass) decimators of the C ABI (include/sxfir_complex.h): plan creation and the band-pass designer.  The plan
// is an ordinary sxfir_plan with `cx` set -- the kernel table (sxfir_plan.hip.h) gives it decim4_cx_kernel and
// decim_cx_generic_kernel, decim_geom / launch_decim (sxfir_launch.hip.h) choose between the two per call, every other entry point takes it as it is.  Included by sxfir.hip last; not a stand-alone translation unit.
#pragma once

extern "C" {

int sxfir_complex_abi_version(void) { return SXFIR_COMPLEX_ABI_VERSION; }

int sxfir_create_complex(sxfir_plan **out, int mode, const float *taps_iq, int ntaps, int ratio, int nchan, int fmt, int device)
{
    if (!out || !taps_iq) return fail(SXFIR_EINVAL, "NULL argument");
    *out = nullptr;
    if (mode != SXFIR_DECIMATE && mode != SXFIR_INTERPOLATE) return fail(SXFIR_EINVAL, "bad mode %d", mode);
    if (ntaps < 1 || ntaps > 65536) return fail(SXFIR_EINVAL, "ntaps %d out of range", ntaps);
    if (ratio < 1 || ratio > 4096) return fail(SXFIR_EINVAL, "ratio %d out of range", ratio);
    if (nchan < 1 || nchan > 65535) return fail(SXFIR_EINVAL, "nchan %d out of range", nchan);
    if (fmt != SXFIR_CF32 && fmt != SXFIR_CF16 && fmt != SXFIR_S32) return fail(SXFIR_EINVAL, "bad format %d", fmt);
    if (mode == SXFIR_INTERPOLATE)
        return fail(SXFIR_EUNSUPPORTED, "complex taps: decimators only (no complex-tap interpolator kernel exists)");

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

    sxfir_plan *p = new (std::nothrow) sxfir_plan();       // value-initialised: no real-tap kernel family is enabled
    if (!p) return fail(SXFIR_ENOMEM, "out of host memory");
    p->mode = mode;
    p->ntaps = ntaps;
    p->ratio = ratio;
    p->nchan = nchan;
    p->fmt = fmt;
    p->device = device;
    p->kernel = SXFIR_KERNEL_AUTO;
    p->compute_units = prop.multiProcessorCount;
    p->hist_len = (ntaps + 1) & ~1;
    p->cx = true;
    p->cx_tiled = fmt == SXFIR_CF32 && ratio == 4 && ntaps == 128;
    p->tap_table = TAPS_SCALED;                             // (no second tap table: taps_scaled_dev stays NULL)
    p->thr2 = 1.0e-3f * 1.0e-3f;
    p->oversub = 16;
    p->occ_cx = 8;
#ifdef SXFIR_PROFILING
    p->join_drop = -1;
#endif
    // The numeric contract of a REAL-tap plan of this shape (sxfir_create): two row halves and column groups of 4 where the
    // adjacent-pair trees exist, the rotated form for /48 and /96 with 32 taps per phase, else one chain.
    {
        const int jt = (ntaps + ratio - 1) / ratio;
        const int ncol4 = ratio / 4;
        const bool pow2_cols = ratio % 4 == 0 && (ncol4 & (ncol4 - 1)) == 0 && ncol4 <= 32;
        const bool blocks = ntaps == 32 * ratio && (ratio == 48 || ratio == 96);
        p->rot = blocks ? 1 : 0;
        if (ntaps % ratio == 0 && (pow2_cols || blocks) && jt % 2 == 0) {
            p->jsplit = 2;
            p->cw = 4;
        } else {
            p->jsplit = 1;
            p->cw = ratio;
        }
    }
    resolve_kernels(p);
    query_occupancy(&p->occ_cx, p->k.cx, 64);

    // planar on the device: a[0, ntaps) then b[0, ntaps)
    std::vector<float> planar(2 * (size_t)ntaps);
    for (int k = 0; k < ntaps; ++k) {
        planar[(size_t)k] = taps_iq[2 * k];
        planar[(size_t)ntaps + (size_t)k] = taps_iq[2 * k + 1];
    }
    const size_t hist_bytes = sample_bytes(fmt) * (size_t)p->hist_len * (size_t)nchan;
    hipError_t e = hipMalloc((void **)&p->taps_dev, sizeof(float) * planar.size());
    if (e == hipSuccess) e = hipMalloc(&p->hist_dev, hist_bytes);
    if (e == hipSuccess) e = hipMalloc(&p->hist_alt, hist_bytes);
    if (e == hipSuccess) e = hipMemcpy(p->taps_dev, planar.data(), sizeof(float) * planar.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(p->hist_dev, 0, hist_bytes);
    if (e != hipSuccess) {
        if (p->taps_dev) (void)hipFree(p->taps_dev);
        if (p->hist_dev) (void)hipFree(p->hist_dev);
        if (p->hist_alt) (void)hipFree(p->hist_alt);
        delete p;
        return fail(SXFIR_EHIP, "plan allocation failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return SXFIR_OK;
}

int sxfir_taps_are_complex(const sxfir_plan *p, int *is_complex)
{
    if (!p || !is_complex) return fail(SXFIR_EINVAL, "NULL argument");
    *is_complex = p->cx ? 1 : 0;
    return SXFIR_OK;
}

int sxfir_design_bandpass(int ntaps, int ratio, double beta, double gain, int num, int den, float *taps_iq)
{
    if (ntaps < 1 || ratio < 1 || den < 1 || !taps_iq) return fail(SXFIR_EINVAL, "bad argument");
    std::vector<double> h;
    lowpass_fp64(ntaps, ratio, beta, gain, h);
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int k = 0; k < ntaps; ++k) {
        // the phase in whole den-ths of a turn, reduced in integers; the quarter turns exactly
        const long long r = (((long long)k * num) % den + den) % den;
        double c, s;
        if (r == 0) { c = 1.0; s = 0.0; }
        else if (4 * r == den) { c = 0.0; s = 1.0; }
        else if (2 * r == den) { c = -1.0; s = 0.0; }
        else if (4 * r == 3LL * den) { c = 0.0; s = -1.0; }
        else { c = std::cos(two_pi * (double)r / (double)den); s = std::sin(two_pi * (double)r / (double)den); }
        const double v = h[(size_t)k];
        taps_iq[2 * k] = c == 0.0 ? 0.0f : (float)(v * c);         // (an exact zero is +0.0, whatever the prototype's sign)
        taps_iq[2 * k + 1] = s == 0.0 ? 0.0f : (float)(v * s);
    }
    return SXFIR_OK;
}

}  // extern "C"
