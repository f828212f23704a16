// The tuner bank of the C ABI (include/sxfir_bank.h): plan creation, the streaming and the timed entry point, the plan queries.  The
// plan is of KIND_BANK: a /ratio decimator in everything about the stream -- one history, one position -- with bank_n sets of complex
// taps and a mixer per band; band k has the bits of the sxfir_create_translating plan of its taps and centre.  The kernel table gives
// it decim4_bank_kernel (FORM_BANK: /4 x 128 on CF32) and decim_bank_generic_kernel, decim_geom / launch_call (sxfir_launch.hip.h)
// choose between the two per call, the state entry points take it as it is; sxfir_decimate and its kin refuse it (check_io).
// sxfir_decimate_bank is its own argument checks in front of stream_call.  Included by sxfir.hip last; not a stand-alone
// translation unit.
#pragma once

// The checks of a call's buffers: sxfir_channelize's rules for a plan whose output has bands
static int check_bank_io(const sxfir_plan *p, const CallIO &c)
{
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    if (p->kind != KIND_BANK) return fail(SXFIR_EINVAL, "not a bank plan (sxfir_create_bank, include/sxfir_bank.h)");
    if ((c.n_in && !c.in) || (c.n_out > 0 && !c.out)) return fail(SXFIR_EINVAL, "NULL device buffer");
    if (p->nchan > 1 && c.in_stride < c.n_in) return fail(SXFIR_EINVAL, "channel stride smaller than the block");
    if (c.band_stride < (size_t)c.n_out)
        return fail(SXFIR_EINVAL, "band stride %zu smaller than the call's %lld outputs per band", c.band_stride, c.n_out);
    if (int rc = check_band_layout(p, "out", c.out_stride, c.band_stride, (size_t)c.n_out)) return rc;
    if ((uintptr_t)c.in % sample_bytes(p->fmt) || (uintptr_t)c.out % sample_bytes(p->fmt == SXFIR_S32 ? SXFIR_CF32 : p->fmt))
        return fail(SXFIR_EINVAL, "buffers must be aligned to one complex sample");
    return SXFIR_OK;
}

extern "C" {

int sxfir_bank_abi_version(void) { return SXFIR_BANK_ABI_VERSION; }

int sxfir_create_bank(sxfir_plan **out, const float *taps_iq, int ntaps, int ratio, int nbands, const int *num, const int *den,
                      int nchan, int fmt, int device)
{
    if (out) *out = nullptr;
    if (!num || !den) return fail(SXFIR_EINVAL, "NULL argument");
    if (int rc = check_create_args(out, taps_iq, SXFIR_DECIMATE, ntaps, "ratio", ratio, nchan, fmt)) return rc;
    if (nbands < 1 || nbands > SXFIR_BANK_MAX_BANDS) return fail(SXFIR_EINVAL, "nbands %d out of range (1 .. %d)", nbands, SXFIR_BANK_MAX_BANDS);
    for (int k = 0; k < nbands; ++k)
        if (den[k] < 1 || den[k] > MIX_DEN_MAX) return fail(SXFIR_EINVAL, "band %d: den %d out of range (1 .. %d)", k, den[k], MIX_DEN_MAX);
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, KIND_BANK, SXFIR_DECIMATE, ntaps, ratio, nchan, fmt, device)) return rc;
    p->hist_len = (ntaps + 1) & ~1;
    real_tap_contract(p);
    p->bank_n = nbands;
    for (int k = 0; k < nbands; ++k) {
        p->bank_den[k] = den[k];
        p->bank_num[k] = (int)((((long long)num[k] % den[k]) + den[k]) % den[k]);
        p->bank_s[k] = (int)((long long)p->bank_num[k] * ratio % den[k]);
    }
    p->bands = nbands;                                      // (check_band_layout's count; sxfir_plan_bands answers for channelizers alone)
    set_form(p, fmt == SXFIR_CF32 && ratio == 4 && ntaps == 128 ? &FORM_BANK : nullptr);
    p->tap_table = TAPS_NONE;
    resolve_form(p);

    // planar on the device, band after band: a_k[0, ntaps) then b_k[0, ntaps) at 2 ntaps k
    std::vector<float> planar(2 * (size_t)ntaps * (size_t)nbands);
    for (int k = 0; k < nbands; ++k)
        for (int t = 0; t < ntaps; ++t) {
            planar[2 * (size_t)ntaps * k + (size_t)t] = taps_iq[2 * ((size_t)ntaps * k + t)];
            planar[2 * (size_t)ntaps * k + (size_t)ntaps + (size_t)t] = taps_iq[2 * ((size_t)ntaps * k + t) + 1];
        }
    return plan_to_device(out, p, planar.data(), planar.size());
}

int sxfir_decimate_bank(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                        size_t band_stride, size_t *n_out_p, void *stream)
{
    if (n_out_p) *n_out_p = 0;
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    const CallIO c{in_dev, n_in, in_stride, out_dev, out_stride, p->kind == KIND_BANK ? outputs_for(p, (long long)n_in) : 0, S(stream), band_stride};
    if (int rc = check_bank_io(p, c)) return rc;
    return stream_call(p, c, n_out_p);
}

int sxfir_time_decimate_bank(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride,
                             size_t band_stride, int iters, void *stream, float *ms_per_pass)
{
    if (!p || !ms_per_pass || iters < 1) return fail(SXFIR_EINVAL, "bad argument");
    const CallIO c{in_dev, n_in, in_stride, out_dev, out_stride, p->kind == KIND_BANK ? outputs_for(p, (long long)n_in) : 0, S(stream), band_stride};
    if (int rc = check_bank_io(p, c)) return rc;
    return time_call(p, c, iters, ms_per_pass);
}

int sxfir_plan_bank(const sxfir_plan *p, int *nbands)
{
    if (!p || !nbands) return fail(SXFIR_EINVAL, "NULL argument");
    *nbands = p->kind == KIND_BANK ? p->bank_n : 0;
    return SXFIR_OK;
}

int sxfir_plan_bank_band(const sxfir_plan *p, int band, int *num, int *den)
{
    if (!p || !num || !den) return fail(SXFIR_EINVAL, "NULL argument");
    const int n = p->kind == KIND_BANK ? p->bank_n : 0;             // (a combiner plan carries the same fields: sxfir_plan_bank_tx_band answers for it)
    if (band < 0 || band >= n) return fail(SXFIR_EINVAL, "band %d of %d", band, n);
    *num = p->bank_num[band];
    *den = p->bank_den[band];
    return SXFIR_OK;
}

}  // extern "C"
