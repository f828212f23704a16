// Frequency-translating interpolators of the C ABI (include/sxfir_translate_tx.h): plan creation and the plan query.  The plan is
// a KIND_COMPLEX interpolator that carries a mixer (mix_dev, mix_den, mix_s: sxfir_plan.hip.h -- the fields of the translating
// decimators; the plan's mode tells the two apart): created through the frame of sxfir_plan.hip.h with the complex-tap
// interpolator's history and contract, the kernel table gives it interp_mix_pass_kernel (FORM_IMIX) and interp_mix_generic_kernel,
// launch_call (sxfir_launch.hip.h) hands them the call's phase; every other entry point takes it as the complex-tap interpolator it
// is.  Included by sxfir.hip behind sxfir_translate.hip.h (MIX_DEN_MAX, the table); not a stand-alone translation unit.
#pragma once

extern "C" {

int sxfir_translate_tx_abi_version(void) { return SXFIR_TRANSLATE_TX_ABI_VERSION; }

int sxfir_create_translating_interpolator(sxfir_plan **out, const float *taps_iq, int ntaps, int ratio, int num, int den, int nchan,
                                          int fmt, int device)
{
    if (int rc = check_create_args(out, taps_iq, SXFIR_INTERPOLATE, ntaps, "ratio", ratio, nchan, fmt)) return rc;
    if (ntaps % ratio) return fail(SXFIR_EINVAL, "interpolator needs ntaps %% ratio == 0 (%d, %d)", ntaps, ratio);
    if (den < 1 || den > MIX_DEN_MAX) return fail(SXFIR_EINVAL, "den %d out of range (1 .. %d)", den, MIX_DEN_MAX);
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, KIND_COMPLEX, SXFIR_INTERPOLATE, ntaps, ratio, nchan, fmt, device)) return rc;
    p->hist_len = (ntaps / ratio + 1) & ~1;
    real_tap_contract(p);
    p->mix_den = den;
    p->mix_num = (int)((((long long)num % den) + den) % den);
    p->mix_s = (int)((long long)p->mix_num * ratio % den);
    set_form(p, fmt == SXFIR_CF32 && ((ratio == 4 && ntaps == 128) || (ratio == 8 && ntaps == 256)) ? &FORM_IMIX : nullptr);
    p->tap_table = p->form ? p->form->taps : TAPS_NONE;     // the two pass-major tables, for the shapes the tiled kernel takes
    resolve_form(p);

    // planar on the device, as a complex-tap plan's: a[0, ntaps) then b[0, ntaps); the rotation table of mix_den entries is
    // plan_to_device's (sxfir_design_rotator)
    std::vector<float> planar(2 * (size_t)ntaps);
    for (int k = 0; k < ntaps; ++k) {
        planar[(size_t)k] = taps_iq[2 * k];
        planar[(size_t)ntaps + (size_t)k] = taps_iq[2 * k + 1];
    }
    return plan_to_device(out, p, planar.data(), planar.size());
}

int sxfir_plan_translation_tx(const sxfir_plan *p, int *num, int *den)
{
    if (!p || !num || !den) return fail(SXFIR_EINVAL, "NULL argument");
    const bool mine = p->mix_den && p->mode == SXFIR_INTERPOLATE;
    *num = mine ? p->mix_num : 0;
    *den = mine ? p->mix_den : 0;
    return SXFIR_OK;
}

}  // extern "C"
