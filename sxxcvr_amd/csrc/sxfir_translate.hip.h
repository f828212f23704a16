// Frequency-translating decimators of the C ABI (include/sxfir_translate.h): the rotation table, plan creation and the plan query.
// The plan is a KIND_COMPLEX decimator that carries a mixer (mix_dev, mix_den, mix_s: sxfir_plan.hip.h): created through the
// frame of sxfir_plan.hip.h with the complex creator's history and contract, the kernel table gives it decim4_mix_kernel (FORM_MIX)
// and decim_mix_generic_kernel, launch_call (sxfir_launch.hip.h) hands them the call's phase; every other entry point takes it as
// the complex-tap decimator it is.  Included by sxfir.hip last; not a stand-alone translation unit.
#pragma once

static const int MIX_DEN_MAX = 65536;          // the table at most 512 KiB; every index product of the kernels fits 32 bits

extern "C" {

int sxfir_translate_abi_version(void) { return SXFIR_TRANSLATE_ABI_VERSION; }

int sxfir_design_rotator(int den, float *w_iq)
{
    if (!w_iq) return fail(SXFIR_EINVAL, "NULL argument");
    if (den < 1 || den > MIX_DEN_MAX) return fail(SXFIR_EINVAL, "den %d out of range (1 .. %d)", den, MIX_DEN_MAX);
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int i = 0; i < den; ++i) {
        // i den-ths of a turn, clockwise; the quarter turns exactly, as sxfir_design_bandpass has them (an exact zero is +0.0)
        double c, s;
        if (i == 0) { c = 1.0; s = 0.0; }
        else if (4LL * i == den) { c = 0.0; s = 1.0; }
        else if (2LL * i == den) { c = -1.0; s = 0.0; }
        else if (4LL * i == 3LL * den) { c = 0.0; s = -1.0; }
        else { c = std::cos(two_pi * (double)i / (double)den); s = std::sin(two_pi * (double)i / (double)den); }
        w_iq[2 * i] = c == 0.0 ? 0.0f : (float)c;
        w_iq[2 * i + 1] = s == 0.0 ? 0.0f : (float)-s;
    }
    return SXFIR_OK;
}

int sxfir_create_translating(sxfir_plan **out, const float *taps_iq, int ntaps, int ratio, int num, int den, int nchan, int fmt, int device)
{
    if (int rc = check_create_args(out, taps_iq, SXFIR_DECIMATE, ntaps, "ratio", ratio, nchan, fmt)) return rc;
    if (den < 1 || den > MIX_DEN_MAX) return fail(SXFIR_EINVAL, "den %d out of range (1 .. %d)", den, MIX_DEN_MAX);
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, KIND_COMPLEX, SXFIR_DECIMATE, ntaps, ratio, nchan, fmt, device)) return rc;
    p->hist_len = (ntaps + 1) & ~1;
    real_tap_contract(p);
    p->mix_den = den;
    p->mix_num = (int)((((long long)num % den) + den) % den);
    p->mix_s = (int)((long long)p->mix_num * ratio % den);
    set_form(p, fmt == SXFIR_CF32 && ratio == 4 && ntaps == 128 ? &FORM_MIX : nullptr);
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

int sxfir_plan_translation(const sxfir_plan *p, int *num, int *den)
{
    if (!p || !num || !den) return fail(SXFIR_EINVAL, "NULL argument");
    // (a translating interpolator carries a mixer too: include/sxfir_translate_tx.h, sxfir_plan_translation_tx)
    const bool mine = p->mix_den && p->mode == SXFIR_DECIMATE;
    *num = mine ? p->mix_num : 0;
    *den = mine ? p->mix_den : 0;
    return SXFIR_OK;
}

}  // extern "C"
