// Frequency-translating plans of the C ABI, both directions (include/sxfir_translate.h, include/sxfir_translate_tx.h): the rotation
// table, plan creation and the plan queries.  The plan is a KIND_COMPLEX decimator or interpolator that carries a mixer (mix_dev,
// mix_den, mix_s: sxfir_plan.hip.h; the plan's mode tells the two apart), created by create_complex_plan (sxfir_complex.hip.h): the
// kernel table gives it the mixer instances of the complex-tap kernels (FORM_MIX, FORM_IMIX) and the translating generic kernels,
// launch_call (sxfir_launch.hip.h) hands them the call's phase; every other entry point takes it as the complex-tap plan it is.
// Included by sxfir.hip behind sxfir_complex.hip.h; not a stand-alone translation unit.
#pragma once

static const int MIX_DEN_MAX = 65536;          // the table at most 512 KiB; every index product of the kernels fits 32 bits

// The band centre of a translating plan of direction `mode`; 0 / 0 for every other plan (the other direction's too: each query
// answers for its own header's plans)
static int plan_translation(const sxfir_plan *p, int mode, int *num, int *den)
{
    if (!p || !num || !den) return fail(SXFIR_EINVAL, "NULL argument");
    const bool mine = p->mix_den && p->mode == mode;
    *num = mine ? p->mix_num : 0;
    *den = mine ? p->mix_den : 0;
    return SXFIR_OK;
}

extern "C" {

int sxfir_translate_abi_version(void) { return SXFIR_TRANSLATE_ABI_VERSION; }
int sxfir_translate_tx_abi_version(void) { return SXFIR_TRANSLATE_TX_ABI_VERSION; }

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
    return create_complex_plan(out, SXFIR_DECIMATE, taps_iq, ntaps, ratio, num, den, nchan, fmt, device);
}

int sxfir_create_translating_interpolator(sxfir_plan **out, const float *taps_iq, int ntaps, int ratio, int num, int den, int nchan,
                                          int fmt, int device)
{
    if (int rc = check_create_args(out, taps_iq, SXFIR_INTERPOLATE, ntaps, "ratio", ratio, nchan, fmt)) return rc;
    if (ntaps % ratio) return fail(SXFIR_EINVAL, "interpolator needs ntaps %% ratio == 0 (%d, %d)", ntaps, ratio);
    if (den < 1 || den > MIX_DEN_MAX) return fail(SXFIR_EINVAL, "den %d out of range (1 .. %d)", den, MIX_DEN_MAX);
    return create_complex_plan(out, SXFIR_INTERPOLATE, taps_iq, ntaps, ratio, num, den, nchan, fmt, device);
}

int sxfir_plan_translation(const sxfir_plan *p, int *num, int *den) { return plan_translation(p, SXFIR_DECIMATE, num, den); }
int sxfir_plan_translation_tx(const sxfir_plan *p, int *num, int *den) { return plan_translation(p, SXFIR_INTERPOLATE, num, den); }

}  // extern "C"
