// Complex-tap (band-pass) plans of the C ABI, both directions (include/sxfir_complex.h, include/sxfir_complex_tx.h): plan creation
// and the band-pass designer.  The plan is of KIND_COMPLEX: a decimator or an interpolator under the real-tap contract of its shape,
// created through the frame of sxfir_plan.hip.h -- the kernel table gives it decim4_cx_kernel and decim_cx_generic_kernel, or
// interp_cx_pass_kernel and interp_cx_generic_kernel; decim_geom / interp_geom and launch_call (sxfir_launch.hip.h) choose between
// the two per call, every other entry point takes it as the decimator or interpolator it is.  create_complex_plan is also the
// translating plans' creation path (sxfir_translate.hip.h): the same plan with a mixer.  Included by sxfir.hip; not a stand-alone
// translation unit.
#pragma once

// The one creation path of the KIND_COMPLEX plans, behind the creator's own argument checks: the history of the plan's direction, the
// real-tap contract, the mixer (den 0: none; else the band centre num / den: mix_den, mix_num, mix_s, and plan_to_device makes the
// rotation table), the form of the shapes the tiled kernels take with its tap layout, the taps planar on the device.
static int create_complex_plan(sxfir_plan **out, int mode, const float *taps_iq, int ntaps, int ratio, int num, int den, int nchan,
                               int fmt, int device)
{
    const bool tx = mode == SXFIR_INTERPOLATE;
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, KIND_COMPLEX, mode, ntaps, ratio, nchan, fmt, device)) return rc;
    p->hist_len = ((tx ? ntaps / ratio : ntaps) + 1) & ~1;
    real_tap_contract(p);
    if (den) {
        p->mix_den = den;
        p->mix_num = (int)((((long long)num % den) + den) % den);
        p->mix_s = (int)((long long)p->mix_num * ratio % den);
    }
    const bool x4 = ratio == 4 && ntaps == 128, x8 = ratio == 8 && ntaps == 256;
    const PlanForm *form = tx ? (den ? &FORM_IMIX : &FORM_ICX) : (den ? &FORM_MIX : &FORM_CX);
    set_form(p, fmt == SXFIR_CF32 && (x4 || (tx && x8)) ? form : nullptr);
    // an interpolator's two pass-major tables, for the shapes the tiled kernel takes; a decimator has no second tap table
    p->tap_table = p->form ? p->form->taps : TAPS_NONE;
    resolve_form(p);

    // planar on the device: a[0, ntaps) then b[0, ntaps)
    std::vector<float> planar(2 * (size_t)ntaps);
    for (int k = 0; k < ntaps; ++k) {
        planar[(size_t)k] = taps_iq[2 * k];
        planar[(size_t)ntaps + (size_t)k] = taps_iq[2 * k + 1];
    }
    return plan_to_device(out, p, planar.data(), planar.size());
}

extern "C" {

int sxfir_complex_abi_version(void) { return SXFIR_COMPLEX_ABI_VERSION; }
int sxfir_complex_tx_abi_version(void) { return SXFIR_COMPLEX_TX_ABI_VERSION; }

int sxfir_create_complex(sxfir_plan **out, int mode, const float *taps_iq, int ntaps, int ratio, int nchan, int fmt, int device)
{
    if (int rc = check_create_args(out, taps_iq, mode, ntaps, "ratio", ratio, nchan, fmt)) return rc;
    if (mode == SXFIR_INTERPOLATE)
        return fail(SXFIR_EUNSUPPORTED, "complex taps: decimators only (no complex-tap interpolator kernel exists)");
    return create_complex_plan(out, mode, taps_iq, ntaps, ratio, 0, 0, nchan, fmt, device);
}

int sxfir_create_complex_interpolator(sxfir_plan **out, const float *taps_iq, int ntaps, int ratio, int nchan, int fmt, int device)
{
    if (int rc = check_create_args(out, taps_iq, SXFIR_INTERPOLATE, ntaps, "ratio", ratio, nchan, fmt)) return rc;
    if (ntaps % ratio) return fail(SXFIR_EINVAL, "interpolator needs ntaps %% ratio == 0 (%d, %d)", ntaps, ratio);
    return create_complex_plan(out, SXFIR_INTERPOLATE, taps_iq, ntaps, ratio, 0, 0, nchan, fmt, device);
}

int sxfir_taps_are_complex(const sxfir_plan *p, int *is_complex)
{
    if (!p || !is_complex) return fail(SXFIR_EINVAL, "NULL argument");
    *is_complex = p->kind == KIND_COMPLEX || p->kind == KIND_BANK || p->kind == KIND_BANK_TX;
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
