// Complex-tap (band-pass) interpolators of the C ABI (include/sxfir_complex_tx.h): plan creation.  The plan is of KIND_COMPLEX: an
// interpolator under the real-tap contract of its shape, created through the frame of sxfir_plan.hip.h -- the kernel table gives it
// interp_cx_pass_kernel and interp_cx_generic_kernel, interp_geom / launch_call (sxfir_launch.hip.h) choose between the two per
// call, every other entry point takes it as an interpolator.  Included by sxfir.hip behind sxfir_complex.hip.h; not a stand-alone
// translation unit.
#pragma once

extern "C" {

int sxfir_complex_tx_abi_version(void) { return SXFIR_COMPLEX_TX_ABI_VERSION; }

int sxfir_create_complex_interpolator(sxfir_plan **out, const float *taps_iq, int ntaps, int ratio, int nchan, int fmt, int device)
{
    if (int rc = check_create_args(out, taps_iq, SXFIR_INTERPOLATE, ntaps, "ratio", ratio, nchan, fmt)) return rc;
    if (ntaps % ratio) return fail(SXFIR_EINVAL, "interpolator needs ntaps %% ratio == 0 (%d, %d)", ntaps, ratio);
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, KIND_COMPLEX, SXFIR_INTERPOLATE, ntaps, ratio, nchan, fmt, device)) return rc;
    p->hist_len = (ntaps / ratio + 1) & ~1;
    real_tap_contract(p);
    set_form(p, fmt == SXFIR_CF32 && ((ratio == 4 && ntaps == 128) || (ratio == 8 && ntaps == 256)) ? &FORM_ICX : nullptr);
    p->tap_table = p->form ? p->form->taps : TAPS_NONE;     // the two pass-major tables, for the shapes the tiled kernel takes
    resolve_form(p);

    // planar on the device: a[0, ntaps) then b[0, ntaps)
    std::vector<float> planar(2 * (size_t)ntaps);
    for (int k = 0; k < ntaps; ++k) {
        planar[(size_t)k] = taps_iq[2 * k];
        planar[(size_t)ntaps + (size_t)k] = taps_iq[2 * k + 1];
    }
    return plan_to_device(out, p, planar.data(), planar.size());
}

}  // extern "C"
