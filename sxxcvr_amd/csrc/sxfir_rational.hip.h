// Rational (up / down) resamplers of the C ABI (include/sxfir_rational.h): plan creation and the streaming entry points.  The plan
// is of KIND_RATIONAL: a x up interpolator (mode SXFIR_INTERPOLATE, ratio = up: its history, its contract) of which every down-th
// output is computed, created through the frame of sxfir_plan.hip.h -- the kernel table gives it resample_generic_kernel and, at
// 4/5 x 128 on CF32, resample45_kernel; rational_geom / launch_call (sxfir_launch.hip.h) choose between the two per call;
// outputs_for and sxfir_set_position know its output count; the state entry points take it as it is; sxfir_interpolate and its kin
// refuse it (check_io).  sxfir_resample is its own argument checks in front of stream_call.  Included by sxfir.hip last; not a
// stand-alone translation unit.
#pragma once

static int gcd_of(int a, int b)
{
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

extern "C" {

int sxfir_rational_abi_version(void) { return SXFIR_RATIONAL_ABI_VERSION; }

int sxfir_create_rational(sxfir_plan **out, const float *taps, int ntaps, int up, int down, int nchan, int fmt, int device)
{
    if (!out || !taps) return fail(SXFIR_EINVAL, "NULL argument");
    *out = nullptr;
    if (ntaps < 1 || ntaps > 65536) return fail(SXFIR_EINVAL, "ntaps %d out of range", ntaps);
    if (up < 2 || up > 4096 || down < 2 || down > 4096)
        return fail(SXFIR_EINVAL, "up %d / down %d out of range (2..4096 each: a ratio with up or down 1 is an integer decimator or interpolator, sxfir_create)", up, down);
    if (const int g = gcd_of(up, down); g != 1)
        return fail(SXFIR_EINVAL, "up %d / down %d is not in lowest terms: create the plan for %d/%d", up, down, up / g, down / g);
    if (ntaps % up) return fail(SXFIR_EINVAL, "rational resampler needs ntaps %% up == 0 (%d, %d)", ntaps, up);
    if (nchan < 1 || nchan > 65535) return fail(SXFIR_EINVAL, "nchan %d out of range", nchan);
    if (fmt != SXFIR_CF32 && fmt != SXFIR_CF16 && fmt != SXFIR_S32) return fail(SXFIR_EINVAL, "bad format %d", fmt);
    if (fmt == SXFIR_S32)
        return fail(SXFIR_EUNSUPPORTED, "a rational plan sits on neither wire side: SXFIR_CF32 or SXFIR_CF16 (the same storage in and out)");
    sxfir_plan *p = nullptr;
    if (int rc = new_plan(&p, KIND_RATIONAL, SXFIR_INTERPOLATE, ntaps, up, nchan, fmt, device)) return rc;
    p->down = down;
    p->hist_len = (ntaps / up + 1) & ~1;
    real_tap_contract(p);                                   // the x up interpolator's: a phase's taps in two halves when their count is even
    set_form(p, fmt == SXFIR_CF32 && up == 4 && down == 5 && ntaps == 128 ? &FORM_RAT45 : nullptr);
    prof_settle(p);                                         // (profiling: SXFIR_OVERSUB, the generations per launch)
    resolve_form(p);
    return plan_to_device(out, p, taps, (size_t)ntaps);
}

int sxfir_plan_rational(const sxfir_plan *p, int *up, int *down)
{
    if (!p || !up || !down) return fail(SXFIR_EINVAL, "NULL argument");
    *up = p->kind == KIND_RATIONAL ? p->ratio : 0;
    *down = p->kind == KIND_RATIONAL ? p->down : 0;
    return SXFIR_OK;
}

// What sxfir_resample and sxfir_time_resample check of the plan and the buffers
static int check_rational_io(const sxfir_plan *p, const CallIO &c)
{
    if (p->kind != KIND_RATIONAL)
        return fail(SXFIR_EINVAL, "sxfir_resample takes a rational plan (sxfir_create_rational); this plan takes %s",
                    p->kind == KIND_CHANNELIZER ? "sxfir_channelize" : p->kind == KIND_SYNTHESIZER ? "sxfir_synthesize" : p->kind == KIND_BANK ? "sxfir_decimate_bank" : p->kind == KIND_BANK_TX ? "sxfir_interpolate_bank"
                    : p->kind == KIND_ARBITRARY ? "sxfir_resample_arbitrary" : p->mode == SXFIR_DECIMATE ? "sxfir_decimate" : "sxfir_interpolate");
    return check_buffers(p, c);
}

int sxfir_resample(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride, size_t *n_out_p,
                   void *stream)
{
    if (n_out_p) *n_out_p = 0;
    if (!p) return fail(SXFIR_EINVAL, "plan is NULL");
    const CallIO c{in_dev, n_in, in_stride, out_dev, out_stride, outputs_for(p, (long long)n_in), S(stream)};
    if (int rc = check_rational_io(p, c)) return rc;
    return stream_call(p, c, n_out_p);
}

int sxfir_time_resample(sxfir_plan *p, const void *in_dev, size_t n_in, size_t in_stride, void *out_dev, size_t out_stride, int iters,
                        void *stream, float *ms_per_pass)
{
    if (!p || !ms_per_pass || iters < 1) return fail(SXFIR_EINVAL, "bad argument");
    const CallIO c{in_dev, n_in, in_stride, out_dev, out_stride, outputs_for(p, (long long)n_in), S(stream)};
    if (int rc = check_rational_io(p, c)) return rc;
    return time_call(p, c, iters, ms_per_pass);
}

}  // extern "C"
