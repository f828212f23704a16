// The mixer of the translating plans (include/sxfir_translate.h, include/sxfir_translate_tx.h), gfx950: what the complex-tap
// kernels of both directions carry when their plan turns its samples by a table w[i] = exp(-j 2 pi i / den) in device memory
// (sxfir_design_rotator).  A decimator turns OUTPUT m by w[(m s) mod den], s = (num ratio) mod den; an interpolator turns INPUT m by
// exp(+j 2 pi m s / den) = w[(m t) mod den], t = (den - s) mod den, in front of its filter: both step FORWARD through the table, by
// `step` entries per item -- an add and a conditional subtraction, never a negative value -- from the index of an item whose
// ABSOLUTE position the host reduced in 64 bits (mixer_of, sxfir_launch.hip.h).  den <= 65536: every sum of the kernels stays below
// 2^17, every product below 2^32.
//
// The rotation (mix_rotate): y.re = fsub_rn(fmul_rn(z.re, w.re), fmul_rn(z.im, w.im)), y.im = fadd_rn(fmul_rn(z.re, w.im),
// fmul_rn(z.im, w.re)): six roundings.  The four products pass through an empty asm statement each, so that no compiler setting
// can contract a product and the sum behind it into a fused multiply-add.
//
// A kernel with a mixer takes an argument struct of its own (the plain struct plus the mixer): GenericArgs, DecimTileArgs and
// InterpTileArgs keep their size, so every kernel that takes them keeps its text.
//
// New code: the reference has no mixer behind its decimator or in front of its interpolator (the SX1255's filters are fixed and
// low-pass, SoapySX.cpp:180-208, :1093).
#pragma once

namespace sxfir {

struct Mixer {
    const float *w;         // den (re, im) pairs: w[i] = exp(-j 2 pi i / den) (sxfir_design_rotator)
    unsigned den;           // 1 .. 65536
    unsigned step;          // table entries per item: a decimator's s per output, an interpolator's t per input sample
    unsigned phase;         // table index of the call's first item (the tiled interpolator: of sample -32 of the call, its halo's first)
};

// z * w in six roundings, no fused multiply-add
__device__ __forceinline__ float2 mix_rotate(float2 z, float2 w)
{
    float rr = __fmul_rn(z.x, w.x), ii = __fmul_rn(z.y, w.y);
    float ri = __fmul_rn(z.x, w.y), ir = __fmul_rn(z.y, w.x);
    asm("" : "+v"(rr), "+v"(ii), "+v"(ri), "+v"(ir));
    return make_float2(__fsub_rn(rr, ii), __fadd_rn(ri, ir));
}

}  // namespace sxfir
