// |X|^2 of a complex64 bin the way numpy forms it, shared by every kernel that squares a spectrogram on the way in (mcem_spec.hip:
// McemBatch's X2; classify.hip: the classifier's input), so that they see the same bits.
//
// The magnitude is numpy's for complex64 (its vectorised absolute value: larger * sqrt(fma(r, r, 1)), r = smaller / larger, all in
// float32, correctly rounded operations), squared in float32: bit-identical to `(np.abs(X) ** 2).astype(np.float32)`.  The power layout
// of the walk kernels (v_sqrt_f32 of re^2 + im^2) is within 2 ulp of it but not equal.
#pragma once
#include <math.h>
#include "common.hpp"

namespace dvae {

// correctly rounded square root of x in [1, 2] (no scaling needed): v_sqrt_f32 is within 1 ulp, the two fma residuals pick the
// rounded root among its neighbours (LLVM's own expansion of a correctly rounded sqrt; the sqrt builtins compile to the bare
// instruction here)
__device__ __forceinline__ float sqrt_rn_1_2(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    const float vp = __fmaf_rn(-dn, s, x), vs = __fmaf_rn(-up, s, x);
    s = vp <= 0.f ? dn : s;
    s = vs > 0.f ? up : s;
    return s;
}

__device__ __forceinline__ float np_abs_c64(float re, float im) {
    const float a = fabsf(re), b = fabsf(im);
    if (isnan(a) || isnan(b)) return (isinf(a) || isinf(b)) ? INFINITY : NAN;
    const float l = fmaxf(a, b), s = fminf(a, b);
    if (l == 0.f) return 0.f;
    if (isinf(l)) return INFINITY;
    const float r = __fdiv_rn(s, l);
    return __fmul_rn(l, sqrt_rn_1_2(__fmaf_rn(r, r, 1.f)));
}

// the power of one bin: np_abs_c64 squared in float32
__device__ __forceinline__ float np_power_c64(float re, float im) {
    const float a = np_abs_c64(re, im);
    return __fmul_rn(a, a);
}

}  // namespace dvae
