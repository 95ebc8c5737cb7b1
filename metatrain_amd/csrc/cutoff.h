// The two cutoff functions and the derivative of the taper, shared by the preprocessing, adjoint and training kernels (a
// header: no translation unit depends on device code of another one).
#pragma once
#include "common.h"

namespace pet {

// ----------------------------------------------------------------------------------
// cutoff functions (pet/modules/utilities.py:4-39)
// ----------------------------------------------------------------------------------
__device__ __forceinline__ float cutoff_value(float d, float rc, float width, int fn) {
    float s = (d - (rc - width)) / width;
    if (fn == PET_CUTOFF_BUMP) {
        s = fminf(fmaxf(s, 1e-6f), 1.0f - 1e-6f);
        return 0.5f * (1.0f + tanhf(1.0f / tanf(3.14159274f * s)));
    }
    s = fminf(fmaxf(s, 0.0f), 1.0f);
    return 0.5f * (1.0f + cosf(3.14159274f * s));
}

// d fc / d d0 (zero outside the taper because of the clamp)
__device__ __forceinline__ float cutoff_deriv(float d, float rc, float width, int fn) {
    float s = (d - (rc - width)) / width;
    if (fn == PET_CUTOFF_BUMP) {
        if (!(s >= 1e-6f && s <= 1.0f - 1e-6f)) return 0.0f;
        float x = 3.14159274f * s;
        float sn = sinf(x), cs = cosf(x);
        float t = tanhf(cs / sn);
        // d/ds [0.5 (1 + tanh(cot x))] = 0.5 (1 - t^2) * (-pi / sin^2 x)
        return 0.5f * (1.0f - t * t) * (-3.14159274f / (sn * sn)) / width;
    }
    if (!(s >= 0.0f && s <= 1.0f)) return 0.0f;
    return -0.5f * 3.14159274f * sinf(3.14159274f * s) / width;
}

__device__ __forceinline__ float cutoff_deriv_dev(float d, float rc, float width, int fn) { return cutoff_deriv(d, rc, width, fn); }

// (d fc / d d0, d^2 fc / d d0^2) for the Hessian-vector product's geometry kernel: the same clamps (both zero where the
// clamp of cutoff_value is flat), evaluated in double -- one thread per edge, and (1 - tanh^2) times the bracket of the
// Bump taper's second derivative cancels to nothing in fp32 near both ends of the taper.
//   Bump:   f = (1 + tanh(cot x)) / 2, x = pi s:  f_s = (1 - t^2)/2 (-pi / sin^2 x),
//           f_ss = (1 - t^2) pi^2 (sin x cos x - t) / sin^4 x
//   Cosine: f = (1 + cos x) / 2:  f_s = -pi sin x / 2,  f_ss = -pi^2 cos x / 2
__device__ __forceinline__ void cutoff_deriv2(float d, float rc, float width, int fn, double* f1, double* f2) {
    const float sf = (d - (rc - width)) / width;   // the clamp decides on the fp32 value the forward pass saw
    const double s = ((double)d - ((double)rc - (double)width)) / (double)width, pi = 3.14159265358979323846;
    *f1 = 0.0;
    *f2 = 0.0;
    if (fn == PET_CUTOFF_BUMP) {
        if (!(sf >= 1e-6f && sf <= 1.0f - 1e-6f)) return;
        const double x = pi * s, sn = sin(x), cs = cos(x), ch = cosh(cs / sn), t = tanh(cs / sn);
        const double sech2 = 1.0 / (ch * ch), s2 = sn * sn;   // (cosh overflows to inf where the taper is flat: 0)
        *f1 = 0.5 * sech2 * (-pi / s2) / width;
        *f2 = sech2 * pi * pi * (sn * cs - t) / (s2 * s2) / ((double)width * width);
        return;
    }
    if (!(sf >= 0.0f && sf <= 1.0f)) return;
    *f1 = -0.5 * pi * sin(pi * s) / width;
    *f2 = -0.5 * pi * pi * cos(pi * s) / ((double)width * width);
}

}  // namespace pet
