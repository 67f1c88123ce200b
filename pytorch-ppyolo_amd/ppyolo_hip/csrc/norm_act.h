// Mish and its derivative, shared by the inference kernels (norm_act.hip) and the training kernels (norm_act_train.hip).
#pragma once
#include "common.h"

__device__ __forceinline__ float mish_f32(float v) {
    if (v > 20.f) return v;                     // torch softplus threshold; tanh(v) rounds to 1 from v = 9.02 on
    const float e = expf(v);
    const float n = e * (e + 2.f);              // tanh(log(1 + e)) = ((1 + e)^2 - 1) / ((1 + e)^2 + 1) = n / (n + 2)
    return v * (n / (n + 2.f));
}

__device__ __forceinline__ float norm_act(float v, int act) {
    if (act == PPY_ACT_MISH) return mish_f32(v);
    return ppy_apply_act(v, act);
}

// d mish / d v = t + v * (1 - t^2) * sigmoid(v) with t = tanh(softplus(v)) = n / (n + 2):  n / (n + 2) + v * 4 e (e + 1) / (n + 2)^2.
// The two terms cancel at v = -1.1924 (the minimum of mish), where a float32 evaluation keeps no relative accuracy: evaluated in
// double and rounded once.  v > 20 (torch's softplus threshold): 1 -- tanh is 1 there and v * sech^2 is below 1e-15.
__device__ __forceinline__ float mish_grad_f32(float v) {
    if (v > 20.f) return 1.f;
    const double x = (double)v, e = exp(x), n = e * (e + 2.), d = n + 2.;
    return (float)(n / d + x * 4. * e * (e + 1.) / (d * d));
}

// act'(z) with the forward's own sign rule (z > 0), so the slope pattern is the one the forward applied.
__device__ __forceinline__ float norm_act_grad(float z, int act) {
    if (act == PPY_ACT_RELU) return z > 0.f ? 1.f : 0.f;
    if (act == PPY_ACT_LEAKY) return z > 0.f ? 1.f : 0.1f;
    if (act == PPY_ACT_MISH) return mish_grad_f32(z);
    return 1.f;
}
