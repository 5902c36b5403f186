// ImageBGSubtract's surface (include/sequitr_hip.h "Frame cleaning"): the tile cutter (sq_frontend.hip) evaluates it, the
// fit and residual kernels (sq_frame_clean.hip) take its coordinates from here:
//     bg(u, v) = c0 + c1 s + c2 t + c3 s^2 + c4 s t + c5 t^2,  s = (u - (W-1)/2) / ((W-1)/2),  t likewise for row v.
// Every multiply-add of the surface is one fused operation, written out, so that its roundings do not depend on the
// including file's contraction setting.
#pragma once

namespace {

struct BgAxis { double centre, inv; };                          // scaled coordinate = (index - centre) * inv
__host__ __device__ inline BgAxis bg_axis(int L) {
    const double c = 0.5 * (double)(L - 1);
    return {c, 1.0 / c};
}

// by rows: (c0 + c2 t + c5 t^2) + s ((c1 + c4 t) + c3 s)
struct BgRow { double a, b, c; };
__device__ __forceinline__ BgRow bg_row(const double *__restrict__ k, double t) {
    return {__builtin_fma(t, __builtin_fma(k[5], t, k[2]), k[0]), __builtin_fma(k[4], t, k[1]), k[3]};
}
__device__ __forceinline__ double bg_eval(const BgRow &r, double s) {
    return __builtin_fma(s, __builtin_fma(r.c, s, r.b), r.a);
}

}  // namespace
