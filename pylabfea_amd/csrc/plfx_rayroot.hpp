// plfx_rayroot.hpp -- the root search of a ray (DESIGN sections 25 and 29): the one x with f(x) = 0 that the marching bracket
// of ML_full_yf (material.py:468-486) isolates, made symmetric.  Called by k_yield_scale; k_tex_yield_scale (plfx_tex.hpp)
// holds the same statements written out, for the reason given there.  Plain C++17, no HIP header needed, so the host program of
// tests/test_rayroot_cpu.py runs the same text on scalar functions.
//
// The search: from x0 down by factors 0.98 while f >= 0 (until x < 0.01 x0) or up by factors 1.02 while f < 0 (until
// x > 5 x0), then bisection of the bracket f(lo) < 0 <= f(hi) until lo and hi are neighbouring doubles; of the two the one
// with the smaller |f| is the root.  Every loop is capped.
// Status: 0 root found; 1 no bracket in [0.01 x0, 5 x0], or f returned NaN; 2 refinement cap reached.  3, a degenerate ray
// (no direction, a non-finite input, x0 <= 0), is decided by the callers before the search, each on its own inputs.
// The root is NaN unless the status is 0.
//
// Contract of f: f(x) is called once per step, and on the device by all 16 lanes of a row together, with the same x: it holds
// the row's DPP sum (svc_row_decision), so no lane of the row may skip a call.  Every lane gets the same bits back, which
// keeps the search row-uniform; the rows of a wave diverge freely.
// The search's own arithmetic is x * 0.98, x * 1.02, 0.01 * x0, 5. * x0 and lo + 0.5 * (hi - lo): single roundings but for
// the last, where 0.5 * (hi - lo) is exact, so fusing it into the sum changes nothing -- the search gives the same bits with
// and without FMA contraction, on the host and on the device.
#pragma once

#ifdef __HIPCC__
#define PLFX_RAYROOT_FN __host__ __device__ __forceinline__
#else
#define PLFX_RAYROOT_FN inline
#endif

namespace plfx {

constexpr int YS_CAP_DOWN = 240, YS_CAP_UP = 90, YS_CAP_BISECT = 80;   // 0.98^228 = 0.01, 1.02^82 = 5, 2 % of x in ulps: 2^47

template <class F>
PLFX_RAYROOT_FN int ray_root(double x0, F &&f, double &root)
{
    int st = 0, phase = 0, cnt = 0;   // phase: 0 first point, 1 marching down, 2 marching up, 3 bracket found, 4 bisection
    double x = x0, lo = 0., hi = 0., flo = 0., fhi = 0.;
    root = __builtin_nan("");
    for (;;) {
        const double fx = f(x);   // the only evaluation site
        if (fx != fx) {
            st = 1;
            break;
        }
        if (phase == 0) phase = (fx >= 0.) ? 1 : 2;
        if (phase == 1) {
            if (fx < 0.) {
                lo = x, flo = fx, phase = 3;
            } else {
                hi = x, fhi = fx;
                if (x < 0.01 * x0 || ++cnt > YS_CAP_DOWN) {
                    st = 1;
                    break;
                }
                x *= 0.98;
                continue;
            }
        } else if (phase == 2) {
            if (fx >= 0.) {
                hi = x, fhi = fx, phase = 3;
            } else {
                lo = x, flo = fx;
                if (x > 5. * x0 || ++cnt > YS_CAP_UP) {
                    st = 1;
                    break;
                }
                x *= 1.02;
                continue;
            }
        } else if (fx < 0.) {
            lo = x, flo = fx;
        } else {
            hi = x, fhi = fx;
        }
        if (phase == 3) phase = 4, cnt = 0;
        const double mid = lo + 0.5 * (hi - lo);
        if (!(mid > lo && mid < hi)) {   // lo and hi are neighbours
            root = (-flo < fhi) ? lo : hi;
            break;
        }
        if (++cnt > YS_CAP_BISECT) {
            st = 2;
            break;
        }
        x = mid;
    }
    return st;
}

}  // namespace plfx
