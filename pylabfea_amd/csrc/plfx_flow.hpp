// plfx_flow.hpp -- flow curves along fixed stress directions: the loop of plot_sig_eps in the reference's
// examples/train_hardening.py:83-133, whole chains on the device.  Per curve, with the plastic strain epl = epl0:
//   x_0 = the point of the yield locus along su at epl; record (x_0, epl, yf_0); then, while eps_eq(epl) + depl <= epl_max
//   and k < max_steps:  peeq = eps_eq(epl) + depl;  a = calc_fgrad(su (x_k + peeq predictor), epl);
//   epl += a depl / eps_eq(a);  x_{k+1} = the point of the locus at the new epl; record it.
// Included from plfx_material.hip after plfx_kernels.hpp.
//
// k_flow_curve<NF>: the SVC kinds, NF = 6 / 15.  Block, table staging and lane contract are k_yield_scale's (DESIGN section
// 27): 16 lanes per curve, four curves per wave, svc_row_tables / svc_row_trips, rows closed by row_allsum.  The step loop
// runs inside the kernel; the chain of a curve is sequential, the rows of a wave diverge freely.  Every root is ray_root on
// svc_row_decision with the features formed as k_yield_scale<NF> forms them -- fma(x, u_f, -v_f), w_f = epl_f / scale_wh --
// from the previous root (the first one from sy: the directions are of unit J2 stress, so sy = sy / seq_J2(su)), hence
// x_{k+1} has the bits of plfx_yield_scale(su, epl_{k+1}, x0 = x_k).  Everything a row computes holds the same bits in its 16
// lanes, so every decision below is row-uniform.
// k_flow_curve_analytic: Hill / J2 / Drucker on Voigt stresses, one thread per curve, closed-form root.
//
// Status per curve: 0 complete; 1 / 2 the status of ray_root at the step where the curve ended; 3 a degenerate direction
// (su = 0, a non-finite input; analytic: seq(su) <= 0); 4 eps_eq(a) zero or not finite.  nsteps = recorded points - 1; what
// lies past a curve's last recorded point is NaN.
#pragma once

namespace plfx {

// The gradient of the decision function of one row w.r.t. the stress features, and the sum of its components w.r.t. the
// plastic-strain features, on the trips of svc_row_trips: per slot six accumulators ga_f += w (x_f - v_f) and one
// gw += w sum_f (w_f - v_6+f), w = dual e.  The caller applies -2 gamma / scale_seq (and the scaling of the hardening value)
// once, after the row sum.  diff(v, f): feature f of the point minus v[f], f < 6 the stress features, 6 <= f < 12 the
// plastic-strain ones (NF = 15 only); it is called twice per vector, for the distance and for the terms, so that no
// difference is held across the exp2 chains.  The order of a curve's sum depends on nsv alone; it is not the order of the
// thread-per-point gradient (YfSvcWhT::fgrad_raw), which it matches within rounding.
template <int NF, class DIFF>
__device__ __forceinline__ void svc_row_gradient(const double *psv, const double *pdu, int nsv, double g, DIFF &&diff,
                                                 double *ga, double &gw)
{
    constexpr int NW = (NF == 15) ? 6 : 0;
    double acc[2][7];
    const double *vp[2] = {psv, psv};
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int f = 0; f < 7; f++) acc[c][f] = 0.;
    svc_row_trips<NF>(
        psv, pdu, nsv, g,
        [&](const double *v, int c) {
            double hh = 0.;
            vp[c] = v;
#pragma unroll
            for (int f = 0; f < 6 + NW; f++) {
                const double d = diff(v, f);
                hh = fma(d, d, hh);
            }
#pragma unroll
            for (int f = 6 + NW; f < NF; f++) hh = fma(v[f], v[f], hh);
            return hh;
        },
        [&](int c, double du, double e) {
            const double w = du * e;
#pragma unroll
            for (int f = 0; f < 6; f++) acc[c][f] = fma(w, diff(vp[c], f), acc[c][f]);
            if constexpr (NW > 0) {
                double ds = 0.;
#pragma unroll
                for (int f = 6; f < 12; f++) ds += diff(vp[c], f);
                acc[c][6] = fma(w, ds, acc[c][6]);
            }
        });
#pragma unroll
    for (int f = 0; f < 6; f++) ga[f] = YfSvcRow<1>::row_allsum(acc[0][f] + acc[1][f]);
    gw = (NW > 0) ? YfSvcRow<1>::row_allsum(acc[0][6] + acc[1][6]) : 0.;
}

// what lies past the last recorded point of curve i: NaN, written by the row's lanes (lane0 + stride, ...)
__device__ __forceinline__ void flow_fill_nan(size_t i, int max_steps, int rec, int nhk, int lane0, int stride, double *x_out,
                                              double *epl_out, double *yf_out, double *hk_out)
{
    const double qnan = __builtin_nan("");
    const size_t K1 = (size_t)max_steps + 1;
    for (int j = rec + lane0; j <= max_steps; j += stride) {
        x_out[i * K1 + j] = qnan;
        yf_out[i * K1 + j] = qnan;
#pragma unroll
        for (int c = 0; c < 6; c++) epl_out[(i * K1 + j) * 6 + c] = qnan;
    }
    if (hk_out)
        for (int j = nhk + lane0; j < max_steps; j += stride) hk_out[i * (size_t)max_steps + j] = qnan;
}

template <int NF>
__global__ void __launch_bounds__(YS_BLOCK)
k_flow_curve(const MatDev *__restrict__ gmat, int nmat, int lds_doubles, int mat, int n, const double *__restrict__ su_in,
             const double *__restrict__ epl0_in, int max_steps, double depl, double epl_max, double predictor,
             double *__restrict__ x_out, double *__restrict__ epl_out, double *__restrict__ yf_out, double *__restrict__ hk_out,
             int32_t *__restrict__ nsteps, int32_t *__restrict__ status)
{
    static_assert(NF == 6 || NF == 15, "6 stress features, or 15 with the work-hardening ones");
    constexpr int NW = (NF == 15) ? 6 : 0;    // plastic-strain features
    __shared__ MatDev smat[MAXMAT];
    stage_materials(smat, gmat, nmat);
    __syncthreads();
    const double *psv, *pdu;
    svc_row_tables(smat, nmat, lds_doubles, mat, psv, pdu);
    const MatDev &m = smat[mat];
    const int nsv = m.nsv;
    const int l16 = threadIdx.x & 15, rpb = blockDim.x >> 4;
    const double g = -m.gamma * LOG2E;
    const size_t K1 = (size_t)max_steps + 1;
    for (int i = blockIdx.x * rpb + (threadIdx.x >> 4); i < n; i += gridDim.x * rpb) {  // row-uniform
        double s[6], e[6], u[6], w[NW > 0 ? NW : 1];
        bool fin = true, zero = true;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            s[c] = su_in[6 * (size_t)i + c];
            e[c] = epl0_in ? epl0_in[6 * (size_t)i + c] : 0.;
            fin = fin && isfinite(s[c]) && isfinite(e[c]);
            zero = zero && s[c] == 0.;
        }
        svc_features(m, s, u);
#pragma unroll
        for (int c = 0; c < NW; c++) w[c] = e[c] / m.scale_wh;
        auto decision = [&](const double &x) {   // the decision function at x su, as k_yield_scale<NF> forms it
            return svc_row_decision<NF>(psv, pdu, nsv, g, m.intercept, [&](const double *v, int) {
                double hh = 0.;
#pragma unroll
                for (int f = 0; f < 6; f++) {
                    const double d = fma(x, u[f], -v[f]);
                    hh = fma(d, d, hh);
                }
#pragma unroll
                for (int f = 0; f < NW; f++) {
                    const double d = w[f] - v[6 + f];
                    hh = fma(d, d, hh);
                }
#pragma unroll
                for (int f = 6 + NW; f < NF; f++) hh = fma(v[f], v[f], hh);
                return hh;
            });
        };
        double x = m.sy;
        int st = (!fin || zero || !isfinite(x) || !(x > 0.)) ? 3 : 0;
        int k = 0, rec = 0;   // steps completed, points recorded
        while (st == 0) {
            double root;
            st = ray_root(x, decision, root);
            if (st != 0) break;
            x = root;
            const double f = decision(x);
            if (l16 == 0) {
                x_out[i * K1 + k] = x;
                yf_out[i * K1 + k] = f;
#pragma unroll
                for (int c = 0; c < 6; c++) epl_out[(i * K1 + k) * 6 + c] = e[c];
            }
            rec = k + 1;
            const double peeq = eps_eq(e) + depl;
            if (k >= max_steps || !(peeq <= epl_max)) break;
            const double xs = x + peeq * predictor;
            double a[6], gw;
            svc_row_gradient<NF>(
                psv, pdu, nsv, g,
                [&](const double *v, int f) { return f < 6 ? fma(xs, u[f < 6 ? f : 0], -v[f]) : w[NW > 0 ? f - 6 : 0] - v[f]; }, a,
                gw);
            const double c2 = -2. * m.gamma;
#pragma unroll
            for (int c = 0; c < 6; c++) a[c] *= c2 / m.scale_seq;
            const double ea = eps_eq(a);
            if (!(ea > 0.) || !isfinite(ea)) {
                st = 4;
                break;
            }
            if (l16 == 0 && hk_out) hk_out[i * (size_t)max_steps + k] = NW > 0 ? -(gw * c2) * m.scale_seq / m.scale_wh : __builtin_nan("");
#pragma unroll
            for (int c = 0; c < 6; c++) e[c] += a[c] * depl / ea;
#pragma unroll
            for (int c = 0; c < NW; c++) w[c] = e[c] / m.scale_wh;
            k++;
        }
        flow_fill_nan(i, max_steps, rec, k, l16, 16, x_out, epl_out, yf_out, hk_out);
        if (l16 == 0) {
            nsteps[i] = rec > 0 ? rec - 1 : 0;
            status[i] = st;
        }
    }
}

// Hill / J2 / Drucker on Voigt stresses: homogeneous of degree one, so the point of the locus is sflow(epl) / seq(su) and the
// gradient is hill_fgrad; one thread per curve.  No hardening value: hk is NaN.
__global__ void __launch_bounds__(BLOCK)
k_flow_curve_analytic(const MatDev *__restrict__ gmat, int mat, int n, const double *__restrict__ su_in,
                      const double *__restrict__ epl0_in, int max_steps, double depl, double epl_max, double predictor,
                      double *__restrict__ x_out, double *__restrict__ epl_out, double *__restrict__ yf_out,
                      double *__restrict__ hk_out, int32_t *__restrict__ nsteps, int32_t *__restrict__ status)
{
    const MatDev &m = gmat[mat];
    const size_t K1 = (size_t)max_steps + 1;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        double s[6], e[6];
        bool fin = true;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            s[c] = su_in[6 * (size_t)i + c];
            e[c] = epl0_in ? epl0_in[6 * (size_t)i + c] : 0.;
            fin = fin && isfinite(s[c]) && isfinite(e[c]);
        }
        const double seq = hill_seq(m, s);
        int st = (fin && seq > 0.) ? 0 : 3;
        int k = 0, rec = 0;
        while (st == 0) {
            const double sf = sflow_of(m, e), x = sf / seq;
            if (!isfinite(x)) {
                st = 3;
                break;
            }
            double sg[6], a[6];
#pragma unroll
            for (int c = 0; c < 6; c++) sg[c] = s[c] * x;
            x_out[i * K1 + k] = x;
            yf_out[i * K1 + k] = hill_seq(m, sg) - sf;
#pragma unroll
            for (int c = 0; c < 6; c++) epl_out[(i * K1 + k) * 6 + c] = e[c];
            rec = k + 1;
            const double peeq = eps_eq(e) + depl;
            if (k >= max_steps || !(peeq <= epl_max)) break;
            const double xs = x + peeq * predictor;
#pragma unroll
            for (int c = 0; c < 6; c++) sg[c] = s[c] * xs;
            hill_fgrad(m, sg, a);
            const double ea = eps_eq(a);
            if (!(ea > 0.) || !isfinite(ea)) {
                st = 4;
                break;
            }
#pragma unroll
            for (int c = 0; c < 6; c++) e[c] += a[c] * depl / ea;
            k++;
        }
        flow_fill_nan(i, max_steps, rec, 0, 0, 1, x_out, epl_out, yf_out, hk_out);
        nsteps[i] = rec > 0 ? rec - 1 : 0;
        status[i] = st;
    }
}

}  // namespace plfx
