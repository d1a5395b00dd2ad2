// plfx_texflow.hpp -- flow rule and stress update of the texture-dependent SVC yield function: the
// gradient of calc_yf(sig, tex=) w.r.t. the stress (k_tex_fgrad), ML_full_yf(sig, tex=) (k_tex_full_yf) and
// Material.response(..., tex=) (k_tex_response).  Included from plfx_material.hip after plfx_tex.hpp, whose tables, staging and
// features these kernels share.  The reference has none of this (its calc_fgrad and ML_full_yf fail for a texture material);
// the semantics are the project's own and are stated where they are implemented.
//
// Notation of k_tex_yf: s = sig (its deviator for a dev_only set), f_j = (s_j - mean_j) / scale_j for j < 6, f_6+t the
// standardised texture features, K_i = exp(-gamma |f - v_i|^2).  The gradient:
//     g_j = -2 gamma sum_i dual_i K_i (f_j - v_ij),  a_j = g_j / scale_j,  j < 6,
// and for a dev_only set (a_0 + a_1 + a_2) / 3 is taken off a_0 .. a_2: the chain rule through the deviator.
#pragma once

namespace plfx {

// the scaling that closes a gradient: the sums acc_j = sum_i dual_i K_i (f_j - v_ij) to d calc_yf / d sig.  Once per point.
__device__ __forceinline__ void tex_grad_close(const TexSvcPar &P, const double (&acc)[6], double *a)
{
#pragma clang fp contract(off)
    const double c2 = -2. * P.gamma;
#pragma unroll
    for (int j = 0; j < 6; j++) a[j] = (c2 * acc[j]) / P.scale[j];
    if (P.dev_only) {
        const double p = (a[0] + a[1] + a[2]) / 3.;
        a[0] = a[0] - p;
        a[1] = a[1] - p;
        a[2] = a[2] - p;
    }
}

// calc_fgrad(sig, tex=) at n points, 16 lanes per point.  Per vector the differences and the squared distance of
// tex_decision (feature order, fma(d, d, hh), exp2_neg_n<2> through svc_row_trips); w = dual K enters six accumulators per
// slot, fma(w, d_j, acc_j), with the six stress differences formed again after the exp2 chains (the same bits; none is held
// across them, as in svc_row_gradient).  The rows are closed by the butterfly of the other 16-lane kernels: the order of a
// point's sums depends on nsv alone.  Texture selection as in k_tex_yf; a non-finite stress or texture component makes that
// point's six outputs NaN and nothing else.
template <int NFP>
__global__ void __launch_bounds__(TEX_BLOCK)
k_tex_fgrad(const TexSvcPar P, const double *__restrict__ gsv, const double *__restrict__ gdu, int n,
            const double *__restrict__ sig_in, int ntex, const double *__restrict__ tex_in, const int32_t *__restrict__ tex_id,
            double *__restrict__ grad)
{
    const double *psv, *pdu;
    tex_tables<NFP>(P, gsv, gdu, psv, pdu);
    const int l16 = threadIdx.x & 15, rpb = blockDim.x >> 4;
    const double g = -P.gamma * LOG2E;
    for (int i = blockIdx.x * rpb + (threadIdx.x >> 4); i < n; i += gridDim.x * rpb) {   // row-uniform
        const int t = tex_id ? tex_id[i] : (ntex == 1 ? 0 : i);
        double s[6], f[NFP];
        bool fin = true;
        tex_stress(P, sig_in + 6 * (size_t)i, s, fin);
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 6; j++) f[j] = (s[j] - P.mean[j]) / P.scale[j];
        }
        tex_features<NFP>(P, tex_in + (size_t)t * P.tdim, f, fin);
        double acc[2][6];
        const double *vp[2] = {psv, psv};
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int j = 0; j < 6; j++) acc[c][j] = 0.;
        svc_row_trips<tex_stride(NFP)>(
            psv, pdu, P.nsv, g,
            [&](const double *v, int c) {
                double hh = 0.;
                vp[c] = v;
#pragma unroll
                for (int j = 0; j < NFP; j++) {
                    const double d = f[j] - v[j];
                    hh = fma(d, d, hh);
                }
                return hh;
            },
            [&](int c, double du, double e) {
                const double w = du * e;
#pragma unroll
                for (int j = 0; j < 6; j++) acc[c][j] = fma(w, f[j] - vp[c][j], acc[c][j]);
            });
        double sum[6], a[6];
#pragma unroll
        for (int j = 0; j < 6; j++) sum[j] = YfSvcRow<1>::row_allsum(acc[0][j] + acc[1][j]);
        tex_grad_close(P, sum, a);
        if (l16 < 6) {
            double out = a[0];
#pragma unroll
            for (int j = 1; j < 6; j++) out = (l16 == j) ? a[j] : out;
            grad[6 * (size_t)i + l16] = fin ? out : __builtin_nan("");
        }
    }
}

// The decision function of the texture SVC and its gradient at one point, one thread per point: the source that the policy
// YfTexSvc = YfSvcT<6, TexSvcPoint> hands to response_point.  Everything of the 6-feature policy that does not touch the tables
// is YfSvcT's own code -- seq (the Hill / J2 form of the material record), sflow = sy + khard peeq, kh, and the search of
// ML_full_yf (full_ld), which runs on this decision function.  The point's standardised texture features are formed once
// (ft, slots 6 .. NFP - 1; the slots below are never read) and stay in registers: an evaluation forms the six stress
// features and, per vector, sums the squared distance in the feature order of tex_decision.  The row loop is uniform across
// the wave, so the table reads are broadcasts.  The vectors are summed in index order: the sum of a point is not the 16-lane
// row sum of k_tex_yf, which it matches within rounding.
template <int NFP>
struct TexSvcPoint {
    const TexSvcPar &P;
    const double *psv, *pdu;
    const double (&ft)[NFP];
    const double g;
    __device__ TexSvcPoint(const TexSvcPar &pp, const double *s, const double *d, const double (&f)[NFP])
        : P(pp), psv(s), pdu(d), ft(f), g(-pp.gamma * LOG2E) {}
    __device__ __forceinline__ void stress_features(const double *s, double (&fs)[6]) const
    {
#pragma clang fp contract(off)
        double sd[6];
        bool fin = true;
        tex_stress(P, s, sd, fin);
#pragma unroll
        for (int j = 0; j < 6; j++) fs[j] = (sd[j] - P.mean[j]) / P.scale[j];
    }
    __device__ __forceinline__ double dist2(const double *v, const double (&fs)[6]) const
    {
        double hh = 0.;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double d = fs[j] - v[j];
            hh = fma(d, d, hh);
        }
#pragma unroll
        for (int j = 6; j < NFP; j++) {
            const double d = ft[j] - v[j];
            hh = fma(d, d, hh);
        }
        return hh;
    }
    __device__ inline double decision(const double *s) const
    {
        double fs[6], f = 0.;
        stress_features(s, fs);
        for (int k = 0; k < P.nsv; k++)
            f = fma(pdu[k], exp2_neg(g * dist2(psv + (size_t)k * tex_stride(NFP), fs)), f);
        return f + P.intercept;
    }
    __device__ inline void fgrad(const double *s, double *a) const
    {
        double fs[6], acc[6] = {0., 0., 0., 0., 0., 0.};
        stress_features(s, fs);
        for (int k = 0; k < P.nsv; k++) {
            const double *v = psv + (size_t)k * tex_stride(NFP);
            const double w = pdu[k] * exp2_neg(g * dist2(v, fs));
#pragma unroll
            for (int j = 0; j < 6; j++) acc[j] = fma(w, fs[j] - v[j], acc[j]);
        }
        tex_grad_close(P, acc, a);
    }
};
template <int NFP>
using YfTexSvc = YfSvcT<6, TexSvcPoint<NFP>>;

// the inputs of point i that both thread-per-point kernels share: its texture features; fin false where a component of
// the texture is not finite
template <int NFP>
__device__ __forceinline__ void tex_point_features(const TexSvcPar &P, int i, int ntex, const double *tex_in,
                                                   const int32_t *tex_id, double (&ft)[NFP], bool &fin)
{
    const int t = tex_id ? tex_id[i] : (ntex == 1 ? 0 : i);
#pragma unroll
    for (int j = 0; j < 6; j++) ft[j] = 0.;
    tex_features<NFP>(P, tex_in + (size_t)t * P.tdim, ft, fin);
}

// ML_full_yf(sig, tex=) at n points, one thread per point: YfTexSvc::full_ld with epl = 0, so sflow = sy of material `mat`.
// status 0 / 1 / 2 as plfx_full_yf_batch.  A non-finite stress or texture component is decided before the search: NaN, status 1.
template <int NFP>
__global__ void __launch_bounds__(BLOCK)
k_tex_full_yf(const MatDev *gmat, int nmat, int mat, const TexSvcPar P, const double *__restrict__ gsv,
              const double *__restrict__ gdu, int n, const double *__restrict__ sig_in, int ntex,
              const double *__restrict__ tex_in, const int32_t *__restrict__ tex_id, double *__restrict__ yf,
              int32_t *__restrict__ status)
{
    __shared__ MatDev smat[MAXMAT];
    stage_materials(smat, gmat, nmat);
    const double *psv, *pdu;
    tex_tables<NFP>(P, gsv, gdu, psv, pdu);   // its barrier publishes smat as well
    const MatDev &m = smat[mat];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        double sig[6], ft[NFP];
        bool fin = true;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            sig[c] = sig_in[6 * (size_t)i + c];
            fin = fin && isfinite(sig[c]);
        }
        tex_point_features<NFP>(P, i, ntex, tex_in, tex_id, ft, fin);
        double f = __builtin_nan("");
        int st = 1;
        if (fin) {
            const double z[6] = {0., 0., 0., 0., 0., 0.};
            const TexSvcPoint<NFP> src(P, psv, pdu, ft);
            const YfTexSvc<NFP> pol(m, src);
            f = pol.full_ld(sig, z, nullptr, &st);
        }
        yf[i] = f;
        status[i] = st;
    }
}

// Material.response(sig, epl, deps, CV, maxit, tex=) at n points, one thread per point: response_point (response_light /
// response_heavy, shared with every other material) on YfTexSvc.  The material record `mat` -- elastic matrix, sy, khard, the
// Hill form of seq -- is one of the context's materials; the tables are the context's texture set.  A point with a non-finite
// sig, epl, deps, texture or flow stress is decided before the update starts: all outputs NaN, nsteps = -1; no loop of the
// update ever runs on a NaN input.
template <int NFP>
__global__ void __launch_bounds__(BLOCK)
k_tex_response(const MatDev *gmat, int nmat, int mat, const TexSvcPar P, const double *__restrict__ gsv,
               const double *__restrict__ gdu, int n, const double *__restrict__ sig_in, const double *__restrict__ epl_in,
               const double *__restrict__ deps_in, int ntex, const double *__restrict__ tex_in,
               const int32_t *__restrict__ tex_id, double *__restrict__ fy, double *__restrict__ sig_out,
               double *__restrict__ depl_out, double *__restrict__ ct_out, int32_t *__restrict__ nsteps, int maxit)
{
    __shared__ MatDev smat[MAXMAT];
    stage_materials(smat, gmat, nmat);
    const double *psv, *pdu;
    tex_tables<NFP>(P, gsv, gdu, psv, pdu);   // its barrier publishes smat as well
    const MatDev &m = smat[mat];
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        double sig[6], epl[6], deps[6], depl[6], Ct[21], ft[NFP], f = 0.;
        bool fin = true;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            sig[c] = sig_in[6 * (size_t)i + c];
            epl[c] = epl_in[6 * (size_t)i + c];
            deps[c] = deps_in[6 * (size_t)i + c];
            fin = fin && isfinite(sig[c]) && isfinite(epl[c]) && isfinite(deps[c]);
        }
        tex_point_features<NFP>(P, i, ntex, tex_in, tex_id, ft, fin);
        fin = fin && isfinite(sflow_of(m, epl));
        int ns = -1;
        if (fin) {
            const TexSvcPoint<NFP> src(P, psv, pdu, ft);
            const YfTexSvc<NFP> pol(m, src);
            ns = response_point(m, pol, sig, epl, deps, f, depl, Ct, maxit);
        } else {
            f = __builtin_nan("");
#pragma unroll
            for (int c = 0; c < 6; c++) sig[c] = depl[c] = f;
#pragma unroll
            for (int c = 0; c < 21; c++) Ct[c] = f;
        }
        fy[i] = f;
        nsteps[i] = ns;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            sig_out[6 * (size_t)i + c] = sig[c];
            depl_out[6 * (size_t)i + c] = depl[c];
        }
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) ct_out[36 * (size_t)i + r * 6 + c] = Ct[sym_idx(r, c)];
    }
}

}  // namespace plfx
