// plfx_tex.hpp -- the texture-dependent SVC yield function: an RBF C-SVC on the features
// [six stresses | tdim texture coefficients], every column standardised with its own mean and scale (the reference's
// StandardScaler on a txdat material, material.py:2347-2361), evaluated at points (k_tex_yf) and searched along rays
// (k_tex_yield_scale: the loci of examples/Texture/train_texture.py, every texture x every ray in one launch).
// Included from plfx_host.hpp (for TexSvcPar) after plfx_kernels.hpp; its kernels are launched by plfx_material.hip alone.  The set belongs to the context, not to a material record.
//
// Tables: nsv vectors of NFP feature slots, NFP = 8 / 12 / 16 the padded 6 + tdim, stored with a row stride of NFP + 2 doubles
// both in device memory and in LDS: the stride in dwords is then 4 (mod 8) x odd, so the 16 lanes of a row, which read 16
// consecutive vectors with ds_read_b64, fall on 16 different bank pairs (strides of 8 / 12 / 16 doubles would be 4-, 2- and
// 8-way conflicts).  Slots 6 + tdim .. NFP - 1 hold 0 in the table and in the point: their difference is an exact 0 and
// fma(0, 0, hh) = hh, so no result depends on the padding.  The two stride slots are never read.
// Lane contract of DESIGN section 27: 16 lanes per point / ray, svc_row_decision; the order of a point's sum depends on nsv
// alone.
#pragma once

namespace plfx {

constexpr int TEX_DMAX = 16;    // 6 stresses + up to 10 texture coefficients (SMO_DMAX of the training kernels)
constexpr int TEX_TMAX = 10;
constexpr int TEX_BLOCK = 512;

struct TexSvcPar {
    double mean[TEX_DMAX], scale[TEX_DMAX];   // per feature column; slots past 6 + tdim: 0 and 1
    double gamma, intercept;
    int32_t nsv, tdim, dev_only, staged;      // staged: the tables fit the dynamic LDS and are copied there by every block
};

__host__ __device__ constexpr int tex_stride(int nfp) { return nfp + 2; }

// the tables of the set: in dynamic LDS when staged (the barrier publishes them), else where they lie in device memory
template <int NFP>
__device__ __forceinline__ void tex_tables(const TexSvcPar &P, const double *gsv, const double *gdu, const double *&psv,
                                           const double *&pdu)
{
    psv = gsv, pdu = gdu;
    if (P.staged) {   // block-uniform
        const int nt = P.nsv * tex_stride(NFP);
        for (int i = threadIdx.x; i < nt; i += blockDim.x) dyn_lds[i] = gsv[i];
        for (int i = threadIdx.x; i < P.nsv; i += blockDim.x) dyn_lds[nt + i] = gdu[i];
        psv = dyn_lds, pdu = dyn_lds + nt;
    }
    __syncthreads();
}

// the stresses that enter the features: sig, or its deviator for a dev_only set (basic.sig_dev: the mean of the three normal
// components, summed in order, taken off each of them)
__device__ __forceinline__ void tex_stress(const TexSvcPar &P, const double *sig, double (&s)[6], bool &fin)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 6; c++) {
        s[c] = sig[c];
        fin = fin && isfinite(s[c]);
    }
    if (P.dev_only) {
        const double p = (s[0] + s[1] + s[2]) / 3.;
        s[0] = s[0] - p;
        s[1] = s[1] - p;
        s[2] = s[2] - p;
    }
}

// standardised texture features f[6 + t] = (tex_t - mean) / scale, true divisions; padding slots 0
template <int NFP>
__device__ __forceinline__ void tex_features(const TexSvcPar &P, const double *tex, double (&f)[NFP], bool &fin)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 6; j < NFP; j++) {
        f[j] = 0.;
        if (j - 6 < P.tdim) {
            const double t = tex[j - 6];
            fin = fin && isfinite(t);
            f[j] = (t - P.mean[j]) / P.scale[j];
        }
    }
}

// the decision function at the features f: the one vector loop of both kernels.  Squared distance from the differences in
// feature order; trips, row sum and intercept are svc_row_decision's.
template <int NFP>
__device__ __forceinline__ double tex_decision(const double *psv, const double *pdu, int nsv, double g, double intercept,
                                               const double (&f)[NFP])
{
    return svc_row_decision<tex_stride(NFP)>(psv, pdu, nsv, g, intercept, [&](const double *v, int) {
        double hh = 0.;
#pragma unroll
        for (int j = 0; j < NFP; j++) {
            const double d = f[j] - v[j];
            hh = fma(d, d, hh);
        }
        return hh;
    });
}

// calc_yf(sig, tex=) at n points.  The texture of point i: tex_id[i] when given, else row 0 (ntex = 1, shared) or row i
// (ntex = n).  A non-finite stress or texture component makes that point NaN and nothing else.
template <int NFP>
__global__ void __launch_bounds__(TEX_BLOCK)
k_tex_yf(const TexSvcPar P, const double *__restrict__ gsv, const double *__restrict__ gdu, int n,
         const double *__restrict__ sig_in, int ntex, const double *__restrict__ tex_in, const int32_t *__restrict__ tex_id,
         double *__restrict__ yf)
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
        double y = tex_decision<NFP>(psv, pdu, P.nsv, g, P.intercept, f);
        if (!fin) y = __builtin_nan("");
        if (l16 == 0) yf[i] = y;
    }
}

// yield_scale(su, tex=) on ntex x nray rays, texture-major: ray q = t nray + r runs along the unit stress r at the texture t.
// Only x moves along a ray: u_j = s_j / scale_j and c_j = mean_j / scale_j are set up once (s the deviator for a dev_only set),
// the texture features as in k_tex_yf, and every evaluation forms f_j = fma(x, u_j, -c_j) once -- not per vector -- before the
// vector loop of tex_decision.  The search, its caps and its status values 0 / 1 / 2 are ray_root's (plfx_rayroot.hpp), but
// written out in the kernel as k_hessian_row writes out its trips: called through ray_root the NFP = 12 instantiation is
// allocated 120 instead of 134 VGPRs, arranges an evaluation differently and measured 27.6 % slower on 432 rays, 2.4 % on
// 504 000.  A change to the search is made in both places; tests/test_gpu_texture.py holds this copy to
// the fixture's status and roots.  Status 3 is decided here: su = 0, a non-finite stress, texture or x0, x0 <= 0.
template <int NFP>
__global__ void __launch_bounds__(TEX_BLOCK)
k_tex_yield_scale(const TexSvcPar P, const double *__restrict__ gsv, const double *__restrict__ gdu, int nray,
                  const double *__restrict__ su_in, int ntex, const double *__restrict__ tex_in,
                  const double *__restrict__ x0_in, double *__restrict__ x_out, int32_t *__restrict__ status)
{
    const double *psv, *pdu;
    tex_tables<NFP>(P, gsv, gdu, psv, pdu);
    const int l16 = threadIdx.x & 15, rpb = blockDim.x >> 4;
    const int nq = ntex * nray;
    const double g = -P.gamma * LOG2E;
    for (int q = blockIdx.x * rpb + (threadIdx.x >> 4); q < nq; q += gridDim.x * rpb) {   // row-uniform
        const int t = q / nray, r = q - t * nray;
        double s[6], u[6], cc[6], f[NFP];
        bool fin = true, zero = true;
#pragma unroll
        for (int c = 0; c < 6; c++) zero = zero && su_in[6 * (size_t)r + c] == 0.;
        tex_stress(P, su_in + 6 * (size_t)r, s, fin);
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 6; j++) {
                u[j] = s[j] / P.scale[j];
                cc[j] = P.mean[j] / P.scale[j];
            }
        }
        tex_features<NFP>(P, tex_in + (size_t)t * P.tdim, f, fin);
        const double x0 = x0_in[q];
        int st = 0;
        double root = __builtin_nan("");
        if (!fin || zero || !isfinite(x0) || !(x0 > 0.)) st = 3;
        if (st == 0) {
            int phase = 0, cnt = 0;   // the search of ray_root, written out: see the comment above the kernel
            double x = x0, lo = 0., hi = 0., flo = 0., fhi = 0.;
            for (;;) {
                // ---- f(x): the decision function at x su (the only evaluation site)
#pragma unroll
                for (int j = 0; j < 6; j++) f[j] = fma(x, u[j], -cc[j]);
                const double fx = tex_decision<NFP>(psv, pdu, P.nsv, g, P.intercept, f);
                // ---- the search
                if (!(fx == fx)) {
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
        }
        if (l16 == 0) {
            x_out[q] = root;
            status[q] = st;
        }
    }
}

}  // namespace plfx
