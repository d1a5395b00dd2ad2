// plfx_path.hpp -- Material.load_path: a material point driven along a load path of K increments, some
// components prescribed as strain and the others as stress, the whole path in one launch.
//   path_point<YF>   the step loop, the Newton loop of the stress-controlled components and the masked solve around
//                    response_point, which is shared with the response kernels and not copied
//   k_path_batch     one thread per path (KIND 1 | 2 | 5, the policies of k_response_batch)
//   k_path_row       16 lanes per path on the row policy of k_response_row; lane 0 of a row stores
// and, for the work-hardening SVC (kind 7), whose hardening modulus is state of the path:
//   k_path_batch<7>  one thread per path on the policy and the tables of k_response_batch<7>: the yardstick form
//   k_path_wh_wave   one wave per path on YfSvcWhT<1>, the policy of k_sweep_wh_wave; lane 0 of a wave stores
#pragma once

namespace plfx {

// what a load-path kernel takes besides the material.  Step-major results: record (k, i) of a [K][n][w] array lies at
// (k n + i) w, so the lanes of a wave store neighbouring records at each step.
struct PathArgs {
    int n, K;
    const double *dload;       // [K][nd][6], nd = n, or 1 with dl_stride = 0 (a path shared by the points: a wave-uniform address)
    int dl_stride;             // doubles from one point's increment to the next: 6 or 0
    const int32_t *control;    // [n] bit c: component c is stress-controlled; or null (strain control)
    const double *sig0, *epl0; // [n][6] or null (zeros)
    int maxit, newton;
    double stol, eps_cap;
    double *sig, *epl, *deps;  // [K][n][6]
    double *fy;                // [K][n]
    int32_t *nsteps, *newton_out;   // [K][n]
    int32_t *ksteps, *status;  // [n]
    double *ct;                // [n][36] or null
};

// ... and what the paths of a work-hardening SVC material take on top: the hardening modulus at the start of every path and
// the one after every accepted step.  A type of its own: the kernels on PathArgs keep their arguments.
struct PathArgsWh : PathArgs {
    const double *khard0;      // [n]
    double *khard;             // [K][n]
};

// Whether a path on policy YF carries the hardening modulus from step to step: the work-hardening policies do (their modulus
// is a by-product of every gradient evaluation), no other has such state.
template <class YF>
struct PathCarriesKh {
    static constexpr bool value = false;
};
template <int WAVE>
struct PathCarriesKh<YfSvcWhT<WAVE>> {
    static constexpr bool value = true;
};

// LDL^T of the masked tangent A = M Ct M + (I - M), M the 0/1 diagonal of the stress-controlled components `ctrl`, without
// pivoting, and the solve A x = M b.  Fully unrolled: every index is a constant, so nothing is addressed at run time and the
// arrays stay in registers.  Returns false when a pivot is zero or not finite (x is then not to be used).  Rows and columns of
// strain-controlled components are those of the identity: x is zero there.
__device__ __forceinline__ bool path_masked_solve(const double *Ct, int ctrl, const double *b, double *x)
{
#pragma clang fp contract(off)
    double L[21], y[6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) {
            const bool both = ((ctrl >> i) & 1) && ((ctrl >> j) & 1);
            L[sym_idx(i, j)] = both ? Ct[sym_idx(i, j)] : ((i == j) ? 1. : 0.);
        }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {   // column j: L[sym_idx(j, j)] becomes d_j, L[sym_idx(j, i)] becomes l_ij (i > j)
        double d = L[sym_idx(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[sym_idx(k, j)] * L[sym_idx(k, j)] * L[sym_idx(k, k)];
        ok = ok && (d != 0.) && (fabs(d) <= 1.7976931348623157e308);   // (a NaN fails the second test)
        L[sym_idx(j, j)] = d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = L[sym_idx(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[sym_idx(k, i)] * L[sym_idx(k, j)] * L[sym_idx(k, k)];
            L[sym_idx(j, i)] = s / d;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {   // L y = M b
        double s = ((ctrl >> i) & 1) ? b[i] : 0.;
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[sym_idx(k, i)] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {  // L^T x = D^-1 y
        double s = y[i] / L[sym_idx(i, i)];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[sym_idx(i, k)] * x[k];
        x[i] = s;
    }
    return ok;
}

// The policy a path hands to response_point: the kernel's own, under a type of its own.  response_point<YF> then keeps its one
// caller in the response kernels, and the compiler goes on inlining it there as it did before the path kernels existed
// (compiled with a second caller, k_response_row and k_response_batch<5> call it out of line; tools/kernel_resources_ab.py).
template <class YF>
struct PathYf : YF {
    __device__ __forceinline__ explicit PathYf(const YF &y) : YF(y) {}
};

// One trial of a thread kernel: response_point between memory and memory, out of line -- the setting in which the response
// kernels compile it.  Inlined into the step loop, among the path's own arithmetic, the compiler cuts the sub-divided phase
// into other basic blocks and contracts other products into its sums: the same operations in number, last bits that differ
// from k_response_batch's (seen on the Hill material at nsteps = maxit - 1).  The row kernel inlines it and has its bits.
template <class YF>
__device__ __noinline__ int path_trial(const MatDev &m, const YF &yf, const double *sig_in, const double *epl_in, const double *deps_in,
                                       int maxit, double *fy, double *sig_out, double *depl_out, double *ct_out)
{
    double sig[6], epl[6], deps[6], depl[6], Ct[21], f = 0.;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        sig[c] = sig_in[c];
        epl[c] = epl_in[c];
        deps[c] = deps_in[c];
    }
    const int ns = response_point(m, yf, sig, epl, deps, f, depl, Ct, maxit);
    *fy = f;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        sig_out[c] = sig[c];
        depl_out[c] = depl[c];
    }
#pragma unroll
    for (int c = 0; c < 21; c++) ct_out[c] = Ct[c];
    return ns;
}

// One path, point i of a.  `elastic`: the material has no yield function (kind 0): the trial is sig + CV deps with the tangent
// CV.  `store`: this lane writes the results (lane 0 of a row; every thread of k_path_batch).  Every value a row branches on
// is the same in its 16 lanes.  Loops: K steps, at most newton + 1 trials per step, the fixed counts of the solve.
// Contraction is off in this function: epl + depl is one rounded add of the rounded depl, as NumPy forms it between two
// response_batch calls, and no product formed here is fused into an addition of response_point.
// Work-hardening policies (PathCarriesKh, A = PathArgsWh): every trial of a step runs on a policy of its own that enters with
// the step's modulus kh, as k_response_batch<7> builds one from kh_in[i]; the accepted trial's modulus is the next step's.
// For every other policy none of this exists: the trial runs on the path's one policy object.
template <bool OUTLINE, class YF, class A>
__device__ __forceinline__ void path_point(const MatDev &m, const YF &yf, bool elastic, const A &a, int i, bool store)
{
#pragma clang fp contract(off)
    constexpr bool CARRY = PathCarriesKh<YF>::value;
    const PathYf<YF> pyf(yf);
    double kh = 0., kh2 = 0.;
    if constexpr (CARRY) kh = a.khard0[i];
    const int ctrl = a.control ? (a.control[i] & 63) : 0;
    const size_t n = (size_t)a.n;
    double sig[6], epl[6], tgt[6], Ct[21];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        sig[c] = a.sig0 ? a.sig0[6 * (size_t)i + c] : 0.;
        epl[c] = a.epl0 ? a.epl0[6 * (size_t)i + c] : 0.;
        tgt[c] = sig[c];
    }
#pragma unroll
    for (int c = 0; c < 21; c++) Ct[c] = m.CV[c];
    int status = 0, k = 0;
    for (; k < a.K; k++) {
        double deps[6], s2[6], depl[6], Ct2[21], f = 0.;
        const double *dl = a.dload + ((size_t)k * (a.dl_stride ? n : 1) + (a.dl_stride ? (size_t)i : 0)) * 6;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const double d = dl[c];
            const bool F = (ctrl >> c) & 1;
            tgt[c] = F ? tgt[c] + d : tgt[c];   // the stress target accumulates from the targets: one rounded add per step
            deps[c] = F ? 0. : d;
        }
        if (ctrl) {   // deps_F from the tangent of the last accepted step: Ct_FF deps_F = (t - sig)_F - Ct_FS deps_S
            double b[6], x[6], cs[6];
            symv(Ct, deps, cs);   // (deps is zero on F)
#pragma unroll
            for (int c = 0; c < 6; c++) b[c] = (tgt[c] - sig[c]) - cs[c];
            if (!path_masked_solve(Ct, ctrl, b, x)) {
                status = 2;
                break;
            }
#pragma unroll
            for (int c = 0; c < 6; c++) deps[c] = ((ctrl >> c) & 1) ? x[c] : deps[c];
        }
        int ns = 0, nw = 0;
        for (int trial = 0; trial <= a.newton; trial++) {
            double big = 0.;
            bool fin = true;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                fin = fin && (fabs(deps[c]) <= 1.7976931348623157e308);
                big = fmax(big, fabs(deps[c]));
            }
            if (!fin || big > a.eps_cap) {   // no trial on an increment that is not finite or beyond the cap
                status = 3;
                break;
            }
#pragma unroll
            for (int c = 0; c < 6; c++) s2[c] = sig[c];
            if (elastic) {
                double ds[6];
                symv(m.CV, deps, ds);
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    s2[c] = sig[c] + ds[c];
                    depl[c] = 0.;
                }
#pragma unroll
                for (int c = 0; c < 21; c++) Ct2[c] = m.CV[c];
                f = 0.;
                ns = 0;
            } else if constexpr (CARRY) {
                const PathYf<YF> tyf(YF(m, yf.sv, yf.dual, kh));
                if constexpr (OUTLINE)
                    ns = path_trial(m, tyf, sig, epl, deps, a.maxit, &f, s2, depl, Ct2);
                else
                    ns = response_point(m, tyf, s2, epl, deps, f, depl, Ct2, a.maxit);
                kh2 = tyf.kh();
            } else {
                if constexpr (OUTLINE)
                    ns = path_trial(m, pyf, sig, epl, deps, a.maxit, &f, s2, depl, Ct2);
                else
                    ns = response_point(m, pyf, s2, epl, deps, f, depl, Ct2, a.maxit);
            }
            if (!ctrl) break;
            double r[6], x[6];
            bool within = true;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                r[c] = s2[c] - tgt[c];
                if ((ctrl >> c) & 1) within = within && (fabs(r[c]) <= a.stol);   // (a NaN residual is not within)
            }
            if (within) break;
            if (trial == a.newton) {
                status = 1;
                break;
            }
            if (!path_masked_solve(Ct2, ctrl, r, x)) {
                status = 2;
                break;
            }
#pragma unroll
            for (int c = 0; c < 6; c++) deps[c] = ((ctrl >> c) & 1) ? deps[c] - x[c] : deps[c];
            nw++;
        }
        if (status) break;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            sig[c] = s2[c];
            epl[c] = epl[c] + depl[c];
        }
#pragma unroll
        for (int c = 0; c < 21; c++) Ct[c] = Ct2[c];
        if constexpr (CARRY) kh = kh2;
        if (store) {
            const size_t rec = (size_t)k * n + i;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                a.sig[6 * rec + c] = sig[c];
                a.epl[6 * rec + c] = epl[c];
                a.deps[6 * rec + c] = deps[c];
            }
            a.fy[rec] = f;
            a.nsteps[rec] = ns;
            a.newton_out[rec] = nw;
            if constexpr (CARRY) a.khard[rec] = kh;
        }
    }
    if (!store) return;
    a.ksteps[i] = k;
    a.status[i] = status;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int kk = k; kk < a.K; kk++) {   // steps the path did not complete: NaN, -1
        const size_t rec = (size_t)kk * n + i;
#pragma unroll
        for (int c = 0; c < 6; c++) a.sig[6 * rec + c] = a.epl[6 * rec + c] = a.deps[6 * rec + c] = nan;
        a.fy[rec] = nan;
        a.nsteps[rec] = -1;
        a.newton_out[rec] = -1;
        if constexpr (CARRY) a.khard[rec] = nan;
    }
    if (a.ct) {
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) a.ct[36 * (size_t)i + r * 6 + c] = Ct[sym_idx(r, c)];
    }
}

// Material.load_path on the n paths of material `mat`, one thread per path: block and grid as k_response_batch
template <int KIND>
__global__ void __launch_bounds__(BLOCK)
k_path_batch(const MatDev *gmat, int nmat, int mat, PathArgs a)
{
    __shared__ MatDev smat[MAXMAT];
    stage_materials(smat, gmat, nmat);
    __syncthreads();
    const MatDev &m = smat[mat];
    const typename YfOf<KIND>::type yf = YfOf<KIND>::make(m, nullptr, nullptr);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += gridDim.x * BLOCK)
        path_point<true>(m, yf, KIND == 1 && m.kind == 0, a, i, true);
}

// ... of the work-hardening SVC material `mat` (kind 7): the tables where k_response_batch<7> takes them from -- staged in
// dynamic LDS by stage_svc where they fit, read from device memory otherwise -- and the trial out of line through path_trial,
// so that a strain-controlled path has the bits of the host loop over plfx_response_batch_kh.
template <int KIND>
__global__ void __launch_bounds__(BLOCK)
k_path_batch(const MatDev *gmat, int nmat, int lds_doubles, int mat, PathArgsWh a)
{
    static_assert(KIND == 7, "the kinds without tables take PathArgs");
    __shared__ MatDev smat[MAXMAT];
    stage_materials(smat, gmat, nmat);
    __syncthreads();
    int svc_mat = -1;
    const double *sv = nullptr, *dual = nullptr;
    stage_svc(smat, nmat, dyn_lds, lds_doubles, svc_mat, sv, dual, KIND, mat);
    __syncthreads();
    const MatDev &m = smat[mat];
    const bool staged = (mat == svc_mat);
    const YfSvcWh yf(m, staged ? sv : m.sv, staged ? dual : m.dual, 0.);   // (every trial enters with its step's modulus)
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += gridDim.x * BLOCK)
        path_point<true>(m, yf, false, a, i, true);
}

// ... and one wave per path, blockDim / 64 paths per block: the policy of k_sweep_wh_wave, which splits the support-vector
// sums over the 64 lanes and closes each with wave_allsum, so that every lane holds the same bits and every value the wave
// branches on is wave-uniform; all other arithmetic runs redundantly in lock-step.  Lane 0 stores.  A path's sums depend on
// nsv alone, not on n, the path's place or the grid.  The trial goes through path_trial, out of line: the state of the path
// (sig, epl, targets, deps, two tangents, kh: some 100 doubles) then lies in scratch between two trials and not in registers
// across the sum loops -- inlined, the kernel spills 137 VGPRs around them (DESIGN.md section 45 has both sets of figures).
#ifdef PLFX_UNIT_MATERIALS
__global__ void __launch_bounds__(BLOCK)
k_path_wh_wave(const MatDev *__restrict__ gmat, int nmat, int lds_doubles, int mat, PathArgsWh a)
{
    __shared__ MatDev smat[MAXMAT];
    stage_materials(smat, gmat, nmat);
    __syncthreads();
    int svc_mat = -1;
    const double *sv = nullptr, *dual = nullptr;
    stage_svc(smat, nmat, dyn_lds, lds_doubles, svc_mat, sv, dual, 7, mat);
    __syncthreads();
    const MatDev &m = smat[mat];
    const bool staged = (mat == svc_mat);
    const YfSvcWhT<1> yf(m, staged ? sv : m.sv, staged ? dual : m.dual, 0.);
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int i = blockIdx.x * wpb + (threadIdx.x >> 6); i < a.n; i += gridDim.x * wpb)   // wave-uniform
        path_point<true>(m, yf, false, a, i, lane == 0);
}
#endif

// ... and 16 lanes per path for the row-kernel SVC material `mat` (tables in LDS or in device memory, column scales, texture
// field: the instantiations of k_response_row, and its grid)
template <bool INLDS, bool COLS = false, bool TEXF = false, class... TF>
__global__ void __launch_bounds__(512)
k_path_row(const MatDev *__restrict__ gmat, int nmat, int mat, PathArgs a, TF... tf)
{
    static_assert(sizeof...(TF) == (TEXF ? 1 : 0), "a texture-field instantiation takes the field, the others nothing");
    __shared__ MatDev smat[MAXMAT];
    stage_materials(smat, gmat, nmat);
    __syncthreads();
    const int npad = INLDS ? stage_svc_row(smat, mat) : smat[mat].rowpad;
    __syncthreads();
    const MatDev &m = smat[mat];
    const int l16 = threadIdx.x & 15, rpb = blockDim.x >> 4;
    for (int i = blockIdx.x * rpb + (threadIdx.x >> 4); i < a.n; i += gridDim.x * rpb) {  // row-uniform
        const auto yf = row_policy<4, INLDS, COLS>(m, npad, i, tf...);
        path_point<false>(m, yf, false, a, i, l16 == 0);
    }
}

}  // namespace plfx
