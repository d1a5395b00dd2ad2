// plfx_svm.hpp — training of binary RBF C-SVC yield functions (Material.train_SVC, material.py:1596-1640): a batched SMO
// solver and a batched decision function.  Included from plfx.hip after its error helpers (fail, HIPCHK).
//
// The problem is libsvm's C-SVC dual, min 1/2 a'Qa - e'a, 0 <= a <= C, y'a = 0, Q_ij = y_i y_j exp(-g |x_i - x_j|^2), solved
// by libsvm's NON-shrinking solver step for step (Fan, Chen & Lin, JMLR 6, 2005; Chang & Lin, ACM TIST 2, 2011): a = 0,
// G = -e; second-order working-set selection with tau = 1e-12; the analytic two-variable update with clipping; G updated
// from both kernel rows; stop when m(a) - M(a) < tol; rho from the free a (midpoint of the bounds when none is free).
// The arithmetic is libsvm's as well: kernel rows in FP64 as exp(-g (|x_i|^2 + |x_j|^2 - 2 x_i.x_j)) stored as FP32
// (libsvm's Qfloat), a and G in FP64, no FMA contraction.  Ties in the selection go to the LAST index, as libsvm's
// `>=` / `<=` comparisons do, and the rows are in the order libsvm sees them inside scikit-learn: its class labels are
// sorted, so the rows of label -1 come first with internal label +1.  Shrinking (a CPU cache heuristic) is not built.
//
// Kernel shape: one workgroup (1024 threads, 16 waves) per problem (C, gamma, fold), all problems of a call in one
// launch, largest first.  The problems share one upload of X and y and pick their rows through an index list.  Thread t
// owns rows t, t + 1024, ...: their a, G, |x|^2, Q_ii and the FP32 entry of the current row i stay with it (global memory,
// L2-resident), so only the two reductions of an iteration cross threads, and the winner's own values ride along in the
// reduction slots.  Per iteration: a wave64 shuffle reduction + one LDS exchange for i (fused into the G update of the
// previous iteration), the row of i with the reduction for j, then the update with the row of j.  Two barriers per
// iteration; the LDS slots of the two reductions alternate, so no third barrier is needed.  No inter-workgroup traffic.
// A launch runs at most SMO_CHUNK iterations and leaves its state in HBM; the host resumes the problems that have not
// converged, bounded by max_iter.
#pragma once

namespace {

constexpr int SMO_BLOCK = 1024;
constexpr int SMO_WAVES = SMO_BLOCK / 64;
constexpr int SMO_DMAX = 16;
constexpr int SMO_CHUNK = 2048;   // iterations per launch: keeps a launch near 10-20 ms at n = 15 000
constexpr double SMO_TAU = 1e-12;

struct SmoArgs {
    const double *X;        // [n*d] shared features
    int d;
    const int32_t *off;     // [nprob+1] row range of each problem in the arrays below
    const int32_t *row;     // [total] row of X, in libsvm's order (label -1 first)
    const int8_t *yi;       // [total] libsvm's internal label: +1 for label -1, -1 for label +1
    const double *C, *gam;  // [nprob]
    const int32_t *maxit;   // [nprob]
    double *alpha, *G, *qd, *xsq;   // [total]
    float *qrow;            // [total] FP32 row of the current i (each entry written and read by its owner thread)
    int32_t *st;            // [2*nprob] iterations, state (0 running, 1 optimal, 2 max_iter reached)
    double tol;
};

struct SmoSlotA {
    double v, a;
    int idx;
};
struct SmoSlotB {
    double v, a, g, q, g2;
    int idx;
};

__device__ inline void smo_load_x(const double *X, int d, int r, double (&x)[SMO_DMAX])
{
#pragma unroll
    for (int f = 0; f < SMO_DMAX; f++) x[f] = f < d ? X[(size_t)r * d + f] : 0.;
}

// libsvm's Kernel::kernel_rbf, then (Qfloat)(y_i y_k K)
__device__ inline float smo_q(const double (&xi)[SMO_DMAX], double xsq_i, int yy, const double *X, int d, int r,
                              double xsq_k, double g)
{
#pragma clang fp contract(off)
    double dot = 0.;
#pragma unroll
    for (int f = 0; f < SMO_DMAX; f++)
        if (f < d) dot = dot + xi[f] * X[(size_t)r * d + f];
    const double t = (xsq_i + xsq_k) - 2. * dot;
    return (float)((double)yy * exp(-g * t));
}

__global__ void __launch_bounds__(256) k_smo_init(SmoArgs a)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    const int o = a.off[p], n = a.off[p + 1] - o;
    const double g = a.gam[p];
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const int r = a.row[o + k];
        double s = 0.;
        for (int f = 0; f < a.d; f++) s = s + a.X[(size_t)r * a.d + f] * a.X[(size_t)r * a.d + f];
        a.xsq[o + k] = s;
        a.qd[o + k] = exp(-g * ((s + s) - 2. * s));   // kernel(i, i) as libsvm's QD (double)
        a.alpha[o + k] = 0.;
        a.G[o + k] = -1.;
    }
    if (threadIdx.x == 0) a.st[2 * p] = a.st[2 * p + 1] = 0;
}

__global__ void __launch_bounds__(SMO_BLOCK) k_smo(SmoArgs a, const int32_t *active, int chunk)
{
#pragma clang fp contract(off)
    __shared__ SmoSlotA sa[SMO_WAVES];
    __shared__ SmoSlotB sb[SMO_WAVES];
    const int p = active[blockIdx.x];
    if (a.st[2 * p + 1] != 0) return;
    const int o = a.off[p], n = a.off[p + 1] - o;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double C = a.C[p], g = a.gam[p], tol = a.tol;
    const int d = a.d, maxit = a.maxit[p];
    double *al = a.alpha + o, *G = a.G + o;
    const double *qd = a.qd + o, *xsq = a.xsq + o;
    float *qr = a.qrow + o;
    const int32_t *row = a.row + o;
    const int8_t *yv = a.yi + o;
    const double INF = __builtin_huge_val();

    // candidate for i: max over I_up of -y G, ties to the last index (libsvm: `>=`)
    double av = -INF, aa = 0.;
    int ai = -1;
    for (int k = tid; k < n; k += SMO_BLOCK) {
        const double ak = al[k], gk = G[k];
        if (yv[k] > 0) {
            if (!(ak >= C) && -gk >= av) av = -gk, ai = k, aa = ak;
        } else if (!(ak <= 0.) && gk >= av) av = gk, ai = k, aa = ak;
    }
    int iter = a.st[2 * p], state = 0;
    for (int step = 0;; step++) {
        if (iter >= maxit) {
            state = 2;
            break;
        }
        if (step == chunk) break;
        // ---- reduction for i
        {
            double v = av;
            int ix = ai;
            for (int m = 32; m >= 1; m >>= 1) {
                const double v2 = __shfl_xor(v, m, 64);
                const int i2 = __shfl_xor(ix, m, 64);
                if (v2 > v || (v2 == v && i2 > ix)) v = v2, ix = i2;
            }
            if ((ix >= 0 && ai == ix) || (ix < 0 && lane == 0)) sa[wave] = SmoSlotA{v, aa, ix};
        }
        __syncthreads();
        double Gmax = -INF, alpha_i = 0.;
        int i = -1;
        for (int w = 0; w < SMO_WAVES; w++) {
            const SmoSlotA s = sa[w];
            if (s.v > Gmax || (s.v == Gmax && s.idx > i)) Gmax = s.v, i = s.idx, alpha_i = s.a;
        }
        if (i < 0) {   // Gmax = -INF: libsvm finds no j either
            state = 1;
            break;
        }
        i = __builtin_amdgcn_readfirstlane(i);   // uniform: the loads of row i's data become scalar loads
        const int y_i = yv[i];
        const double G_i = y_i > 0 ? -Gmax : Gmax, qd_i = qd[i], xsq_i = xsq[i];
        double xi[SMO_DMAX];
        smo_load_x(a.X, d, row[i], xi);

        // ---- row i, candidate for j (min of the second-order objective decrease, ties to the last index), and Gmax2
        double bv = INF, ba = 0., bg = 0., bq = 0., g2 = -INF;
        int bj = -1;
        for (int k = tid; k < n; k += SMO_BLOCK) {
            const int yk = yv[k];
            const float q = smo_q(xi, xsq_i, y_i * yk, a.X, d, row[k], xsq[k], g);
            qr[k] = q;
            const double ak = al[k], gk = G[k];
            if (yk > 0) {
                if (!(ak <= 0.)) {
                    const double gd = Gmax + gk;
                    if (gk >= g2) g2 = gk;
                    if (gd > 0.) {
                        const double quad = (qd_i + qd[k]) - (2.0 * y_i) * (double)q;
                        const double od = quad > 0. ? -(gd * gd) / quad : -(gd * gd) / SMO_TAU;
                        if (od <= bv) bv = od, bj = k, ba = ak, bg = gk, bq = q;
                    }
                }
            } else if (!(ak >= C)) {
                const double gd = Gmax - gk;
                if (-gk >= g2) g2 = -gk;
                if (gd > 0.) {
                    const double quad = (qd_i + qd[k]) + (2.0 * y_i) * (double)q;
                    const double od = quad > 0. ? -(gd * gd) / quad : -(gd * gd) / SMO_TAU;
                    if (od <= bv) bv = od, bj = k, ba = ak, bg = gk, bq = q;
                }
            }
        }
        {
            double v = bv, m2 = g2;
            int ix = bj;
            for (int m = 32; m >= 1; m >>= 1) {
                const double v2 = __shfl_xor(v, m, 64);
                const int i2 = __shfl_xor(ix, m, 64);
                m2 = fmax(m2, __shfl_xor(m2, m, 64));
                if (v2 < v || (v2 == v && i2 > ix)) v = v2, ix = i2;
            }
            if ((ix >= 0 && bj == ix) || (ix < 0 && lane == 0)) sb[wave] = SmoSlotB{v, ba, bg, bq, m2, ix};
        }
        __syncthreads();
        double omin = INF, alpha_j = 0., G_j = 0., Q_ij = 0., Gmax2 = -INF;
        int j = -1;
        for (int w = 0; w < SMO_WAVES; w++) {
            const SmoSlotB s = sb[w];
            Gmax2 = fmax(Gmax2, s.g2);
            if (s.v < omin || (s.v == omin && s.idx > j)) omin = s.v, j = s.idx, alpha_j = s.a, G_j = s.g, Q_ij = s.q;
        }
        if (Gmax + Gmax2 < tol || j < 0) {
            state = 1;
            break;
        }
        ++iter;
        j = __builtin_amdgcn_readfirstlane(j);

        // ---- the two-variable update (Solver::Solve), computed alike by every thread
        const int y_j = yv[j];
        const double qd_j = qd[j];
        double ni, nj;
        if (y_i != y_j) {
            double quad = (qd_i + qd_j) + 2. * Q_ij;
            if (quad <= 0.) quad = SMO_TAU;
            const double delta = (-G_i - G_j) / quad;
            const double diff = alpha_i - alpha_j;
            ni = alpha_i + delta;
            nj = alpha_j + delta;
            if (diff > 0.) {
                if (nj < 0.) nj = 0., ni = diff;
            } else if (ni < 0.) {
                ni = 0., nj = -diff;
            }
            if (diff > 0.) {   // C_i - C_j = 0
                if (ni > C) ni = C, nj = C - diff;
            } else if (nj > C) {
                nj = C, ni = C + diff;
            }
        } else {
            double quad = (qd_i + qd_j) - 2. * Q_ij;
            if (quad <= 0.) quad = SMO_TAU;
            const double delta = (G_i - G_j) / quad;
            const double sum = alpha_i + alpha_j;
            ni = alpha_i - delta;
            nj = alpha_j + delta;
            if (sum > C) {
                if (ni > C) ni = C, nj = sum - C;
            } else if (nj < 0.) {
                nj = 0., ni = sum;
            }
            if (sum > C) {
                if (nj > C) nj = C, ni = sum - C;
            } else if (ni < 0.) {
                ni = 0., nj = sum;
            }
        }
        const double dai = ni - alpha_i, daj = nj - alpha_j, xsq_j = xsq[j];
        double xj[SMO_DMAX];
        smo_load_x(a.X, d, row[j], xj);
        // ---- G from both rows, the new a, and the candidate for the next i
        av = -INF, ai = -1, aa = 0.;
        for (int k = tid; k < n; k += SMO_BLOCK) {
            const int yk = yv[k];
            const float qj = smo_q(xj, xsq_j, y_j * yk, a.X, d, row[k], xsq[k], g);
            const double gk = G[k] + ((double)qr[k] * dai + (double)qj * daj);
            G[k] = gk;
            double ak = al[k];
            if (k == i) al[k] = ak = ni;
            if (k == j) al[k] = ak = nj;
            if (yk > 0) {
                if (!(ak >= C) && -gk >= av) av = -gk, ai = k, aa = ak;
            } else if (!(ak <= 0.) && gk >= av) av = gk, ai = k, aa = ak;
        }
    }
    if (tid == 0) {
        a.st[2 * p] = iter;
        a.st[2 * p + 1] = state;
    }
}

// decision values sum_k coef_k exp(-g |x_q - x_k|^2) + intercept, k in the order given (libsvm's predict: the squared
// distance from the differences, terms summed in support-vector order); one thread per query point, blockIdx.y = problem
__global__ void __launch_bounds__(256) k_svc_decision(const double *X, int d, const int32_t *sv_off, const int32_t *sv_idx,
                                                      const double *coef, const double *icpt, const double *gam,
                                                      const int32_t *q_off, const int32_t *q_idx, double *out)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int q0 = q_off[p], nq = q_off[p + 1] - q0;
    if (t >= nq) return;
    double xq[SMO_DMAX];
    smo_load_x(X, d, q_idx[q0 + t], xq);
    const double g = gam[p];
    double s = 0.;
    for (int k = sv_off[p]; k < sv_off[p + 1]; k++) {
        const int r = sv_idx[k];
        double ss = 0.;
#pragma unroll
        for (int f = 0; f < SMO_DMAX; f++)
            if (f < d) {
                const double df = xq[f] - X[(size_t)r * d + f];
                ss = ss + df * df;
            }
        s = s + coef[k] * exp(-g * ss);
    }
    out[q0 + t] = s + icpt[p];
}

// device buffers of one call, released on every exit path
struct SvmBuffers {
    std::vector<void *> p;
    template <class T>
    int get(plfx_ctx *c, T **q, size_t n)
    {
        HIPCHK(c, hipMalloc((void **)q, std::max<size_t>(n, 1) * sizeof(T)));
        p.push_back(*q);
        return 0;
    }
    ~SvmBuffers()
    {
        for (void *q : p) hipFree(q);
    }
};

#define SVMCHK(call)           \
    do {                       \
        const int rc_ = (call); \
        if (rc_) return rc_;   \
    } while (0)

int svm_check_rows(plfx_ctx *c, const char *fn, int n, int d, const double *X, int nprob, const int32_t *off,
                   const int32_t *idx, const double *gamma)
{
    if (!c) return PLFX_ERR_ARG;
    if (n < 1 || !X || nprob < 1 || !off || !idx || !gamma) return fail(c, PLFX_ERR_ARG, "%s: null or empty argument", fn);
    if (d < 1 || d > SMO_DMAX) return fail(c, PLFX_ERR_ARG, "%s: d = %d features, 1 <= d <= %d supported", fn, d, SMO_DMAX);
    if (off[0] != 0) return fail(c, PLFX_ERR_ARG, "%s: offsets must start at 0", fn);
    for (int p = 0; p < nprob; p++) {
        if (off[p + 1] < off[p]) return fail(c, PLFX_ERR_ARG, "%s: offsets of problem %d decrease", fn, p);
        if (!(gamma[p] > 0.) || !std::isfinite(gamma[p]))
            return fail(c, PLFX_ERR_ARG, "%s: gamma of problem %d must be > 0 (got %g)", fn, p, gamma[p]);
    }
    for (int k = 0; k < off[nprob]; k++)
        if (idx[k] < 0 || idx[k] >= n) return fail(c, PLFX_ERR_ARG, "%s: row index %d at position %d out of range", fn, idx[k], k);
    for (size_t k = 0; k < (size_t)n * d; k++)
        if (!std::isfinite(X[k])) return fail(c, PLFX_ERR_ARG, "%s: X holds a non-finite value at %zu", fn, k);
    return 0;
}

// libsvm's Solver::calculate_rho (sequential, as there) on the internal labels
double smo_rho(int n, const double *al, const double *G, const int8_t *y, double C)
{
    double ub = __builtin_huge_val(), lb = -ub, sum = 0.;
    int nfree = 0;
    for (int k = 0; k < n; k++) {
        const double yG = y[k] * G[k];
        if (al[k] >= C) {
            if (y[k] == -1) ub = std::min(ub, yG);
            else lb = std::max(lb, yG);
        } else if (al[k] <= 0.) {
            if (y[k] == +1) ub = std::min(ub, yG);
            else lb = std::max(lb, yG);
        } else {
            ++nfree;
            sum += yG;
        }
    }
    return nfree > 0 ? sum / nfree : (ub + lb) / 2;
}

int svc_fit_batch_impl(plfx_ctx *c, int n, int d, const double *X, const double *y, int nprob, const int32_t *off,
                       const int32_t *idx, const double *C, const double *gamma, double tol, int64_t max_iter,
                       double *alpha, double *rho, double *obj, int32_t *iters, int32_t *status)
{
    SVMCHK(svm_check_rows(c, "plfx_svc_fit_batch", n, d, X, nprob, off, idx, gamma));
    if (!y || !C || !alpha || !rho || !iters || !status) return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_batch: null argument");
    if (!(tol > 0.) || !std::isfinite(tol)) return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_batch: tol must be > 0 (got %g)", tol);
    for (int k = 0; k < n; k++)
        if (y[k] != 1. && y[k] != -1.)
            return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_batch: label %g at row %d; binary labels -1 / +1 expected", y[k], k);
    const int total = off[nprob];
    std::vector<int32_t> hrow(total), hpos(total), hmax(nprob);
    std::vector<int8_t> hy(total);
    for (int p = 0; p < nprob; p++) {
        if (!(C[p] > 0.) || !std::isfinite(C[p]))
            return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_batch: C of problem %d must be > 0 (got %g)", p, C[p]);
        // libsvm's order: label -1 first (internal +1), then label +1, each in the caller's order
        int m = off[p];
        for (int pass = 0; pass < 2; pass++)
            for (int k = off[p]; k < off[p + 1]; k++)
                if ((y[idx[k]] < 0.) == (pass == 0)) {
                    hrow[m] = idx[k];
                    hpos[m] = k;
                    hy[m] = pass == 0 ? 1 : -1;
                    m++;
                }
        const int np = off[p + 1] - off[p];
        int nneg = 0;
        for (int k = off[p]; k < off[p + 1]; k++) nneg += hy[k] > 0;
        if (nneg == 0 || nneg == np)
            return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_batch: problem %d holds only one class", p);
        hmax[p] = (int)std::min<int64_t>(max_iter > 0 ? max_iter : std::max<int64_t>(10000000, 100 * (int64_t)np), INT32_MAX);
    }
    HIPCHK(c, hipSetDevice(c->device));
    SvmBuffers B;
    SmoArgs a;
    double *dX, *dC, *dg;
    int32_t *doff, *drow, *dmax, *dact;
    int8_t *dy;
    SVMCHK(B.get(c, &dX, (size_t)n * d));
    SVMCHK(B.get(c, &doff, nprob + 1));
    SVMCHK(B.get(c, &drow, total));
    SVMCHK(B.get(c, &dy, total));
    SVMCHK(B.get(c, &dC, nprob));
    SVMCHK(B.get(c, &dg, nprob));
    SVMCHK(B.get(c, &dmax, nprob));
    SVMCHK(B.get(c, &dact, nprob));
    SVMCHK(B.get(c, &a.alpha, total));
    SVMCHK(B.get(c, &a.G, total));
    SVMCHK(B.get(c, &a.qd, total));
    SVMCHK(B.get(c, &a.xsq, total));
    SVMCHK(B.get(c, &a.qrow, total));
    SVMCHK(B.get(c, &a.st, 2 * nprob));
    HIPCHK(c, hipMemcpyAsync(dX, X, (size_t)n * d * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(doff, off, (size_t)(nprob + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(drow, hrow.data(), (size_t)total * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dy, hy.data(), (size_t)total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dC, C, (size_t)nprob * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dg, gamma, (size_t)nprob * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dmax, hmax.data(), (size_t)nprob * 4, hipMemcpyHostToDevice, c->stream));
    a.X = dX, a.d = d, a.off = doff, a.row = drow, a.yi = dy, a.C = dC, a.gam = dg, a.maxit = dmax, a.tol = tol;
    hipLaunchKernelGGL(k_smo_init, dim3(nprob), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    // active problems, largest first; each launch advances every one of them by up to SMO_CHUNK iterations
    std::vector<int32_t> act(nprob), hst(2 * nprob, 0);
    for (int p = 0; p < nprob; p++) act[p] = p;
    std::stable_sort(act.begin(), act.end(), [&](int u, int v) { return off[u + 1] - off[u] > off[v + 1] - off[v]; });
    while (!act.empty()) {
        HIPCHK(c, hipMemcpyAsync(dact, act.data(), act.size() * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_smo, dim3((unsigned)act.size()), dim3(SMO_BLOCK), 0, c->stream, a, (const int32_t *)dact, SMO_CHUNK);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hst.data(), a.st, (size_t)nprob * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<int32_t> next;
        for (int p : act)
            if (hst[2 * p + 1] == 0) next.push_back(p);
        act.swap(next);
    }
    std::vector<double> hal(total), hG(total);
    HIPCHK(c, hipMemcpyAsync(hal.data(), a.alpha, (size_t)total * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hG.data(), a.G, (size_t)total * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int p = 0; p < nprob; p++) {
        const int o = off[p], np = off[p + 1] - o;
        // rho in the caller's label convention: decision = sum_k label_k alpha_k K(x, x_k) - rho (libsvm's is -rho)
        rho[p] = -smo_rho(np, &hal[o], &hG[o], &hy[o], C[p]);
        if (obj) {
            double v = 0.;
            for (int k = o; k < o + np; k++) v += hal[k] * (hG[k] - 1.);
            obj[p] = v / 2;
        }
        iters[p] = hst[2 * p];
        status[p] = hst[2 * p + 1] == 2 ? 1 : 0;
        for (int k = o; k < o + np; k++) alpha[hpos[k]] = hal[k];
    }
    return PLFX_OK;
}

int svc_decision_batch_impl(plfx_ctx *c, int n, int d, const double *X, int nprob, const int32_t *sv_off,
                            const int32_t *sv_idx, const double *coef, const double *intercept, const double *gamma,
                            const int32_t *q_off, const int32_t *q_idx, double *dec)
{
    SVMCHK(svm_check_rows(c, "plfx_svc_decision_batch", n, d, X, nprob, sv_off, sv_idx, gamma));
    SVMCHK(svm_check_rows(c, "plfx_svc_decision_batch", n, d, X, nprob, q_off, q_idx, gamma));
    if (!coef || !intercept || !dec) return fail(c, PLFX_ERR_ARG, "plfx_svc_decision_batch: null argument");
    const int nsv = sv_off[nprob], nq = q_off[nprob];
    if (nq == 0) return PLFX_OK;
    int qmax = 0;
    for (int p = 0; p < nprob; p++) qmax = std::max(qmax, q_off[p + 1] - q_off[p]);
    HIPCHK(c, hipSetDevice(c->device));
    SvmBuffers B;
    double *dX, *dcoef, *dic, *dg, *dout;
    int32_t *dsvo, *dsvi, *dqo, *dqi;
    SVMCHK(B.get(c, &dX, (size_t)n * d));
    SVMCHK(B.get(c, &dsvo, nprob + 1));
    SVMCHK(B.get(c, &dsvi, nsv));
    SVMCHK(B.get(c, &dcoef, nsv));
    SVMCHK(B.get(c, &dic, nprob));
    SVMCHK(B.get(c, &dg, nprob));
    SVMCHK(B.get(c, &dqo, nprob + 1));
    SVMCHK(B.get(c, &dqi, nq));
    SVMCHK(B.get(c, &dout, nq));
    HIPCHK(c, hipMemcpyAsync(dX, X, (size_t)n * d * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dsvo, sv_off, (size_t)(nprob + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (nsv) {
        HIPCHK(c, hipMemcpyAsync(dsvi, sv_idx, (size_t)nsv * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dcoef, coef, (size_t)nsv * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(dic, intercept, (size_t)nprob * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dg, gamma, (size_t)nprob * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dqo, q_off, (size_t)(nprob + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dqi, q_idx, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_svc_decision, dim3((unsigned)((qmax + 255) / 256), (unsigned)nprob), dim3(256), 0, c->stream,
                       dX, d, dsvo, dsvi, dcoef, dic, dg, dqo, dqi, dout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(dec, dout, (size_t)nq * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PLFX_OK;
}

#undef SVMCHK

}  // namespace
