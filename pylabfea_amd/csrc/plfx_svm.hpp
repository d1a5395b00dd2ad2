// plfx_svm.hpp — training of binary RBF C-SVC yield functions (Material.train_SVC, material.py:1596-1640): a batched SMO
// solver and a batched decision function.  Included from plfx_material.hip after the error helpers (fail, HIPCHK).
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

// libsvm's Kernel::kernel_rbf, then (Qfloat)(y_i y_k K): the entry from the dot product x_i.x_k summed feature by feature
__device__ inline float smo_qdot(double dot, double xsq_i, double xsq_k, int yy, double g)
{
#pragma clang fp contract(off)
    const double t = (xsq_i + xsq_k) - 2. * dot;
    return (float)((double)yy * exp(-g * t));
}

// x_i.x_k with x_k in registers (k_smo_wide) or in X (k_smo), features in order
template <int D>
__device__ inline double smo_dot(const double (&xi)[SMO_DMAX], const double (&xk)[D], int d)
{
#pragma clang fp contract(off)
    double dot = 0.;
#pragma unroll
    for (int f = 0; f < D; f++)
        if (f < d) dot = dot + xi[f] * xk[f];
    return dot;
}

__device__ inline float smo_q(const double (&xi)[SMO_DMAX], double xsq_i, int yy, const double *X, int d, int r,
                              double xsq_k, double g)
{
#pragma clang fp contract(off)
    double dot = 0.;
#pragma unroll
    for (int f = 0; f < SMO_DMAX; f++)
        if (f < d) dot = dot + xi[f] * X[(size_t)r * d + f];
    return smo_qdot(dot, xsq_i, xsq_k, yy, g);
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

// ---- the in-workgroup parts of an SMO iteration, shared by k_smo and k_smo_wide (same arithmetic, same order)

// candidate for i from one row: max over I_up of -y G, ties to the last index (libsvm: `>=`)
__device__ inline void smo_cand_i(int yk, double ak, double gk, double C, int k, double &av, int &ai, double &aa)
{
    if (yk > 0) {
        if (!(ak >= C) && -gk >= av) av = -gk, ai = k, aa = ak;
    } else if (!(ak <= 0.) && gk >= av) av = gk, ai = k, aa = ak;
}

// candidate for j from one row (min of the second-order objective decrease, ties to the last index) and Gmax2
__device__ inline void smo_cand_j(int yk, double ak, double gk, double qdk, float q, int k, double C, double Gmax, int y_i,
                                  double qd_i, double &bv, int &bj, double &ba, double &bg, double &bq, double &g2)
{
#pragma clang fp contract(off)
    if (yk > 0) {
        if (!(ak <= 0.)) {
            const double gd = Gmax + gk;
            if (gk >= g2) g2 = gk;
            if (gd > 0.) {
                const double quad = (qd_i + qdk) - (2.0 * y_i) * (double)q;
                const double od = quad > 0. ? -(gd * gd) / quad : -(gd * gd) / SMO_TAU;
                if (od <= bv) bv = od, bj = k, ba = ak, bg = gk, bq = q;
            }
        }
    } else if (!(ak >= C)) {
        const double gd = Gmax - gk;
        if (-gk >= g2) g2 = -gk;
        if (gd > 0.) {
            const double quad = (qd_i + qdk) + (2.0 * y_i) * (double)q;
            const double od = quad > 0. ? -(gd * gd) / quad : -(gd * gd) / SMO_TAU;
            if (od <= bv) bv = od, bj = k, ba = ak, bg = gk, bq = q;
        }
    }
}

// wave64 reductions; the result is exact and independent of the order of the rows (max / min with last-index ties)
__device__ inline void smo_wave_max(double &v, int &ix)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const double v2 = __shfl_xor(v, m, 64);
        const int i2 = __shfl_xor(ix, m, 64);
        if (v2 > v || (v2 == v && i2 > ix)) v = v2, ix = i2;
    }
}
__device__ inline void smo_wave_min(double &v, int &ix, double &m2)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const double v2 = __shfl_xor(v, m, 64);
        const int i2 = __shfl_xor(ix, m, 64);
        m2 = fmax(m2, __shfl_xor(m2, m, 64));
        if (v2 < v || (v2 == v && i2 > ix)) v = v2, ix = i2;
    }
}

// merge of per-wave (or per-workgroup) winners, slots in index order
template <int NS>
__device__ inline void smo_merge_a(const SmoSlotA *s, int ns, double &Gmax, int &i, double &alpha_i)
{
    for (int w = 0; w < (NS > 0 ? NS : ns); w++) {
        const SmoSlotA t = s[w];
        if (t.v > Gmax || (t.v == Gmax && t.idx > i)) Gmax = t.v, i = t.idx, alpha_i = t.a;
    }
}
template <int NS>
__device__ inline void smo_merge_b(const SmoSlotB *s, int ns, double &omin, int &j, double &alpha_j, double &G_j,
                                   double &Q_ij, double &Gmax2)
{
    for (int w = 0; w < (NS > 0 ? NS : ns); w++) {
        const SmoSlotB t = s[w];
        Gmax2 = fmax(Gmax2, t.g2);
        if (t.v < omin || (t.v == omin && t.idx > j)) omin = t.v, j = t.idx, alpha_j = t.a, G_j = t.g, Q_ij = t.q;
    }
}

// the two-variable update of Solver::Solve, computed alike by every thread
__device__ inline void smo_pair(int y_i, int y_j, double qd_i, double qd_j, double Q_ij, double G_i, double G_j,
                                double alpha_i, double alpha_j, double C, double &ni, double &nj)
{
#pragma clang fp contract(off)
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
}

// new G of one row from the two kernel rows
__device__ inline double smo_g_update(double gk, float qi, float qj, double dai, double daj)
{
#pragma clang fp contract(off)
    return gk + ((double)qi * dai + (double)qj * daj);
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

    double av = -INF, aa = 0.;
    int ai = -1;
    for (int k = tid; k < n; k += SMO_BLOCK) smo_cand_i(yv[k], al[k], G[k], C, k, av, ai, aa);
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
            smo_wave_max(v, ix);
            if ((ix >= 0 && ai == ix) || (ix < 0 && lane == 0)) sa[wave] = SmoSlotA{v, aa, ix};
        }
        __syncthreads();
        double Gmax = -INF, alpha_i = 0.;
        int i = -1;
        smo_merge_a<SMO_WAVES>(sa, SMO_WAVES, Gmax, i, alpha_i);
        if (i < 0) {   // Gmax = -INF: libsvm finds no j either
            state = 1;
            break;
        }
        i = __builtin_amdgcn_readfirstlane(i);   // uniform: the loads of row i's data become scalar loads
        const int y_i = yv[i];
        const double G_i = y_i > 0 ? -Gmax : Gmax, qd_i = qd[i], xsq_i = xsq[i];
        double xi[SMO_DMAX];
        smo_load_x(a.X, d, row[i], xi);

        // ---- row i, candidate for j and Gmax2
        double bv = INF, ba = 0., bg = 0., bq = 0., g2 = -INF;
        int bj = -1;
        for (int k = tid; k < n; k += SMO_BLOCK) {
            const int yk = yv[k];
            const float q = smo_q(xi, xsq_i, y_i * yk, a.X, d, row[k], xsq[k], g);
            qr[k] = q;
            smo_cand_j(yk, al[k], G[k], qd[k], q, k, C, Gmax, y_i, qd_i, bv, bj, ba, bg, bq, g2);
        }
        {
            double v = bv, m2 = g2;
            int ix = bj;
            smo_wave_min(v, ix, m2);
            if ((ix >= 0 && bj == ix) || (ix < 0 && lane == 0)) sb[wave] = SmoSlotB{v, ba, bg, bq, m2, ix};
        }
        __syncthreads();
        double omin = INF, alpha_j = 0., G_j = 0., Q_ij = 0., Gmax2 = -INF;
        int j = -1;
        smo_merge_b<SMO_WAVES>(sb, SMO_WAVES, omin, j, alpha_j, G_j, Q_ij, Gmax2);
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
        smo_pair(y_i, y_j, qd_i, qd_j, Q_ij, G_i, G_j, alpha_i, alpha_j, C, ni, nj);
        const double dai = ni - alpha_i, daj = nj - alpha_j, xsq_j = xsq[j];
        double xj[SMO_DMAX];
        smo_load_x(a.X, d, row[j], xj);
        // ---- G from both rows, the new a, and the candidate for the next i
        av = -INF, ai = -1, aa = 0.;
        for (int k = tid; k < n; k += SMO_BLOCK) {
            const int yk = yv[k];
            const float qj = smo_q(xj, xsq_j, y_j * yk, a.X, d, row[k], xsq[k], g);
            const double gk = smo_g_update(G[k], qr[k], qj, dai, daj);
            G[k] = gk;
            double ak = al[k];
            if (k == i) al[k] = ak = ni;
            if (k == j) al[k] = ak = nj;
            smo_cand_i(yk, ak, gk, C, k, av, ai, aa);
        }
    }
    if (tid == 0) {
        a.st[2 * p] = iter;
        a.st[2 * p + 1] = state;
    }
}

// ---- k_smo_wide: ONE problem over nwg workgroups (plfx_svc_fit_wide).  The same iteration sequence as k_smo bit for bit:
// the only values that cross threads are the arg-max for i, the arg-min for j (with their last-index ties and the
// winner's own a, G, Q_ij) and the max Gmax2; all three are exact and do not depend on how rows are partitioned, and the
// two-variable update is the same scalar arithmetic in every thread.  Rows go to threads in contiguous slices of R
// (thread t of the grid owns rows t R .. t R + R - 1); each thread keeps its rows' features, a, G, |x|^2, Q_ii, label and
// FP32 row-i entry in registers for the whole launch and writes a and G back at its end (resume, host rho).
//
// Exchange: two grid-wide all-gathers per iteration (select i; select j).  Each workgroup reduces its rows (wave
// shuffles + LDS, as k_smo), then ONE lane publishes the workgroup's record: the payload as 8-byte agent-scope atomic
// stores (sc1, write-through), s_waitcnt vmcnt(0), then the tag granule (epoch << 32 | index) -- cdna_hip_programming.md
// Guideline 16, recipe R1 with the flag folded into the record.  Wave 0 of every workgroup then sweeps the tags of all
// nwg records with relaxed agent-scope loads until every one carries this epoch, reads the payloads with the same sc1
// loads (no other load of the kernel reads bytes another workgroup writes in the launch, so the acquire is the wavefront
// fence of the Guideline's sc1 form), and reduces the records in slot order.  epoch = 2 (step + 1) - 1 for i and
// 2 (step + 1) for j, counted within the launch; the record block is zeroed by a memset before every launch.  One
// record per phase suffices: a workgroup overwrites its i record of step s + 1 only after it has seen every j record of
// step s, which every workgroup publishes after it has read all i records of step s (likewise for j).
// Every spin is bounded (SMOW_SPIN_TICKS of the 100 MHz s_memrealtime clock); on timeout, or when another workgroup has
// set the error word, all workgroups leave and the host reports PLFX_ERR_HIP.  The grid is at most one workgroup per CU
// and is launched with hipLaunchCooperativeKernel, which rejects a grid that cannot be co-resident.
constexpr int SMOW_BLOCK = 256;
constexpr int SMOW_WAVES = SMOW_BLOCK / 64;
constexpr int SMOW_CHUNK = 8192;   // iterations per launch
constexpr int SMOW_RMAX = 8;       // rows per thread; above this the problem goes to k_smo
constexpr uint64_t SMOW_SPIN_TICKS = 200000000ull;   // 2 s
constexpr int SMOW_A = 4, SMOW_B = 8;                // 8-byte words of the i and j records

typedef __attribute__((address_space(1))) unsigned long long smow_gu64;

struct SmoWideArgs {
    const double *X;
    int d, n, nwg;
    const int32_t *row;     // [n] row of X in libsvm's order
    const int8_t *yi;       // [n] internal labels
    const double *qd, *xsq; // [n]
    double *alpha, *G;      // [n]
    int32_t *st;            // [2] iterations, state
    unsigned long long *xch;   // [nwg * (SMOW_A + SMOW_B) + 2]: records, then the error word
    double C, g, tol;
    int maxit, chunk;
};

__device__ inline void smow_st(unsigned long long *p, unsigned long long v)
{
    __hip_atomic_store((smow_gu64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline unsigned long long smow_ld(const unsigned long long *p)
{
    return __hip_atomic_load((smow_gu64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline unsigned long long smow_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ inline double smow_dbl(unsigned long long v) { return __longlong_as_double((long long)v); }

// publish one record (the calling lane only): payload words, drain, then the tag word
__device__ inline void smow_publish(unsigned long long *rec, const double *w, int nw, int idx, unsigned epoch)
{
    for (int k = 0; k < nw; k++) smow_st(rec + k, smow_bits(w[k]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    smow_st(rec + nw, ((unsigned long long)epoch << 32) | (unsigned)idx);
}

// wave 0: wait until the tag word (offset tagw) of every record carries epoch; false on timeout or a foreign error
__device__ inline bool smow_wait(const SmoWideArgs &a, const unsigned long long *base, int stride, int tagw, unsigned epoch,
                                 int lane)
{
    unsigned long long *err = a.xch + (size_t)a.nwg * (SMOW_A + SMOW_B);
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        bool ok = true;
        for (int w = lane; w < a.nwg; w += 64) ok &= (unsigned)(smow_ld(base + (size_t)w * stride + tagw) >> 32) == epoch;
        if (__all(ok)) break;
        if (smow_ld(err) != 0) return false;
        if (__builtin_amdgcn_s_memrealtime() - t0 > SMOW_SPIN_TICKS) {
            if (lane == 0) smow_st(err, 1);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // every load of the records below is an sc1 load
    return true;
}

template <int R, int D>
__global__ void __launch_bounds__(SMOW_BLOCK, 1) k_smo_wide(SmoWideArgs a)
{
#pragma clang fp contract(off)
    __shared__ SmoSlotA sa[SMOW_WAVES];
    __shared__ SmoSlotB sb[SMOW_WAVES];
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wg = blockIdx.x;
    const int k0 = (wg * SMOW_BLOCK + tid) * R;
    const double C = a.C, g = a.g, tol = a.tol;
    const int d = a.d, n = a.n;
    const double INF = __builtin_huge_val();
    unsigned long long *recA = a.xch, *recB = a.xch + (size_t)a.nwg * SMOW_A;

    double x[R][D], al[R], G[R], xsq[R], qd[R];
    float qr[R];
    int yv[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int k = k0 + r;
        const bool own = k < n;
        const int rr = own ? a.row[k] : 0;
#pragma unroll
        for (int f = 0; f < D; f++) x[r][f] = own && f < d ? a.X[(size_t)rr * d + f] : 0.;
        al[r] = own ? a.alpha[k] : 0.;
        G[r] = own ? a.G[k] : 0.;
        xsq[r] = own ? a.xsq[k] : 0.;
        qd[r] = own ? a.qd[k] : 0.;
        yv[r] = own ? a.yi[k] : 0;   // label 0: a row that is not there is never a candidate
        qr[r] = 0.f;
    }
    if (tid == 0) bad = 0;

    double av = -INF, aa = 0.;
    int ai = -1;
#pragma unroll
    for (int r = 0; r < R; r++)
        if (yv[r] != 0) smo_cand_i(yv[r], al[r], G[r], C, k0 + r, av, ai, aa);
    int iter = a.st[0], state = 0;
    const int maxit = a.maxit;
    bool fault = false;
    for (int step = 0;; step++) {
        if (iter >= maxit) {
            state = 2;
            break;
        }
        if (step == a.chunk) break;
        const unsigned epA = 2u * (unsigned)step + 1u, epB = epA + 1u;
        // ---- selection of i: workgroup, then grid
        {
            double v = av;
            int ix = ai;
            smo_wave_max(v, ix);
            if ((ix >= 0 && ai == ix) || (ix < 0 && lane == 0)) sa[wave] = SmoSlotA{v, aa, ix};
        }
        __syncthreads();
        if (wave == 0) {
            if (lane == 0) {
                double Gm = -INF, ali = 0.;
                int ii = -1;
                smo_merge_a<SMOW_WAVES>(sa, SMOW_WAVES, Gm, ii, ali);
                const double w[2] = {Gm, ali};
                smow_publish(recA + (size_t)wg * SMOW_A, w, 2, ii, epA);
            }
            if (smow_wait(a, recA, SMOW_A, 2, epA, lane)) {
                // every lane takes the records w = lane, lane + 64, ... (merge order is immaterial: the result is exact)
                double v = -INF, al2 = 0.;
                int ix = -1;
                for (int w = lane; w < a.nwg; w += 64) {
                    const unsigned long long *r = recA + (size_t)w * SMOW_A;
                    const SmoSlotA t{smow_dbl(smow_ld(r)), smow_dbl(smow_ld(r + 1)), (int)(unsigned)smow_ld(r + 2)};
                    smo_merge_a<1>(&t, 1, v, ix, al2);
                }
                double vv = v;
                int iw = ix;
                smo_wave_max(vv, iw);
                if ((iw >= 0 && ix == iw) || (iw < 0 && lane == 0)) sa[0] = SmoSlotA{vv, al2, iw};
            } else if (lane == 0) {
                bad = 1;
            }
        }
        __syncthreads();
        if (bad) {
            fault = true;
            break;
        }
        const double Gmax = sa[0].v, alpha_i = sa[0].a;
        int i = sa[0].idx;
        if (i < 0) {
            state = 1;
            break;
        }
        i = __builtin_amdgcn_readfirstlane(i);
        const int y_i = a.yi[i];
        const double G_i = y_i > 0 ? -Gmax : Gmax, qd_i = a.qd[i], xsq_i = a.xsq[i];
        double xi[SMO_DMAX];
        smo_load_x(a.X, d, a.row[i], xi);

        // ---- row i, candidate for j and Gmax2
        double bv = INF, ba = 0., bg = 0., bq = 0., g2 = -INF;
        int bj = -1;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (yv[r] == 0) continue;
            const float q = smo_qdot(smo_dot<D>(xi, x[r], d), xsq_i, xsq[r], y_i * yv[r], g);
            qr[r] = q;
            smo_cand_j(yv[r], al[r], G[r], qd[r], q, k0 + r, C, Gmax, y_i, qd_i, bv, bj, ba, bg, bq, g2);
        }
        {
            double v = bv, m2 = g2;
            int ix = bj;
            smo_wave_min(v, ix, m2);
            if ((ix >= 0 && bj == ix) || (ix < 0 && lane == 0)) sb[wave] = SmoSlotB{v, ba, bg, bq, m2, ix};
        }
        __syncthreads();
        if (wave == 0) {
            if (lane == 0) {
                double om = INF, alj = 0., gj = 0., qij = 0., gm2 = -INF;
                int jj = -1;
                smo_merge_b<SMOW_WAVES>(sb, SMOW_WAVES, om, jj, alj, gj, qij, gm2);
                const double w[5] = {om, alj, gj, qij, gm2};
                smow_publish(recB + (size_t)wg * SMOW_B, w, 5, jj, epB);
            }
            if (smow_wait(a, recB, SMOW_B, 5, epB, lane)) {
                double v = INF, alj = 0., gj = 0., qij = 0., gm2 = -INF;
                int ix = -1;
                for (int w = lane; w < a.nwg; w += 64) {
                    const unsigned long long *r = recB + (size_t)w * SMOW_B;
                    const SmoSlotB t{smow_dbl(smow_ld(r)),     smow_dbl(smow_ld(r + 1)), smow_dbl(smow_ld(r + 2)),
                                     smow_dbl(smow_ld(r + 3)), smow_dbl(smow_ld(r + 4)), (int)(unsigned)smow_ld(r + 5)};
                    smo_merge_b<1>(&t, 1, v, ix, alj, gj, qij, gm2);
                }
                double vv = v, mm = gm2;
                int iw = ix;
                smo_wave_min(vv, iw, mm);
                if ((iw >= 0 && ix == iw) || (iw < 0 && lane == 0)) sb[0] = SmoSlotB{vv, alj, gj, qij, mm, iw};
            } else if (lane == 0) {
                bad = 1;
            }
        }
        __syncthreads();
        if (bad) {
            fault = true;
            break;
        }
        const double alpha_j = sb[0].a, G_j = sb[0].g, Q_ij = sb[0].q, Gmax2 = sb[0].g2;
        int j = sb[0].idx;
        if (Gmax + Gmax2 < tol || j < 0) {
            state = 1;
            break;
        }
        ++iter;
        j = __builtin_amdgcn_readfirstlane(j);

        // ---- the two-variable update, G from both rows, the new a, the candidate for the next i
        const int y_j = a.yi[j];
        const double qd_j = a.qd[j];
        double ni, nj;
        smo_pair(y_i, y_j, qd_i, qd_j, Q_ij, G_i, G_j, alpha_i, alpha_j, C, ni, nj);
        const double dai = ni - alpha_i, daj = nj - alpha_j, xsq_j = a.xsq[j];
        double xj[SMO_DMAX];
        smo_load_x(a.X, d, a.row[j], xj);
        av = -INF, ai = -1, aa = 0.;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (yv[r] == 0) continue;
            const float qj = smo_qdot(smo_dot<D>(xj, x[r], d), xsq_j, xsq[r], y_j * yv[r], g);
            G[r] = smo_g_update(G[r], qr[r], qj, dai, daj);
            if (k0 + r == i) al[r] = ni;
            if (k0 + r == j) al[r] = nj;
            smo_cand_i(yv[r], al[r], G[r], C, k0 + r, av, ai, aa);
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
        if (k0 + r < n) {
            a.alpha[k0 + r] = al[r];
            a.G[k0 + r] = G[r];
        }
    if (wg == 0 && tid == 0 && !fault) {
        a.st[0] = iter;
        a.st[1] = state;
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
    CallBuffers B;
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

template <int R, int D>
hipError_t smow_launch(int nwg, SmoWideArgs &a, hipStream_t s)
{
    void *args[] = {&a};
    return hipLaunchCooperativeKernel(reinterpret_cast<const void *>(&k_smo_wide<R, D>), dim3(nwg), dim3(SMOW_BLOCK), args, 0, s);
}

template <int R, int D>
int smow_resident(plfx_ctx *c)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, &k_smo_wide<R, D>, SMOW_BLOCK, 0) != hipSuccess) return 0;
    return nb;
}

// one problem over all rows of X on nwg workgroups (0: automatic); falls back to k_smo (plfx_svc_fit_batch) when the rows
// exceed SMOW_RMAX per thread of the largest grid
int svc_fit_wide_impl(plfx_ctx *c, int n, int d, const double *X, const double *y, double C, double gamma, double tol,
                      int64_t max_iter, int nwg, double *alpha, double *rho, double *obj, int32_t *iters, int32_t *status)
{
    if (!c) return PLFX_ERR_ARG;
    if (n < 1 || !X || !y || !alpha || !rho || !iters || !status) return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_wide: null or empty argument");
    if (nwg < 0) return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_wide: nwg = %d, must be >= 0 (0: automatic)", nwg);
    const int32_t off[2] = {0, n};
    std::vector<int32_t> idx(n);
    for (int k = 0; k < n; k++) idx[k] = k;
    const int cus = c->prop.multiProcessorCount;
    const int D = d <= 8 ? 8 : 16;
    int resident = 0;
    switch (D) {   // workgroups per CU the kernel admits (1 at most is used); R does not change the register budget class
    case 8: resident = smow_resident<SMOW_RMAX, 8>(c); break;
    default: resident = smow_resident<SMOW_RMAX, 16>(c); break;
    }
    const int gmax = std::min(cus, cus * std::max(resident, 0));
    const int64_t per_wg = (int64_t)SMOW_BLOCK * SMOW_RMAX;
    if (gmax < 1 || (nwg == 0 && (int64_t)n > per_wg * gmax))   // too many rows for registers: the one-workgroup solver
        return svc_fit_batch_impl(c, n, d, X, y, 1, off, idx.data(), &C, &gamma, tol, max_iter, alpha, rho, obj, iters, status);
    SVMCHK(svm_check_rows(c, "plfx_svc_fit_wide", n, d, X, 1, off, idx.data(), &gamma));
    if (!(C > 0.) || !std::isfinite(C)) return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_wide: C must be > 0 (got %g)", C);
    if (!(tol > 0.) || !std::isfinite(tol)) return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_wide: tol must be > 0 (got %g)", tol);
    if (nwg > gmax)
        return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_wide: nwg = %d exceeds the %d co-resident workgroups (one per CU)", nwg, gmax);
    if (nwg == 0) nwg = (int)std::max<int64_t>(1, (n + per_wg - 1) / per_wg);   // grows with n: fewest workgroups
    int R = 1;
    while ((int64_t)R * SMOW_BLOCK * nwg < n) R *= 2;
    if (R > SMOW_RMAX)
        return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_wide: %d rows need more than %d rows per thread on %d workgroups", n,
                    SMOW_RMAX, nwg);
    std::vector<int32_t> hrow(n), hpos(n);
    std::vector<int8_t> hy(n);
    int m = 0;
    for (int pass = 0; pass < 2; pass++)   // libsvm's order: label -1 first (internal +1)
        for (int k = 0; k < n; k++) {
            if (y[k] != 1. && y[k] != -1.)
                return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_wide: label %g at row %d; binary labels -1 / +1 expected", y[k], k);
            if ((y[k] < 0.) == (pass == 0)) hrow[m] = k, hpos[m] = k, hy[m] = pass == 0 ? 1 : -1, m++;
        }
    int nneg = 0;
    for (int k = 0; k < n; k++) nneg += hy[k] > 0;
    if (nneg == 0 || nneg == n) return fail(c, PLFX_ERR_ARG, "plfx_svc_fit_wide: the problem holds only one class");
    const int hmax = (int)std::min<int64_t>(max_iter > 0 ? max_iter : std::max<int64_t>(10000000, 100 * (int64_t)n), INT32_MAX);
    int coop = 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, c->device));
    if (!coop) return fail(c, PLFX_ERR_HIP, "plfx_svc_fit_wide: the device does not support cooperative launches");
    CallBuffers B;
    SmoArgs ia;
    double *dX, *dC, *dg;
    int32_t *doff, *drow, *dmax;
    int8_t *dy;
    unsigned long long *dx;
    const size_t nxch = (size_t)nwg * (SMOW_A + SMOW_B) + 2;
    SVMCHK(B.get(c, &dX, (size_t)n * d));
    SVMCHK(B.get(c, &doff, 2));
    SVMCHK(B.get(c, &drow, n));
    SVMCHK(B.get(c, &dy, n));
    SVMCHK(B.get(c, &dC, 1));
    SVMCHK(B.get(c, &dg, 1));
    SVMCHK(B.get(c, &dmax, 1));
    SVMCHK(B.get(c, &ia.alpha, n));
    SVMCHK(B.get(c, &ia.G, n));
    SVMCHK(B.get(c, &ia.qd, n));
    SVMCHK(B.get(c, &ia.xsq, n));
    SVMCHK(B.get(c, &ia.st, 2));
    SVMCHK(B.get(c, &dx, nxch));
    HIPCHK(c, hipMemcpyAsync(dX, X, (size_t)n * d * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(doff, off, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(drow, hrow.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dy, hy.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dC, &C, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dg, &gamma, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dmax, &hmax, 4, hipMemcpyHostToDevice, c->stream));
    ia.X = dX, ia.d = d, ia.off = doff, ia.row = drow, ia.yi = dy, ia.C = dC, ia.gam = dg, ia.maxit = dmax, ia.tol = tol;
    ia.qrow = nullptr;
    hipLaunchKernelGGL(k_smo_init, dim3(1), dim3(256), 0, c->stream, ia);   // a = 0, G = -1, |x|^2, Q_ii, st = 0
    HIPCHK(c, hipGetLastError());
    SmoWideArgs a;
    a.X = dX, a.d = d, a.n = n, a.nwg = nwg, a.row = drow, a.yi = dy, a.qd = ia.qd, a.xsq = ia.xsq, a.alpha = ia.alpha;
    a.G = ia.G, a.st = ia.st, a.xch = dx, a.C = C, a.g = gamma, a.tol = tol, a.maxit = hmax, a.chunk = SMOW_CHUNK;
    int32_t hst[2] = {0, 0};
    unsigned long long herr = 0;
    for (;;) {
        HIPCHK(c, hipMemsetAsync(dx, 0, nxch * 8, c->stream));   // records and the error word, before every launch
        hipError_t e = hipSuccess;
#define SMOW_CASE(RR, DD) \
    if (R == RR && D == DD) e = smow_launch<RR, DD>(nwg, a, c->stream);
        SMOW_CASE(1, 8) SMOW_CASE(2, 8) SMOW_CASE(4, 8) SMOW_CASE(8, 8)
        SMOW_CASE(1, 16) SMOW_CASE(2, 16) SMOW_CASE(4, 16) SMOW_CASE(8, 16)
#undef SMOW_CASE
        HIPCHK(c, e);
        HIPCHK(c, hipMemcpyAsync(hst, ia.st, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&herr, dx + nxch - 2, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (herr)
            return fail(c, PLFX_ERR_HIP, "plfx_svc_fit_wide: a grid-wide exchange timed out after %.1f s on %d workgroups "
                                         "(iteration %d); the fit was abandoned", SMOW_SPIN_TICKS * 1e-8, nwg, hst[0]);
        if (hst[1] != 0) break;
    }
    std::vector<double> hal(n), hG(n);
    HIPCHK(c, hipMemcpyAsync(hal.data(), ia.alpha, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hG.data(), ia.G, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rho[0] = -smo_rho(n, hal.data(), hG.data(), hy.data(), C);
    if (obj) {
        double v = 0.;
        for (int k = 0; k < n; k++) v += hal[k] * (hG[k] - 1.);
        obj[0] = v / 2;
    }
    iters[0] = hst[0];
    status[0] = hst[1] == 2 ? 1 : 0;
    for (int k = 0; k < n; k++) alpha[hpos[k]] = hal[k];
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
    CallBuffers B;
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

// ---- epsilon-SVR (Material.setup_fgrad_SVM, material.py:2058-2131): libsvm's solve_epsilon_svr on the same solver rules.
// A problem of l rows has 2l variables: k < l with sign +1 and linear term eps - t_k, k + l with sign -1 and eps + t_k;
// Q_ab = s_a s_b K(a mod l, b mod l); a = 0, G = p.  Selection, update, clipping, tie-break and stopping rule are the
// functions above, with the sign of a variable in the place of the internal label.  The rows stay in the caller's order
// (scikit-learn does not reorder regression rows).  k_svr is a sibling of k_smo, which is left as it was: thread t owns
// the ROWS t, t + 512, ... and with each row both of its variables, so the kernel entry K(i mod l, r) is computed once
// per row (libsvm's SVR_Q::get_Q: (Qfloat)K, then the two signs, which are exact) and serves r and r + l.  A thread
// keeps one candidate per half; the upper half wins ties, as its indices are the larger ones, which is the order in which
// libsvm's loop over 0 .. 2l - 1 meets them.  Reductions, LDS slots and barriers are those of k_smo.
struct SvrArgs {
    const double *X;        // [n*d] shared features
    int d;
    const int32_t *off;     // [nprob+1] row range of each problem
    const int32_t *row;     // [total] row of X, in the caller's order
    const double *t;        // [total] targets in that order
    const double *C, *gam, *eps;   // [nprob]
    const int32_t *maxit;   // [nprob]
    double *alpha, *G;      // [2*total]: problem p at 2 off[p]; variable k < l, then k + l
    double *qd, *xsq;       // [total]
    float *krow;            // [total] FP32 K(i mod l, r) of the current i
    int32_t *st;            // [2*nprob] iterations, state (0 running, 1 optimal, 2 max_iter reached)
    double tol;
};

__global__ void __launch_bounds__(256) k_svr_init(SvrArgs a)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    const int o = a.off[p], l = a.off[p + 1] - o;
    const double g = a.gam[p], eps = a.eps[p];
    double *al = a.alpha + 2 * (size_t)o, *G = a.G + 2 * (size_t)o;
    for (int k = threadIdx.x; k < l; k += blockDim.x) {
        const int r = a.row[o + k];
        double s = 0.;
        for (int f = 0; f < a.d; f++) s = s + a.X[(size_t)r * a.d + f] * a.X[(size_t)r * a.d + f];
        a.xsq[o + k] = s;
        a.qd[o + k] = exp(-g * ((s + s) - 2. * s));
        al[k] = al[k + l] = 0.;
        G[k] = eps - a.t[o + k];
        G[k + l] = eps + a.t[o + k];
    }
    if (threadIdx.x == 0) a.st[2 * p] = a.st[2 * p + 1] = 0;
}

// 512 threads: a thread carries two variables per row, so this is the work per thread of k_smo's 1024, and the 256
// registers a thread may then use hold both halves' candidates and the 16 feature loads in flight without scratch
constexpr int SVR_BLOCK = 512;
constexpr int SVR_WAVES = SVR_BLOCK / 64;

__global__ void __launch_bounds__(SVR_BLOCK) k_svr(SvrArgs a, const int32_t *active, int chunk)
{
#pragma clang fp contract(off)
    __shared__ SmoSlotA sa[SVR_WAVES];
    __shared__ SmoSlotB sb[SVR_WAVES];
    const int p = active[blockIdx.x];
    if (a.st[2 * p + 1] != 0) return;
    const int o = a.off[p], l = a.off[p + 1] - o;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double C = a.C[p], g = a.gam[p], tol = a.tol;
    const int d = a.d, maxit = a.maxit[p];
    double *al = a.alpha + 2 * (size_t)o, *G = a.G + 2 * (size_t)o;
    const double *qd = a.qd + o, *xsq = a.xsq + o;
    float *kr = a.krow + o;
    const int32_t *row = a.row + o;
    const double INF = __builtin_huge_val();

    double av = -INF, aa = 0.;
    int ai = -1;
    {
        double av2 = -INF, aa2 = 0.;
        int ai2 = -1;
        for (int r = tid; r < l; r += SVR_BLOCK) {
            smo_cand_i(1, al[r], G[r], C, r, av, ai, aa);
            smo_cand_i(-1, al[r + l], G[r + l], C, r + l, av2, ai2, aa2);
        }
        if (ai2 >= 0 && av2 >= av) av = av2, ai = ai2, aa = aa2;
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
            smo_wave_max(v, ix);
            if ((ix >= 0 && ai == ix) || (ix < 0 && lane == 0)) sa[wave] = SmoSlotA{v, aa, ix};
        }
        __syncthreads();
        double Gmax = -INF, alpha_i = 0.;
        int i = -1;
        smo_merge_a<SVR_WAVES>(sa, SVR_WAVES, Gmax, i, alpha_i);
        if (i < 0) {
            state = 1;
            break;
        }
        i = __builtin_amdgcn_readfirstlane(i);
        const int s_i = i < l ? 1 : -1, ri = i < l ? i : i - l;
        const double G_i = s_i > 0 ? -Gmax : Gmax, qd_i = qd[ri], xsq_i = xsq[ri];
        double xi[SMO_DMAX];
        smo_load_x(a.X, d, row[ri], xi);

        // ---- row i mod l once per row, candidates for j in both halves, Gmax2
        double bv = INF, ba = 0., bg = 0., bq = 0., g2 = -INF;
        int bj = -1;
        {
            double bv2 = INF, ba2 = 0., bg2 = 0., bq2 = 0.;
            int bj2 = -1;
            for (int r = tid; r < l; r += SVR_BLOCK) {
                const float K = smo_q(xi, xsq_i, 1, a.X, d, row[r], xsq[r], g);
                kr[r] = K;
                const float q = s_i > 0 ? K : -K;
                smo_cand_j(1, al[r], G[r], qd[r], q, r, C, Gmax, s_i, qd_i, bv, bj, ba, bg, bq, g2);
                smo_cand_j(-1, al[r + l], G[r + l], qd[r], -q, r + l, C, Gmax, s_i, qd_i, bv2, bj2, ba2, bg2, bq2, g2);
            }
            if (bj2 >= 0 && bv2 <= bv) bv = bv2, bj = bj2, ba = ba2, bg = bg2, bq = bq2;
        }
        {
            double v = bv, m2 = g2;
            int ix = bj;
            smo_wave_min(v, ix, m2);
            if ((ix >= 0 && bj == ix) || (ix < 0 && lane == 0)) sb[wave] = SmoSlotB{v, ba, bg, bq, m2, ix};
        }
        __syncthreads();
        double omin = INF, alpha_j = 0., G_j = 0., Q_ij = 0., Gmax2 = -INF;
        int j = -1;
        smo_merge_b<SVR_WAVES>(sb, SVR_WAVES, omin, j, alpha_j, G_j, Q_ij, Gmax2);
        if (Gmax + Gmax2 < tol || j < 0) {
            state = 1;
            break;
        }
        ++iter;
        j = __builtin_amdgcn_readfirstlane(j);

        // ---- the two-variable update, G of both halves from the two rows, the candidate for the next i
        const int s_j = j < l ? 1 : -1, rj = j < l ? j : j - l;
        const double qd_j = qd[rj];
        double ni, nj;
        smo_pair(s_i, s_j, qd_i, qd_j, Q_ij, G_i, G_j, alpha_i, alpha_j, C, ni, nj);
        const double dai = ni - alpha_i, daj = nj - alpha_j, xsq_j = xsq[rj];
        double xj[SMO_DMAX];
        smo_load_x(a.X, d, row[rj], xj);
        av = -INF, ai = -1, aa = 0.;
        double av2 = -INF, aa2 = 0.;
        int ai2 = -1;
        for (int r = tid; r < l; r += SVR_BLOCK) {
            const float Kj = smo_q(xj, xsq_j, 1, a.X, d, row[r], xsq[r], g), Ki = kr[r];
            const float qi = s_i > 0 ? Ki : -Ki, qj = s_j > 0 ? Kj : -Kj;
            const double gl = smo_g_update(G[r], qi, qj, dai, daj), gu = smo_g_update(G[r + l], -qi, -qj, dai, daj);
            G[r] = gl;
            G[r + l] = gu;
            double ak = al[r], au = al[r + l];
            if (r == i) al[r] = ak = ni;
            if (r == j) al[r] = ak = nj;
            if (r + l == i) al[r + l] = au = ni;
            if (r + l == j) al[r + l] = au = nj;
            smo_cand_i(1, ak, gl, C, r, av, ai, aa);
            smo_cand_i(-1, au, gu, C, r + l, av2, ai2, aa2);
        }
        if (ai2 >= 0 && av2 >= av) av = av2, ai = ai2, aa = aa2;
    }
    if (tid == 0) {
        a.st[2 * p] = iter;
        a.st[2 * p + 1] = state;
    }
}

// predictions of up to SVR_MMAX RBF models that share their training rows and gamma: K(x_q, x_r) once per pair, one
// accumulator per model, coef [n][SVR_MMAX] with zeros where a row is no support vector of a model (and in the unused
// columns).  Rows in order: adding an exact 0 K leaves an FP64 sum as it is, so every column is libsvm's sum over its
// support vectors in their order.  One thread per query point; the row loop is uniform, so the row and its coefficients
// are scalar loads shared by the wave.
constexpr int SVR_MMAX = 8;

// the row loop of the prediction, shared by k_svr_predict and k_response_svr (same code, same bits): one pass over the rows
// in row order, the distance formed feature by feature, one accumulator per model; s must come in zeroed
__device__ __forceinline__ void svr_row_sums(const double *__restrict__ X, int n, int d, double g,
                                             const double *__restrict__ coef, const double (&xq)[SMO_DMAX],
                                             double (&s)[SVR_MMAX])
{
#pragma clang fp contract(off)
    for (int r = 0; r < n; r++) {
        double ss = 0.;
#pragma unroll
        for (int f = 0; f < SMO_DMAX; f++)
            if (f < d) {
                const double df = xq[f] - X[(size_t)r * d + f];
                ss = ss + df * df;
            }
        const double k = exp(-g * ss);
#pragma unroll
        for (int c = 0; c < SVR_MMAX; c++) s[c] = s[c] + coef[(size_t)r * SVR_MMAX + c] * k;
    }
}

__global__ void __launch_bounds__(256) k_svr_predict(const double *__restrict__ X, int n, int d, double g,
                                                     const double *__restrict__ coef, const double *__restrict__ icpt, int m,
                                                     const double *__restrict__ Q, int nq, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq) return;
    double xq[SMO_DMAX];
    smo_load_x(Q, d, t, xq);
    double s[SVR_MMAX];
#pragma unroll
    for (int c = 0; c < SVR_MMAX; c++) s[c] = 0.;
    svr_row_sums(X, n, d, g, coef, xq, s);
#pragma unroll
    for (int c = 0; c < SVR_MMAX; c++)
        if (c < m) out[(size_t)t * m + c] = s[c] + icpt[c];
}

// ---- Material.response under the SVR flow rule (plfx_set_svr_flow; material.py:207-346 with ML_grad set).  The update is
// k_response_batch<7>'s (response_point on the work-hardening SVC policy); only the gradient source differs: every gradient
// evaluation standardises [sig | epl], takes the seven predictions from svr_row_sums -- k_svr_predict's loop, hence its bits --
// and scales them back: six components of the normal (not normalised) and the hardening modulus (not clipped), which
// replaces the point's modulus as calc_fgrad overwrites Material.khard (:752-764).  One launch per material with a rule:
// the tables are kernel arguments, the row loop is uniform across the wave and its loads are scalar.
static_assert(SVR_FLOW_M == SVR_MMAX, "SvrFlowDev carries one slot per accumulator of svr_row_sums");

struct YfSvrFlow : YfSvcWhT<0> {
    const SvrFlowDev &r;
    const double *__restrict__ X, *__restrict__ coef;   // r.X, r.coef as the kernel's own restrict arguments (scalar loads)
    __device__ YfSvrFlow(const MatDev &mm, const double *s, const double *d, double k0, const SvrFlowDev &rr,
                         const double *__restrict__ xx, const double *__restrict__ cc)
        : YfSvcWhT<0>(mm, s, d, k0), r(rr), X(xx), coef(cc) {}
    __device__ inline void fgrad(const double *s, const double *epl, double *a) const
    {
#pragma clang fp contract(off)
        double xq[SMO_DMAX], acc[SVR_MMAX];
#pragma unroll
        for (int f = 0; f < 6; f++) {   // StdScaler.transform: (x - mean) / scale
            xq[f] = (s[f] - r.fmean[f]) / r.fscale[f];
            xq[6 + f] = (epl[f] - r.fmean[6 + f]) / r.fscale[6 + f];
        }
#pragma unroll
        for (int f = 12; f < SMO_DMAX; f++) xq[f] = 0.;
#pragma unroll
        for (int c = 0; c < SVR_MMAX; c++) acc[c] = 0.;
        svr_row_sums(X, r.l, 12, r.gamma, coef, xq, acc);
#pragma unroll
        for (int c = 0; c < 6; c++) a[c] = (acc[c] + r.icpt[c]) * r.oscale[c] + r.omean[c];   // inverse_transform
        K = (acc[6] + r.icpt[6]) * r.oscale[6] + r.omean[6];
        touch = 1;
    }
    // ML_full_yf once a gradient evaluation of this call has overwritten khard.  The reference's khard is then a (1,) ARRAY
    // (sc_khard.inverse_transform(...)[0], :763), and so is get_sflow's result; in ML_full_yf `x0 = sflow` and `x1 = x0`
    // (:467, :474) are then ONE array that the in-place `*=` of both marches (:480, :486) and of the pure-shear correction
    // (:473) work on.  The march down to a negative and up to a non-negative yield function therefore ends with x0 = x1 =
    // sflow, `x1 < 5 sflow` (:484) never ends the second march, f0 = f1 fails the bracket test (:495) and the function
    // returns its conservative estimate seq - 0.85 sflow with the MARCHED value -- the first 2 % step outside the yield locus
    // along the ray -- instead of the root.  Every ML_full_yf of a call after its first gradient evaluation takes this path
    // (with a float khard, i.e. before it, the root search of YfSvcWhT::full_ld); reproduced as it is.
    __device__ inline double full(const double *s, const double *epl) const
    {
#pragma clang fp contract(off)
        if (!touch) return YfSvcWhT<0>::full(s, epl);
        const double seqv = seq(s);
        double x = sflow(epl);
        if (seqv < 0.01) return seqv - 0.85 * x;
        double su[6], xs[6];
#pragma unroll
        for (int i = 0; i < 6; i++) su[i] = s[i] / seqv;
        if (su[0] * su[1] < -1.e-5) x *= 0.5;
        auto f = [&](double v) {
#pragma unroll
            for (int i = 0; i < 6; i++) xs[i] = v * su[i];
            return plain(xs, epl);
        };
        double fx = f(x);
        while (fx >= 0. && x > 0.01) {   // :475-480
            x *= 0.98;
            fx = f(x);
        }
        while (fx < 0. && x < 5. * x) {  // :481-486: x1 < 5 sflow on the one array; false only once x has overflowed
            x *= 1.02;
            fx = f(x);
        }
        return seqv - 0.85 * x;          // f0 = f1: "could not bracket" (:495-499); an exact zero of f is not distinguished
    }
};

constexpr int SVR_FLOW_BLOCK = BLOCK;

__global__ void __launch_bounds__(SVR_FLOW_BLOCK)
k_response_svr(const MatDev *gmat, int nmat, int lds_doubles, int mat, const SvrFlowDev flow,
               const double *__restrict__ svr_X /* flow.X */, const double *__restrict__ svr_coef /* flow.coef */, int n, const int32_t *mat_id,
               const double *sig_in, const double *epl_in, const double *deps_in, double *fy, double *sig_out,
               double *depl_out, double *ct_out, int32_t *nsteps, const double *kh_in, double *kh_out, int maxit)
{
    __shared__ MatDev smat[MAXMAT];
    stage_materials(smat, gmat, nmat);
    __syncthreads();
    int svc_mat = -1;
    const double *sv = nullptr, *dual = nullptr;
    stage_svc(smat, nmat, dyn_lds, lds_doubles, svc_mat, sv, dual, 7, mat);   // this launch's material, if its tables fit
    __syncthreads();
    const MatDev &m = smat[mat];
    const bool staged = (mat == svc_mat);
    for (int i = blockIdx.x * SVR_FLOW_BLOCK + threadIdx.x; i < n; i += gridDim.x * SVR_FLOW_BLOCK) {
        if ((mat_id ? mat_id[i] : 0) != mat) continue;  // another material's launch
        double sig[6], epl[6], deps[6], depl[6], Ct[21], f = 0.;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            sig[c] = sig_in[6 * (size_t)i + c];
            epl[c] = epl_in[6 * (size_t)i + c];
            deps[c] = deps_in[6 * (size_t)i + c];
        }
        const YfSvrFlow yf(m, staged ? sv : m.sv, staged ? dual : m.dual, kh_in[i], flow, svr_X, svr_coef);
        const int ns = response_point(m, yf, sig, epl, deps, f, depl, Ct, maxit);
        kh_out[i] = yf.kh();
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

int svr_fit_batch_impl(plfx_ctx *c, int n, int d, const double *X, int nprob, const int32_t *off, const int32_t *idx,
                       const double *t, const double *C, const double *gamma, const double *epsilon, double tol,
                       int64_t max_iter, double *coef, double *rho, double *obj, int32_t *iters, int32_t *status)
{
    SVMCHK(svm_check_rows(c, "plfx_svr_fit_batch", n, d, X, nprob, off, idx, gamma));
    if (!t || !C || !epsilon || !coef || !rho || !iters || !status)
        return fail(c, PLFX_ERR_ARG, "plfx_svr_fit_batch: null argument");
    if (!(tol > 0.) || !std::isfinite(tol)) return fail(c, PLFX_ERR_ARG, "plfx_svr_fit_batch: tol must be > 0 (got %g)", tol);
    const int total = off[nprob];
    if ((int64_t)total * 2 > INT32_MAX) return fail(c, PLFX_ERR_ARG, "plfx_svr_fit_batch: too many rows (%d)", total);
    std::vector<int32_t> hmax(nprob);
    for (int p = 0; p < nprob; p++) {
        if (!(C[p] > 0.) || !std::isfinite(C[p]))
            return fail(c, PLFX_ERR_ARG, "plfx_svr_fit_batch: C of problem %d must be > 0 (got %g)", p, C[p]);
        if (!(epsilon[p] >= 0.) || !std::isfinite(epsilon[p]))
            return fail(c, PLFX_ERR_ARG, "plfx_svr_fit_batch: epsilon of problem %d must be >= 0 (got %g)", p, epsilon[p]);
        const int l = off[p + 1] - off[p];
        if (l < 1) return fail(c, PLFX_ERR_ARG, "plfx_svr_fit_batch: problem %d holds no row", p);
        // libsvm counts the 2l variables of the solver
        hmax[p] = (int)std::min<int64_t>(max_iter > 0 ? max_iter : std::max<int64_t>(10000000, 200 * (int64_t)l), INT32_MAX);
    }
    for (int k = 0; k < total; k++)
        if (!std::isfinite(t[k])) return fail(c, PLFX_ERR_ARG, "plfx_svr_fit_batch: target %d is not finite", k);
    HIPCHK(c, hipSetDevice(c->device));
    CallBuffers B;
    SvrArgs a;
    double *dX, *dC, *dg, *de, *dt;
    int32_t *doff, *drow, *dmax, *dact;
    SVMCHK(B.get(c, &dX, (size_t)n * d));
    SVMCHK(B.get(c, &doff, nprob + 1));
    SVMCHK(B.get(c, &drow, total));
    SVMCHK(B.get(c, &dt, total));
    SVMCHK(B.get(c, &dC, nprob));
    SVMCHK(B.get(c, &dg, nprob));
    SVMCHK(B.get(c, &de, nprob));
    SVMCHK(B.get(c, &dmax, nprob));
    SVMCHK(B.get(c, &dact, nprob));
    SVMCHK(B.get(c, &a.alpha, 2 * (size_t)total));
    SVMCHK(B.get(c, &a.G, 2 * (size_t)total));
    SVMCHK(B.get(c, &a.qd, total));
    SVMCHK(B.get(c, &a.xsq, total));
    SVMCHK(B.get(c, &a.krow, total));
    SVMCHK(B.get(c, &a.st, 2 * nprob));
    HIPCHK(c, hipMemcpyAsync(dX, X, (size_t)n * d * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(doff, off, (size_t)(nprob + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(drow, idx, (size_t)total * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dt, t, (size_t)total * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dC, C, (size_t)nprob * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dg, gamma, (size_t)nprob * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(de, epsilon, (size_t)nprob * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dmax, hmax.data(), (size_t)nprob * 4, hipMemcpyHostToDevice, c->stream));
    a.X = dX, a.d = d, a.off = doff, a.row = drow, a.t = dt, a.C = dC, a.gam = dg, a.eps = de, a.maxit = dmax, a.tol = tol;
    hipLaunchKernelGGL(k_svr_init, dim3(nprob), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    std::vector<int32_t> act(nprob), hst(2 * nprob, 0);
    for (int p = 0; p < nprob; p++) act[p] = p;
    std::stable_sort(act.begin(), act.end(), [&](int u, int v) { return off[u + 1] - off[u] > off[v + 1] - off[v]; });
    while (!act.empty()) {
        HIPCHK(c, hipMemcpyAsync(dact, act.data(), act.size() * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_svr, dim3((unsigned)act.size()), dim3(SVR_BLOCK), 0, c->stream, a, (const int32_t *)dact, SMO_CHUNK);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hst.data(), a.st, (size_t)nprob * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<int32_t> next;
        for (int p : act)
            if (hst[2 * p + 1] == 0) next.push_back(p);
        act.swap(next);
    }
    std::vector<double> hal(2 * (size_t)total), hG(2 * (size_t)total);
    HIPCHK(c, hipMemcpyAsync(hal.data(), a.alpha, hal.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hG.data(), a.G, hG.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int8_t> sgn;
    for (int p = 0; p < nprob; p++) {
        const int o = off[p], l = off[p + 1] - o;
        const double *al = &hal[2 * (size_t)o], *G = &hG[2 * (size_t)o];
        sgn.assign(2 * (size_t)l, 1);
        std::fill(sgn.begin() + l, sgn.end(), (int8_t)-1);
        rho[p] = smo_rho(2 * l, al, G, sgn.data(), C[p]);   // libsvm's rho: prediction = sum_k coef_k K(x, x_k) - rho
        if (obj) {
            double v = 0.;
            for (int k = 0; k < l; k++) v += al[k] * (G[k] + (epsilon[p] - t[o + k]));
            for (int k = 0; k < l; k++) v += al[k + l] * (G[k + l] + (epsilon[p] + t[o + k]));
            obj[p] = v / 2;
        }
        iters[p] = hst[2 * p];
        status[p] = hst[2 * p + 1] == 2 ? 1 : 0;
        for (int k = 0; k < l; k++) coef[o + k] = al[k] - al[k + l];
    }
    return PLFX_OK;
}

int svr_predict_multi_impl(plfx_ctx *c, int n, int d, const double *X, double gamma, int m, const double *coef,
                           const double *intercept, int nq, const double *Q, double *out)
{
    if (!c) return PLFX_ERR_ARG;
    if (n < 1 || !X || !coef || !intercept || nq < 0 || (nq > 0 && (!Q || !out)))
        return fail(c, PLFX_ERR_ARG, "plfx_svr_predict_multi: null or empty argument");
    if (d < 1 || d > SMO_DMAX)
        return fail(c, PLFX_ERR_ARG, "plfx_svr_predict_multi: d = %d features, 1 <= d <= %d supported", d, SMO_DMAX);
    if (m < 1 || m > SVR_MMAX)
        return fail(c, PLFX_ERR_ARG, "plfx_svr_predict_multi: m = %d models, 1 <= m <= %d supported", m, SVR_MMAX);
    if (!(gamma > 0.) || !std::isfinite(gamma))
        return fail(c, PLFX_ERR_ARG, "plfx_svr_predict_multi: gamma must be > 0 (got %g)", gamma);
    if (nq == 0) return PLFX_OK;
    std::vector<double> hc((size_t)n * SVR_MMAX, 0.), hi(SVR_MMAX, 0.);
    for (int r = 0; r < n; r++)
        for (int k = 0; k < m; k++) hc[(size_t)r * SVR_MMAX + k] = coef[(size_t)r * m + k];
    for (int k = 0; k < m; k++) hi[k] = intercept[k];
    HIPCHK(c, hipSetDevice(c->device));
    CallBuffers B;
    double *dX, *dc, *di, *dQ, *dout;
    SVMCHK(B.get(c, &dX, (size_t)n * d));
    SVMCHK(B.get(c, &dc, hc.size()));
    SVMCHK(B.get(c, &di, hi.size()));
    SVMCHK(B.get(c, &dQ, (size_t)nq * d));
    SVMCHK(B.get(c, &dout, (size_t)nq * m));
    HIPCHK(c, hipMemcpyAsync(dX, X, (size_t)n * d * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dc, hc.data(), hc.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(di, hi.data(), hi.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dQ, Q, (size_t)nq * d * 8, hipMemcpyHostToDevice, c->stream));
    EvPair *ev;
    tim_begin(c, 0, &ev);   // family 0, like the other batched point kernels: the kernel alone, without the copies
    hipLaunchKernelGGL(k_svr_predict, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, c->stream, (const double *)dX, n, d,
                       gamma, (const double *)dc, (const double *)di, m, (const double *)dQ, nq, dout);
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)nq * m * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PLFX_OK;
}

int set_svr_flow_impl(plfx_ctx *c, int mat, int l, const double *X, const double *coef, const double *intercept, double gamma,
                      const double *feat_mean, const double *feat_scale, const double *out_mean, const double *out_scale)
{
    if (!c) return PLFX_ERR_ARG;
    if (!c->dmat) return fail(c, PLFX_ERR_STATE, "set_materials first");
    if (mat < 0 || mat >= c->nmat) return fail(c, PLFX_ERR_ARG, "plfx_set_svr_flow: material %d out of range", mat);
    if (l < 0) return fail(c, PLFX_ERR_ARG, "plfx_set_svr_flow: l = %d rows", l);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_sync(c));   // no launch may still read the tables that go
    if (l == 0) {
        free_svr_flow(c, mat);
        return PLFX_OK;
    }
    if (c->hmat[mat].kind != PLFX_SVC_WH)
        return fail(c, PLFX_ERR_UNSUPPORTED, "plfx_set_svr_flow: material %d is of kind %d; an SVR flow rule attaches to a "
                    "6-feature work-hardening SVC material (PLFX_SVC_WH) only", mat, c->hmat[mat].kind);
    if (!X || !coef || !intercept || !feat_mean || !feat_scale || !out_mean || !out_scale)
        return fail(c, PLFX_ERR_ARG, "plfx_set_svr_flow: null argument");
    if (!(gamma > 0.) || !std::isfinite(gamma)) return fail(c, PLFX_ERR_ARG, "plfx_set_svr_flow: gamma must be > 0 (got %g)", gamma);
    for (int f = 0; f < 12; f++)
        if (!std::isfinite(feat_mean[f]) || !std::isfinite(feat_scale[f]) || feat_scale[f] == 0.)
            return fail(c, PLFX_ERR_ARG, "plfx_set_svr_flow: feature %d has no finite mean and non-zero scale", f);
    for (int k = 0; k < 7; k++)
        if (!std::isfinite(out_mean[k]) || !std::isfinite(out_scale[k]) || !std::isfinite(intercept[k]))
            return fail(c, PLFX_ERR_ARG, "plfx_set_svr_flow: output %d has no finite intercept, mean and scale", k);
    SvrFlowDev f = SvrFlowDev();
    std::vector<double> hc((size_t)l * SVR_MMAX, 0.);
    for (int r = 0; r < l; r++)
        for (int k = 0; k < 7; k++) hc[(size_t)r * SVR_MMAX + k] = coef[(size_t)r * 7 + k];
    double *dX = nullptr, *dc = nullptr;
    HIPCHK(c, hipMalloc((void **)&dX, (size_t)l * 12 * 8));
    if (hipMalloc((void **)&dc, hc.size() * 8) != hipSuccess) {
        hipFree(dX);
        return fail(c, PLFX_ERR_HIP, "plfx_set_svr_flow: out of device memory");
    }
    if (hipMemcpy(dX, X, (size_t)l * 12 * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dc, hc.data(), hc.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(dX);
        hipFree(dc);
        return fail(c, PLFX_ERR_HIP, "plfx_set_svr_flow: copy to the device failed");
    }
    f.X = dX, f.coef = dc, f.l = l, f.gamma = gamma;
    for (int k = 0; k < 7; k++) f.icpt[k] = intercept[k], f.omean[k] = out_mean[k], f.oscale[k] = out_scale[k];
    for (int k = 0; k < 12; k++) f.fmean[k] = feat_mean[k], f.fscale[k] = feat_scale[k];
    free_svr_flow(c, mat);
    c->svr_flow[mat] = f;
    c->svr_mask |= 1u << mat;
    return PLFX_OK;
}

#undef SVMCHK

}  // namespace
