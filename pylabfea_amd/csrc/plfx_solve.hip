// plfx_solve.hip -- libplfx.so: the linear solve of a load step: PCG with the Jacobi or the multigrid preconditioner, the
// interpolated start and its tests, restarted GMRES for an indefinite tangent stiffness, the fall-back to Jacobi.
// Unit map and the one-owner rule for kernels: DESIGN.md sections 39 and 42; what the units share: plfx_host.hpp.
#define PLFX_UNIT_SOLVE
#include "plfx_host.hpp"
#include "plfx_mg.hpp"

using namespace plfx;
using namespace plfx::host;

namespace plfx {
namespace host {

// launch k_cg_check and fetch the scalars: through the pinned mailbox (host spins on the sequence number) or, without
// it, by a device->host copy + stream synchronisation
// post: launch k_cg_check (with the mailbox: it also publishes the scalars); wait: fetch them.  Work enqueued between the
// two overlaps the round trip.
unsigned long long cg_check_post(plfx_ctx *c, const double *part_rr, int gn, int it_done)
{
    if (!c->mbox) {
        hipLaunchKernelGGL(k_cg_check, dim3(1), dim3(BLOCK), 0, c->stream, part_rr, gn, c->sc, it_done,
                           (CgMbox *)nullptr, 0ull);
        return 0;
    }
    const unsigned long long seq = ++c->mbox_seq;
    hipLaunchKernelGGL(k_cg_check, dim3(1), dim3(BLOCK), 0, c->stream, part_rr, gn, c->sc, it_done, c->mbox, seq);
    return seq;
}

// the set-up of the scalars (k_cg_setup) and the first test in one launch
unsigned long long cg_setup_check_post(plfx_ctx *c, const double *part_bb, const double *part_rr, int gn, double rtol)
{
    const unsigned long long seq = c->mbox ? ++c->mbox_seq : 0ull;
    hipLaunchKernelGGL(k_cg_setup_check, dim3(1), dim3(BLOCK), 0, c->stream, part_bb, part_rr, gn, rtol, c->sc, 0, c->mbox, seq);
    return seq;
}

int cg_check_wait(plfx_ctx *c, unsigned long long seq, CgScalars *hs)
{
    if (!c->mbox) {  // note: waits for everything enqueued so far
        HIPCHK(c, hipMemcpyAsync(hs, c->sc, sizeof(*hs), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
        return 0;
    }
    HIPCHK(c, hipGetLastError());
    {
        const int rcw = mbox_wait(c, seq);
        if (rcw) return rcw;
    }
    *hs = c->mbox->sc;
    return 0;
}

// sum of per-block partials on the host (strip: all-reduced first): n slots of MAXPART doubles starting at `part`
int host_sums(plfx_ctx *c, double *part, int nslots, int gn, double *out)
{
    int rc;
    if ((rc = part_allreduce(c, part, (size_t)(nslots - 1) * MAXPART + gn))) return rc;
    std::vector<double> h((size_t)(nslots - 1) * MAXPART + gn);
    if ((rc = fetch_results(c, part, (int)h.size(), h.data()))) return rc;
    for (int s = 0; s < nslots; s++) {
        double t = 0.;
        for (int i = 0; i < gn; i++) t += h[(size_t)s * MAXPART + i];
        out[s] = t;
    }
    return 0;
}

// Right-preconditioned restarted GMRES on P K P x = P b from the iterate in c->x (see plfx_mg.hpp): x = x0 + B t with t in the
// Krylov space of K B.  Returns 0 = |P(b - K x)| <= rtol |b|, 1 = iteration limit, < 0 = error.
constexpr int GMRES_BLK = 32;  // basis vectors per allocation
constexpr int GMRES_M = 1200;      // restart length (round 6): restarts stall on indefinite K -- a solve that needs 500 iterations took three cycles of
                                   // 400 (1176 iterations) or none at all (residual stuck at 1e-6 after the first restart, profiles/r07e_*); with
                                   // the basis read twice instead of four times per iteration a cycle three times as long costs what it cost,
                                   // and the blocks are allocated as a cycle grows into them.  Reduced until the basis fits into a third of the
                                   // free HBM (2048^2: 81 GB); PLFX_GMRES_M overrides
int gmres_solve(plfx_ctx *c, double rtol, int maxit, int *iters, double *relres)
{
    const size_t nd = c->ndof;
    const int nn = c->nnode, gn = c->grid_nodes;
    const int olo = own_lo(c), ohi = own_hi(c);
    int rc;
    // LOCK-STEP: the first-use block below holds a collective.  Every rank of a communicator reaches it in the same
    // solve, because what sends a solve here -- PCG's breakdown / stall flags -- is decided from partial sums that were
    // all-reduced element-wise (strip) or computed redundantly on identical data (replicated solve): bitwise the same on every
    // rank; gm_m is reset together with the mesh on all of them.
    if (c->gm_m == 0) {
        size_t fr = 0, tot = 0;
        HIPCHK(c, hipMemGetInfo(&fr, &tot));
        c->gm_m = getenv("PLFX_GMRES_M") ? std::max(25, atoi(getenv("PLFX_GMRES_M"))) : GMRES_M;
        c->gm_m = std::min(c->gm_m, 40 * GMRES_BLK - 1);
        while (c->gm_m > 25 && (size_t)(c->gm_m + 1) * nd * 8 > fr / 3) c->gm_m = (c->gm_m * 2) / 3;
        if (comm_active(c)) {  // every rank must run the same cycle length (paired collectives of a strip; identical iterates of a replicated solve)
            double mv = c->gm_m;
            HIPCHK(c, hipMemcpyAsync(c->small, &mv, 8, hipMemcpyHostToDevice, c->stream));
            if ((rc = allreduce(c, c->small, 1, NCCL_FLOAT64, NCCL_MIN, "GMRES basis length"))) return rc;
            if ((rc = fetch_results(c, c->small, 1, &mv))) return rc;
            c->gm_m = (int)mv;
        }
    }
    const int M = c->gm_m;
    if (!c->gm_part && (rc = dalloc(c, &c->gm_part, (size_t)8 * MAXPART))) return rc;
    // The basis grows with the cycle (round 4): most of these solves end after 40-100 iterations, a few need the whole cycle --
    // the 401 vectors of a full cycle are 27 GB at 2048^2, the first block 2.2 GB.  Every rank of a communicator walks the same
    // j, so the blocks appear in lock-step; the cycle LENGTH was agreed above from the memory that is free.
    auto need = [&](int j) -> int {
        while ((int)c->gm_blk.size() * GMRES_BLK <= j) {
            double *b = nullptr;
            const int e = dalloc(c, &b, (size_t)GMRES_BLK * nd);
            if (e) return e;
            c->gm_blk.push_back(b);
        }
        return 0;
    };
    auto Vj = [&](int j) { return c->gm_blk[j / GMRES_BLK] + (size_t)(j % GMRES_BLK) * nd; };
    if ((rc = need(0))) return rc;
    double *P_rz = c->part + 3 * MAXPART, *P_rr = c->part + 4 * MAXPART, *P_bb = c->part + 5 * MAXPART;
    const bool use_mg = mg_active(c);
    auto apply_B = [&]() -> int {  // c->z = B c->r
        int e;
        if (c->strip.on && (e = halo_refresh(c, c->r))) return e;
        if (use_mg) return mg_vcycle(c);
        launch_jacobi_z(c);
        return 0;
    };
    int itn = 0, cycles = 0, poor = 0;
    double rl = 0., rr_prev = -1.;
    std::vector<double> H((size_t)(M + 1) * M), cs(M), sn(M), g(M + 1), hcol(M + 2);
    std::vector<double> Hraw((size_t)(M + 1) * M);
    static const bool gm_dbg = getenv("PLFX_GMRES_DEBUG") != nullptr;
    if ((rc = ensure_dinv(c))) return rc;   // (k_cg_start's z = dinv r, the Jacobi form of apply_B)
    c->pred_d_kept = false;
    while (true) {
        // r0 = P (b - K x) -> c->r; beta = |r0|
        LAUNCH_OP1(k_cg_start, matfree(c), dim3(gn), c->op, nn, 1, (const double2 *)c->x, (const double2 *)c->rhs,
                   (const double2 *)c->dinv, (double2 *)c->r, (double2 *)c->z, P_rz, P_rr, P_bb, olo, ohi);
        HIPCHK(c, hipGetLastError());
        double o[3];
        if ((rc = host_sums(c, P_rz, 3, gn, o))) return rc;
        const double rr = o[1], bb = o[2];
        hipLaunchKernelGGL(k_cg_setup, dim3(1), dim3(BLOCK), 0, c->stream, P_bb, gn, rtol, c->sc);  // clears the sticky done flag
        const double tol = rtol * std::sqrt(bb);
        rl = bb > 0. ? std::sqrt(rr / bb) : 0.;
        if (getenv("PLFX_SOLVE_DEBUG")) fprintf(stderr, "[gmres] cycle %d starts at iteration %d: true relative residual %.3e\n", cycles, itn, rl);
        if (rr_prev >= 0. && rr > 0.25 * rr_prev) poor++;  // a whole cycle bought less than a factor of two
        else poor = 0;
        rr_prev = rr;
        if (std::sqrt(rr) <= tol || itn >= maxit || poor >= 2 || cycles >= 20) {
            if (iters) *iters = itn;
            if (relres) *relres = rl;
            return std::sqrt(rr) <= tol ? 0 : 1;
        }
        cycles++;
        const double beta = std::sqrt(rr);
        hipLaunchKernelGGL(k_scale_copy, dim3(grid_for(nn)), dim3(BLOCK), 0, c->stream, nn, 1. / beta, (const double2 *)c->r,
                           (double2 *)Vj(0), (double2 *)nullptr);
        std::fill(g.begin(), g.end(), 0.);
        g[0] = beta;
        int k = 0;  // columns built in this cycle
        // ---- Arnoldi with delayed re-orthogonalisation (plfx_mg.hpp: k_gmres_dots3 / k_gmres_update2).
        // State at the top of iteration j >= 1: q_0 .. q_{j-1} final in V_0 .. V_{j-1}; u = V_j the once-projected candidate
        // for q_j (u = w_{j-1} - Q_j h1, h1 = the first-pass coefficients kept in h1p); column j-1 of the Hessenberg matrix
        // still open.  One operator application z = A u, one dots pass (s = Q_j^T u, t = Q_j^T z, u.u, u.z), then on the host
        //   alpha^2 = u.u - s.s                      (q_j = (u - Q_j s) / alpha: the delayed second pass of vector j)
        //   column j-1 of H:  h1 + s  over  alpha    -> Givens, residual estimate, convergence test (one iteration late)
        //   w_j = A q_j = (z - A Q_j s) / alpha,  A Q_j s = Q_j (H s) + q_j rho,  rho = alpha s_{j-1}     (Arnoldi relation)
        //   first pass of w_j:  c = Q_j^T w_j = (t - H s) / alpha,   d = q_j^T w_j = ((u.z - s.t) / alpha - rho) / alpha
        //   next candidate      w_j - Q_j c - q_j d = (z - Q_j t) / alpha - e (u - Q_j s),   e = (rho / alpha + d) / alpha
        // and one update pass over Q_j that writes q_j into V_j and the next candidate into V_{j+1}.
        std::vector<double> h1p, sv(M + 2), tv(M + 2), cf(2 * (size_t)M + 4), red(2 * (size_t)M + 4);
        const int ncolmax = 2 * M + 4;
        if (!c->gm_part2 && (rc = dalloc(c, &c->gm_part2, (size_t)ncolmax * MAXPART))) return rc;
        if (!c->gm_red && (rc = dalloc(c, &c->gm_red, (size_t)ncolmax))) return rc;
        if (!c->gm_coef && (rc = dalloc(c, &c->gm_coef, (size_t)ncolmax))) return rc;
        GmBlocks GB;
        auto fill_blocks = [&]() { for (int q = 0; q < 40; q++) GB.blk[q] = q < (int)c->gm_blk.size() ? c->gm_blk[q] : c->gm_blk[0]; };
        // sums over the basis: columns 2k (V_k . a), 2k+1 (V_k . b), then a.a, a.b -- one reduction kernel, one host round trip
        auto dots = [&](int j, const double *a, const double *bvec) -> int {
            fill_blocks();
            const int gd = std::min(gn, std::max(1, (ohi - olo + 2 * BLOCK - 1) / (2 * BLOCK)));   // tiles of 512 nodes
            for (int b0 = 0; b0 < j; b0 += GM_KC)
                hipLaunchKernelGGL(k_gmres_dots3, dim3(gd), dim3(BLOCK), 0, c->stream, olo, ohi, b0, std::min(GM_KC, j - b0), GB, nd,
                                   (const double2 *)a, (const double2 *)bvec, b0 == 0 ? 2 * j : -1, c->gm_part2);
            const int ncol = 2 * j + 2;
            hipLaunchKernelGGL(k_gmres_reduce, dim3((ncol + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, c->stream, ncol, gd,
                               (const double *)c->gm_part2, c->gm_red);
            HIPCHK(c, hipGetLastError());
            int e;
            if (comm_active(c) && c->strip.on && (e = allreduce(c, c->gm_red, (size_t)ncol, NCCL_FLOAT64, NCCL_SUM, "GMRES sums"))) return e;
            return fetch_results(c, c->gm_red, ncol, red.data());
        };
        // c->q = K B v (through c->r, c->z).  Defined behind the cycle's k_cg_start, as the launches it replaces were: the kernel
        // templates appear in the code object in the order of their first use, and that order is kept
        auto apply_A = [&](const double *v) -> int {
            hipLaunchKernelGGL(k_scale_copy, dim3(grid_for(nn)), dim3(BLOCK), 0, c->stream, nn, 1., (const double2 *)v, (double2 *)c->r, (double2 *)nullptr);
            if (const int e = apply_B()) return e;
            LAUNCH_OP1(k_minres_apply, matfree(c), dim3(gn), c->op, nn, 1., (const double2 *)c->z, (const double2 *)c->dinv,
                       (const double2 *)c->z, (double2 *)c->p[0], (double2 *)c->q, c->gm_part, c->gm_part + MAXPART, olo, ohi);
            HIPCHK(c, hipGetLastError());
            return 0;
        };
        // first step: w_0 = A q_0; h1 = q_0 . w_0; candidate u_1 = w_0 - q_0 h1 -> V_1
        itn++;
        if ((rc = apply_A(Vj(0)))) return rc;
        if ((rc = need(1))) return rc;
        if ((rc = dots(1, c->q, nullptr))) return rc;
        h1p.assign(1, red[0]);
        cf[0] = red[0];
        HIPCHK(c, hipMemcpyAsync(c->gm_coef + ncolmax / 2, cf.data(), 8, hipMemcpyHostToDevice, c->stream));
        fill_blocks();
        hipLaunchKernelGGL(k_gmres_update2, dim3(gn), dim3(BLOCK), 0, c->stream, nn, nd, 1, GB, (const double *)c->gm_coef,
                           (const double *)(c->gm_coef + ncolmax / 2), 1., 0., (const double2 *)c->q, (const double2 *)nullptr,
                           (double2 *)nullptr, (double2 *)Vj(1));
        HIPCHK(c, hipGetLastError());
        for (int j = 1; j <= M; j++) {
            const bool more = j < M && itn < maxit;   // another basis vector may still be built after this one
            // z = A u -> c->q   (the operator application of iteration j + 1, on the candidate: one ahead of the finished basis)
            itn++;
            if ((rc = apply_A(Vj(j)))) return rc;
            if ((rc = dots(j, Vj(j), c->q))) return rc;
            double ss = 0., st = 0.;
            for (int q = 0; q < j; q++) {
                sv[q] = red[2 * q];
                tv[q] = red[2 * q + 1];
                ss += sv[q] * sv[q];
                st += sv[q] * tv[q];
            }
            const double uu = red[2 * j], uz = red[2 * j + 1];
            const double a2 = uu - ss;
            const double alpha = (a2 > 0. && std::isfinite(a2)) ? std::sqrt(a2) : 0.;
            if (gm_dbg) {
                double smax = 0.;
                for (int q = 0; q < j; q++) smax = std::max(smax, std::fabs(sv[q]));
                fprintf(stderr, "[gmres-d] j %d u.u %.6e s.s %.3e max|s| %.3e alpha %.6e |g| %.3e\n", j, uu, ss, smax, alpha, std::fabs(g[j - 1]));
            }
            // column j-1 of the Hessenberg matrix is complete: first-pass coefficients + the delayed second pass, alpha below
            std::fill(hcol.begin(), hcol.end(), 0.);
            for (int q = 0; q < j; q++) hcol[q] = h1p[q] + sv[q];
            hcol[j] = alpha;
            for (int q = 0; q <= j; q++) Hraw[(size_t)q * M + (j - 1)] = hcol[q];
            for (int q = 0; q < j - 1; q++) {
                const double t = cs[q] * hcol[q] + sn[q] * hcol[q + 1];
                hcol[q + 1] = -sn[q] * hcol[q] + cs[q] * hcol[q + 1];
                hcol[q] = t;
            }
            const double den = std::hypot(hcol[j - 1], hcol[j]);
            cs[j - 1] = den > 0. ? hcol[j - 1] / den : 1.;
            sn[j - 1] = den > 0. ? hcol[j] / den : 0.;
            hcol[j - 1] = den;
            hcol[j] = 0.;
            g[j] = -sn[j - 1] * g[j - 1];
            g[j - 1] = cs[j - 1] * g[j - 1];
            for (int q = 0; q < j; q++) H[(size_t)q * M + (j - 1)] = hcol[q];
            k = j;
            if (std::fabs(g[j]) <= tol || !(alpha > 0.) || !more) break;
            // first pass of the next vector, from the sums at hand
            const double ia = 1. / alpha;
            const double rho = alpha * sv[j - 1];
            const double d = ((uz - st) * ia - rho) * ia;
            const double e = (rho * ia + d) * ia;
            h1p.assign(j + 1, 0.);
            for (int q = 0; q < j; q++) {
                double r = 0.;   // (H s)_q over the finished columns (upper Hessenberg: column p reaches row p + 1)
                for (int p2 = (q > 0 ? q - 1 : 0); p2 < j; p2++) r += Hraw[(size_t)q * M + p2] * sv[p2];
                h1p[q] = (tv[q] - r) * ia;
                cf[q] = sv[q];
                cf[ncolmax / 2 + q] = tv[q] * ia - e * sv[q];
            }
            h1p[j] = d;
            if ((rc = need(j + 1))) return rc;
            fill_blocks();
            HIPCHK(c, hipMemcpyAsync(c->gm_coef, cf.data(), (size_t)8 * j, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->gm_coef + ncolmax / 2, cf.data() + ncolmax / 2, (size_t)8 * j, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_gmres_update2, dim3(gn), dim3(BLOCK), 0, c->stream, nn, nd, j, GB, (const double *)c->gm_coef,
                               (const double *)(c->gm_coef + ncolmax / 2), ia, e, (const double2 *)Vj(j), (const double2 *)c->q,
                               (double2 *)Vj(j), (double2 *)Vj(j + 1));
            HIPCHK(c, hipGetLastError());
        }
        c->n_gmres_its += k;
        // y = H^-1 g (upper triangular); t = V y -> c->r; x += B t
        std::vector<double> y(k, 0.);
        for (int q = k - 1; q >= 0; q--) {
            double t = g[q];
            for (int p2 = q + 1; p2 < k; p2++) t -= H[(size_t)q * M + p2] * y[p2];
            y[q] = H[(size_t)q * M + q] != 0. ? t / H[(size_t)q * M + q] : 0.;
        }
        HIPCHK(c, hipMemsetAsync(c->r, 0, 8 * nd, c->stream));
        for (int b0 = 0; b0 < k; b0 += 8) {
            const int n8 = std::min(8, k - b0);
            Ptr8 V8;
            Coef8 C8;
            for (int q = 0; q < 8; q++) {
                V8.p[q] = (const double2 *)Vj(b0 + std::min(q, n8 - 1));
                C8.c[q] = q < n8 ? y[b0 + q] : 0.;
            }
            hipLaunchKernelGGL(k_gmres_axpy, dim3(gn), dim3(BLOCK), 0, c->stream, nn, n8, (double2 *)c->r, V8, C8);
        }
        if ((rc = apply_B())) return rc;
        {
            Ptr8 V8;
            Coef8 C8;
            for (int q = 0; q < 8; q++) {
                V8.p[q] = (const double2 *)c->z;
                C8.c[q] = q == 0 ? 1. : 0.;
            }
            hipLaunchKernelGGL(k_gmres_axpy, dim3(gn), dim3(BLOCK), 0, c->stream, nn, 1, (double2 *)c->x, V8, C8);
        }
        HIPCHK(c, hipGetLastError());
        // next cycle starts from the true residual of x (and ends the solve if it is small enough)
    }
}

// What one solve carries from phase to phase (solve_impl and the functions it calls): a plain aggregate on the stack.
struct SolveRun {
    // partial-sum slots; r.z[1], r.r[1], b.b (written together by k_cg_start) are contiguous: one all-reduce in a strip
    double *P_pq, *P_rz[2], *P_rr[2], *P_bb;
    int olo, ohi, gn, nn;
    size_t nd;
    bool multi, mg;   // sharded SpMV (one all-reduce of q per CG step); multigrid-PCG (a strip's Jacobi fall-back included)
    CgScalars hs;
    int done, it;
    bool pred_active, pred_fused;    // a history exists: this solve may be answered by x + alpha d; K d came with the start kernel's pass
    bool pred_d_ready, pred_moved;   // (d = x - pred_x is in pred_d; the start x + alpha d was accepted as the solution)
    bool pred_finished;              // (... and k_pred_finish has composed du and advanced the history already)
    bool du_early;                   // the gated k_compose_du behind the first test has composed du (that test passed)
    bool test_only;                  // started by k_cg_start_test: r, z and r.z are not there until k_cg_start follows
    bool d_kept;                     // pred_d already holds this solve's d (plfx_ctx::pred_d_kept and x as the last solve left it): no k_pred_diff
};

// PLFX_WAIT_FIRST=0: a solve never waits for its first test before it enqueues the interpolated start (always speculate, as before DESIGN 24)
bool wait_first_on() { static const bool on = !(getenv("PLFX_WAIT_FIRST") && atoi(getenv("PLFX_WAIT_FIRST")) == 0); return on; }

// The node code for the kernels of an interpolated start, or null: they read dinv / is_presc as ever.  One GPU, no
// strip, no communicator, the matrix-free operator of cells all alike, and a code formed with the Dirichlet set in force.
const uint8_t *node_code(plfx_ctx *c)
{
    return ((c->node_code & 1) && c->code_ok && !c->sharded && !c->strip.on && !comm_active(c) && matfree(c) && !c->op.colr) ? c->ncode : nullptr;
}
// ... and whether a start kernel given that code may take rhs as +0.0 off bc_rows: asked at the launch, where rhs_rows_ok says
// that the last full k_bc_finish ran without a force vector and only k_spmv_rows has written rhs since
int code_b_sparse(plfx_ctx *c, const uint8_t *code) { return (code && (c->node_code & 2) && c->rhs_rows_ok) ? 1 : 0; }

bool solve_debug_on() { static const bool on = getenv("PLFX_SOLVE_DEBUG") && atoi(getenv("PLFX_SOLVE_DEBUG")) != 0; return on; }

// z = (the rest of the V-cycle)(r) and the partials of r.z in `slot`: written by the last post-smoothing launch of the cycle
// where that can be done, by k_dot_rz otherwise; all-reduced in a strip.  `vcycle_ev` (may be null) closes the timing of the cycle.
int precondition_rz(plfx_ctx *c, double *slot, EvPair *vcycle_ev = nullptr)
{
    bool fused = false;
    const int rc = mg_vcycle_rest(c, slot, &fused);
    tim_end(c, vcycle_ev);
    if (rc) return rc;
    if (!fused)
        hipLaunchKernelGGL(k_dot_rz, dim3(c->grid_nodes), dim3(BLOCK), 0, c->stream, own_lo(c), own_hi(c), (const double2 *)c->r,
                           (const double2 *)c->z, slot);
    return part_allreduce(c, slot, c->grid_nodes);
}

// p = z + beta p_old and q = K p of iteration `it`, partials of p.q
void launch_direction(plfx_ctx *c, const SolveRun &s, int it)
{
    const int cur = it & 1, prev = cur ^ 1;  // (cur: the partial slot written by this iteration's update kernel)
    const double2 *pold = (const double2 *)c->p[prev];
    double2 *pnew = (double2 *)c->p[cur];
    if (!s.multi && march_pcg(c)) {  // marching form of the matrix-free operator (bit-identical q, p)
        if (it == 0)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_march<2>), dim3(s.gn), dim3(BLOCK), 0, c->stream, c->op, pold, (const double2 *)c->z,
                               pnew, (double2 *)c->q, s.P_rz[prev], s.P_rz[cur], s.P_rr[prev], s.gn, s.P_pq, c->sc, it, s.olo, s.ohi);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_march<1>), dim3(s.gn), dim3(BLOCK), 0, c->stream, c->op, pold, (const double2 *)c->z,
                               pnew, (double2 *)c->q, s.P_rz[prev], s.P_rz[cur], s.P_rr[prev], s.gn, s.P_pq, c->sc, it, s.olo, s.ohi);
    } else if (it == 0 && !s.multi)  // first iteration: p = z, p_old untouched
        LAUNCH_OP2(k_spmv, 2, matfree(c), dim3(s.gn), c->op, 0, s.nn, pold, (const double2 *)c->z, pnew, (double2 *)c->q, s.P_rz[prev],
                   s.P_rz[cur], s.P_rr[prev], s.gn, s.P_pq, c->sc, it, s.olo, s.ohi);
    else
        LAUNCH_OP2(k_spmv, 1, matfree(c), dim3(s.gn), c->op, s.multi ? c->own_n0 : 0, s.multi ? c->own_n1 : s.nn, pold, (const double2 *)c->z,
                   pnew, (double2 *)c->q, s.P_rz[prev], s.P_rz[cur], s.P_rr[prev], s.gn, s.P_pq, c->sc, it, s.olo, s.ohi);
}

// du = x on the free DOFs, the prescribed values elsewhere (strip: x is valid on owned + 2 columns: complete the halo first)
// (coded: the Dirichlet set from the node code where there is one -- the end of a PCG solve; GMRES and the Jacobi fall-back read is_presc)
int compose_du(plfx_ctx *c, bool coded = false)
{
    int rc;
    if (c->strip.on && (rc = halo_refresh(c, c->x))) return rc;
    const uint8_t *code = coded ? node_code(c) : nullptr;
    hipLaunchKernelGGL(k_compose_du, dim3(grid_for(c->ndof)), dim3(BLOCK), 0, c->stream, c->ndof, c->x, c->dup, c->is_presc, c->du,
                       (const CgScalars *)nullptr, code);
    if (code) c->n_code_vector++;
    HIPCHK(c, hipGetLastError());
    return 0;
}

// the system just solved, for the shortcut at the top of solve_impl
void remember(plfx_ctx *c, double rtol, double relres, bool valid) { c->memo = {valid, rtol, relres}; }

// x0, the history of the initial guess, r0 (and z0 or K d), the scalars of a Jacobi-PCG solve
int solve_start(plfx_ctx *c, SolveRun &s, double rtol, int warm, int site)
{
    const size_t nd = s.nd;
    const int nn = s.nn, gn = s.gn;
    // x0: the previous solution restricted to the free DOFs is still in c->x when neither du nor the Dirichlet set changed
    const bool x_kept = warm && c->x_is_du;
    if (!x_kept) {
        hipLaunchKernelGGL(k_x0, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->du, c->is_presc, warm, 1., c->x);
        c->pred_d_kept = false;   // (x rewritten)
    }
    c->x_is_du = false;
    int rc = 0;
    // Initial guess from the last TWO solutions (round 5; acceptance rule of round 6).  A warm start uses
    // the previous solution x as it is.  The systems of consecutive solves differ by a tangent update and / or a scaled load
    // increment, and so do their solutions, by nearly the same vector as last time: with d = x - (the last solution that differed
    // from it; zero on DOFs that are prescribed now) and the alpha in [0, 1] that minimises | P (b - K (x + alpha d)) | -- one
    // operator pass, two sums, after the plain start has failed the tolerance test -- x + alpha d is taken ONLY IF IT SATISFIES THE
    // TOLERANCE AS IT IS (k_pred_try: one more pass over r and K d that writes nothing).  Otherwise x, r and z are what the plain
    // warm start left and the solve iterates from x: every iterating solve is bit-identical to PLFX_PREDICT=0.  Why: the error a
    // residual tolerance leaves sits in the soft modes of the plastic tangents, and it is the iterations of a long solve after a
    // moved start that let those components drift (round 5 guarded that with an iteration-count threshold tuned on the test set;
    // this rule follows from the mechanism and has no constant).  x itself is never rescaled (beta != 1 rescales its converged soft
    // components, 4e-6 in the fields of the sensitive traces).  Tried on multigrid-PCG solves of meshes where a V-cycle costs more
    // than the extra passes and the host round trips (>= 16384 nodes; the reference traces of the parity tests, <= 32 x 32
    // elements, run the plain warm start).  Strips: x and the solution before it are valid on the halo columns, the sums are
    // taken over the owned columns and all-reduced (host_sums / part_allreduce).  PLFX_PREDICT=0 at plfx_create switches it off.
    // (every rank of a communicator takes the same decisions: the global node count and -- through the all-reduced sums -- alpha
    // and the test are the same everywhere; a replicated solve computes everything redundantly)
    const long long nn_global = c->strip.on ? (long long)(c->strip.gnx + 1) * (c->gy + 1) : (long long)c->nnode;
    if (c->predict && warm && !s.multi && mg_active(c) && nn_global >= 16384) {
        if (!c->pred_x && (rc = dalloc(c, &c->pred_x, nd))) return rc;
        if (!c->pred_d && (rc = dalloc(c, &c->pred_d, nd))) return rc;
        if (c->pred_valid)
            s.pred_active = true;
        else {
            HIPCHK(c, hipMemcpyAsync(c->pred_x, c->x, 8 * nd, hipMemcpyDeviceToDevice, c->stream));
            c->pred_valid = true;
            c->pred_d_kept = false;   // (pred_x rewritten)
        }
    } else
        c->pred_valid = c->pred_d_kept = false;   // a cold start or another solver: the history starts again
    // d of the interpolated start is in pred_d already (k_pred_finish of the solve that last moved x wrote it)
    s.d_kept = s.pred_active && c->pred_d_kept && x_kept && (c->short_solve & 2) && !c->strip.on && !comm_active(c);
    // A solve that may be answered by x + alpha d needs K d as well as K x: where the plain start is not expected to pass its
    // test, both come from ONE pass over the generators (k_cg_start_pred) instead of k_cg_start and k_spmv<0>.  A site
    // whose last solve was answered by the plain start (the predictor solve of a load step) keeps k_cg_start: it would pay for a
    // K d that nobody reads.  Matrix-free operator with cells all alike, one GPU, no strip.  If the plain start passes after
    // all, pred_d and p[0] hold a d and a K d that nothing reads: pred_d_ready stays false, the next solve forms its own.
    s.pred_fused = s.pred_active && matfree(c) && !c->op.colr && !c->strip.on && !comm_active(c) && site >= 0 && !c->first_test_hint[site];
    if (s.pred_fused) {
        // d = x - (solution before) first (k_pred_diff without the flag: the test of this solve has not run yet), then
        // r = P(b - K x) and K d -> p[0]; partials of r.r and b.b -> slot 1 (z and r.z: written by the V-cycle if there is one)
        if (s.d_kept)
            c->n_d_kept++;
        else
            hipLaunchKernelGGL(k_pred_diff, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->x, c->pred_x, c->dinv, c->pred_d,
                               (const CgScalars *)nullptr);
        const uint8_t *code = node_code(c);
        const int b_sparse = code_b_sparse(c, code);
        hipLaunchKernelGGL(k_cg_start_pred, dim3(gn), dim3(BLOCK), 0, c->stream, c->op, nn, (const double2 *)c->x, (const double2 *)c->pred_d,
                           (const double2 *)c->rhs, (const double2 *)c->dinv, (double2 *)c->r, (double2 *)c->p[0], s.P_rr[1], s.P_bb,
                           code, b_sparse);
        if (code) c->n_code_start++, c->n_code_bsparse += b_sparse;
    } else if (c->test_starts && s.mg && wait_first_on() && s.pred_active && site >= 0 && c->first_test_hint[site] && !c->strip.on &&
               !comm_active(c) && matfree(c)) {
        // solve_first_test will wait for the first test before it enqueues anything that reads r or z, and expects it to pass:
        // the sums of that test alone.  If it fails, k_cg_start follows there.
        const uint8_t *code = node_code(c);   // (null with per-column widths)
        const int b_sparse = code_b_sparse(c, code);
#define TEST_START(G)                                                                                                          \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cg_start_test<G>), dim3(gn), dim3(BLOCK), 0, c->stream, c->op, nn, 1, (const double2 *)c->x, \
                       (const double2 *)c->rhs, (const double2 *)c->dinv, s.P_rr[1], s.P_bb, s.olo, s.ohi, code, b_sparse)
        if (c->op.colr) TEST_START(2); else TEST_START(1);   // (the matrix-free instantiations, as LAUNCH_OP1 picks them)
#undef TEST_START
        if (code) c->n_code_start++, c->n_code_bsparse += b_sparse;
        s.test_only = true;
        c->n_test_starts++;
    } else {   // r = P(b - K x0), z = Minv r; partials -> slot 1 ("iteration -1"); one pass (no q round trip)
        if ((rc = ensure_dinv(c))) return rc;   // (z = dinv r)
        LAUNCH_OP1(k_cg_start, matfree(c), dim3(gn), c->op, nn, warm ? 1 : 0, (const double2 *)c->x, (const double2 *)c->rhs,
                   (const double2 *)c->dinv, (double2 *)c->r, (double2 *)c->z, s.P_rz[1], s.P_rr[1], s.P_bb, s.olo, s.ohi);
    }
    if (c->strip.on) {  // sums of the whole grid; r valid on every local column (the V-cycle reads the halo)
        if ((rc = part_allreduce(c, s.P_rz[1], (size_t)3 * MAXPART))) return rc;
        if ((rc = halo_refresh(c, c->r))) return rc;
    }
    if (!s.mg) {   // Jacobi-PCG reads dinv's values in every update (the plain start above has formed a late one already)
        if ((rc = ensure_dinv(c))) return rc;
        hipLaunchKernelGGL(k_cg_setup, dim3(1), dim3(BLOCK), 0, c->stream, s.P_bb, gn, rtol, c->sc);
    }
    return 0;
}

// multigrid-PCG: z0 = V-cycle(r0) replaces the Jacobi z of k_cg_init -- unless x0 already satisfies the tolerance.  Leaves
// s.done / s.hs as the host saw them and, while not done, the head of the V-cycle enqueued.
int solve_first_test(plfx_ctx *c, SolveRun &s, double rtol, int site)
{
    const size_t nd = s.nd;
    const int nn = s.nn, gn = s.gn, olo = s.olo, ohi = s.ohi;
    int rc;
    bool first_passed = false, pred_first_passed = false;
    unsigned long long seq = cg_setup_check_post(c, s.P_bb, s.P_rr[1], gn, rtol);   // (scalars set up and first test: one launch)
    const bool wait_first = wait_first_on();
    if (wait_first && s.pred_active && site >= 0 && c->first_test_hint[site] && !c->strip.on) {
        // the predictor solve of a load step repeats the system of the solve before it up to the last bits of its boundary
        // values: x passes the first test.  Learn that before enqueuing what would return at once (six launches, 28 us)
        // du of a passed test is composed under the round trip: gated on the flag the test just wrote, a no-op otherwise
        const bool early = c->bc_rows_on && c->reuse && !comm_active(c);
        if (early) {
            const uint8_t *code = node_code(c);
            hipLaunchKernelGGL(k_compose_du, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->x, c->dup, c->is_presc, c->du,
                               (const CgScalars *)c->sc, code);
            if (code) c->n_code_vector++;
            HIPCHK(c, hipGetLastError());
        }
        if ((rc = cg_check_wait(c, seq, &s.hs))) return rc;
        s.done = s.hs.done;
        first_passed = s.done != 0;
        if (early && s.done == 1) {
            s.du_early = true;
            c->n_du_early++;
        }
        if (s.test_only && !first_passed) {
            // the hint was wrong: r, z and r.z after all -- one operator pass more than without the test-only start.  The sums of
            // r.r and b.b are rewritten with the bits the test has seen.
            if ((rc = ensure_dinv(c))) return rc;
            LAUNCH_OP1(k_cg_start, matfree(c), dim3(gn), c->op, nn, 1, (const double2 *)c->x, (const double2 *)c->rhs,
                       (const double2 *)c->dinv, (double2 *)c->r, (double2 *)c->z, s.P_rz[1], s.P_rr[1], s.P_bb, olo, ohi);
            HIPCHK(c, hipGetLastError());
            s.test_only = false;
            c->n_test_retries++;
        }
    }
    if (first_passed) {
        pred_first_passed = true;   // (nothing to do: done, hs as the chain below would have left them)
    } else if (s.pred_active) {
        // Everything the interpolated start needs is enqueued behind the first test and returns at once if that test passed
        // (the reference repeats solves of one system: x satisfies the tolerance as it is); the host waits ONCE, for the second
        // test (round 6: three round trips -> one).  d = x - (solution before), K d, the two sums, alpha on the device
        // (k_pred_alpha), | P (r - alpha K d) |^2 into the free slot P_rr[0] without touching x, r, z, the test on it.
        if (!s.pred_fused) {   // (the fused start has left d in pred_d and K d in p[0])
            if (s.d_kept)
                c->n_d_kept++;
            else
                hipLaunchKernelGGL(k_pred_diff, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->x, c->pred_x, c->dinv, c->pred_d, c->sc);
            launch_spmv_plain(c, c->pred_d, c->p[0], c->sc);
        }
        const int gp = MAXPART;   // (one size on every rank: the all-reduce of the partial sums pairs up)
        const uint8_t *code = node_code(c);
        hipLaunchKernelGGL(k_pred_dots, dim3(gp), dim3(BLOCK), 0, c->stream, (size_t)2 * olo, (size_t)2 * ohi, c->dinv, c->r, c->p[0],
                           c->part, c->sc, code);
        HIPCHK(c, hipGetLastError());
        if (c->strip.on && (rc = part_allreduce(c, c->part, (size_t)2 * MAXPART))) return rc;
        hipLaunchKernelGGL(k_pred_try, dim3(gn), dim3(BLOCK), 0, c->stream, nn, c->sc, (const double *)c->part, gp, (const double2 *)c->r,
                           (const double2 *)c->p[0], (const double2 *)c->dinv, s.P_rr[0], olo, ohi, code);
        if (code) c->n_code_vector += 2;
        HIPCHK(c, hipGetLastError());
        if (c->strip.on && (rc = part_allreduce(c, s.P_rr[0], gn))) return rc;
        seq = cg_check_post(c, s.P_rr[0], gn, -2);   // (iters = -2 marks "converged by the interpolated start")
        if (!c->strip.on) {   // x, du and the history in one pass -- behind the test, before the host has seen it (no-op unless accepted)
            hipLaunchKernelGGL(k_pred_finish, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, (const CgScalars *)c->sc, c->x,
                               c->pred_d, c->pred_x, (const double *)c->dup, (const double *)c->is_presc, c->du,
                               ((c->short_solve & 2) && !comm_active(c)) ? 1 : 0, code);
            if (code) c->n_code_vector++;
        }
        if ((rc = cg_check_wait(c, seq, &s.hs))) return rc;
        s.done = s.hs.done;
        if (s.done == 1 && s.hs.iters == -2) {   // it is the solution: commit x (r, z are not read again: the loop is skipped)
            // (k_pred_finish has moved x and pred_x -- and, told to, left the d of the next start in pred_d; k_pred_commit moves x alone)
            c->pred_d_kept = !c->strip.on && (c->short_solve & 2) && !comm_active(c);
            if (!c->strip.on)
                s.pred_finished = true;
            else
                hipLaunchKernelGGL(k_pred_commit, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, (const CgScalars *)c->sc, c->x, c->pred_d);
            HIPCHK(c, hipGetLastError());
            s.hs.iters = 0;
            c->n_pred++;
            s.pred_d_ready = true;
            s.pred_moved = true;
        } else if (!s.done) {
            s.pred_d_ready = true;
            if (s.hs.aux > 0.) c->n_pred_rejected++;
            else c->n_pred_skipped++;
        }
        if (!s.done) {
            if ((rc = mg_ensure(c))) return rc;
            if ((rc = mg_vcycle_head(c))) return rc;
        }
        pred_first_passed = s.done == 1 && !s.pred_moved;
    } else if (c->mg_pending) {
        // the coarse levels are stale (mg_ensure): learn first whether a V-cycle is needed at all
        if ((rc = cg_check_wait(c, seq, &s.hs))) return rc;
        s.done = s.hs.done;
        if (!s.done) {
            if ((rc = mg_ensure(c))) return rc;
            if ((rc = mg_vcycle_head(c))) return rc;
        }
    } else {
        if ((rc = ensure_dinv(c))) return rc;     // (never late here -- a late dinv has a pending set-up beside it -- but cheap to say)
        if ((rc = mg_vcycle_head(c))) return rc;  // speculative: its kernels return at once if the flag says converged
        if ((rc = cg_check_wait(c, seq, &s.hs))) return rc;
        s.done = s.hs.done;
    }
    if (site >= 0 && s.pred_active) c->first_test_hint[site] = pred_first_passed;
    return 0;
}

// the PCG loop: at most `maxit` iterations from s.it = 0, until the flag says done
int pcg_iterate(plfx_ctx *c, SolveRun &s, int maxit)
{
    const int nn = s.nn, gn = s.gn, olo = s.olo, ohi = s.ohi;
    const bool mg = s.mg, multi = s.multi;
    double *const P_pq = s.P_pq, *const *P_rz = s.P_rz, *const *P_rr = s.P_rr;
    CgScalars &hs = s.hs;
    int rc;
    const int chunk = mg ? 1 : 50;  // multigrid: the flag is polled inside the iteration, before the V-cycle
    int &it = s.it;
    if (it < maxit && !s.done) c->pred_d_kept = false;   // (the update kernels move x)
    while (it < maxit && !s.done) {
        const int stop = std::min(maxit, it + chunk);
        for (; it < stop; it++) {
            const int cur = it & 1;  // partial slot written by this iteration's update kernel
            const int prev = cur ^ 1;
            double *pold = c->p[prev], *pnew = c->p[cur];
            EvPair *ev;
            tim_begin(c, 1, &ev);
            launch_direction(c, s, it);
            tim_end(c, ev);
            if ((rc = part_allreduce(c, P_pq, gn))) return rc;
            if (multi) {
                hipLaunchKernelGGL(k_p_update_outside, dim3(gn), dim3(BLOCK), 0, c->stream, nn, c->own_n0,
                                   c->own_n1, (const double2 *)pold, (const double2 *)c->z, (double2 *)pnew,
                                   (double2 *)c->q, P_rz[prev], P_rz[cur], P_rr[prev], gn, c->sc);
                if ((rc = allreduce(c, c->q, s.nd, NCCL_FLOAT64, NCCL_SUM, "q"))) return rc;
                hipLaunchKernelGGL(k_dot_pq, dim3(gn), dim3(BLOCK), 0, c->stream, nn, (const double2 *)pnew,
                                   (const double2 *)c->q, P_pq, c->sc);
            }
            if (mg) {
                tim_begin(c, 2, &ev);
                hipLaunchKernelGGL(k_cg_update_mg, dim3(gn), dim3(BLOCK), 0, c->stream, nn, (const double2 *)pnew,
                                   (const double2 *)c->q, (const double2 *)c->dinv, (double2 *)c->x,
                                   (double2 *)c->r, P_pq, gn, P_rz[prev], gn, P_rr[cur], c->sc, olo, ohi);
                tim_end(c, ev);
                if (c->strip.on) {
                    if ((rc = part_allreduce(c, P_rr[cur], gn))) return rc;
                    if ((rc = halo_refresh(c, c->r))) return rc;  // the one vector exchange of a PCG iteration
                }
                // stop here if this update converged: the V-cycle below would only prepare the next iteration
                const unsigned long long seq = cg_check_post(c, P_rr[cur], gn, it + 1);
                EvPair *evv;
                tim_begin(c, 4, &evv);
                if ((rc = mg_vcycle_head(c))) return rc;  // overlaps the round trip of the flag
                if ((rc = cg_check_wait(c, seq, &hs))) return rc;
                if (hs.done) {
                    tim_end(c, evv);
                    if (c->tim.on) c->tim.noop[4]++;  // a head that returned at once is not a V-cycle
                    it++;
                    break;
                }
                if ((rc = precondition_rz(c, P_rz[cur], evv))) return rc;
            } else {
                tim_begin(c, 2, &ev);
                hipLaunchKernelGGL(k_cg_update, dim3(gn), dim3(BLOCK), 0, c->stream, nn, (const double2 *)pnew,
                                   (const double2 *)c->q, (const double2 *)c->dinv, (double2 *)c->x,
                                   (double2 *)c->r, (double2 *)c->z, P_pq, gn, P_rz[prev], P_rr[prev], gn,
                                   P_rz[cur], P_rr[cur], c->sc);
                tim_end(c, ev);
            }
        }
        HIPCHK(c, hipGetLastError());
        if (!mg) {
            HIPCHK(c, hipMemcpyAsync(&hs, c->sc, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, stream_sync(c));
        }
        s.done = hs.done;
    }
    return 0;
}

// PLFX_SOLVE_DEBUG: what made multigrid-PCG give up: sums of the last iteration, NaN census
void solve_debug_dump(plfx_ctx *c, const SolveRun &s)
{
    const size_t nd = s.nd;
    const int gn = s.gn, it = s.it;
    const CgScalars &hs = s.hs;
    stream_sync(c);
    std::vector<double> hp((size_t)6 * MAXPART), hv(nd);
    hipMemcpy(hp.data(), c->part, hp.size() * 8, hipMemcpyDeviceToHost);
    auto psum = [&](int slot) { double t = 0.; for (int i = 0; i < gn; i++) t += hp[(size_t)slot * MAXPART + i]; return t; };
    auto census = [&](const double *dev, const char *name) {
        hipMemcpy(hv.data(), dev, nd * 8, hipMemcpyDeviceToHost);
        size_t nan = 0, neg = 0; double mx = 0., mn = 1e300;
        for (size_t i = 0; i < nd; i++) { const double v = hv[i]; if (!(v == v)) nan++; else { if (v < 0.) neg++; mx = std::max(mx, std::fabs(v)); if (v != 0.) mn = std::min(mn, std::fabs(v)); } }
        fprintf(stderr, "    %-5s nan %zu  negative %zu  max|.| %.3e  min nonzero|.| %.3e\n", name, nan, neg, mx, mn);
    };
    fprintf(stderr, "[plfx_solve] multigrid-PCG gave up after %d iterations: done %d rr_final %.3e thresh2 %.3e | p.q %.6e  r.z %.6e / %.6e  r.r %.6e / %.6e  b.b %.6e\n",
            it, hs.done, hs.rr_final, hs.thresh2, psum(0), psum(1), psum(3), psum(2), psum(4), psum(5));
    census(c->dinv, "dinv"); census(c->r, "r"); census(c->z, "z"); census(c->x, "x"); census(c->q, "q");
    {
        std::vector<double> hm((size_t)6 * c->nel_total);
        hipMemcpy(hm.data(), matfree(c) ? c->Mop : c->Mel, hm.size() * 8, hipMemcpyDeviceToHost);
        size_t nan = 0; double mx = 0.;
        for (double v : hm) { if (!(v == v)) nan++; else mx = std::max(mx, std::fabs(v)); }
        fprintf(stderr, "    generators nan %zu  max|.| %.3e\n", nan, mx);
        // per element: smallest eigenvalue of the 3 x 3 generator matrix [XX XY XS; XY YY YS; XS YS SS] (PSD for a PSD tangent)
        const size_t ne = c->nel_total;
        size_t nneg = 0, worst = 0; double wv = 0.;
        for (size_t e = 0; e < ne; e++) {
            const bool pr = matfree(c);  // layout of the array read above
            const double a = hm[gen_index(pr, 0, ne, e)], b = hm[gen_index(pr, 1, ne, e)], cc = hm[gen_index(pr, 2, ne, e)],
                         d = hm[gen_index(pr, 3, ne, e)], f = hm[gen_index(pr, 4, ne, e)], g = hm[gen_index(pr, 5, ne, e)];
            // Sylvester: leading minors
            const double m1 = a, m2 = a * d - b * b, m3 = a * (d * g - f * f) - b * (b * g - f * cc) + cc * (b * f - d * cc);
            const double sc1 = std::fabs(a) + std::fabs(d) + std::fabs(g);
            const double bad = std::min(m1 / sc1, std::min(m2 / (sc1 * sc1), m3 / (sc1 * sc1 * sc1)));
            if (bad < -1e-9) { nneg++; if (bad < wv) { wv = bad; worst = e; } }
        }
        fprintf(stderr, "    elements with an indefinite generator matrix: %zu of %zu (worst scaled minor %.3e at element %zu)\n", nneg, ne, wv, worst);
        if (nneg && worst >= (size_t)c->e0 && worst < (size_t)c->e0 + c->nel) {
            const size_t e = worst - c->e0, n = c->nel;
            double v[21]; int ms = 0; double fy = 0.;
            fprintf(stderr, "      class %d material %d kind %d  M =", (int)c->hcls_id[worst], c->hcls[c->hcls_id[worst]].mat, (int)c->hmat[c->hcls[c->hcls_id[worst]].mat].kind);
            for (int k = 0; k < 6; k++) fprintf(stderr, " %.6e", hm[gen_index(matfree(c), k, ne, worst)]);
            for (int k = 0; k < 6; k++) hipMemcpy(&v[k], c->sig + k * n + e, 8, hipMemcpyDeviceToHost);
            fprintf(stderr, "\n      sig = %.6e %.6e %.6e %.6e %.6e %.6e", v[0], v[1], v[2], v[3], v[4], v[5]);
            for (int k = 0; k < 6; k++) hipMemcpy(&v[k], c->res_sig + k * n + e, 8, hipMemcpyDeviceToHost);
            fprintf(stderr, "\n      res_sig = %.6e %.6e %.6e %.6e %.6e %.6e", v[0], v[1], v[2], v[3], v[4], v[5]);
            for (int k = 0; k < 6; k++) hipMemcpy(&v[k], c->epl + k * n + e, 8, hipMemcpyDeviceToHost);
            fprintf(stderr, "\n      epl = %.6e %.6e %.6e %.6e %.6e %.6e", v[0], v[1], v[2], v[3], v[4], v[5]);
            for (int k = 0; k < 6; k++) hipMemcpy(&v[k], c->res_depl + k * n + e, 8, hipMemcpyDeviceToHost);
            fprintf(stderr, "\n      res_depl = %.6e %.6e %.6e %.6e %.6e %.6e", v[0], v[1], v[2], v[3], v[4], v[5]);
            {
                double *tmp = nullptr;
                if (!dalloc(c, &tmp, 21 * n)) {
                    launch_tangent_expand(c, tmp, 0);
                    hipStreamSynchronize(c->stream);
                    for (int k = 0; k < 21; k++) hipMemcpy(&v[k], tmp + k * n + e, 8, hipMemcpyDeviceToHost);
                    dfree(tmp);
                }
            }
            fprintf(stderr, "\n      elstiff(21) =");
            for (int k = 0; k < 21; k++) fprintf(stderr, " %.5e", v[k]);
            hipMemcpy(&ms, c->max_steps + e, 4, hipMemcpyDeviceToHost);
            hipMemcpy(&fy, c->fyn + e, 8, hipMemcpyDeviceToHost);
            fprintf(stderr, "\n      max_steps %d  fyn %.6e\n", ms, fy);
        }
    }
}

// negative curvature met (p.K p <= 0) or a NaN residual: the tangent stiffness is not positive definite (lstsq
// correction of Material.response, material.py:324-338) -- the reference's LU solves such systems, and so does
// right-preconditioned GMRES with the V-cycle of the operator as it is (need not be SPD), from PCG's last iterate
int finish_by_gmres(plfx_ctx *c, const SolveRun &s, double rtol, int maxit_all, int *iters, double *relres)
{
    int itm = 0, rc;
    double rl = 0.;
    c->n_indefinite++;
    c->pred_d_kept = false;   // (GMRES moves x)
    const int rcm = gmres_solve(c, rtol, maxit_all, &itm, &rl);
    if (rcm < 0) return rcm;
    c->n_gmres++;
    if (solve_debug_on()) fprintf(stderr, "[plfx_solve] GMRES(%d): rc %d, %d iterations, relative residual %.3e\n", c->gm_m, rcm, itm, rl);
    if ((rc = compose_du(c))) return rc;
    c->x_is_du = true;
    if (iters) *iters = s.it + itm;
    if (relres) *relres = rl;
    c->pred_valid = c->pred_d_kept = false;   // (not a plain PCG solve: the history of the initial guess starts again)
    remember(c, rtol, rl, rcm == 0);
    return rcm == 0 ? PLFX_OK : 1;
}

// breakdown (indefinite tangent, preconditioner not SPD) or stagnation of multigrid-PCG: Jacobi-PCG, warm-started from the
// last iterate.  Strip: every rank sees the same all-reduced sums and comes here together; Jacobi-PCG runs through the same
// loop (owned-only sums, halo refresh of r per iteration) with z = D^-1 r in place of the V-cycle (strip_jacobi).
int fall_back_to_jacobi(plfx_ctx *c, const SolveRun &s, double rtol, int maxit_all, int *iters, double *relres)
{
    int rc;
    c->pred_d_kept = false;
    if ((rc = ensure_dinv(c))) return rc;   // (Jacobi-PCG: z = dinv r throughout)
    if ((rc = compose_du(c))) return rc;
    const int saved = c->precond;   // (changed and restored off a strip only)
    if (c->strip.on) c->strip_jacobi = true;
    else c->precond = 0;
    c->mg_fallbacks++;
    int it2 = 0;
    const int rc2 = solve_impl(c, rtol, maxit_all, 1, -1, &it2, relres);
    if (c->strip.on) c->strip_jacobi = false;
    else c->precond = saved;
    // (the strip branch never printed this line: kept so, every rank would print it)
    if (!c->strip.on && solve_debug_on()) fprintf(stderr, "[plfx_solve] Jacobi fall-back: rc %d, %d iterations, relative residual %.3e\n", rc2, it2, relres ? *relres : -1.);
    if (iters) *iters = s.it + it2;
    return rc2;
}

// the last residual if no test has seen it, du, the history of the initial guess, the memo
int solve_finish(plfx_ctx *c, SolveRun &s, double rtol, int *iters, double *relres)
{
    const size_t nd = s.nd;
    CgScalars &hs = s.hs;
    int rc, done = s.done;
    const int it = s.it;
    if (done == 2) done = 0;  // Jacobi-PCG breakdown: report as not converged
    if (!done) {
        // the convergence test of iteration `it` has not run yet: evaluate the last residual
        hipLaunchKernelGGL(k_cg_final, dim3(1), dim3(BLOCK), 0, c->stream, s.P_rr[(it - 1) & 1], s.gn, c->sc);
        HIPCHK(c, hipMemcpyAsync(&hs, c->sc, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
    }
    if (!s.pred_finished && !s.du_early && (rc = compose_du(c, true))) return rc;
    c->x_is_du = true;  // x = du on the free DOFs, 0 on the prescribed ones: the next warm start
    const int its_done = (done && hs.iters >= 0) ? hs.iters : it;
    // history of the initial guess: the solution this solve started from becomes "the one before" -- only if this solve moved
    // away from it (the reference repeats solves of one system: such a solve ends where it started and must not erase d)
    if (s.pred_d_ready && !s.pred_finished && (s.pred_moved || its_done > 0)) {
        hipLaunchKernelGGL(k_pred_advance, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->pred_x, c->pred_d);
        c->pred_d_kept = false;   // (pred_x moved)
    }
    if (iters) *iters = its_done;
    if (c->tim.on && done) {  // launches after convergence are no-ops: keep them out of the averages
        c->tim.noop[1] += it - hs.iters;
        c->tim.noop[2] += it - hs.iters;
    }
    const double bb = hs.thresh2 / (rtol * rtol);
    const double rl = (bb > 0. && hs.rr_final >= 0.) ? std::sqrt(hs.rr_final / bb) : 0.;
    if (relres) *relres = rl;
    remember(c, rtol, rl, done == 1);
    return done ? PLFX_OK : 1;  // 1 = iteration limit reached (soft failure, like co_nconv)
}

// The solve behind plfx_solve and plfx_load_step.  The caller guarantees c != null and c->bc_set (plfx_solve checks them;
// step_solve runs behind a successful step_apply_bc).  site: see plfx_ctx::first_test_hint, -1 = no site.
int solve_impl(plfx_ctx *c, double rtol, int maxit, int warm, int site, int *iters, double *relres)
{
    c->spec_setup = c->spec_kdu = false;   // (a solve overwrites c->q: nothing enqueued behind a sweep's flags is valid beyond it)
    if (maxit < 1) maxit = 1;
    if (c->reuse && warm && c->x_is_du && c->memo.valid && c->memo.rtol == rtol) {
        // the system of the previous converged solve (no assembly, no other boundary values since): du is its solution
        c->n_reuse_solve++;
        if (iters) *iters = 0;
        if (relres) *relres = c->memo.relres;
        return PLFX_OK;
    }
    SolveRun s{c->part, {c->part + MAXPART, c->part + 3 * MAXPART}, {c->part + 2 * MAXPART, c->part + 4 * MAXPART}, c->part + 5 * MAXPART,
               own_lo(c), own_hi(c), c->grid_nodes, c->nnode, (size_t)c->ndof};   // (the rest: false / zero)
    if (c->strip.on && !mg_active(c)) return fail(c, PLFX_ERR_STATE, "a strip solves with the multigrid preconditioner only");
    // Sharded run with the assembled operator: every rank applies its own rows, one all-reduce of the global vector per
    // CG step.  With the matrix-free operator every rank holds all generators and a full K p costs ~50 us at 1024^2 --
    // several times less than all-reducing 16.8 MB over xGMI -- so the product is computed redundantly and the solve has
    // no collective at all (PLFX_SHARD_SPMV=1 restores the sharded rows + all-reduce).
    static const bool force_shard_spmv = getenv("PLFX_SHARD_SPMV") && atoi(getenv("PLFX_SHARD_SPMV")) != 0;
    s.multi = comm_active(c) && (!matfree(c) || force_shard_spmv);
    s.mg = mg_active(c);
    int rc;
    if ((rc = solve_start(c, s, rtol, warm, site))) return rc;
    if (s.mg && (rc = solve_first_test(c, s, rtol, site))) return rc;
    if (s.mg && !s.done && (rc = precondition_rz(c, s.P_rz[1]))) return rc;
    // beta of the first iteration is 0 (k_spmv<1> takes p = z for it == 0 without touching p_old); only the sharded
    // k_p_update_outside path still derives it from the partials: rz_old = +inf, p_old = 0
    if (s.multi) {
        hipLaunchKernelGGL(k_fill, dim3(1), dim3(BLOCK), 0, c->stream, s.P_rz[0], (size_t)s.gn, (double)INFINITY);
        HIPCHK(c, hipMemsetAsync(c->p[1], 0, 8 * s.nd, c->stream));
    }
    HIPCHK(c, hipGetLastError());
    // multigrid-PCG converges in tens of iterations or not at all (PLFX_MG_MAXIT: the cap, for tests of the fall-back)
    const int mg_cap = getenv("PLFX_MG_MAXIT") ? std::max(1, atoi(getenv("PLFX_MG_MAXIT"))) : 300;
    const int maxit_pcg = (s.mg && !c->strip_jacobi) ? std::min(maxit, mg_cap) : maxit;
    if ((rc = pcg_iterate(c, s, maxit_pcg))) return rc;
    if (solve_debug_on() && s.mg && s.done != 1) solve_debug_dump(c, s);
    if (s.done != 1 && s.hs.done == 2) return finish_by_gmres(c, s, rtol, maxit, iters, relres);
    if (s.mg && s.done != 1 && !c->strip_jacobi) return fall_back_to_jacobi(c, s, rtol, maxit, iters, relres);
    return solve_finish(c, s, rtol, iters, relres);
}

}  // namespace host
}  // namespace plfx

extern "C" {

int plfx_predict_info(plfx_ctx *c, int64_t *applied, int64_t *skipped, int64_t *rejected)
{
    if (!c) return PLFX_ERR_ARG;
    if (applied) *applied = c->n_pred;
    if (skipped) *skipped = c->n_pred_skipped;
    if (rejected) *rejected = c->n_pred_rejected;
    return PLFX_OK;
}

int plfx_indefinite_info(plfx_ctx *c, int64_t *solves, int64_t *by_minres_surrogate, int64_t *by_gmres, int64_t *surrogates_built,
                         int64_t *elements_shifted)
{
    if (!c) return PLFX_ERR_ARG;
    if (solves) *solves = c->n_indefinite;
    if (by_minres_surrogate) *by_minres_surrogate = 0;
    if (by_gmres) *by_gmres = c->n_gmres;
    if (surrogates_built) *surrogates_built = 0;
    if (elements_shifted) *elements_shifted = 0;
    return PLFX_OK;
}

int plfx_solve_fallbacks(plfx_ctx *c, int64_t *count)
{
    if (!c || !count) return PLFX_ERR_ARG;
    *count = (int64_t)c->mg_fallbacks + c->n_indefinite;
    return PLFX_OK;
}

int plfx_solve(plfx_ctx *c, double rtol, int maxit, int warm, int *iters, double *relres)
{
    if (!c || !c->bc_set) return c ? fail(c, PLFX_ERR_STATE, "apply_bc first") : PLFX_ERR_STATE;
    return solve_impl(c, rtol, maxit, warm, -1, iters, relres);
}

}  // extern "C"
