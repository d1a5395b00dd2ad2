// plfx_step.hip -- libplfx.so: sweeps, load step, state update, state access, global sums, element fields.
// The material-point functions are plfx_material.hip, the linear solve plfx_solve.hip, everything else of the host side
// plfx.hip.  Unit map and the one-owner rule for kernels: DESIGN.md sections 39 and 42; what the units share: plfx_host.hpp.
#define PLFX_UNIT_STEP
#include "plfx_host.hpp"

using namespace plfx;
using namespace plfx::host;

namespace plfx {
namespace host {

// the stored eps field, brought up to date: eps = class_strain(u) (k_update_state forms it for the sums and does not store it)
int ensure_eps(plfx_ctx *c)
{
    if (!c->eps_stale) return 0;
    hipLaunchKernelGGL(k_eps_from_u, dim3(grid_for(c->nel, MAXPART)), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, c->dcls, c->ncls,
                       c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->u, c->eps);
    HIPCHK(c, hipGetLastError());
    c->eps_stale = false;
    return 0;
}

// res_sig as a field of its own again (after an exchange c->sig holds both): copy, then the two buffers are independent
int split_res_sig(plfx_ctx *c)
{
    if (!c->res_is_sig) return 0;
    HIPCHK(c, hipMemcpyAsync(c->res_sig, c->sig, (size_t)48 * c->nel, hipMemcpyDeviceToDevice, c->stream));
    c->res_is_sig = false;
    return 0;
}

#ifdef PLFX_PROF_REGIONS
bool prof_regions_add_step(unsigned long long h[16])
{
    unsigned long long mine[16];
    if (hipMemcpyFromSymbol(mine, HIP_SYMBOL(g_prof), sizeof(mine)) != hipSuccess) return false;
    for (int i = 0; i < 16; i++) h[i] += mine[i];
    return true;
}
#endif

// every stored tangent in full form: into `out` ([21][nel]); to_full: the store itself goes to the full form as well
void launch_tangent_expand(plfx_ctx *c, double *out, int to_full)
{
    hipLaunchKernelGGL(k_tangent_expand, dim3((c->nel + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream,
                       c->dmat, c->dcls, c->nel, c->dcls_id, tan_store(c), out, to_full);
}

// Dynamic-LDS limits of the kernels this unit launches (called by plfx_set_materials).  The order in which this file names the
// row kernels for the first time is the order in which the compiler emits them, and the registers it gives k_sweep_svc_row
// follow that order: the sweep and scf kernels come first, k_response_row (launch_response_row, below) after them.
// Whoever reorders these functions runs tools/kernel_resources_ab.py on the device assembly before and after.
static int raise_sweep_lds(plfx_ctx *c)
{
    if (c->svc_wave_lds > 0) {
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_svc_row<0, true>, c->svc_wave_lds));
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_svc_row<1, true>, c->svc_wave_lds));
        HIPCHK(c, set_dyn_lds((const void *)k_scf_row<true>, c->svc_wave_lds));
        if (c->svc_cols_mask & c->svc_row_lds) {
            HIPCHK(c, set_dyn_lds((const void *)k_sweep_svc_row<0, true, true>, c->svc_wave_lds));
            HIPCHK(c, set_dyn_lds((const void *)k_sweep_svc_row<1, true, true>, c->svc_wave_lds));
            HIPCHK(c, set_dyn_lds((const void *)k_scf_row<true, true>, c->svc_wave_lds));
            // (a texture field can be attached to any of them)
            HIPCHK(c, set_dyn_lds((const void *)k_sweep_svc_row<0, true, true, true, TexFieldDev>, c->svc_wave_lds));
            HIPCHK(c, set_dyn_lds((const void *)k_sweep_svc_row<1, true, true, true, TexFieldDev>, c->svc_wave_lds));
            HIPCHK(c, set_dyn_lds((const void *)k_scf_row<true, true, true, TexFieldDev>, c->svc_wave_lds));
        }
    }
    if (c->has_svc || c->has_svc3 || c->has_svcwh) {  // the SVC kernels that stage whole tables
        const int bytes = (int)dyn_lds_bytes(c);
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_light<6>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_heavy<6>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_light<3>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_heavy<3>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_scf_elements, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_light<7>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_heavy<7>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_wh_wave<0>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_sweep_wh_wave<1>, bytes));
    }
    return 0;
}

// The response of the points of row-kernel material k (response_batch_impl, plfx.hip).  k_response_row lives here
// and not with the other point functions because it shares its non-inlined device functions (response_light on a YfSvcRow) with
// k_sweep_svc_row: compiled apart, the register allocation of the sweep kernels comes out differently (unit map).
void launch_response_row(plfx_ctx *c, int k, const int32_t *tex_id, int n, const int32_t *mat_id, const double *sig, const double *epl,
                         const double *deps, double *fy, double *sig_out, double *depl, double *ct, int32_t *nsteps)
{
    LAUNCH_ROW1(c, k, tex_id, k_response_row, dim3(std::max(1, std::min((n + 31) / 32, 1024))),
               c->dmat, c->nmat, k, n, mat_id, sig, epl, deps, fy, sig_out, depl, ct, nsteps, c->resp_maxit);
}

int raise_step_lds(plfx_ctx *c)
{
    if (int rc = raise_sweep_lds(c)) return rc;
    if (c->svc_wave_lds > 0) {
        HIPCHK(c, set_dyn_lds((const void *)k_response_row<true>, c->svc_wave_lds));
        if (c->svc_cols_mask & c->svc_row_lds) {
            HIPCHK(c, set_dyn_lds((const void *)k_response_row<true, true>, c->svc_wave_lds));
            HIPCHK(c, set_dyn_lds((const void *)k_response_row<true, true, true, TexFieldDev>, c->svc_wave_lds));
        }
        HIPCHK(c, set_dyn_lds((const void *)k_path_row<true>, c->svc_wave_lds));
        if (c->svc_cols_mask & c->svc_row_lds) {
            HIPCHK(c, set_dyn_lds((const void *)k_path_row<true, true>, c->svc_wave_lds));
            HIPCHK(c, set_dyn_lds((const void *)k_path_row<true, true, true, TexFieldDev>, c->svc_wave_lds));
        }
    }
    return 0;
}

// The load paths of row-kernel material k (plfx_load_path, plfx.hip): here for the reason given at launch_response_row, and
// behind every other row kernel of this file, so that theirs are named first.  Grid as k_response_row.
void launch_path_row(plfx_ctx *c, int k, const int32_t *tex_id, const PathArgs &a)
{
    LAUNCH_ROW1(c, k, tex_id, k_path_row, dim3(std::max(1, std::min((a.n + 31) / 32, 1024))), c->dmat, c->nmat, k, a);
}

}  // namespace host
}  // namespace plfx

extern "C" {

// Grid of k_sweep_light_plane: the element grid (PLFX_SWEEP_BLOCKS included), but no more blocks than the device holds
// at once -- 4 SIMDs per CU at the waves per SIMD the kernel is compiled for.  A count that is off costs speed only.
static int plane_sweep_grid(const plfx_ctx *c)
{
    const int resident = c->prop.multiProcessorCount * (PLANE_SWEEP_WAVES * 4 * 64 / BLOCK);
    int g = std::min(c->grid_el, std::max(resident, 1));
    if (g >= 16) g &= ~7;   // (xcd_tile, as grid_xcd)
    return g;
}

// Before a sweep or calc_scf of a model with a texture field: every element of a field material has a row that exists.  Nothing
// is launched on an index out of range.
static int tex_field_check(plfx_ctx *c)
{
    if (!c->tex_field_mask) return PLFX_OK;
    if (c->strip.on || c->sharded || comm_active(c))
        return fail(c, PLFX_ERR_UNSUPPORTED, "a texture field runs on one GPU without strips or shards");
    if (c->tex_ids_ok || !c->tex_ids) return PLFX_OK;   // (no array: row 0, and an attached field has at least one row)
    for (int e = 0; e < c->nel; e++) {
        const int k = c->hcls[c->hcls_id[(size_t)c->e0 + e]].mat;
        if (!((c->tex_field_mask >> k) & 1u)) continue;
        const int32_t t = c->htex_ids[e];
        if (t < 0 || t >= c->tex_field_rows[k])
            return fail(c, PLFX_ERR_ARG, "texture row %d of element %d is outside the %d rows of material %d", (int)t, e,
                        c->tex_field_rows[k], k);
    }
    c->tex_ids_ok = true;
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ state
int plfx_state_reset(plfx_ctx *c)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    const size_t ne = c->nel, nd = c->ndof;
    HIPCHK(c, hipMemsetAsync(c->sig, 0, 48 * ne, c->stream));
    HIPCHK(c, hipMemsetAsync(c->epl, 0, 48 * ne, c->stream));
    HIPCHK(c, hipMemsetAsync(c->eps, 0, 48 * ne, c->stream));
    HIPCHK(c, hipMemsetAsync(c->res_sig, 0, 48 * ne, c->stream));
    HIPCHK(c, hipMemsetAsync(c->res_depl, 0, 48 * ne, c->stream));
    HIPCHK(c, hipMemsetAsync(c->fyn, 0, 8 * ne, c->stream));
    HIPCHK(c, hipMemsetAsync(c->max_steps, 0, 4 * ne, c->stream));
    HIPCHK(c, hipMemsetAsync(c->u, 0, 8 * nd, c->stream));
    HIPCHK(c, hipMemsetAsync(c->f, 0, 8 * nd, c->stream));
    HIPCHK(c, hipMemsetAsync(c->du, 0, 8 * nd, c->stream));
    HIPCHK(c, hipMemsetAsync(c->flags, 0, 32, c->stream));
    HIPCHK(c, hipMemsetAsync(c->bflags, 0, (size_t)8 * SWEEP_SLOTS, c->stream));
    {   // hardening modulus of every material point = its material's khard (Material.khard before the first response call)
        std::vector<double> kh(c->nel);
        for (int e = 0; e < c->nel; e++) kh[e] = c->hmat[c->hcls[c->hcls_id[c->e0 + e]].mat].khard;
        HIPCHK(c, hipMemcpyAsync(c->kh_el, kh.data(), (size_t)8 * c->nel, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, stream_sync(c));
        for (int m = 0; m < c->nmat && m < 16; m++) c->wh_carry[m] = c->hmat[m].khard;
        c->kh_out_valid = false;
    }
    hipLaunchKernelGGL(k_init_tangent, dim3((c->nel + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream,
                       c->dmat, c->dcls, c->nel, c->dcls_id, tan_store(c), c->Mel + c->e0, c->nel_total);
    if (c->sharded)
        hipLaunchKernelGGL(k_init_M_all, dim3((c->nel_total + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream,
                           c->dmat, c->dcls, c->nel_total, c->dcls_all, c->Mel);
    HIPCHK(c, hipGetLastError());
    // plane columns: the four state arrays are zero from the memsets above; rows 4 and 5 of the factors, which tan_alloc and
    // k_init_tangent leave as they are, are zeroed here -- the invariant holds from this point on
    c->plane_off_by = !c->plane_switch ? PLFX_PLANE_SWITCH : (c->sharded || c->strip.on || comm_active(c)) ? PLFX_PLANE_SHARDED :
                      !c->plane_mats_ok ? PLFX_PLANE_MATERIALS : PLFX_PLANE_ON;
    c->plane_cols = c->plane_off_by == PLFX_PLANE_ON;
    if (c->plane_cols) HIPCHK(c, hipMemsetAsync(c->elfac + 4 * ne, 0, 16 * ne, c->stream));
    c->assembled = false, c->M_dirty = true;
    c->direct_done = c->setup_owed = c->live_owed = false;   // (every generator was rewritten above; the next assembly is a full one)
    c->x_is_du = false;
    c->rhs_rows_ok = c->dinv_ok = false;   // (a new history starts with one full k_bc_finish)
    // (... which writes dinv for every DOF and clears dinv_late there: until then a late dinv stays owed, bc_set still stands)
    c->pred_d_kept = false;   // (the first solve rebuilds x from du)
    c->res_is_sig = c->res_fresh = c->eps_stale = c->res_partial = false;
    c->last_heavy = -1;  // the next sweep launches its corrector kernels whatever the one before found
    return PLFX_OK;
}

// what the end of a load step does with sig: exchange it with res_sig (true) or run the kernel as ever (false)
static int finish_mode(plfx_ctx *c, bool *swap)
{
    *swap = c->nonlin && !c->has_elastic && c->res_fresh;
    if (*swap) return 0;
    return split_res_sig(c);   // no sweep since the last exchange: res_sig == sig, as the kernel will read it
}

static void finish_done(plfx_ctx *c, bool swap)
{
    if (swap) {
        std::swap(c->sig, c->res_sig);
        c->res_is_sig = true;
        c->res_fresh = false;
    }
    c->eps_stale = true;
}

// readers of res_sig / res_depl / fyn: not between a sweep that left them partial (plfx_ctx::res_partial) and its successor
static int res_complete(plfx_ctx *c, const char *who)
{
    if (!c->res_partial) return 0;
    return fail(c, PLFX_ERR_STATE, "%s: the last sweep left res_sig / res_depl / fyn partial (a load step ended in an error "
                                   "between two sweeps): sweep again first", who);
}

static int state_ptr(plfx_ctx *c, int which, double **p, size_t *comps, size_t *n, bool *soa)
{
    *soa = true;
    *n = c->nel;
    if (which == 3 || which == 4 || which == 9) {
        const int rcp = res_complete(c, "state");
        if (rcp) return rcp;
    }
    if (which == 1 || which == 6) {   // eps is read, or eps / u is about to be overwritten: the stored field first
        const int rce = ensure_eps(c);
        if (rce) return rce;
    }
    switch (which) {
    case 0: *p = c->sig; *comps = 6; break;
    case 1: *p = c->eps; *comps = 6; break;
    case 2: *p = c->epl; *comps = 6; break;
    case 3: *p = c->res_is_sig ? c->sig : c->res_sig; *comps = 6; break;
    case 4: *p = c->res_depl; *comps = 6; break;
    case 5: *p = c->elstiff; *comps = 21; break;
    case 6: *p = c->u; *comps = 1; *n = c->ndof; *soa = false; break;
    case 7: *p = c->f; *comps = 1; *n = c->ndof; *soa = false; break;
    case 8: *p = c->du; *comps = 1; *n = c->ndof; *soa = false; break;
    case 9: *p = c->fyn; *comps = 1; *soa = false; break;
    case 11: *p = (wh_sequential(c) && c->kh_out_valid) ? c->kh_out : c->kh_el; *comps = 1; *soa = false; break;  // exit moduli of the last sweep
    default: return fail(c, PLFX_ERR_ARG, "unknown state id %d", which);
    }
    return 0;
}

int plfx_state_get(plfx_ctx *c, int which, double *out)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (!out) return fail(c, PLFX_ERR_ARG, "null output");
    if (which == 10) {
        std::vector<int32_t> t(c->nel);
        HIPCHK(c, hipMemcpyAsync(t.data(), c->max_steps, (size_t)4 * c->nel, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
        for (int e = 0; e < c->nel; e++) out[e] = t[e];
        return PLFX_OK;
    }
    double *p;
    size_t comps, n;
    bool soa;
    int rc = state_ptr(c, which, &p, &comps, &n, &soa);
    if (rc) return rc;
    if (!soa) {
        HIPCHK(c, hipMemcpyAsync(out, p, 8 * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
        return PLFX_OK;
    }
    std::vector<double> t(comps * n);
    if (which == 5) {  // the tangent store expanded to 21 entries per element
        double *tmp = nullptr;
        if ((rc = dalloc(c, &tmp, 21 * n))) return rc;
        launch_tangent_expand(c, tmp, 0);
        hipError_t er = hipGetLastError();
        if (er == hipSuccess) er = hipMemcpyAsync(t.data(), tmp, 8 * comps * n, hipMemcpyDeviceToHost, c->stream);
        if (er == hipSuccess) er = stream_sync(c);
        dfree(tmp);
        HIPCHK(c, er);
    } else {
        HIPCHK(c, hipMemcpyAsync(t.data(), p, 8 * comps * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
    }
    if (comps == 6) {
        for (size_t e = 0; e < n; e++)
            for (int k = 0; k < 6; k++) out[6 * e + k] = t[(size_t)k * n + e];
    } else {  // symmetric 21 -> full 36
        for (size_t e = 0; e < n; e++)
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) out[36 * e + 6 * i + j] = t[(size_t)sym_idx(i, j) * n + e];
    }
    return PLFX_OK;
}

int plfx_state_set(plfx_ctx *c, int which, const double *in)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (!in) return fail(c, PLFX_ERR_ARG, "null input");
    if (which == 10) return fail(c, PLFX_ERR_ARG, "max_steps is read-only");
    double *p;
    size_t comps, n;
    bool soa;
    int rc = (which == 0 || which == 3) ? split_res_sig(c) : 0;   // sig / res_sig written from outside: two buffers first
    if (rc) return rc;
    rc = state_ptr(c, which, &p, &comps, &n, &soa);
    if (rc) return rc;
    if (!soa) {
        c->x_is_du = false;  // u / f / du written from outside
        c->pred_d_kept = false;   // (the next solve rebuilds x from du: pred_d belongs to the x that was there)
        HIPCHK(c, hipMemcpyAsync(p, in, 8 * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, stream_sync(c));
        return PLFX_OK;
    }
    std::vector<double> t(comps * n);
    if (comps == 6) {
        for (size_t e = 0; e < n; e++)
            for (int k = 0; k < 6; k++) t[(size_t)k * n + e] = in[6 * e + k];
    } else {
        for (size_t e = 0; e < n; e++)
            for (int i = 0; i < 6; i++)
                for (int j = i; j < 6; j++) t[(size_t)sym_idx(i, j) * n + e] = in[36 * e + 6 * i + j];
    }
    if (c->plane_cols && (which == 0 || which == 2 || which == 3 || which == 4)) {   // a non-zero in column 3 or 4 ends the plane mode
        const double *c34 = t.data() + 3 * n;
        for (size_t i = 0; i < 2 * n; i++)
            if (c34[i] != 0.) {
                plane_off(c, PLFX_PLANE_STATE_SET);
                break;
            }
    }
    if (which == 5) plane_off(c, PLFX_PLANE_TANGENT_SET);   // (conservative: a tangent from outside may couple the shears)
    HIPCHK(c, hipMemcpyAsync(p, t.data(), 8 * comps * n, hipMemcpyHostToDevice, c->stream));
    if (which == 5) {  // every element's tangent is now held in full form
        c->M_dirty = true;
        if (int rcw = before_M_write(c)) return rcw;
        HIPCHK(c, hipMemsetAsync(c->eltag, TAN_FULL, n, c->stream));
        hipLaunchKernelGGL(k_refresh_M, dim3((c->nel + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream,
                           c->dmat, c->dcls, c->nel, c->dcls_id, tan_store(c), c->Mel + c->e0, c->nel_total);
        HIPCHK(c, hipGetLastError());
        int rcm = sync_M(c);
        if (rcm) return rcm;
    }
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_gather(plfx_ctx *c, int which, int n, const int32_t *idx, double *out)
{
    if (!c || !c->u) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (n < 0 || !idx || !out) return fail(c, PLFX_ERR_ARG, "bad argument");
    if (n == 0) return PLFX_OK;
    const double *src = which == 6 ? c->u : which == 7 ? c->f : which == 8 ? c->du : nullptr;
    if (!src) return fail(c, PLFX_ERR_ARG, "gather supports u(6), f(7), du(8)");
    for (int k = 0; k < n; k++)
        if (idx[k] < 0 || idx[k] >= c->ndof) return fail(c, PLFX_ERR_ARG, "idx[%d] out of range", k);
    int rc = ensure_tmp(c, n);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->idx_tmp, idx, (size_t)4 * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_gather, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, n, c->idx_tmp, src, c->val_tmp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->val_tmp, (size_t)8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

}  // extern "C"

namespace {

// calc_BC through the registered plan for the current increments; returns the first inconsistent entry or -1
int step_apply_bc(plfx_ctx *c, const plfx_step *st, const double *dbcr, const double *dbct, const double *dbcn, int *bad)
{
    auto &P = c->plan;
    const double *val[5] = {st->bcl0, st->bcb0, dbcr, dbct, dbcn};
    std::vector<double> seg(P.nseg);
    for (int i = 0; i < P.nseg; i++) seg[i] = val[P.src[i]][P.k[i]];
    const double *fext = nullptr;
    bool any = false;
    size_t o = 0;
    for (size_t f = 0; f < P.fsrc.size(); f++) {  // edge / node-set forces (model.py:1145-1151, 1173-1179, 1203-1205)
        const double v = val[P.fsrc[f]][P.fk[f]];
        if (v != 0.) {
            if (!any) P.fext.assign(c->ndof, 0.);
            any = true;
            for (int q = 0; q < P.flen[f]; q++) P.fext[P.fidx[o + q]] += v * P.fshare[o + q];
        }
        o += P.flen[f];
    }
    if (any) fext = P.fext.data();
    int b = -1;
    int rc = plfx_apply_bc_plan(c, seg.data(), fext, &b);
    if (bad && *bad < 0) *bad = b;
    return rc;
}

// site: which of the two solves of a load step this is (0 predictor, 1 stiffness iteration; plfx_ctx::first_test_hint)
int step_solve(plfx_ctx *c, plfx_step *st, int warm, int site)
{
    int it = 0;
    double rr = 0.;
    const int rc = solve_impl(c, st->rtol, st->maxit, warm, site, &it, &rr);
    if (rc < 0) return rc;
    if (st->nsolves < 40) {
        st->its[st->nsolves] = it;
        st->relres[st->nsolves] = rr;
    }
    st->nsolves++;
    if (rc == 1) st->soft_fail++;
    return 0;
}
}  // namespace

extern "C" {

int plfx_load_step(plfx_ctx *c, plfx_step *st, double *u_at, double *f_at, double *sums18)
{
    if (!c || !st) return PLFX_ERR_ARG;
    if (!c->plan.valid || !c->plan.sources) return fail(c, PLFX_ERR_STATE, "set_bc_plan / set_bc_sources first");
    if (!c->fin_dev) return fail(c, PLFX_ERR_STATE, "set_finish_set first");
    st->nit = st->nconv = st->nsweeps = st->nsolves = st->soft_fail = 0;
    st->inconsistent_entry = -1;
    st->scale_bc = 1.;
    int rc;
    double dbcr[2] = {st->max_dbcr[0], st->max_dbcr[1]}, dbct[2] = {st->max_dbct[0], st->max_dbct[1]};
    double *dbcn = st->max_dbcn;  // the reference's dbcn IS max_dbcn (alias, model.py:1285)
    // elastic predictor with the stiffness of the previous step (model.py:1290-1291)
    if ((rc = step_apply_bc(c, st, dbcr, dbct, dbcn, &st->inconsistent_entry))) return rc;
    if ((rc = step_solve(c, st, st->warm, 0))) return rc;
    if (st->nonlin) {
        if (st->il < 10) {  // calc_scf (model.py:1036-1067, 1296)
            int64_t cnt = 0;
            double mn = 0., sm = 0., s2 = 0.;
            if ((rc = plfx_scf_all(c, st->sld, &cnt, &mn, &sm, &s2))) return rc;
            if (cnt > 0) {
                const double mean = sm / (double)cnt, sd = std::sqrt(s2 / (double)cnt);
                double scf = (sd < 0.1) ? mn : std::max(1.e-3, mean - sd);
                if (scf < 1.e-3) scf = 1.e-3;
                st->scale_bc = scf;
            }
        }
        for (int k = 0; k < 2; k++) {
            dbcr[k] = st->max_dbcr[k] * st->scale_bc;
            dbct[k] = st->max_dbct[k] * st->scale_bc;
        }
        int nit = 0, change = 1, conv = 0;
        while ((change || !conv) && nit <= 15) {  // model.py:1306
            if (st->il < 6 && nit > 1) {          // reduce the load increment to reach convergence (:1308-1330)
                const double hs = 0.5;
                auto halve = [&](double mx, double tot, double cur0, double &d) {
                    if (mx >= 0.)
                        d = std::max(0.05 * mx, std::min(tot - cur0, d * hs));
                    else
                        d = std::min(0.05 * mx, std::max(tot - cur0, d * hs));
                };
                for (int k = 0; k < 2; k++) {
                    halve(st->max_dbcr[k], st->bcr[k], st->bcr0[k], dbcr[k]);
                    halve(st->max_dbct[k], st->bct[k], st->bct0[k], dbct[k]);
                    if (st->has_nodeset) {  // d and mx are the same variable here
                        const double mx = dbcn[k];
                        halve(mx, st->bcn[k], st->bcn0[k], dbcn[k]);
                    }
                }
            }
            if ((rc = plfx_assemble(c))) return rc;  // updated tangent stiffness (model.py:1333)
            if ((rc = step_apply_bc(c, st, dbcr, dbct, dbcn, &st->inconsistent_entry))) return rc;
            if ((rc = step_solve(c, st, 1, 1))) return rc;
            // (the loop goes on after this sweep only if nit + 1 <= 15: then -- and only then -- what follows the flags is decided
            // by the flags alone and can be enqueued behind them with device-side predicates)
            c->spec_arm = (nit + 1 <= 15) && c->reuse && !wh_sequential(c);
            // (... and a sweep that changes a tangent is then followed by one that rewrites every plastic element's response)
            c->dead_arm = (nit + 1 <= 15) && !wh_sequential(c);
            rc = plfx_sweep(c, nit, &change, &conv);  // model.py:1340-1361
            c->spec_arm = c->dead_arm = false;
            if (rc) return rc;
            st->nsweeps++;
            if (!conv) st->nconv++;
            nit++;
        }
        st->nit = nit;
    }
    for (int k = 0; k < 2; k++) {
        st->dbcr[k] = dbcr[k];
        st->dbct[k] = dbct[k];
        st->dbcn[k] = dbcn[k];
    }
    if (st->defer_slot == 1 || st->defer_slot == 2) {
        if (!c->mbox) return fail(c, PLFX_ERR_UNSUPPORTED, "deferred results need the pinned mailbox (PLFX_MAILBOX=0 is set)");
        c->fin_defer = st->defer_slot - 1;
    }
    return plfx_finish_step(c, u_at, f_at, sums18);
}

int plfx_set_finish_set(plfx_ctx *c, int n, const int32_t *idx)
{
    if (!c || !c->u) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (n < 0 || (n > 0 && !idx)) return fail(c, PLFX_ERR_ARG, "bad argument");
    for (int k = 0; k < n; k++)
        if (idx[k] < 0 || idx[k] >= c->ndof) return fail(c, PLFX_ERR_ARG, "idx[%d] out of range", k);
    HIPCHK(c, stream_sync(c));
    dfree(c->fin_idx);
    dfree(c->fin_dev);
    c->fin_pin_n = 0;  // slots are re-allocated for the new set at the next deferred step
    c->fin_pending[0] = c->fin_pending[1] = false;
    if (c->fin_host) hipHostFree(c->fin_host);
    c->fin_host = nullptr;
    int rc;
    if ((rc = dalloc(c, &c->fin_idx, (size_t)std::max(n, 1)))) return rc;
    if ((rc = dalloc(c, &c->fin_dev, (size_t)2 * n + 18))) return rc;
    HIPCHK(c, hipHostMalloc((void **)&c->fin_host, ((size_t)2 * n + 18) * 8));
    if (n > 0) HIPCHK(c, hipMemcpyAsync(c->fin_idx, idx, (size_t)4 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, stream_sync(c));
    c->fin_n = n;
    return PLFX_OK;
}

int plfx_finish_step(plfx_ctx *c, double *u_at, double *f_at, double *sums18)
{
    if (!c || !c->fin_dev) return c ? fail(c, PLFX_ERR_STATE, "set_finish_set first") : PLFX_ERR_STATE;
    if (!c->assembled) return fail(c, PLFX_ERR_STATE, "assemble first");
    if (res_complete(c, "finish_step")) return PLFX_ERR_STATE;
    // plfx_update_state with calc_global's element sums fused into the state-update kernel (one pass over the state)
    const size_t nd = c->ndof;
    int rc = 0;
    const bool kdu_done = c->spec_kdu && c->spec_h0 == 0 && c->spec_h1 == 0 && !c->strip.on;   // (ran behind the last sweep's flags)
    c->spec_setup = c->spec_kdu = false;
    if (kdu_done)   // u += du, f += K du happened in that pass
        c->n_spec_kdu++;
    else if (!comm_active(c) && !c->strip.on)   // K du over all DOFs (reaction forces, model.py:1384) with the two updates in its epilogue
        launch_kdu_uf(c, nullptr);
    else {
        if ((rc = plain_spmv(c, c->du, c->q))) return rc;
        hipLaunchKernelGGL(k_axpy_uf, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->du, c->q, c->u, c->f);
    }
    const int g = grid_for(c->nel, SUMPART);
    bool swap;
    if ((rc = finish_mode(c, &swap))) return rc;
    if (plane_active(c)) {   // 
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update_state_plane<1>), dim3(g), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, c->dcls, c->ncls,
                           c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->du, (const double2 *)c->u, c->sig, c->epl,
                           tan_store(c), c->res_sig, c->res_depl, c->nonlin ? 1 : 0, swap ? 1 : 0, c->part_g);
        c->n_plane_updates++;
    } else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update_state<1>), dim3(g), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, c->dcls, c->ncls,
                           c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->du, (const double2 *)c->u, c->sig, c->epl,
                           tan_store(c), c->res_sig, c->res_depl, c->nonlin ? 1 : 0, swap ? 1 : 0, c->part_g,
                           c->strip.on ? c->strip.eown_lo : 0, c->strip.on ? c->strip.eown_hi : 0x7fffffff);
    finish_done(c, swap);
    const int n = c->fin_n;
    const int tot = 2 * n + 18;
    const int sl = c->fin_defer;  // >= 0: post into that pinned slot and return without waiting (plfx_finish_fetch collects)
    c->fin_defer = -1;
    if (sl >= 0 && c->fin_pin_n < tot) {
        HIPCHK(c, stream_sync(c));
        for (int q = 0; q < 2; q++) {
            if (c->fin_pin[q]) hipHostFree(c->fin_pin[q]);
            c->fin_pin[q] = nullptr;
            HIPCHK(c, hipHostMalloc((void **)&c->fin_pin[q], (size_t)8 * tot, hipHostMallocMapped | hipHostMallocCoherent));
            if (!c->fin_box[q]) {
                HIPCHK(c, hipHostMalloc((void **)&c->fin_box[q], sizeof(CgMbox), hipHostMallocMapped | hipHostMallocCoherent));
                memset(c->fin_box[q], 0, sizeof(CgMbox));
            }
            c->fin_pending[q] = false;
        }
        c->fin_pin_n = tot;
    }
    // Deferred and no all-reduce pending: the gather / reduction kernels write the pinned slot themselves (32 + 32 + 18 blocks
    // instead of one workgroup pushing 131 KB through PCIe: 25 -> 4 us on the stream at 1024^2) and the post only publishes the
    // sequence number -- their stores are visible to the host before the post kernel starts (kernel boundary on one stream)
    static const bool direct_ok = !(getenv("PLFX_FINISH_DIRECT") && atoi(getenv("PLFX_FINISH_DIRECT")) == 0);
    const bool direct = sl >= 0 && direct_ok && !comm_active(c);
    double *out = direct ? c->fin_pin[sl] : c->fin_dev;
    // boundary values of u and f and the 18 row sums: independent, one launch (the first blocks gather, the last 18 reduce)
    hipLaunchKernelGGL(k_finish_out, dim3((n + BLOCK - 1) / BLOCK + 18), dim3(BLOCK), 0, c->stream, n, c->fin_idx, (const double *)c->u,
                       (const double *)c->f, out, out + n, (const double *)c->part_g, 18, g, out + 2 * (size_t)n);
    HIPCHK(c, hipGetLastError());
    if (comm_active(c) &&  // element sums of the whole mesh (calc_global, model.py:1473-1511)
        (rc = allreduce(c, c->fin_dev + 2 * (size_t)n, 18, NCCL_FLOAT64, NCCL_SUM, "sums")))
        return rc;
    if (sl >= 0) {
        // a slot that was never collected (caller left its loop early) is simply overwritten: the sequence number tells
        // plfx_finish_fetch which post it is waiting for
        const unsigned long long seq = ++c->fin_seq[sl];
        launch_mbox_post(c, c->fin_dev, direct ? 0 : tot, c->fin_pin[sl], c->fin_box[sl], seq);
        HIPCHK(c, hipGetLastError());
        c->fin_pending[sl] = true;
        return PLFX_OK;
    }
    if ((rc = fetch_results(c, c->fin_dev, 2 * n + 18, c->fin_host))) return rc;
    if (u_at && n > 0) memcpy(u_at, c->fin_host, (size_t)8 * n);
    if (f_at && n > 0) memcpy(f_at, c->fin_host + n, (size_t)8 * n);
    if (sums18) memcpy(sums18, c->fin_host + 2 * (size_t)n, 18 * 8);
    return PLFX_OK;
}

int plfx_finish_fetch(plfx_ctx *c, int slot, double *u_at, double *f_at, double *sums18)
{
    if (!c || !c->fin_dev) return c ? fail(c, PLFX_ERR_STATE, "set_finish_set first") : PLFX_ERR_STATE;
    if (slot < 0 || slot > 1 || !c->fin_pending[slot]) return fail(c, PLFX_ERR_STATE, "no deferred results in slot %d", slot);
    int rc = mbox_wait(c, c->fin_seq[slot], c->fin_box[slot]);
    if (rc) return rc;
    c->fin_pending[slot] = false;
    const int n = c->fin_n;
    const double *h = c->fin_pin[slot];
    if (u_at && n > 0) memcpy(u_at, h, (size_t)8 * n);
    if (f_at && n > 0) memcpy(f_at, h + n, (size_t)8 * n);
    if (sums18) memcpy(sums18, h + 2 * (size_t)n, 18 * 8);
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ non-linear driver pieces
static int sweep_once(plfx_ctx *c, int nit, int *changed, int *conv, bool wh_seq)
{
    if (int rct = tex_field_check(c)) return rct;
    // (flags / bflags are left zeroed by the k_sweep_flags of the previous sweep)
    // every plastic element's res_sig is written below: the buffer is a field of its own again, whatever it held
    c->res_is_sig = false;
    c->res_fresh = true;
    // Armed by plfx_load_step alone (plfx_sweep from anywhere else stores everything): if this sweep changes a tangent, the loop
    // there launches another one before anything reads res_sig, res_depl or fyn.  One GPU, no strip, no communicator.
    // (k_sweep_light<1> and <2> honour it: only a model with one of their materials is armed)
    const int dead = (c->dead_arm && c->dead_stores && !comm_active(c) && !c->strip.on && !wh_seq && (c->has_analytic || c->has_princ)) ? 1 : 0;
    c->dead_arm = false;
    c->res_partial = dead != 0;   // (until the final flags are known below; an error return on the way leaves it standing)
    // what follows the flags can be enqueued behind them (plfx_load_step arms it; see below)
    const bool mb_flags = !comm_active(c) && c->mbox && c->mb_cap >= 2;
    const bool skip_heavy = mb_flags && !c->strip.on && c->last_heavy == 0;
    const bool spec = c->spec_arm && !comm_active(c) && c->mbox && c->mb_cap >= 2 && matfree(c) && !c->strip.on && c->assembled;
    c->spec_arm = false;
    // Direct sweep: an assembly follows this sweep whenever it changes a tangent, the snapshot equals the live array,
    // and the plane kernel alone writes generators (no corrector enqueued) -- it stores them into the snapshot itself and the
    // set-up pass behind the flags is left out.  Bit 2: into the snapshot alone.
    const bool plane_only = plane_active(c) && c->has_analytic && !c->has_princ && !c->has_barlat && !c->has_svc && !c->has_svc3 &&
                            !c->has_svcwh && !c->svc_row_all;
    const bool direct = (c->direct_snap & 1) && spec && plane_only && skip_heavy && !c->M_dirty && !c->op.colr && !wh_seq && c->Mop;
    const bool direct_only = direct && (c->direct_snap & 2);
    if (!direct)
        if (int rcw = before_M_write(c)) return rcw;
    EvPair *ev;
    tim_begin(c, 0, &ev);
#define SWEEP_ARGS(lds) c->dmat, c->nmat, c->dcls, c->ncls, lds, c->nel, c->e0, c->dconn, c->dcls_id,          \
                        (const double2 *)c->du, c->sig, c->epl, tan_store(c), c->Mel + c->e0, c->nel_total, \
                        c->res_sig, c->res_depl, c->fyn, c->max_steps, nit, c->flags, c->bflags, c->heavy_list
    // phase 1 per material kind present (the first launched instantiation also clears fyn of elastic elements)
    int first = 1;
    const unsigned fast = c->svc_row_all;   // these materials run on the row kernels, the thread-per-element kernels skip them
    const bool svc_thread = c->has_svc && (c->svc6_mask & ~fast);
    const int grid_r = std::max(1, std::min((c->nel + 31) / 32, 1024));   // 16 lanes per element: 32 elements per block and round
#define ROW_ARGS c->dmat, c->nmat, c->dcls, c->ncls, c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->du,  \
                  c->sig, c->epl, tan_store(c), c->Mel + c->e0, c->nel_total, c->res_sig, c->res_depl, c->fyn,       \
                  c->max_steps, nit, c->flags, c->bflags, c->heavy_list
    if (c->has_analytic || (c->has_elastic && !c->has_princ && !c->has_svc && !c->has_svc3 && !c->has_barlat && !c->has_svcwh && !c->svc_cols_mask)) {
        if (plane_active(c)) {   // (the same timing family)
            if (direct)   // (SWEEP_ARGS with the live array left out or not)
                hipLaunchKernelGGL(k_sweep_light_plane, dim3(plane_sweep_grid(c)), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, c->dcls,
                                   c->ncls, 0, c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->du, c->sig, c->epl, tan_store(c),
                                   direct_only ? (double *)nullptr : c->Mel + c->e0, c->nel_total, c->res_sig, c->res_depl, c->fyn,
                                   c->max_steps, nit, c->flags, c->bflags, c->heavy_list, first, 0u, dead, c->Mop);
            else
                hipLaunchKernelGGL(k_sweep_light_plane, dim3(plane_sweep_grid(c)), dim3(BLOCK), 0, c->stream, SWEEP_ARGS(0), first, 0u, dead,
                                   (double *)nullptr);
            c->n_plane_sweeps++;
        } else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_light<1>), dim3(c->grid_el), dim3(BLOCK), 0, c->stream,
                               SWEEP_ARGS(0), first, 0u, dead);
        first = 0;
    }
    if (c->has_princ) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_light<2>), dim3(c->grid_el), dim3(BLOCK), 0, c->stream,
                           SWEEP_ARGS(0), first, 0u, dead);
        first = 0;
    }
    if (c->has_barlat) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_light<5>), dim3(c->grid_el), dim3(BLOCK), 0, c->stream,
                           SWEEP_ARGS(0), first, 0u, 0);
        first = 0;
    }
    if (svc_thread) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_light<3>), dim3(c->grid_el), dim3(BLOCK), dyn_lds_bytes(c),
                           c->stream, SWEEP_ARGS(c->svc_lds_need), first, fast, 0);
        first = 0;
        c->n_svc_thread_launches++;
    }
    if (fast) {
        for (int k = 0; k < c->nmat; k++)   // one launch per material: its tables fill the LDS
            if ((fast >> k) & 1u) {
                LAUNCH_ROW2(c, k, (const int32_t *)c->tex_ids, k_sweep_svc_row, 0, dim3(grid_r), ROW_ARGS, first, k);
                first = 0;
                c->n_svc_row_launches++;
            }
    }
    if (c->has_svc3) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_light<6>), dim3(c->grid_el), dim3(BLOCK), dyn_lds_bytes(c),
                           c->stream, SWEEP_ARGS(c->svc_lds_need), first, 0u, 0);
        first = 0;
    }
    // work-hardening SVC materials: one wave per element (PLFX_WH_WAVE=0: one thread per element, rounds 2-3)
    const bool wh_wave = !(getenv("PLFX_WH_WAVE") && atoi(getenv("PLFX_WH_WAVE")) == 0);   // read per sweep: tests compare the two forms
    const int grid_wh = std::max(1, std::min((c->nel + 3) / 4, SWEEP_SLOTS));  // one bflags slot pair per block (the kernel grid-strides)
    if (c->has_svcwh && wh_wave) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_wh_wave<0>), dim3(grid_wh), dim3(BLOCK), dyn_lds_bytes(c), c->stream,
                           c->dmat, c->nmat, c->dcls, c->ncls, c->svc_lds_need, c->nel, c->e0, c->dconn, c->dcls_id,
                           (const double2 *)c->du, c->sig, c->epl, tan_store(c), c->Mel + c->e0, c->nel_total, c->res_sig, c->res_depl,
                           c->fyn, c->max_steps, nit, c->flags, c->bflags, c->heavy_list, first, c->kh_el,
                           wh_seq ? c->kh_out : (double *)nullptr, wh_seq ? c->kh_touch : (int32_t *)nullptr);
        first = 0;
    } else if (c->has_svcwh) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_light<7>), dim3(c->grid_el), dim3(BLOCK), dyn_lds_bytes(c),
                           c->stream, SWEEP_ARGS(c->svc_lds_need), first, 0u, 0, c->kh_el, wh_seq ? c->kh_out : (double *)nullptr,
                           wh_seq ? c->kh_touch : (int32_t *)nullptr);
        first = 0;
    }
    tim_end(c, ev);  // family 0: the streaming phase (one launch per material kind present)
    // phase 2 reads the list length from the device; an empty list costs one empty launch per kind.  Single GPU with the mailbox:
    // after a sweep whose list was empty the launches are left out, k_sweep_flags reports a list that turned up after all, and
    // the launches follow then (one more round trip, in the first sweep that grows a list: DESIGN 22)
    auto launch_phase2 = [&]() {
        tim_begin(c, 6, &ev);  // family 6: the compacted 50-sub-step corrector
        if (c->has_analytic)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_heavy<1>), dim3(c->grid_el), dim3(BLOCK), 0, c->stream,
                               SWEEP_ARGS(0), 0u);
        if (c->has_princ)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_heavy<2>), dim3(c->grid_el), dim3(BLOCK), 0, c->stream,
                               SWEEP_ARGS(0), 0u);
        if (c->has_barlat)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_heavy<5>), dim3(c->grid_el), dim3(BLOCK), 0, c->stream,
                               SWEEP_ARGS(0), 0u);
        if (svc_thread)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_heavy<3>), dim3(c->grid_el), dim3(BLOCK), dyn_lds_bytes(c),
                               c->stream, SWEEP_ARGS(c->svc_lds_need), fast);
        if (fast)
            for (int k = 0; k < c->nmat; k++)
                if ((fast >> k) & 1u) LAUNCH_ROW2(c, k, (const int32_t *)c->tex_ids, k_sweep_svc_row, 1, dim3(grid_r), ROW_ARGS, 0, k);
        if (c->has_svc3)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_heavy<6>), dim3(c->grid_el), dim3(BLOCK), dyn_lds_bytes(c),
                               c->stream, SWEEP_ARGS(c->svc_lds_need), 0u);
        if (c->has_svcwh && wh_wave)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_wh_wave<1>), dim3(grid_wh), dim3(BLOCK), dyn_lds_bytes(c), c->stream,
                               c->dmat, c->nmat, c->dcls, c->ncls, c->svc_lds_need, c->nel, c->e0, c->dconn, c->dcls_id,
                               (const double2 *)c->du, c->sig, c->epl, tan_store(c), c->Mel + c->e0, c->nel_total, c->res_sig, c->res_depl,
                               c->fyn, c->max_steps, nit, c->flags, c->bflags, c->heavy_list, 0, c->kh_el,
                               wh_seq ? c->kh_out : (double *)nullptr, wh_seq ? c->kh_touch : (int32_t *)nullptr);
        else if (c->has_svcwh)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_heavy<7>), dim3(c->grid_el), dim3(BLOCK), dyn_lds_bytes(c),
                               c->stream, SWEEP_ARGS(c->svc_lds_need), 0u, c->kh_el, wh_seq ? c->kh_out : (double *)nullptr,
                               wh_seq ? c->kh_touch : (int32_t *)nullptr);
        tim_end(c, ev);
    };
#undef SWEEP_ARGS
#undef ROW_ARGS
    if (skip_heavy)
        c->n_heavy_skipped++;
    else
        launch_phase2();
    int h[4];
    if (mb_flags) {   // single GPU: the flags kernel posts its results itself
        const unsigned long long seq = ++c->mbox_seq;
        hipLaunchKernelGGL(k_sweep_flags, dim3(1), dim3(BLOCK), 0, c->stream, c->bflags, c->flags, c->flags + 4,
                           reinterpret_cast<int *>(c->mb_buf), c->mbox, seq, spec ? c->flags + 8 : (int *)nullptr,
                           spec ? c->spec_sc : (CgScalars *)nullptr, skip_heavy ? 1 : 0);
        if (spec) {
            // what the host would enqueue after reading the flags, enqueued now (the round trip overlaps it): the set-up pass of
            // plfx_assemble if a tangent changed, else -- if every element converged as well -- the K du of plfx_finish_step
            if (!direct) launch_spec_setup(c);
            // (u += du and f += K du in the same pass, MODE 3: the predicate is exactly "plfx_finish_step comes next")
            launch_kdu_uf(c, c->spec_sc);
            c->spec_was_clean = !c->M_dirty;
            c->spec_setup = !direct;
            c->spec_kdu = true;
            if (direct) c->n_direct_sweeps++;
        }
        HIPCHK(c, hipGetLastError());
        bool recovered = false;
        const int rcw = mbox_wait(c, seq);
        if (rcw) return rcw;
        memcpy(h, c->mb_buf, sizeof(h));
        if (skip_heavy && h[0] < 0) {
            // elements need the corrector after all: the flags kernel left its inputs alone and told the two speculative kernels to
            // do nothing; the corrector launches and an unarmed flags kernel follow, and their results are the sweep's
            c->n_heavy_recovered++;
            c->spec_setup = c->spec_kdu = false;
            recovered = true;
            if (direct_only) {   // the corrector writes part of the live array: what this sweep left in the snapshot alone first
                c->live_owed = true;
                if (int rcl = ensure_live_M(c)) return rcl;
            }
            launch_phase2();
            const unsigned long long seq2 = ++c->mbox_seq;
            hipLaunchKernelGGL(k_sweep_flags, dim3(1), dim3(BLOCK), 0, c->stream, c->bflags, c->flags, c->flags + 4,
                               reinterpret_cast<int *>(c->mb_buf), c->mbox, seq2, (int *)nullptr, (CgScalars *)nullptr, 0);
            HIPCHK(c, hipGetLastError());
            const int rcw2 = mbox_wait(c, seq2);
            if (rcw2) return rcw2;
            memcpy(h, c->mb_buf, sizeof(h));
        }
        c->spec_h0 = h[0];
        c->spec_h1 = h[1];
        // the speculative set-up pass rewrote c->diag exactly if the flags kernel it sits behind reported a changed tangent
        // (its predicate flags[8] is "h[0] == 0" of that kernel; after a recovery it was told to skip, and plfx_assemble launches)
        if (spec && h[0]) c->dinv_ok = false;
        // a direct sweep that changed tangents and needed no corrector: the snapshot is taken, plfx_assemble has nothing to launch
        if (direct && h[0] && !recovered) {
            c->direct_done = true;
            if (direct_only) c->live_owed = true;
        }
    } else {
        hipLaunchKernelGGL(k_sweep_flags, dim3(1), dim3(BLOCK), 0, c->stream, c->bflags, c->flags, c->flags + 4);
        HIPCHK(c, hipGetLastError());
        if (comm_active(c)) {  // changed / not-converged / list length of the whole mesh: no host-side collective needed
            // strip: the counts of rewritten tangents / sub-stepped elements stay local (halo elements are replicas)
            const int rca = allreduce(c, c->flags + 4, c->strip.on ? 2 : 4, NCCL_INT32, NCCL_SUM, "flags");
            if (rca) return rca;
        }
        const int rcf = fetch_results(c, reinterpret_cast<const double *>(c->flags + 4), 2, reinterpret_cast<double *>(h));
        if (rcf) return rcf;
    }
    if (h[0] || !c->reuse) {  // the replicated generators are exchanged only when some rank rewrote some of its own
        int rcm = sync_M(c);
        if (rcm) return rcm;
    }
    if (changed) *changed = h[0];
    if (conv) *conv = h[1] ? 0 : 1;
    if (h[0]) c->M_dirty = true;  // generators are rewritten exactly where a tangent changed (finish_element)
    c->n_sweeps++;
    c->n_tangents_rewritten += h[3];
    // the final flags (after a corrector recovery, if there was one): a changed tangent in an armed sweep = fields left partial
    c->res_partial = dead && h[0];
    if (dead) {
        c->n_dead_sweeps++;
        c->n_dead_tangents += h[3];
    }
    c->last_heavy = h[2];
    return PLFX_OK;
}

// Sweep of a model with a work-hardening SVC material in the reference's semantics: ONE hardening modulus per Material object,
// handed from element to element in index order (material.py:808-814, model.py:1340-1359).  The entry modulus of an element is
// the exit modulus of the last element before it whose call evaluated a gradient (else what the material held when the sweep
// began) -- a chain the data-parallel sweep resolves as a fixed point: sweep with guessed entry values (those of the previous
// sweep), derive the entry values that sweep implies (k_wh_entry), repeat while any element's entry value changed.  What a
// sweep rewrites besides its outputs -- tangents and stiffness generators -- is restored from a snapshot before every
// repetition, so the last pass IS the sequential loop's sweep, bit for bit in its inputs.  A handful of passes in practice
// (an entry value only enters the yield check of its call, material.py:259-265 via get_sflow).
static int sweep_wh_sequential(plfx_ctx *c, int nit, int *changed, int *conv)
{
    int rc;
    const size_t ne = c->nel;
    const int nblk = (int)((ne + BLOCK - 1) / BLOCK);
    if (!c->kh_out) {
        if ((rc = dalloc(c, &c->kh_out, ne)) || (rc = dalloc(c, &c->kh_new, ne)) || (rc = dalloc(c, &c->kh_touch, ne)) ||
            (rc = dalloc(c, &c->wh_bmax, (size_t)nblk)) || (rc = dalloc(c, &c->wh_cnt, 4)) ||
            (rc = dalloc(c, &c->wh_snap_el, tan_words(ne))) || (rc = dalloc(c, &c->wh_snap_M, (size_t)6 * c->nel_total)) ||
            (rc = dalloc(c, &c->wh_snap_ms, ne)))
            return rc;
    }
    if ((rc = before_M_write(c))) return rc;   // (the snapshot copies read the live generators)
    HIPCHK(c, hipMemcpyAsync(c->wh_snap_el, c->tan_buf, tan_words(ne) * 8, hipMemcpyDeviceToDevice, c->stream));  // tags and factors too
    HIPCHK(c, hipMemcpyAsync(c->wh_snap_M, c->Mel, (size_t)6 * c->nel_total * 8, hipMemcpyDeviceToDevice, c->stream));
    // max_steps is a running maximum (sweep_epilogue): passes that ran with entry moduli the chain does not confirm must not leave their counts
    HIPCHK(c, hipMemcpyAsync(c->wh_snap_ms, c->max_steps, ne * 4, hipMemcpyDeviceToDevice, c->stream));
    const int64_t sw0 = c->n_sweeps, tr0 = c->n_tangents_rewritten;
    int64_t tr_before = tr0;
    bool any_changed = false;
    const bool dirty0 = c->M_dirty;
    int32_t last[16];
    // every pass confirms at least one more element of the chain (the first one whose entry value was wrong now runs with the
    // right one, everything before it is final), so ne + 2 passes always reach the sequential loop's sweep; two or three do
    // on every trace seen so far (the exit modulus of a call hardly depends on its entry modulus)
    // ... but a pass is a whole sweep + three snapshot restores + host round trips: a chain that resolves one element per pass on
    // a large mesh would cost O(ne) sweeps without a word.  Cap (PLFX_WH_MAXPASS, default 512; never more than ne + 2): beyond it
    // the sweep is reported unresolved (plfx_wh_info) and says so on stderr -- its tangents are those of the last pass
    static const int wh_cap = getenv("PLFX_WH_MAXPASS") ? std::max(2, atoi(getenv("PLFX_WH_MAXPASS"))) : 512;
    const int max_pass = (int)std::min<size_t>(ne + 2, (size_t)wh_cap);
    int pass = 0;
    for (;; pass++) {
        if (pass > 0) {
            HIPCHK(c, hipMemcpyAsync(c->tan_buf, c->wh_snap_el, tan_words(ne) * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->Mel, c->wh_snap_M, (size_t)6 * c->nel_total * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->max_steps, c->wh_snap_ms, ne * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        int ch = 0, cv = 0;
        tr_before = c->n_tangents_rewritten;
        if ((rc = sweep_once(c, nit, &ch, &cv, true))) return rc;
        any_changed = (ch != 0);   // of the accepted (last) pass: the earlier ones are undone by the snapshot
        if (changed) *changed = ch;
        if (conv) *conv = cv;
        // entry values this pass implies
        HIPCHK(c, hipMemcpyAsync(c->kh_new, c->kh_el, ne * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->wh_cnt, 0, 16, c->stream));
        for (int m = 0; m < c->nmat && m < 16; m++) {
            last[m] = -1;
            if (c->hmat[m].kind != 7) continue;
            hipLaunchKernelGGL(k_wh_blockmax, dim3(nblk), dim3(BLOCK), 0, c->stream, c->nel, m, c->dcls, c->dcls_id, c->kh_touch, c->wh_bmax);
            hipLaunchKernelGGL(k_wh_scan, dim3(1), dim3(BLOCK), 0, c->stream, nblk, c->wh_bmax, c->wh_cnt + 1);
            hipLaunchKernelGGL(k_wh_entry, dim3(nblk), dim3(BLOCK), 0, c->stream, c->nel, m, c->dcls, c->dcls_id, c->kh_touch, c->wh_bmax,
                               (const double *)c->kh_out, c->wh_carry[m], (const double *)c->kh_el, c->kh_new, c->wh_cnt);
            HIPCHK(c, hipGetLastError());
            int32_t h2[2];
            HIPCHK(c, hipMemcpyAsync(h2, c->wh_cnt, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, stream_sync(c));
            last[m] = h2[1];   // (h2[0] accumulates over the materials)
        }
        int32_t nch = 0;
        HIPCHK(c, hipMemcpyAsync(&nch, c->wh_cnt, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
        c->n_wh_passes++;
        if (getenv("PLFX_WH_DEBUG")) {
            std::vector<double> ko(ne), ki(ne);
            std::vector<int32_t> tc(ne);
            hipMemcpy(ko.data(), c->kh_out, ne * 8, hipMemcpyDeviceToHost);
            hipMemcpy(ki.data(), c->kh_el, ne * 8, hipMemcpyDeviceToHost);
            hipMemcpy(tc.data(), c->kh_touch, ne * 4, hipMemcpyDeviceToHost);
            int nt = 0;
            double kmax = 0., imax = 0.;
            for (size_t e = 0; e < ne; e++) nt += tc[e], kmax = std::max(kmax, ko[e]), imax = std::max(imax, ki[e]);
            fprintf(stderr, "[wh] sweep %lld pass %d: %d entries changed, %d touched, max entry %.6g, max exit %.6g, last touched %d, carry %.6g\n",
                    (long long)c->n_wh_sweeps, pass, nch, nt, imax, kmax, last[0], c->wh_carry[0]);
        }
        if (nch == 0) break;
        if (pass + 1 >= max_pass) {  // (ne + 2 passes always resolve the chain; the cap above may end it earlier)
            if (c->n_wh_unresolved++ == 0)
                fprintf(stderr, "[plfx] work-hardening carry chain not resolved after %d passes (%d entry moduli still changed): "
                                "PLFX_WH_MAXPASS raises the cap (plfx_wh_info counts such sweeps)\n", pass + 1, (int)nch);
            break;
        }
        std::swap(c->kh_el, c->kh_new);
    }
    // the material objects now hold what their last gradient evaluation of this sweep left
    for (int m = 0; m < c->nmat && m < 16; m++)
        if (c->hmat[m].kind == 7 && last[m] >= 0)
            HIPCHK(c, hipMemcpy(&c->wh_carry[m], c->kh_out + last[m], 8, hipMemcpyDeviceToHost));
    c->kh_out_valid = true;
    c->n_wh_sweeps++;
    c->n_sweeps = sw0 + 1;   // one sweep of the load-step loop, however many passes it took
    c->n_tangents_rewritten = tr0 + (c->n_tangents_rewritten - tr_before);   // ... and the rewrites of its last pass
    c->M_dirty = dirty0 || any_changed;   // (sweep_once set it in passes the snapshot has undone)
    return PLFX_OK;
}

int plfx_sweep(plfx_ctx *c, int nit, int *changed, int *conv)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (c->n_noflow) return fail(c, PLFX_ERR_UNSUPPORTED, "a Tresca / Barlat material without flow rule is loaded (material.py:822-825)");
    c->spec_setup = c->spec_kdu = false;
    if (wh_sequential(c)) return sweep_wh_sequential(c, nit, changed, conv);
    return sweep_once(c, nit, changed, conv, false);
}

// moduli calc_scf reads (model.py:1036-1067: calc_yf / ML_full_yf -> get_sflow with the value the material holds NOW): per
// point, or -- sequential carry -- the material object's current value for every element of that material
static const double *scf_moduli(plfx_ctx *c)
{
    if (!wh_sequential(c)) return c->kh_el;
    if (!c->kh_new && dalloc(c, &c->kh_new, (size_t)c->nel)) return c->kh_el;
    WhCarry w;
    for (int m = 0; m < 16; m++) w.v[m] = c->wh_carry[m];
    hipLaunchKernelGGL(k_wh_fill, dim3(grid_for(c->nel)), dim3(BLOCK), 0, c->stream, c->nel, c->dcls, c->dcls_id, w, c->kh_new);
    return c->kh_new;
}

int plfx_set_wh_mode(plfx_ctx *c, int sequential)
{
    if (!c) return PLFX_ERR_STATE;
    c->wh_mode = sequential ? 1 : 0;
    c->kh_out_valid = false;
    return PLFX_OK;
}

int plfx_wh_info(plfx_ctx *c, int *sequential_in_use, int64_t *sweeps, int64_t *passes, int64_t *unresolved)
{
    if (!c) return PLFX_ERR_STATE;
    if (unresolved) *unresolved = c->n_wh_unresolved;
    if (sequential_in_use) *sequential_in_use = wh_sequential(c) ? 1 : 0;
    if (sweeps) *sweeps = c->n_wh_sweeps;
    if (passes) *passes = c->n_wh_passes;
    return PLFX_OK;
}

int plfx_wh_carry(plfx_ctx *c, int mat, const double *set, double *get)
{
    if (!c || mat < 0 || mat >= c->nmat || mat >= 16) return c ? fail(c, PLFX_ERR_ARG, "material %d out of range", mat) : PLFX_ERR_STATE;
    if (set) c->wh_carry[mat] = *set;
    if (get) *get = c->wh_carry[mat];
    return PLFX_OK;
}

// calc_scf per element: hh and multiplicity of every owned element into scf_hh / scf_mult (sld at small + 32)
static void launch_scf_elements(plfx_ctx *c)
{
    const unsigned fast = c->svc_row_all;
    hipLaunchKernelGGL(k_scf_elements, dim3(c->grid_el), dim3(BLOCK), dyn_lds_bytes(c), c->stream,
                       c->dmat, c->nmat, c->dcls, c->ncls, c->svc_lds_need, c->nel, c->e0, c->dconn,
                       c->dcls_id, (const double2 *)c->du, c->sig, c->epl, tan_store(c),
                       c->small + 32, c->scf_hh, c->scf_mult, scf_moduli(c), fast);
    for (int k = 0; k < c->nmat; k++)
        if ((fast >> k) & 1u)
            LAUNCH_ROW1(c, k, (const int32_t *)c->tex_ids, k_scf_row, dim3(std::max(1, std::min((c->nel + 31) / 32, 1024))),
                       c->dmat, c->nmat, c->dcls, k, c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->du,
                       c->sig, c->epl, tan_store(c), c->small + 32, c->scf_hh, c->scf_mult);
}

int plfx_scf_stats(plfx_ctx *c, const double *sld, double *sum, double *sumsq_c, double *minv,
                   int64_t *count, double mean_in, int pass)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    const int g = grid_for(c->nel, 256);
    if (pass == 0) {
        if (!sld) return fail(c, PLFX_ERR_ARG, "sld required");
        if (int rct = tex_field_check(c)) return rct;
        HIPCHK(c, hipMemcpyAsync(c->small + 32, sld, 48, hipMemcpyHostToDevice, c->stream));
        launch_scf_elements(c);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_scf_reduce, dim3(g), dim3(BLOCK), 0, c->stream, c->nel, c->scf_hh, c->scf_mult,
                       mean_in, pass, c->part_g);
    HIPCHK(c, hipGetLastError());
    std::vector<double> h((size_t)3 * g);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->part_g, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    double s = 0., cnt = 0., mn = 1.e300;
    for (int b = 0; b < g; b++) {
        s += h[b];
        cnt += h[g + b];
        mn = std::min(mn, h[2 * (size_t)g + b]);
    }
    if (pass == 0) {
        if (sum) *sum = s;
        if (count) *count = (int64_t)(cnt + 0.5);
        if (minv) *minv = mn;
    } else if (sumsq_c) {
        *sumsq_c = s;
    }
    return PLFX_OK;
}

int plfx_scf_all(plfx_ctx *c, const double *sld, int64_t *count, double *minv, double *sum, double *sumsq_c)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (!sld) return fail(c, PLFX_ERR_ARG, "sld required");
    if (int rct = tex_field_check(c)) return rct;
    const int g = grid_for(c->nel, 256);
    HIPCHK(c, hipMemcpyAsync(c->small + 32, sld, 48, hipMemcpyHostToDevice, c->stream));
    launch_scf_elements(c);
    const int elo = c->strip.on ? c->strip.eown_lo : 0, ehi = c->strip.on ? c->strip.eown_hi : 0x7fffffff;
    hipLaunchKernelGGL(k_scf_reduce, dim3(g), dim3(BLOCK), 0, c->stream, c->nel, c->scf_hh, c->scf_mult, 0., 0,
                       c->part_g, (const double *)nullptr, elo, ehi);
    hipLaunchKernelGGL(k_scf_finish, dim3(1), dim3(BLOCK), 0, c->stream, c->part_g, g, 0, c->small + 40);
    if (comm_active(c)) {  // statistics of the whole mesh: sum, count (SUM) and minimum (MIN), then the global mean
        int rca = allreduce(c, c->small + 40, 2, NCCL_FLOAT64, NCCL_SUM, "scf sums");
        if (!rca) rca = allreduce(c, c->small + 42, 1, NCCL_FLOAT64, NCCL_MIN, "scf min");
        if (rca) return rca;
        hipLaunchKernelGGL(k_scf_mean, dim3(1), dim3(64), 0, c->stream, c->small + 40);
    }
    // second pass with the mean taken from device memory: no host round trip between the passes
    hipLaunchKernelGGL(k_scf_reduce, dim3(g), dim3(BLOCK), 0, c->stream, c->nel, c->scf_hh, c->scf_mult, 0., 1,
                       c->part_g, (const double *)(c->small + 43), elo, ehi);
    hipLaunchKernelGGL(k_scf_finish, dim3(1), dim3(BLOCK), 0, c->stream, c->part_g, g, 1, c->small + 40);
    if (comm_active(c)) {
        const int rca = allreduce(c, c->small + 44, 1, NCCL_FLOAT64, NCCL_SUM, "scf squares");
        if (rca) return rca;
    }
    HIPCHK(c, hipGetLastError());
    double h[5];
    {
        const int rcf = fetch_results(c, c->small + 40, 5, h);
        if (rcf) return rcf;
    }
    if (sum) *sum = h[0];
    if (count) *count = (int64_t)(h[1] + 0.5);
    if (minv) *minv = h[2];
    if (sumsq_c) *sumsq_c = h[4];
    return PLFX_OK;
}

int plfx_update_state(plfx_ctx *c)
{
    if (!c || !c->assembled) return c ? fail(c, PLFX_ERR_STATE, "assemble first") : PLFX_ERR_STATE;
    if (res_complete(c, "update_state")) return PLFX_ERR_STATE;
    const size_t nd = c->ndof;
    int rc = 0;
    const bool kdu_done = c->spec_kdu && c->spec_h0 == 0 && c->spec_h1 == 0 && !c->strip.on;   // (ran behind the last sweep's flags)
    c->spec_setup = c->spec_kdu = false;
    if (kdu_done)   // u += du, f += K du happened in that pass
        c->n_spec_kdu++;
    else if (!comm_active(c) && !c->strip.on)   // K du over all DOFs (reaction forces, model.py:1384) with the two updates in its epilogue
        launch_kdu_uf(c, nullptr);
    else {
        if ((rc = plain_spmv(c, c->du, c->q))) return rc;
        hipLaunchKernelGGL(k_axpy_uf, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->du, c->q, c->u, c->f);
    }
    bool swap;
    if ((rc = finish_mode(c, &swap))) return rc;
    if (plane_active(c)) {   // 
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update_state_plane<0>), dim3(grid_for(c->nel, MAXPART)), dim3(BLOCK), 0, c->stream,
                           c->dmat, c->nmat, c->dcls, c->ncls, c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->du,
                           (const double2 *)c->u, c->sig, c->epl, tan_store(c), c->res_sig,
                           c->res_depl, c->nonlin ? 1 : 0, swap ? 1 : 0, (double *)nullptr);
        c->n_plane_updates++;
    } else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update_state<0>), dim3(grid_for(c->nel, MAXPART)), dim3(BLOCK), 0, c->stream,
                           c->dmat, c->nmat, c->dcls, c->ncls, c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->du,
                           (const double2 *)c->u, c->sig, c->epl, tan_store(c), c->res_sig,
                           c->res_depl, c->nonlin ? 1 : 0, swap ? 1 : 0, (double *)nullptr);
    HIPCHK(c, hipGetLastError());
    finish_done(c, swap);
    return PLFX_OK;
}

int plfx_global_sums(plfx_ctx *c, double *out18)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (!out18) return fail(c, PLFX_ERR_ARG, "null output");
    if (res_complete(c, "global_sums")) return PLFX_ERR_STATE;
    const int g = grid_for(c->nel, SUMPART);  // same grid as the fused sums of plfx_finish_step: identical numbers
    const int rce = ensure_eps(c);
    if (rce) return rce;
    hipLaunchKernelGGL(k_global_partials, dim3(g), dim3(BLOCK), 0, c->stream, c->dcls, c->nel, c->dcls_id,
                       c->sig, c->eps, c->epl, c->part_g);
    hipLaunchKernelGGL(k_reduce_rows, dim3(18), dim3(BLOCK), 0, c->stream, c->part_g, 18, g, c->small);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out18, c->small, 18 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

// Element result fields (Model.field / fields / field_range): reads the state, changes none of it and none of its flags
int plfx_element_fields(plfx_ctx *c, int nsel, const int32_t *sel, double *out, double *range)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (nsel < 0 || (nsel > 0 && !sel)) return fail(c, PLFX_ERR_ARG, "bad selector list");
    for (int k = 0; k < nsel; k++)
        if (sel[k] < 0 || sel[k] >= FLD_COUNT) return fail(c, PLFX_ERR_ARG, "unknown field selector %d (sel[%d])", sel[k], k);
    if (nsel == 0 || (!out && !range)) return PLFX_OK;
    const size_t ne = c->nel;
    FieldPlan pl{};
    int first[FLD_COUNT];   // first position of a selector in the list: the row the kernel writes
    for (int id = 0; id < FLD_COUNT; id++) first[id] = -1;
    for (int k = 0; k < nsel; k++)
        if (first[sel[k]] < 0) first[sel[k]] = k;
    bool disp = false, strain = false, all_kinds = false;
    for (int id = 0; id < FLD_COUNT; id++) {
        if (first[id] < 0) continue;
        pl.want |= 1u << id;
        pl.row[id] = first[id];
        switch (id) {
        case FLD_STRAIN1: pl.eps_cols |= 1u; strain = true; break;
        case FLD_STRAIN2: pl.eps_cols |= 2u; strain = true; break;
        case FLD_STRAIN12: pl.eps_cols |= 32u; strain = true; break;
        case FLD_ETOT: pl.eps_cols |= 63u; strain = true; break;
        case FLD_STRESS1: pl.sig_cols |= 1u; break;
        case FLD_STRESS2: pl.sig_cols |= 2u; break;
        case FLD_STRESS12: pl.sig_cols |= 32u; break;
        case FLD_SEQ: case FLD_SEQJ2: pl.sig_cols |= 63u; break;
        case FLD_PLASTIC1: pl.epl_cols |= 1u; break;
        case FLD_PLASTIC2: pl.epl_cols |= 2u; break;
        case FLD_PLASTIC12: pl.epl_cols |= 32u; break;
        case FLD_PEEQ: pl.epl_cols |= 63u; break;
        default: disp = true; break;   // ux, uy
        }
    }
    pl.eps_from_u = (strain && c->eps_stale) ? 1 : 0;   // never a stale c->eps; eps_stale and the stored field stay as they are
    if (pl.eps_from_u) pl.eps_cols = 0;
    pl.need_u = (disp || pl.eps_from_u) ? 1 : 0;
    pl.store = out ? 1 : 0;
    if ((pl.want >> FLD_SEQ) & 1u)
        for (int m = 0; m < c->nmat; m++) {
            const int kd = c->hmat[m].kind;
            if (kd == 2 || kd == 4 || kd == 5 || kd == 6) all_kinds = true;
        }
    int rc;
    if (out && c->fld_cap < (size_t)nsel * ne) {
        if ((rc = dalloc(c, &c->fld_buf, (size_t)nsel * ne))) return rc;
        c->fld_cap = (size_t)nsel * ne;
    }
    if (range && !c->fld_part && (rc = dalloc(c, &c->fld_part, (size_t)2 * FLD_COUNT * MAXPART))) return rc;
    const int g = grid_for(ne, MAXPART);
    EvPair *ev;
    tim_begin(c, 0, &ev);   // family 0, like the batched point kernels: the kernel alone, without the copies
    // sig through c->sig at launch time: after an exchange it holds the current stress, the other buffer is scratch
#define PLFX_FLD_LAUNCH(A, R)                                                                                                  \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_element_fields<A, R>), dim3(g), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, c->dcls,  \
                       c->ncls, c->nel, c->e0, c->dconn, c->dcls_id, (const double2 *)c->u, c->sig, c->epl, c->eps, pl,        \
                       c->fld_buf, c->fld_part)
    if (all_kinds) {
        if (range) PLFX_FLD_LAUNCH(1, 1); else PLFX_FLD_LAUNCH(1, 0);
    } else {
        if (range) PLFX_FLD_LAUNCH(0, 1); else PLFX_FLD_LAUNCH(0, 0);
    }
#undef PLFX_FLD_LAUNCH
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    if (out) {
        for (int k = 0; k < nsel; k++)   // a selector named again: its row once more
            if (first[sel[k]] != k)
                HIPCHK(c, hipMemcpyAsync(c->fld_buf + (size_t)k * ne, c->fld_buf + (size_t)first[sel[k]] * ne, 8 * ne,
                                         hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(out, c->fld_buf, (size_t)nsel * ne * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (range) {
        c->fld_host.resize((size_t)2 * FLD_COUNT * g);
        HIPCHK(c, hipMemcpyAsync(c->fld_host.data(), c->fld_part, (size_t)2 * FLD_COUNT * g * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, stream_sync(c));
    if (range)   // at most MAXPART partials per scalar: the last stage on the host
        for (int k = 0; k < nsel; k++) {
            const double *pmin = c->fld_host.data() + (size_t)(2 * sel[k]) * g, *pmax = pmin + g;
            double lo = pmin[0], hi = pmax[0];
            bool isnan_ = false;
            for (int b = 0; b < g; b++) {
                isnan_ = isnan_ || pmin[b] != pmin[b] || pmax[b] != pmax[b];
                lo = std::min(lo, pmin[b]);
                hi = std::max(hi, pmax[b]);
            }
            range[2 * k] = isnan_ ? std::nan("") : lo;
            range[2 * k + 1] = isnan_ ? std::nan("") : hi;
        }
    return PLFX_OK;
}

}  // extern "C"
