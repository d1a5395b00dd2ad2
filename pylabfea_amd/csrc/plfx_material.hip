// plfx_material.hip -- libplfx.so: the material tables of a context, the material-point functions (batched point evaluation,
// yield loci, flow curves, load paths, committees), the texture SVC, and the SVC / SVR training and SVR-flow entries.
// Unit map and the one-owner rule for kernels: DESIGN.md sections 39 and 42; what the units share: plfx_host.hpp.
#define PLFX_UNIT_MATERIALS
#include "plfx_host.hpp"
#include "plfx_texflow.hpp"
#include "plfx_flow.hpp"

using namespace plfx;
using namespace plfx::host;

namespace plfx {
namespace host {

#ifdef PLFX_PROF_REGIONS
bool prof_regions_add_material(unsigned long long h[16])
{
    unsigned long long mine[16];
    if (hipMemcpyFromSymbol(mine, HIP_SYMBOL(g_prof), sizeof(mine)) != hipSuccess) return false;
    for (int i = 0; i < 16; i++) h[i] += mine[i];
    return true;
}
#endif

// 6x6 symmetric (row-major 36) -> 21
void pack_sym(const double *A, double *S)
{
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) S[sym_idx(i, j)] = A[i * 6 + j];
}

// inverse of the leading n x n block (n = 2 or 3) by Gauss-Jordan with partial pivoting
bool inv_small(const double *A, int lda, int n, double *Ai)
{
    double w[3][6];
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            w[i][j] = A[i * lda + j];
            w[i][n + j] = (i == j) ? 1. : 0.;
        }
    for (int col = 0; col < n; col++) {
        int piv = col;
        for (int r = col + 1; r < n; r++)
            if (std::fabs(w[r][col]) > std::fabs(w[piv][col])) piv = r;
        if (w[piv][col] == 0.) return false;
        if (piv != col)
            for (int j = 0; j < 2 * n; j++) std::swap(w[col][j], w[piv][j]);
        const double d = w[col][col];
        for (int j = 0; j < 2 * n; j++) w[col][j] /= d;
        for (int r = 0; r < n; r++)
            if (r != col) {
                const double fct = w[r][col];
                for (int j = 0; j < 2 * n; j++) w[r][j] -= fct * w[col][j];
            }
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) Ai[i * n + j] = w[i][n + j];
    return true;
}

void free_tex_field(plfx_ctx *c, int k)
{
    TexFieldDev &f = c->tex_field[k];
    if (f.coef) hipFree((void *)f.coef);
    if (f.sabs) hipFree((void *)f.sabs);
    f = TexFieldDev();
    c->tex_field_mask &= ~(1u << k);
    c->tex_field_rows[k] = 0;
    c->tex_field_launches[k] = 0;
    c->tex_ids_ok = false;
}

void free_svr_flow(plfx_ctx *c, int k)
{
    SvrFlowDev &f = c->svr_flow[k];
    if (f.X) hipFree((void *)f.X);
    if (f.coef) hipFree((void *)f.coef);
    f = SvrFlowDev();
    c->svr_mask &= ~(1u << k);
    c->svr_launches[k] = 0;
}

void free_materials(plfx_ctx *c)
{
    for (int k = 0; k < MAXMAT; k++) free_svr_flow(c, k);   // a rule belongs to the material it was attached to
    for (int k = 0; k < MAXMAT; k++) free_tex_field(c, k);  // ... and so does a texture field
    for (double *p : c->dsv) hipFree(p);
    c->dsv.clear();
    dfree(c->dmat);
    c->hmat.clear();
    c->nmat = 0;
}

}  // namespace host
}  // namespace plfx

#include "plfx_svm.hpp"

extern "C" {

// ------------------------------------------------------------------------------ materials
// Plane columns.  The closure argument asks of every material of the table, used or not: elastic or analytic Hill /
// J2 (the kinds whose gradient takes components 3 and 4 from components 3 and 4 alone), CV and SV exactly 0.0 between
// {xx, yy, zz, xy} and {yz, zx}, and everything that multiplies a zero of those columns finite (0 * inf is not 0).
static bool plane_materials_ok(const std::vector<MatDev> &mats)
{
    for (const MatDev &m : mats) {
        if (m.kind != PLFX_ELASTIC && m.kind != PLFX_HILL6) return false;
        for (int i : {0, 1, 2, 5})
            for (int j : {3, 4})
                if (m.CV[sym_idx(i, j)] != 0. || m.SV[sym_idx(i, j)] != 0.) return false;
        for (const double *T : {m.CV, m.SV})
            if (!std::isfinite(T[sym_idx(3, 3)]) || !std::isfinite(T[sym_idx(4, 4)]) || !std::isfinite(T[sym_idx(3, 4)])) return false;
        if (!std::isfinite(m.hill[3]) || !std::isfinite(m.hill[4]) || !std::isfinite(m.sy) || !std::isfinite(m.khard) ||
            !std::isfinite(m.d0))
            return false;
    }
    return !mats.empty();
}

int plfx_set_materials(plfx_ctx *c, int nmat, const plfx_material *mats)
{
    if (!c || !c->stream) return PLFX_ERR_STATE;
    if (nmat < 1 || nmat > MAXMAT || !mats) return fail(c, PLFX_ERR_ARG, "nmat must be in 1..%d", MAXMAT);
    if (c->tan_buf && c->dmat && c->nel > 0) {
        // eps and res_sig as stored fields before the tables they were deferred under go away
        int rcs;
        if ((rcs = ensure_eps(c)) || (rcs = split_res_sig(c))) return rcs;
        c->res_fresh = false;
        // the tangent store refers to the CV of the current materials: hold every stored tangent in full form first
        launch_tangent_expand(c, c->elstiff, 1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, stream_sync(c));
    }
    free_materials(c);
    c->has_svc = c->has_svc3 = c->has_analytic = c->has_elastic = c->has_princ = false;
    c->has_barlat = false;
    c->has_svcwh = false;
    c->plane_mats_ok = false;
    c->n_noflow = 0;
    c->svc_lds_need = 0;
    c->svc_row_all = c->svc_row_lds = c->svc6_mask = c->svcwh_mask = c->svc_cols_mask = 0;
    c->svc_wave_lds = 0;
    c->n_svc6 = 0;
    c->nonlin = false;
    c->hmat.resize(nmat);
    bool wave_pad = false;
    for (int k = 0; k < nmat; k++) {
        const plfx_material &s = mats[k];
        MatDev &m = c->hmat[k];
        memset(&m, 0, sizeof(m));
        if (s.kind < PLFX_ELASTIC || s.kind > PLFX_SVC6_COLS)
            return fail(c, PLFX_ERR_ARG, "material %d: unknown kind %d", k, s.kind);
        for (int i = 0; i < 6; i++)
            for (int j = i + 1; j < 6; j++)
                if (std::fabs(s.CV[i * 6 + j] - s.CV[j * 6 + i]) >
                    1e-9 * (std::fabs(s.CV[i * 6 + j]) + std::fabs(s.CV[j * 6 + i]) + 1e-300))
                    return fail(c, PLFX_ERR_ARG, "material %d: CV must be symmetric", k);
        pack_sym(s.CV, m.CV);
        // compliance of the scale-back step (material.py:315-320)
        double SV[36] = {0.};
        const int nb = (s.CV[2 * 6 + 2] > 1.) ? 3 : 2;
        double hh[9];
        if (!inv_small(s.CV, 6, nb, hh)) return fail(c, PLFX_ERR_ARG, "material %d: singular CV block", k);
        for (int i = 0; i < nb; i++)
            for (int j = 0; j < nb; j++) SV[i * 6 + j] = hh[i * nb + j];
        for (int i = 3; i < 6; i++)
            if (s.CV[i * 6 + i] > 1.) SV[i * 6 + i] = 1. / s.CV[i * 6 + i];
        // symmetrise round-off of the Gauss-Jordan inverse
        for (int i = 0; i < 6; i++)
            for (int j = i + 1; j < 6; j++) SV[i * 6 + j] = SV[j * 6 + i] = 0.5 * (SV[i * 6 + j] + SV[j * 6 + i]);
        pack_sym(SV, m.SV);
        for (int i = 0; i < 6; i++) m.hill[i] = (s.kind == PLFX_ELASTIC) ? 1. : s.hill[i];
        m.sy = s.sy;
        m.khard = s.khard;
        m.d0 = (s.kind == PLFX_ELASTIC) ? 0. : s.drucker;
        m.E = s.E;
        m.nu = s.nu;
        m.kind = s.kind;
        m.sdim = (s.kind == PLFX_PRINC3 || s.kind == PLFX_SVC3) ? 3 : 6;
        for (int i = 0; i < 18; i++) m.barlat[i] = s.barlat[i];
        m.barlat_exp = s.barlat_exp;
        m.barlat_normal = (s.kind == PLFX_BARLAT && s.barlat_normal) ? 1 : 0;
        if (s.kind != PLFX_ELASTIC) c->nonlin = true;
        if (s.kind == PLFX_HILL6) c->has_analytic = true;
        if (s.kind == PLFX_PRINC3) c->has_princ = true;
        if (s.kind == PLFX_ELASTIC) c->has_elastic = true;
        if (s.kind == PLFX_BARLAT && s.barlat_normal) c->has_barlat = true;
        if (s.kind == PLFX_TRESCA || (s.kind == PLFX_BARLAT && !s.barlat_normal)) c->n_noflow++;
        const bool cols = (s.kind == PLFX_SVC6_COLS);
        if (s.kind == PLFX_SVC6 || s.kind == PLFX_SVC3 || s.kind == PLFX_SVC_WH || cols) {
            const int nf = (s.kind == PLFX_SVC6 || cols) ? 6 : (s.kind == PLFX_SVC3) ? 2 : 15;
            if (s.kind == PLFX_SVC_WH && !(s.scale_wh > 0.)) return fail(c, PLFX_ERR_ARG, "material %d: scale_wh must be positive", k);
            if (s.nsv < 1 || s.nfeat != nf || !s.sv || !s.dual)
                return fail(c, PLFX_ERR_ARG, "material %d: SVC needs nsv>=1, nfeat==%d, sv and dual", k, nf);
            double *dsv = nullptr, *ddu = nullptr;
            HIPCHK(c, hipMalloc((void **)&dsv, (size_t)s.nsv * nf * 8));
            c->dsv.push_back(dsv);
            HIPCHK(c, hipMalloc((void **)&ddu, (size_t)s.nsv * 8));
            c->dsv.push_back(ddu);
            HIPCHK(c, hipMemcpy(dsv, s.sv, (size_t)s.nsv * nf * 8, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(ddu, s.dual, (size_t)s.nsv * 8, hipMemcpyHostToDevice));
            m.sv = dsv;
            m.dual = ddu;
            m.nsv = s.nsv;
            m.nfeat = nf;
            m.dev_only = s.dev_only;
            m.gamma = s.gamma;
            m.intercept = s.intercept;
            m.scale_seq = s.scale_seq;
            m.scale_wh = (s.kind == PLFX_SVC_WH) ? s.scale_wh : 1.;
            for (int i = 0; i < s.nsv; i++) {
                double vv = 0.;
                for (int f = 0; f < nf; f++) vv += s.sv[(size_t)i * nf + f] * s.sv[(size_t)i * nf + f];
                m.svc_vvmax = std::max(m.svc_vvmax, vv);
                m.svc_sabs += std::fabs(s.dual[i]);
            }
            if (cols) {
                // the row kernels alone run this kind (none of the thread-per-point tables or flags): every column scale is
                // scale_seq until plfx_set_svc_cols says otherwise
                if (!(s.scale_seq > 0.) || !std::isfinite(s.scale_seq))
                    return fail(c, PLFX_ERR_ARG, "material %d: scale_seq must be finite and positive", k);
                for (int j = 0; j < 6; j++) m.col_inv[j] = 1. / s.scale_seq;
                c->svc_cols_mask |= 1u << k;
            } else {
                if (s.nsv * (nf + 1) <= c->lds_doubles) c->svc_lds_need = std::max(c->svc_lds_need, s.nsv * (nf + 1));
                if (s.kind == PLFX_SVC6) c->has_svc = true; else if (s.kind == PLFX_SVC3) c->has_svc3 = true; else c->has_svcwh = true, c->svcwh_mask |= 1u << k;
            }
            if (s.kind == PLFX_SVC6 || cols) {
                if (!cols) {
                    c->n_svc6++;
                    c->svc6_mask |= 1u << k;
                }
                if (c->want_svc_wave || cols) {
                    // the tables of the row kernels in device memory, in the layout of their LDS copy (stage_svc_row): read from
                    // there by the kernels when the material has more support vectors than the LDS of a CU holds
                    const int rp = (s.nsv + 63) & ~63;
                    std::vector<double> T((size_t)9 * rp + SVC_WAVE_EXTRA, 0.);
                    for (int i = 0; i < s.nsv; i++) {
                        double vv = 0.;
                        for (int f = 0; f < 6; f++) {
                            T[(size_t)f * rp + i] = s.sv[(size_t)i * 6 + f];
                            vv = std::fma(s.sv[(size_t)i * 6 + f], s.sv[(size_t)i * 6 + f], vv);
                        }
                        T[(size_t)6 * rp + i] = s.dual[i];
                        T[(size_t)7 * rp + i] = vv;
                    }
                    double *ext = T.data() + (size_t)9 * rp;
                    memcpy(ext, RAYPOLY_MT_HOST, sizeof(double) * RAYPOLY_N * RAYPOLY_N);
                    double a = 1., b = 1.;
                    for (int i = 0; i < 64; i++) {
                        ext[RAYPOLY_N * RAYPOLY_N + i] = a;
                        ext[RAYPOLY_N * RAYPOLY_N + 64 + i] = b;
                        a *= 0.98;
                        b *= 1.02;
                    }
                    double *dT = nullptr;
                    HIPCHK(c, hipMalloc((void **)&dT, T.size() * 8));
                    c->dsv.push_back(dT);
                    HIPCHK(c, hipMemcpy(dT, T.data(), T.size() * 8, hipMemcpyHostToDevice));
                    m.rowtab = dT;
                    m.rowpad = rp;
                    c->svc_row_all |= 1u << k;
                    // v[6], dual, |v|^2, one unused slot + the tables of the sampled-ray form, the vectors padded to 64 (up to
                    // 2176 vectors fit the 160 KB of a CU)
                    if (9 * rp + SVC_WAVE_EXTRA <= c->lds_doubles) {
                        c->svc_row_lds |= 1u << k;
                        c->svc_wave_lds = std::max(c->svc_wave_lds, (9 * rp + SVC_WAVE_EXTRA) * 8);
                    }
                    // kept from the removed wave kernels (tables padded to 256, first fitting material): shrinking it changes the launch
                    const int npad = (s.nsv + 255) & ~255;
                    if (9 * npad + SVC_WAVE_EXTRA <= c->lds_doubles && npad <= 2048 && !wave_pad && !cols) {
                        wave_pad = true;
                        c->svc_wave_lds = std::max(c->svc_wave_lds, (9 * npad + SVC_WAVE_EXTRA) * 8);
                    }
                }
            }
        }
    }
    c->nmat = nmat;
    c->plane_mats_ok = plane_materials_ok(c->hmat);
    if (!c->plane_mats_ok) plane_off(c, PLFX_PLANE_MATERIALS);
    int rc = dalloc(c, &c->dmat, (size_t)nmat);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->dmat, c->hmat.data(), sizeof(MatDev) * nmat, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, stream_sync(c));
    if (int rcl = raise_step_lds(c)) return rcl;   // the sweep, scf and response row kernels, which the step unit launches
    if (c->svc_wave_lds > 0) {
        HIPCHK(c, set_dyn_lds((const void *)k_full_yf_row<true>, c->svc_wave_lds));
        if (c->svc_cols_mask & c->svc_row_lds) {
            HIPCHK(c, set_dyn_lds((const void *)k_full_yf_row<true, true>, c->svc_wave_lds));
            // (a texture field can be attached to any of them)
            HIPCHK(c, set_dyn_lds((const void *)k_full_yf_row<true, true, true, TexFieldDev>, c->svc_wave_lds));
        }
    }
    if (c->has_svc || c->has_svc3 || c->has_svcwh) {  // opt in to > 64 KiB dynamic LDS for the SVC kernels
        const int bytes = (int)dyn_lds_bytes(c);
        HIPCHK(c, set_dyn_lds((const void *)k_response_batch<3>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_response_batch<6>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_point_eval, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_response_batch<7>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)static_cast<void (*)(const MatDev *, int, int, int, PathArgsWh)>(k_path_batch<7>), bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_path_wh_wave, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_response_svr, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_hessian_row<6>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_hessian_row<15>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_yield_scale<6>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_yield_scale<2>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_yield_scale<15>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_committee_yf, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_flow_curve<6>, bytes));
        HIPCHK(c, set_dyn_lds((const void *)k_flow_curve<15>, bytes));
    }
    c->M_dirty = true;
    c->memo.valid = false;
    return PLFX_OK;
}

// the six column scales of a PLFX_SVC6_COLS material: the record keeps their reciprocals (MatDev::col_inv)
int plfx_set_svc_cols(plfx_ctx *c, int mat, const double scale[6])
{
    if (!c) return PLFX_ERR_ARG;
    if (!c->dmat) return fail(c, PLFX_ERR_STATE, "set_materials first");
    if (mat < 0 || mat >= c->nmat || !scale) return fail(c, PLFX_ERR_ARG, "plfx_set_svc_cols: bad argument");
    if (c->hmat[mat].kind != PLFX_SVC6_COLS)
        return fail(c, PLFX_ERR_UNSUPPORTED, "plfx_set_svc_cols: material %d is of kind %d; column scales belong to a "
                    "PLFX_SVC6_COLS material only", mat, c->hmat[mat].kind);
    for (int j = 0; j < 6; j++)
        if (!std::isfinite(scale[j]) || !(scale[j] > 0.))
            return fail(c, PLFX_ERR_ARG, "plfx_set_svc_cols: scale %d must be finite and positive", j);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_sync(c));   // no launch may still read the record that changes
    for (int j = 0; j < 6; j++) c->hmat[mat].col_inv[j] = 1. / scale[j];
    HIPCHK(c, hipMemcpyAsync(c->dmat + mat, &c->hmat[mat], sizeof(MatDev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, stream_sync(c));
    c->memo.valid = false;
    return PLFX_OK;
}

// a PLFX_SVC6_COLS material runs on the row kernels alone: what every other point function answers for it
static int cols_refuse(plfx_ctx *c, int mat, const char *what)
{
    if (c && c->dmat && mat >= 0 && mat < c->nmat && c->hmat[mat].kind == PLFX_SVC6_COLS)
        return fail(c, PLFX_ERR_UNSUPPORTED, "%s: material %d is a PLFX_SVC6_COLS record, which runs on the row kernels only "
                    "(sweeps, calc_scf, response, ML_full_yf)", what, mat);
    return PLFX_OK;
}

// A texture field on a PLFX_SVC6_COLS material: one row of dual coefficients per texture, padded like the row tables
int plfx_set_svc_textures(plfx_ctx *c, int mat, int ntex, const double *coef)
{
    if (!c) return PLFX_ERR_ARG;
    if (!c->dmat) return fail(c, PLFX_ERR_STATE, "set_materials first");
    if (mat < 0 || mat >= c->nmat || ntex < 0 || (ntex > 0 && !coef)) return fail(c, PLFX_ERR_ARG, "plfx_set_svc_textures: bad argument");
    if (c->hmat[mat].kind != PLFX_SVC6_COLS)
        return fail(c, PLFX_ERR_UNSUPPORTED, "plfx_set_svc_textures: material %d is of kind %d; a texture field belongs to a "
                    "PLFX_SVC6_COLS material only", mat, c->hmat[mat].kind);
    const int nsv = c->hmat[mat].nsv, rp = c->hmat[mat].rowpad;
    if ((long long)ntex * rp > (long long)INT32_MAX)
        return fail(c, PLFX_ERR_ARG, "plfx_set_svc_textures: %d rows of %d coefficients are more than INT32_MAX", ntex, rp);
    for (size_t i = 0; i < (size_t)ntex * nsv; i++)
        if (!std::isfinite(coef[i]))
            return fail(c, PLFX_ERR_ARG, "plfx_set_svc_textures: coefficient %zu of row %zu is not finite", i % nsv, i / nsv);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_sync(c));   // no launch may still read the rows that go away
    free_tex_field(c, mat);
    if (ntex == 0) return PLFX_OK;
    std::vector<double> T((size_t)ntex * rp, 0.), S((size_t)ntex, 0.);
    for (int t = 0; t < ntex; t++)
        for (int i = 0; i < nsv; i++) {
            T[(size_t)t * rp + i] = coef[(size_t)t * nsv + i];
            S[t] += std::fabs(coef[(size_t)t * nsv + i]);
        }
    double *dT = nullptr, *dS = nullptr;
    HIPCHK(c, hipMalloc((void **)&dT, T.size() * 8));
    c->tex_field[mat].coef = dT;   // (owned from here on: freed by free_tex_field whatever follows)
    HIPCHK(c, hipMalloc((void **)&dS, S.size() * 8));
    c->tex_field[mat].sabs = dS;
    HIPCHK(c, hipMemcpy(dT, T.data(), T.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dS, S.data(), S.size() * 8, hipMemcpyHostToDevice));
    c->tex_field[mat].stride = rp;
    c->tex_field_rows[mat] = ntex;
    c->tex_field_mask |= 1u << mat;
    return PLFX_OK;
}

int plfx_set_element_textures(plfx_ctx *c, const int32_t *tex_id)
{
    if (!c || !c->sig) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_sync(c));
    c->tex_ids_ok = false;
    if (!tex_id) {
        dfree(c->tex_ids);
        c->htex_ids.clear();
        return PLFX_OK;
    }
    if (!c->tex_ids)
        if (int rc = dalloc(c, &c->tex_ids, (size_t)c->nel)) return rc;
    c->htex_ids.assign(tex_id, tex_id + c->nel);
    HIPCHK(c, hipMemcpy(c->tex_ids, tex_id, (size_t)c->nel * 4, hipMemcpyHostToDevice));
    return PLFX_OK;
}

int plfx_svc_textures_info(plfx_ctx *c, int mat, int *rows, int *staged, int64_t *launches)
{
    if (!c || mat < 0 || mat >= MAXMAT) return c ? fail(c, PLFX_ERR_ARG, "material %d out of range", mat) : PLFX_ERR_ARG;
    if (rows) *rows = c->tex_field_rows[mat];
    if (staged) *staged = 0;   // the rows are read from device memory
    if (launches) *launches = c->tex_field_launches[mat];
    return PLFX_OK;
}

// the rows of the points of a _tid call: checked on the host for the materials that carry a field
static int tex_point_check(plfx_ctx *c, int n, int mat, const int32_t *mat_id, const int32_t *tex_id)
{
    if (!tex_id || !c->tex_field_mask) return PLFX_OK;
    for (int i = 0; i < n; i++) {
        const int k = mat >= 0 ? mat : (mat_id ? mat_id[i] : 0);
        if (k < 0 || k >= c->nmat || !((c->tex_field_mask >> k) & 1u)) continue;
        if (tex_id[i] < 0 || tex_id[i] >= c->tex_field_rows[k])
            return fail(c, PLFX_ERR_ARG, "tex_id[%d] = %d is outside the %d rows of material %d", i, (int)tex_id[i],
                        c->tex_field_rows[k], k);
    }
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ batched point evaluation
// the opening check of a point function of one material; args_ok: what the function asks of its other arguments
static int point_check(plfx_ctx *c, int mat, bool args_ok)
{
    if (!c || !c->dmat) return c ? fail(c, PLFX_ERR_STATE, "set_materials first") : PLFX_ERR_STATE;
    if (mat < 0 || mat >= c->nmat || !args_ok) return fail(c, PLFX_ERR_ARG, "bad argument");
    return PLFX_OK;
}

// f(std::integral_constant<int, NFP>) for the padded width nfp of a texture set (plfx_tex.hpp): the one place that lists the
// instantiations of its kernels
extern "C++" {
template <class F>
static void tex_for_nfp(int nfp, F &&f)
{
    if (nfp == 8)
        f(std::integral_constant<int, 8>());
    else if (nfp == 12)
        f(std::integral_constant<int, 12>());
    else
        f(std::integral_constant<int, 16>());
}
}

static int point_eval(plfx_ctx *c, int what, int mat, int n, const double *sig, const double *epl,
                      const double *ld, double *out, int32_t *status, const int32_t *tex_id = nullptr)
{
    if (int rc = point_check(c, mat, n >= 0 && sig && out)) return rc;
    if (int rc = tex_point_check(c, n, mat, nullptr, tex_id)) return rc;
    const bool cols = (c->hmat[mat].kind == PLFX_SVC6_COLS);
    if (cols && what != 3) return cols_refuse(c, mat, what == 0 ? "calc_seq" : what == 1 ? "calc_fgrad" : "calc_yf");
    if (n == 0) return PLFX_OK;
    const size_t N = n, wout = (what == 1) ? 6 : 1;
    CallBuffers B;
    double *dsig = nullptr, *depl = nullptr, *dout = nullptr, *dld = nullptr;
    int32_t *dst = nullptr;
    if (int rc = B.put(c, &dsig, sig, 6 * N)) return rc;
    if (int rc = B.get(c, &dout, N * wout)) return rc;
    if (epl)
        if (int rc = B.put(c, &depl, epl, 6 * N)) return rc;
    if (ld)
        if (int rc = B.put(c, &dld, ld, 6)) return rc;
    if (status)
        if (int rc = B.get(c, &dst, N)) return rc;
    int32_t *d_tid = nullptr;
    if (tex_id && ((c->tex_field_mask >> mat) & 1u))
        if (int rc = B.put(c, &d_tid, tex_id, N)) return rc;
    static const bool wave_full = !(getenv("PLFX_FULL_YF_WAVE") && atoi(getenv("PLFX_FULL_YF_WAVE")) == 0);
    EvPair *ev;
    tim_begin(c, 0, &ev);   // family 0 like plfx_response_batch: the kernel alone, without the copies
    if (what == 3 && (wave_full || cols) && ((c->svc_row_all >> mat) & 1u))  // ML_full_yf of a row-kernel SVC material
        LAUNCH_ROW1(c, mat, (const int32_t *)d_tid, k_full_yf_row, dim3(std::max(1, std::min((n + 31) / 32, 2048))),
                   c->dmat, c->nmat, mat, n, dsig, depl, dld, dout, dst);
    else
        hipLaunchKernelGGL(k_point_eval, dim3(grid_for(n)), dim3(BLOCK), dyn_lds_bytes(c), c->stream,
                           c->dmat, c->nmat, c->svc_lds_need, what, mat, n, dsig, depl, dld, dout, dst);
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, dout, N * wout * 8, hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(c, hipMemcpyAsync(status, dst, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_seq_batch(plfx_ctx *c, int mat, int n, const double *sig, double *seq)
{
    return point_eval(c, 0, mat, n, sig, nullptr, nullptr, seq, nullptr);
}
int plfx_fgrad_batch(plfx_ctx *c, int mat, int n, const double *sig, double *a)
{
    if (c && mat >= 0 && mat < c->nmat &&
        (c->hmat[mat].kind == PLFX_TRESCA || (c->hmat[mat].kind == PLFX_BARLAT && !c->hmat[mat].barlat_normal)))
        return fail(c, PLFX_ERR_UNSUPPORTED, "calc_fgrad: no analytical gradient for this Tresca / Barlat material (material.py:822-825)");
    return point_eval(c, 1, mat, n, sig, nullptr, nullptr, a, nullptr);
}
int plfx_fgrad_seq_batch(plfx_ctx *c, int mat, int n, const double *sig, const double *seq, double *a)
{
    if (int rc = point_check(c, mat, n >= 0 && sig && seq && a)) return rc;
    const int kind = c->hmat[mat].kind;
    if (kind != PLFX_HILL6 && kind != PLFX_PRINC3)
        return fail(c, PLFX_ERR_UNSUPPORTED, "calc_fgrad(seq=...): analytic Hill materials only (material.py:822-847)");
    if (n == 0) return PLFX_OK;
    const size_t N = n;
    CallBuffers B;
    double *dsig = nullptr, *dseq = nullptr, *dout = nullptr;
    if (int rc = B.put(c, &dsig, sig, 6 * N)) return rc;
    if (int rc = B.put(c, &dseq, seq, N)) return rc;
    if (int rc = B.get(c, &dout, 6 * N)) return rc;
    hipLaunchKernelGGL(k_fgrad_seq, dim3(grid_for(n)), dim3(BLOCK), 0, c->stream, c->dmat, mat, n, dsig, dseq, dout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(a, dout, N * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}
int plfx_yf_batch(plfx_ctx *c, int mat, int n, const double *sig, const double *epl, double *yf)
{
    return point_eval(c, 2, mat, n, sig, epl, nullptr, yf, nullptr);
}
int plfx_full_yf_batch(plfx_ctx *c, int mat, int n, const double *sig, const double *epl,
                       const double *ld, double *yf, int32_t *status)
{
    return point_eval(c, 3, mat, n, sig, epl, ld, yf, status);
}
int plfx_full_yf_batch_tid(plfx_ctx *c, int mat, int n, const double *sig, const double *epl,
                           const double *ld, double *yf, int32_t *status, const int32_t *tex_id)
{
    return point_eval(c, 3, mat, n, sig, epl, ld, yf, status, tex_id);
}

static int response_batch_impl(plfx_ctx *c, int n, const int32_t *mat_id, const double *sig,
                               const double *epl, const double *deps, double *fy, double *sig_out,
                               double *depl, double *ct, int32_t *nsteps, const double *kh_in, double *kh_out,
                               const int32_t *tex_id = nullptr)
{
    if (!c || !c->dmat) return c ? fail(c, PLFX_ERR_STATE, "set_materials first") : PLFX_ERR_STATE;
    if (n < 0 || !sig || !epl || !deps || !fy || !sig_out || !depl || !ct || !nsteps)
        return fail(c, PLFX_ERR_ARG, "null argument");
    if (c->n_noflow) return fail(c, PLFX_ERR_UNSUPPORTED, "a Tresca / Barlat material without flow rule is loaded (material.py:822-825)");
    if (n == 0) return PLFX_OK;
    if (mat_id)
        for (int i = 0; i < n; i++)
            if (mat_id[i] < 0 || mat_id[i] >= c->nmat) return fail(c, PLFX_ERR_ARG, "mat_id[%d] out of range", i);
    if (int rc = tex_point_check(c, n, -1, mat_id, tex_id)) return rc;
    CallBuffers B;
    double *d_in = nullptr, *d_out = nullptr;
    int32_t *d_mid = nullptr, *d_ns = nullptr, *d_tid = nullptr;
    const size_t N = n;
    if (tex_id && c->tex_field_mask)
        if (int rc = B.put(c, &d_tid, tex_id, N)) return rc;
    if (int rc = B.get(c, &d_in, N * 18)) return rc;
    if (int rc = B.get(c, &d_out, N * (1 + 6 + 6 + 36))) return rc;
    if (int rc = B.get(c, &d_ns, N)) return rc;
    HIPCHK(c, hipMemcpyAsync(d_in, sig, N * 48, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in + 6 * N, epl, N * 48, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in + 12 * N, deps, N * 48, hipMemcpyHostToDevice, c->stream));
    if (mat_id)
        if (int rc = B.put(c, &d_mid, mat_id, N)) return rc;
    double *d_fy = d_out, *d_so = d_out + N, *d_dp = d_out + 7 * N, *d_ct = d_out + 13 * N;
    double *d_kh = nullptr;   // [2N]: entry / exit hardening modulus of the work-hardening SVC points
    if (c->has_svcwh) {
        if (int rc = B.get(c, &d_kh, 2 * N)) return rc;
        std::vector<double> k0(N);
        for (size_t i = 0; i < N; i++) k0[i] = kh_in ? kh_in[i] : c->hmat[mat_id ? mat_id[i] : 0].khard;
        HIPCHK(c, hipMemcpyAsync(d_kh, k0.data(), N * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_kh + N, d_kh, N * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, stream_sync(c));
    }
    EvPair *ev;
    tim_begin(c, 0, &ev);
#define RB_ARGS(lds) c->dmat, c->nmat, lds, n, d_mid, d_in, d_in + 6 * N, d_in + 12 * N, d_fy, d_so, d_dp, d_ct, d_ns
#define RB_TAIL (const double *)nullptr, (double *)nullptr, 0u, c->resp_maxit
    if (c->has_analytic || c->has_elastic)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_response_batch<1>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, RB_ARGS(0), RB_TAIL);
    if (c->has_princ)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_response_batch<2>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, RB_ARGS(0), RB_TAIL);
    if (c->has_barlat)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_response_batch<5>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, RB_ARGS(0), RB_TAIL);
    const bool resp_row = !(getenv("PLFX_RESPONSE_ROW") && atoi(getenv("PLFX_RESPONSE_ROW")) == 0);   // read per call: tests compare the two forms
    const unsigned rmask = resp_row ? c->svc_row_all : c->svc_cols_mask;   // (PLFX_SVC6_COLS has no other form)
    if (c->has_svc && (c->svc6_mask & ~rmask))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_response_batch<3>), dim3(grid_for(N)), dim3(BLOCK), dyn_lds_bytes(c),
                           c->stream, RB_ARGS(c->svc_lds_need), (const double *)nullptr, (double *)nullptr, rmask, c->resp_maxit);
    for (int k = 0; k < c->nmat; k++)   // 6-feature SVC materials with tables in LDS: 16 lanes per point (the code path of the sweeps)
        if ((rmask >> k) & 1u)
            launch_response_row(c, k, (const int32_t *)d_tid, n, d_mid, d_in, d_in + 6 * N, d_in + 12 * N, d_fy, d_so, d_dp, d_ct, d_ns);
    if (c->has_svc3)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_response_batch<6>), dim3(grid_for(N)), dim3(BLOCK), dyn_lds_bytes(c),
                           c->stream, RB_ARGS(c->svc_lds_need), RB_TAIL);
    if (c->has_svcwh && (c->svcwh_mask & ~c->svr_mask))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_response_batch<7>), dim3(grid_for(N)), dim3(BLOCK), dyn_lds_bytes(c),
                           c->stream, RB_ARGS(c->svc_lds_need), (const double *)d_kh, d_kh + N, c->svr_mask, c->resp_maxit);
    for (int k = 0; k < c->nmat; k++)   // work-hardening SVC materials with an SVR flow rule attached: one launch per material
        if ((c->svr_mask >> k) & 1u) {
            hipLaunchKernelGGL(k_response_svr, dim3(grid_for(N)), dim3(SVR_FLOW_BLOCK), dyn_lds_bytes(c), c->stream, c->dmat, c->nmat,
                               c->svc_lds_need, k, c->svr_flow[k], c->svr_flow[k].X, c->svr_flow[k].coef, n, d_mid, d_in, d_in + 6 * N, d_in + 12 * N, d_fy, d_so,
                               d_dp, d_ct, d_ns, (const double *)d_kh, d_kh + N, c->resp_maxit);
            c->svr_launches[k]++;
        }
#undef RB_ARGS
#undef RB_TAIL
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(fy, d_fy, N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sig_out, d_so, N * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(depl, d_dp, N * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ct, d_ct, N * 288, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nsteps, d_ns, N * 4, hipMemcpyDeviceToHost, c->stream));
    if (kh_out) {
        if (d_kh)
            HIPCHK(c, hipMemcpyAsync(kh_out, d_kh + N, N * 8, hipMemcpyDeviceToHost, c->stream));
        else
            for (size_t i = 0; i < N; i++) kh_out[i] = kh_in ? kh_in[i] : c->hmat[mat_id ? mat_id[i] : 0].khard;
    }
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_response_batch(plfx_ctx *c, int n, const int32_t *mat_id, const double *sig,
                        const double *epl, const double *deps, double *fy, double *sig_out,
                        double *depl, double *ct, int32_t *nsteps)
{
    return response_batch_impl(c, n, mat_id, sig, epl, deps, fy, sig_out, depl, ct, nsteps, nullptr, nullptr);
}

int plfx_response_batch_tid(plfx_ctx *c, int n, const int32_t *mat_id, const double *sig,
                            const double *epl, const double *deps, double *fy, double *sig_out,
                            double *depl, double *ct, int32_t *nsteps, const int32_t *tex_id)
{
    return response_batch_impl(c, n, mat_id, sig, epl, deps, fy, sig_out, depl, ct, nsteps, nullptr, nullptr, tex_id);
}

int plfx_response_batch_kh(plfx_ctx *c, int n, const int32_t *mat_id, const double *sig, const double *epl,
                           const double *deps, const double *khard_in, double *fy, double *sig_out, double *depl,
                           double *ct, int32_t *nsteps, double *khard_out)
{
    return response_batch_impl(c, n, mat_id, sig, epl, deps, fy, sig_out, depl, ct, nsteps, khard_in, khard_out);
}

int plfx_fgrad_batch_wh(plfx_ctx *c, int mat, int n, const double *sig, const double *epl, double *fgrad, double *khard_raw)
{
    if (int rc = point_check(c, mat, n >= 0 && sig && fgrad)) return rc;
    if (c->hmat[mat].kind != PLFX_SVC_WH) return fail(c, PLFX_ERR_ARG, "material %d has no work-hardening features", mat);
    if (n == 0) return PLFX_OK;
    const size_t N = n;
    CallBuffers B;
    double *dsig = nullptr, *depl = nullptr, *dout = nullptr, *dkh = nullptr;
    if (int rc = B.put(c, &dsig, sig, 6 * N)) return rc;
    if (int rc = B.get(c, &dout, 6 * N)) return rc;
    if (int rc = B.get(c, &dkh, N)) return rc;
    if (epl)
        if (int rc = B.put(c, &depl, epl, 6 * N)) return rc;
    EvPair *ev;
    tim_begin(c, 0, &ev);
    hipLaunchKernelGGL(k_point_eval, dim3(grid_for(n)), dim3(BLOCK), dyn_lds_bytes(c), c->stream, c->dmat, c->nmat,
                       c->svc_lds_need, 1, mat, n, dsig, depl, (const double *)nullptr, dout, (int32_t *)nullptr, dkh);
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(fgrad, dout, N * 48, hipMemcpyDeviceToHost, c->stream));
    if (khard_raw) HIPCHK(c, hipMemcpyAsync(khard_raw, dkh, N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

// Material.calc_hessian of an SVC material: sibling of point_eval with 36 numbers per point and the row kernel
int plfx_hessian_batch(plfx_ctx *c, int mat, int n, const double *sig, const double *epl, double *hess)
{
    if (int rc = point_check(c, mat, n >= 0 && sig && hess)) return rc;
    if (int rc = cols_refuse(c, mat, "calc_hessian")) return rc;
    const int kind = c->hmat[mat].kind;
    if (kind != PLFX_SVC6 && kind != PLFX_SVC_WH)
        return fail(c, PLFX_ERR_UNSUPPORTED, kind == PLFX_SVC3 ? "calc_hessian: not implemented for 3D stress (material.py:950)"
                    : "calc_hessian: no analytical hessian for this Hill / Tresca / Barlat material (material.py:965-970)");
    if (n == 0) return PLFX_OK;
    const size_t N = n;
    CallBuffers B;
    double *dsig = nullptr, *depl = nullptr, *dout = nullptr;
    if (int rc = B.put(c, &dsig, sig, 6 * N)) return rc;
    if (int rc = B.get(c, &dout, 36 * N)) return rc;
    if (epl && kind == PLFX_SVC_WH)
        if (int rc = B.put(c, &depl, epl, 6 * N)) return rc;
    const dim3 grid = row16_grid(c, n, HESS_BLOCK, 4);   // 64 points per block
    EvPair *ev;
    tim_begin(c, 0, &ev);
    if (kind == PLFX_SVC6)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_hessian_row<6>), grid, dim3(HESS_BLOCK), dyn_lds_bytes(c), c->stream,
                           c->dmat, c->nmat, c->svc_lds_need, mat, n, dsig, depl, dout);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_hessian_row<15>), grid, dim3(HESS_BLOCK), dyn_lds_bytes(c), c->stream,
                           c->dmat, c->nmat, c->svc_lds_need, mat, n, dsig, depl, dout);
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hess, dout, N * 288, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

// Material.yield_scale: the factor x with calc_yf(x su) = 0 along n unit stresses.  SVC kinds: the search of k_yield_scale,
// one launch; analytic kinds: the closed form sflow / seq(su).
int plfx_yield_scale(plfx_ctx *c, int mat, int n, const double *su, const double *epl, const double *x0, double *x,
                     int32_t *status)
{
    if (int rc = point_check(c, mat, n >= 0 && su && x && status)) return rc;
    if (int rc = cols_refuse(c, mat, "yield_scale")) return rc;
    const int kind = c->hmat[mat].kind;
    if (kind == PLFX_ELASTIC) return fail(c, PLFX_ERR_ARG, "yield_scale: material %d has no yield strength", mat);
    if (n == 0) return PLFX_OK;
    const size_t N = n;
    CallBuffers B;
    double *dsu = nullptr, *depl = nullptr, *dx0 = nullptr, *dx = nullptr;
    int32_t *dst = nullptr;
    if (int rc = B.get(c, &dsu, 6 * N)) return rc;
    if (int rc = B.get(c, &dx, N)) return rc;
    if (int rc = B.get(c, &dst, N)) return rc;
    // principal-stress kinds (2-feature SVC, Hill-3 / J2 on principal stresses): rays with out-of-plane shear are reduced to
    // their principal stresses here, by the LAPACK replay that the device runs for such states (plfx_sig_princ_host); the order
    // of the principal stresses does not change along a ray.  The kernels then need the closed form of plane states only.
    // (Material.yield_scale has done the same through _princ_rows, material.py, and nothing is left to reduce for its rays;
    // this pass serves callers of the C-ABI.)
    std::vector<double> red;
    if (kind == PLFX_SVC3 || kind == PLFX_PRINC3)
        for (int i = 0; i < n; i++) {
            const double *s = su + 6 * (size_t)i;
            bool fin = true;
            for (int k = 0; k < 6; k++) fin = fin && std::isfinite(s[k]);
            if (!fin || (s[3] == 0. && s[4] == 0.)) continue;
            if (red.empty()) red.assign(su, su + 6 * (size_t)n);
            double *r = red.data() + 6 * (size_t)i;
            lapack3::sig_princ_lapack3(s, r);
            r[3] = r[4] = r[5] = 0.;
        }
    HIPCHK(c, hipMemcpyAsync(dsu, red.empty() ? su : red.data(), N * 48, hipMemcpyHostToDevice, c->stream));
    if (epl)
        if (int rc = B.put(c, &depl, epl, 6 * N)) return rc;
    if (x0)
        if (int rc = B.put(c, &dx0, x0, N)) return rc;
    const int block = row16_block(c, n, YS_BLOCK);
    const dim3 grid = row16_grid(c, n, block, 4);
    EvPair *ev;
    tim_begin(c, 0, &ev);
#define YS_LAUNCH(NF)                                                                                                      \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_yield_scale<NF>), grid, dim3(block), dyn_lds_bytes(c), c->stream, c->dmat, c->nmat, \
                       c->svc_lds_need, mat, n, dsu, depl, dx0, dx, dst)
    if (kind == PLFX_SVC6)
        YS_LAUNCH(6);
    else if (kind == PLFX_SVC3)
        YS_LAUNCH(2);
    else if (kind == PLFX_SVC_WH)
        YS_LAUNCH(15);
#undef YS_LAUNCH
#define YS_LAUNCH(KD)                                                                                                       \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_yield_scale_analytic<KD>), dim3(grid_for(n)), dim3(BLOCK), 0, c->stream, c->dmat, mat, n, \
                       dsu, depl, dx0, dx, dst)
    else if (kind == PLFX_PRINC3)
        YS_LAUNCH(2);
    else if (kind == PLFX_TRESCA)
        YS_LAUNCH(4);
    else if (kind == PLFX_BARLAT)
        YS_LAUNCH(5);
    else
        YS_LAUNCH(1);
#undef YS_LAUNCH
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(x, dx, N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, dst, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

// Material.flow_curve: n flow curves of up to max_steps steps along the unit stresses su, the whole chains
// in ONE launch.  SVC kinds: k_flow_curve, 16 lanes per curve; Hill / J2 / Drucker on Voigt stresses: k_flow_curve_analytic.
int plfx_flow_curve(plfx_ctx *c, int mat, int n, const double *su, const double *epl0, int max_steps, double depl,
                    double epl_max, double predictor, double *x, double *epl, double *yf, double *hk, int32_t *nsteps,
                    int32_t *status)
{
    if (int rc = point_check(c, mat, n >= 0 && su && x && epl && yf && nsteps && status)) return rc;
    if (int rc = cols_refuse(c, mat, "flow_curve")) return rc;
    if (max_steps < 0 || !(depl > 0.) || !std::isfinite(depl) || !std::isfinite(predictor) || epl_max != epl_max)
        return fail(c, PLFX_ERR_ARG, "flow_curve: max_steps >= 0, a finite depl > 0, a finite predictor and an epl_max that is a number expected");
    const int kind = c->hmat[mat].kind;
    if (kind == PLFX_ELASTIC) return fail(c, PLFX_ERR_ARG, "flow_curve: material %d has no yield strength", mat);
    if (kind != PLFX_HILL6 && kind != PLFX_SVC6 && kind != PLFX_SVC_WH)
        return fail(c, PLFX_ERR_ARG, "flow_curve: offered for Hill / J2 / Drucker on Voigt stresses and for the 6- and 15-feature SVC; material %d is of kind %d", mat, kind);
    if (n == 0) return PLFX_OK;
    const size_t N = n, K1 = (size_t)max_steps + 1, K = (size_t)max_steps;
    CallBuffers B;
    double *dsu = nullptr, *de0 = nullptr, *dx = nullptr, *de = nullptr, *dyf = nullptr, *dhk = nullptr;
    int32_t *dns = nullptr, *dst = nullptr;
    if (int rc = B.put(c, &dsu, su, 6 * N)) return rc;
    if (epl0)
        if (int rc = B.put(c, &de0, epl0, 6 * N)) return rc;
    if (int rc = B.get(c, &dx, N * K1)) return rc;
    if (int rc = B.get(c, &de, 6 * N * K1)) return rc;
    if (int rc = B.get(c, &dyf, N * K1)) return rc;
    if (hk && K > 0)
        if (int rc = B.get(c, &dhk, N * K)) return rc;
    if (int rc = B.get(c, &dns, N)) return rc;
    if (int rc = B.get(c, &dst, N)) return rc;
    EvPair *ev;
    tim_begin(c, 0, &ev);
    if (kind == PLFX_HILL6) {
        hipLaunchKernelGGL(k_flow_curve_analytic, dim3(grid_for(n)), dim3(BLOCK), 0, c->stream, c->dmat, mat, n, dsu, de0,
                           max_steps, depl, epl_max, predictor, dx, de, dyf, dhk, dns, dst);
    } else {
        const int block = row16_block(c, n, YS_BLOCK);
        const dim3 grid = row16_grid(c, n, block, 4);
#define FC_LAUNCH(NF)                                                                                                     \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_flow_curve<NF>), grid, dim3(block), dyn_lds_bytes(c), c->stream, c->dmat, c->nmat, \
                       c->svc_lds_need, mat, n, dsu, de0, max_steps, depl, epl_max, predictor, dx, de, dyf, dhk, dns, dst)
        if (kind == PLFX_SVC6)
            FC_LAUNCH(6);
        else
            FC_LAUNCH(15);
#undef FC_LAUNCH
    }
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    c->flow_launches++;
    HIPCHK(c, hipMemcpyAsync(x, dx, N * K1 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(epl, de, N * K1 * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(yf, dyf, N * K1 * 8, hipMemcpyDeviceToHost, c->stream));
    if (dhk) HIPCHK(c, hipMemcpyAsync(hk, dhk, N * K * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nsteps, dns, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, dst, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_flow_info(plfx_ctx *c, int64_t *launches)
{
    if (!c) return PLFX_ERR_ARG;
    if (launches) *launches = c->flow_launches;
    return PLFX_OK;
}

// Material.load_path: n material points of material `mat` along load paths of K increments, every path in
// ONE launch: k_path_batch for the kinds of k_response_batch<1 | 2 | 5>, k_path_row (launch_path_row, plfx_step.hip) for the
// 6-feature SVC materials of the row kernels.  One copy in, one copy out.  Everything is checked before anything is launched.
// form 0 of plfx_load_path_wh takes the wave form up to this many paths.  Measured: the wave form is the
// faster one at every N from 1 to 100 000, 39 times at N = 1, 25 times at N = 10 000 and 4.6 times at N = 100 000, and both forms grow linearly beyond
// the 65 536 paths the thread form holds in one round: there is no crossover within the sizes a call accepts.
constexpr int PATH_WH_WAVE_MAX_N = INT32_MAX;

// wh: the entry is plfx_load_path_wh (material of kind PLFX_SVC_WH; khard0, form and khard are its own arguments)
static int load_path_impl(plfx_ctx *c, bool wh, int mat, int n, int K, const double *dload, int shared, const int32_t *control,
                          const double *sig0, const double *epl0, const int32_t *tex_id, const double *khard0, int form, int maxit,
                          int newton, double stol, double eps_cap, double *sig, double *epl, double *deps, double *fy, double *khard,
                          int32_t *nsteps, int32_t *newton_out, int32_t *ksteps, int32_t *status, double *ct)
{
    if (!c || !c->dmat) return c ? fail(c, PLFX_ERR_STATE, "set_materials first") : PLFX_ERR_STATE;
    if (mat < 0 || mat >= c->nmat) return fail(c, PLFX_ERR_ARG, "load_path: material %d, the context holds %d", mat, c->nmat);
    const MatDev &hm = c->hmat[mat];
    const bool row = !wh && (hm.kind == PLFX_SVC6 || hm.kind == PLFX_SVC6_COLS) && ((c->svc_row_all >> mat) & 1u);
    int kind = 0;   // instantiation of k_path_batch
    if (wh) {
        if (hm.kind != PLFX_SVC_WH)
            return fail(c, PLFX_ERR_UNSUPPORTED, "load_path_wh: offered for the SVC with work-hardening features; material %d is of "
                        "kind %d (plfx_load_path follows the other kinds)", mat, hm.kind);
        if ((c->svr_mask >> mat) & 1u)
            return fail(c, PLFX_ERR_UNSUPPORTED, "load_path_wh: material %d has an SVR flow rule attached, which no path kernel follows", mat);
        kind = 7;
    } else if (hm.kind == PLFX_ELASTIC || hm.kind == PLFX_HILL6)
        kind = 1;
    else if (hm.kind == PLFX_PRINC3)
        kind = 2;
    else if (hm.kind == PLFX_BARLAT && hm.barlat_normal)
        kind = 5;
    else if (!row)
        return fail(c, PLFX_ERR_UNSUPPORTED, "load_path: offered for elastic, Hill / J2 / Drucker materials, Barlat with the native "
                    "normal and the 6-feature SVC of the row kernels; material %d is of kind %d", mat, hm.kind);
    if (n < 0 || K < 0) return fail(c, PLFX_ERR_ARG, "load_path: n >= 0 and K >= 0 expected");
    if (maxit < 1 || newton < 0 || !(stol > 0.) || !std::isfinite(stol) || !(eps_cap > 0.) || !std::isfinite(eps_cap))
        return fail(c, PLFX_ERR_ARG, "load_path: maxit >= 1, newton >= 0 and finite stol > 0, eps_cap > 0 expected");
    if (wh && (form < 0 || form > 2)) return fail(c, PLFX_ERR_ARG, "load_path_wh: form = %d; 0 (by n), 1 (thread per path) or 2 (wave per path) expected", form);
    if (n == 0) return PLFX_OK;
    if (!ksteps || !status || (K > 0 && (!dload || !sig || !epl || !deps || !fy || !nsteps || !newton_out)))
        return fail(c, PLFX_ERR_ARG, "load_path: null argument");
    if (wh && (!khard0 || (K > 0 && !khard))) return fail(c, PLFX_ERR_ARG, "load_path_wh: null argument");
    const size_t N = n, KK = K, nd = shared ? 1 : N;
    const size_t W = wh ? 20 : 19;   // doubles of one record of the step-major results: sig, epl, deps, fy (, khard)
    if (KK * N * W > (size_t)INT32_MAX) return fail(c, PLFX_ERR_ARG, "load_path: K n %zu = %zu exceeds INT32_MAX", W, KK * N * W);
    unsigned any_strain = control ? 0u : 63u;   // components that are strain-controlled at some point (a shared dload)
    if (control)
        for (size_t i = 0; i < N; i++) {
            if (control[i] < 0 || control[i] >= 64) return fail(c, PLFX_ERR_ARG, "load_path: control[%zu] = %d, six bits expected", i, (int)control[i]);
            any_strain |= ~(unsigned)control[i] & 63u;
        }
    for (size_t j = 0; j < KK * nd * 6; j++) {
        if (!std::isfinite(dload[j])) return fail(c, PLFX_ERR_ARG, "load_path: dload is not finite at entry %zu", j);
        const unsigned strain = shared ? any_strain : (control ? ~(unsigned)control[(j / 6) % N] & 63u : 63u);
        if (((strain >> (j % 6)) & 1u) && std::fabs(dload[j]) > eps_cap)
            return fail(c, PLFX_ERR_ARG, "load_path: the strain increment %g at entry %zu of dload is beyond eps_cap = %g", dload[j], j, eps_cap);
    }
    for (const double *p : {sig0, epl0})
        if (p)
            for (size_t j = 0; j < 6 * N; j++)
                if (!std::isfinite(p[j])) return fail(c, PLFX_ERR_ARG, "load_path: %s is not finite at entry %zu", p == sig0 ? "sig0" : "epl0", j);
    if (wh)
        for (size_t i = 0; i < N; i++)
            if (!std::isfinite(khard0[i]) || khard0[i] < 0.)
                return fail(c, PLFX_ERR_ARG, "load_path_wh: khard0[%zu] = %g, a finite modulus >= 0 expected", i, khard0[i]);
    if (int rc = tex_point_check(c, n, mat, nullptr, tex_id)) return rc;
    if (K == 0) {   // nothing to follow: no step completed, the tangent is the elastic one
        for (size_t i = 0; i < N; i++) {
            ksteps[i] = status[i] = 0;
            if (ct)
                for (int r = 0; r < 6; r++)
                    for (int q = 0; q < 6; q++) ct[36 * i + r * 6 + q] = hm.CV[sym_idx(r, q)];
        }
        return PLFX_OK;
    }
    const bool field = tex_id && ((c->tex_field_mask >> mat) & 1u);
    // one buffer in: dload | sig0 | epl0 | khard0 | control, tex_id (int32)
    const size_t o_s0 = KK * nd * 6, o_e0 = o_s0 + (sig0 ? 6 * N : 0), o_k0 = o_e0 + (epl0 ? 6 * N : 0), o_int = o_k0 + (wh ? N : 0);
    const size_t n_int = (control ? N : 0) + (field ? N : 0), in_words = o_int + (n_int + 1) / 2;
    const std::unique_ptr<double[]> hin(new double[std::max<size_t>(in_words, 1)]);   // (not zeroed: every word sent is written)
    memcpy(hin.get(), dload, o_s0 * 8);
    if (sig0) memcpy(hin.get() + o_s0, sig0, N * 48);
    if (epl0) memcpy(hin.get() + o_e0, epl0, N * 48);
    if (wh) memcpy(hin.get() + o_k0, khard0, N * 8);
    int32_t *hint = (int32_t *)(hin.get() + o_int);
    if (n_int & 1) hint[n_int] = 0;
    if (control) memcpy(hint, control, N * 4);
    if (field) memcpy(hint + (control ? N : 0), tex_id, N * 4);
    // one buffer out: sig | epl | deps | fy | khard | ct | nsteps, newton, ksteps, status (int32)
    const size_t KN = KK * N, o_ct = W * KN, o_oi = o_ct + (ct ? 36 * N : 0), out_words = o_oi + KN + N;
    CallBuffers B;
    double *d_in = nullptr, *d_out = nullptr;
    if (int rc = B.put(c, &d_in, (const double *)hin.get(), in_words)) return rc;
    if (int rc = B.get(c, &d_out, out_words)) return rc;
    const int32_t *d_int = (const int32_t *)(d_in + o_int);
    int32_t *d_oi = (int32_t *)(d_out + o_oi);
    PathArgsWh a;
    a.khard0 = wh ? d_in + o_k0 : nullptr;
    a.khard = wh ? d_out + 19 * KN : nullptr;
    a.n = n;
    a.K = K;
    a.dload = d_in;
    a.dl_stride = shared ? 0 : 6;
    a.control = control ? d_int : nullptr;
    a.sig0 = sig0 ? d_in + o_s0 : nullptr;
    a.epl0 = epl0 ? d_in + o_e0 : nullptr;
    a.maxit = maxit;
    a.newton = newton;
    a.stol = stol;
    a.eps_cap = eps_cap;
    a.sig = d_out;
    a.epl = d_out + 6 * KN;
    a.deps = d_out + 12 * KN;
    a.fy = d_out + 18 * KN;
    a.ct = ct ? d_out + o_ct : nullptr;
    a.nsteps = d_oi;
    a.newton_out = d_oi + KN;
    a.ksteps = d_oi + 2 * KN;
    a.status = d_oi + 2 * KN + N;
    const int wave = wh ? (form == 2 || (form == 0 && n <= PATH_WH_WAVE_MAX_N)) : 0;
    EvPair *ev;
    tim_begin(c, 0, &ev);
    if (wh && wave) {
        const int wpb = BLOCK / 64;
        hipLaunchKernelGGL(k_path_wh_wave, dim3((unsigned)((N + wpb - 1) / wpb)), dim3(BLOCK), dyn_lds_bytes(c), c->stream, c->dmat,
                           c->nmat, c->svc_lds_need, mat, a);
    } else if (wh)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_batch<7>), dim3(grid_for(N)), dim3(BLOCK), dyn_lds_bytes(c), c->stream, c->dmat,
                           c->nmat, c->svc_lds_need, mat, a);
    else if (row)
        launch_path_row(c, mat, field ? d_int + (control ? N : 0) : nullptr, a);
    else if (kind == 1)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_batch<1>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, mat, a);
    else if (kind == 2)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_batch<2>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, mat, a);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_batch<5>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, mat, a);
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    if (wh)
        c->path_wh_launches[wave]++;
    else
        c->path_launches++;
    // one copy out: straight into the caller's arrays where they lie in one block in the order of the device buffer (the Python
    // binding's do), else through a staging block
    const bool packed = epl == sig + 6 * KN && deps == sig + 12 * KN && fy == sig + 18 * KN && (!wh || khard == sig + 19 * KN) &&
                        (!ct || ct == sig + o_ct) &&
                        (const void *)nsteps == (const void *)(sig + o_oi) && newton_out == nsteps + KN &&
                        ksteps == nsteps + 2 * KN && status == ksteps + N;
    std::unique_ptr<double[]> hout(packed ? nullptr : new double[out_words]);
    HIPCHK(c, hipMemcpyAsync(packed ? sig : hout.get(), d_out, out_words * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    if (packed) return PLFX_OK;
    memcpy(sig, hout.get(), KN * 48);
    memcpy(epl, hout.get() + 6 * KN, KN * 48);
    memcpy(deps, hout.get() + 12 * KN, KN * 48);
    memcpy(fy, hout.get() + 18 * KN, KN * 8);
    if (wh) memcpy(khard, hout.get() + 19 * KN, KN * 8);
    if (ct) memcpy(ct, hout.get() + o_ct, N * 288);
    const int32_t *hoi = (const int32_t *)(hout.get() + o_oi);
    memcpy(nsteps, hoi, KN * 4);
    memcpy(newton_out, hoi + KN, KN * 4);
    memcpy(ksteps, hoi + 2 * KN, N * 4);
    memcpy(status, hoi + 2 * KN + N, N * 4);
    return PLFX_OK;
}

int plfx_load_path(plfx_ctx *c, int mat, int n, int K, const double *dload, int shared, const int32_t *control,
                   const double *sig0, const double *epl0, const int32_t *tex_id, int maxit, int newton, double stol,
                   double eps_cap, double *sig, double *epl, double *deps, double *fy, int32_t *nsteps, int32_t *newton_out,
                   int32_t *ksteps, int32_t *status, double *ct)
{
    return load_path_impl(c, false, mat, n, K, dload, shared, control, sig0, epl0, tex_id, nullptr, 0, maxit, newton, stol, eps_cap,
                          sig, epl, deps, fy, nullptr, nsteps, newton_out, ksteps, status, ct);
}

int plfx_load_path_info(plfx_ctx *c, int64_t *launches)
{
    if (!c) return PLFX_ERR_ARG;
    if (launches) *launches = c->path_launches;
    return PLFX_OK;
}

// ... of a work-hardening SVC material: the hardening modulus is state of a path, khard0 at its start and
// khard after every accepted step.  form 1: k_path_batch<7>, a thread per path; form 2: k_path_wh_wave, a wave per path;
// form 0: the wave form up to PATH_WH_WAVE_MAX_N paths (every n).  One launch, one copy in, one copy out, as plfx_load_path.
int plfx_load_path_wh(plfx_ctx *c, int mat, int n, int K, const double *dload, int shared, const int32_t *control,
                      const double *sig0, const double *epl0, const double *khard0, int form, int maxit, int newton, double stol,
                      double eps_cap, double *sig, double *epl, double *deps, double *fy, double *khard, int32_t *nsteps,
                      int32_t *newton_out, int32_t *ksteps, int32_t *status, double *ct)
{
    return load_path_impl(c, true, mat, n, K, dload, shared, control, sig0, epl0, nullptr, khard0, form, maxit, newton, stol, eps_cap,
                          sig, epl, deps, fy, khard, nsteps, newton_out, ksteps, status, ct);
}

int plfx_load_path_wh_info(plfx_ctx *c, int64_t *launches_thread, int64_t *launches_wave)
{
    if (!c) return PLFX_ERR_ARG;
    if (launches_thread) *launches_thread = c->path_wh_launches[0];
    if (launches_wave) *launches_wave = c->path_wh_launches[1];
    return PLFX_OK;
}

// A committee of SVC yield functions on n shared unit stresses: all members in ONE launch of k_committee_yf, mean and
// variance over the members per point, and the point of largest variance (the blocks' partials are closed here, in block
// order: a strictly larger variance replaces, so equal variances resolve to the smaller index).
int plfx_committee_yf(plfx_ctx *c, int nmem, const int32_t *mats, const double *scale, int n, const double *su, double *yf,
                      double *mean, double *var, int32_t *best, double *best_var)
{
    static const char *const kind_names[] = {"elastic", "Hill / J2 on Voigt stresses", "Hill / J2 on principal stresses",
                                             "6-feature SVC", "Tresca", "Barlat", "2-feature SVC on principal stresses",
                                             "SVC with work-hardening features", "6-feature SVC with column scales"};
    if (!c || !c->dmat) return c ? fail(c, PLFX_ERR_STATE, "set_materials first") : PLFX_ERR_STATE;
    if (nmem < 1 || nmem > MAXMAT) return fail(c, PLFX_ERR_ARG, "plfx_committee_yf: nmem = %d, must be in 1..%d", nmem, MAXMAT);
    if (!mats || !scale || n < 0 || n > INT32_MAX - CY_BLOCK || (n > 0 && !su)) return fail(c, PLFX_ERR_ARG, "plfx_committee_yf: bad argument");
    CommitteeArgs a = {};
    int32_t staged = 0;
    for (int k = 0; k < nmem; k++) {
        if (mats[k] < 0 || mats[k] >= c->nmat)
            return fail(c, PLFX_ERR_ARG, "plfx_committee_yf: member %d is material %d, the context holds %d", k, mats[k], c->nmat);
        const MatDev &m = c->hmat[mats[k]];
        if (m.kind != PLFX_SVC6)
            return fail(c, PLFX_ERR_UNSUPPORTED, "plfx_committee_yf: member %d (material %d) is of kind %d (%s); only 6-feature SVC "
                        "materials on Voigt stresses form a committee", k, mats[k], m.kind, kind_names[m.kind]);
        if (!std::isfinite(scale[k]) || !(scale[k] > 0.))
            return fail(c, PLFX_ERR_ARG, "plfx_committee_yf: scale of member %d must be finite and positive", k);
        a.mat[k] = mats[k];
        a.scale[k] = scale[k];
        if (m.nsv * (m.nfeat + 1) <= c->svc_lds_need) staged |= 1 << k;   // the test of stage_svc
    }
    if (n == 0) return PLFX_OK;
    const int block = row16_block(c, n, CY_BLOCK), rpb = block / 16, nblk = (n + rpb - 1) / rpb;
    const bool query = best || best_var;
    CallBuffers B;   // [su | yf | mean | var | partial variances], partial indices
    double *dbuf = nullptr;
    int32_t *dpi = nullptr;
    const size_t nn = (size_t)n, o_yf = 6 * nn, o_mean = o_yf + (yf ? (size_t)nmem * nn : 0), o_var = o_mean + (mean ? nn : 0),
                 o_pv = o_var + (var ? nn : 0);
    if (int rc = B.get(c, &dbuf, o_pv + (query ? (size_t)nblk : 0))) return rc;
    if (query)
        if (int rc = B.get(c, &dpi, (size_t)nblk)) return rc;
    HIPCHK(c, hipMemcpyAsync(dbuf, su, nn * 48, hipMemcpyHostToDevice, c->stream));
    EvPair *ev;
    tim_begin(c, 0, &ev);
    hipLaunchKernelGGL(k_committee_yf, dim3(nblk), dim3(block), dyn_lds_bytes(c), c->stream, c->dmat, c->nmat, c->svc_lds_need, nmem,
                       a, n, (const double *)dbuf, yf ? dbuf + o_yf : nullptr, mean ? dbuf + o_mean : nullptr,
                       var ? dbuf + o_var : nullptr, query ? dbuf + o_pv : nullptr, dpi);
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    c->committee_launches++;
    c->committee_staged = staged;
    if (yf) HIPCHK(c, hipMemcpyAsync(yf, dbuf + o_yf, (size_t)nmem * nn * 8, hipMemcpyDeviceToHost, c->stream));
    if (mean) HIPCHK(c, hipMemcpyAsync(mean, dbuf + o_mean, nn * 8, hipMemcpyDeviceToHost, c->stream));
    if (var) HIPCHK(c, hipMemcpyAsync(var, dbuf + o_var, nn * 8, hipMemcpyDeviceToHost, c->stream));
    std::vector<double> pv;
    std::vector<int32_t> pi;
    if (query) {
        pv.resize(nblk);
        pi.resize(nblk);
        HIPCHK(c, hipMemcpyAsync(pv.data(), dbuf + o_pv, (size_t)nblk * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(pi.data(), dpi, (size_t)nblk * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, stream_sync(c));
    if (query) {
        double bv = std::nan("");
        int32_t bi = -1;
        for (int b = 0; b < nblk; b++)
            if (pi[b] >= 0 && (bi < 0 || pv[b] > bv)) bv = pv[b], bi = pi[b];
        if (best) *best = bi;
        if (best_var) *best_var = bv;
    }
    return PLFX_OK;
}

int plfx_committee_info(plfx_ctx *c, int64_t *launches, int32_t *staged_members)
{
    if (!c) return PLFX_ERR_ARG;
    if (launches) *launches = c->committee_launches;
    if (staged_members) *staged_members = c->committee_staged;
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ texture SVC
// The set: vectors padded to NFP = 8 / 12 / 16 slots at a row stride of NFP + 2 doubles (plfx_tex.hpp), coefficients, the
// scaler's mean and scale per column.  nsv = 0 releases the set; a second call replaces it.
int plfx_tex_svc_set(plfx_ctx *c, int nsv, int tdim, const double *sv, const double *dual, double intercept, double gamma,
                     const double *mean, const double *scale, int dev_only)
{
    if (!c) return PLFX_ERR_ARG;
    if (nsv < 0) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: nsv = %d", nsv);
    HIPCHK(c, hipSetDevice(c->device));
    if (nsv == 0) {
        HIPCHK(c, stream_sync(c));
        dfree(c->tex_sv);
        dfree(c->tex_dual);
        c->tex = TexSvcPar();
        c->tex_nfp = 0;
        c->tex_yf_launches = c->tex_ray_launches = 0;
        c->tex_fgrad_launches = c->tex_full_launches = c->tex_resp_launches = 0;
        return PLFX_OK;
    }
    if (tdim < 1 || tdim > TEX_TMAX)
        return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: tdim = %d texture coefficients, 1 <= tdim <= %d supported", tdim, TEX_TMAX);
    if (!sv || !dual || !mean || !scale) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: null argument");
    if (!(gamma > 0.) || !std::isfinite(gamma)) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: gamma must be > 0 (got %g)", gamma);
    if (!std::isfinite(intercept)) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: the intercept is not finite");
    const int d = 6 + tdim, nfp = d <= 8 ? 8 : d <= 12 ? 12 : 16, st = tex_stride(nfp);
    if ((int64_t)nsv * (st + 1) > INT32_MAX) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: nsv = %d is too large", nsv);
    TexSvcPar P = {};
    for (int j = 0; j < TEX_DMAX; j++) P.mean[j] = 0., P.scale[j] = 1.;
    for (int j = 0; j < d; j++) {
        if (!(scale[j] > 0.) || !std::isfinite(scale[j]))
            return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: scale of column %d must be finite and > 0 (got %g)", j, scale[j]);
        if (!std::isfinite(mean[j])) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: mean of column %d is not finite", j);
        P.mean[j] = mean[j], P.scale[j] = scale[j];
    }
    std::vector<double> tab((size_t)nsv * st, 0.);
    for (int k = 0; k < nsv; k++) {
        if (!std::isfinite(dual[k])) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: coefficient %d is not finite", k);
        for (int j = 0; j < d; j++) {
            const double v = sv[(size_t)k * d + j];
            if (!std::isfinite(v)) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_set: vector %d holds a non-finite value", k);
            tab[(size_t)k * st + j] = v;
        }
    }
    P.gamma = gamma, P.intercept = intercept, P.nsv = nsv, P.tdim = tdim, P.dev_only = dev_only ? 1 : 0;
    P.staged = (int64_t)nsv * (st + 1) <= c->lds_doubles ? 1 : 0;
    HIPCHK(c, stream_sync(c));   // no launch of the previous set is in flight when its tables go
    c->tex = TexSvcPar();
    c->tex_nfp = 0;
    if (int rc = dalloc(c, &c->tex_sv, tab.size())) return rc;
    if (int rc = dalloc(c, &c->tex_dual, (size_t)nsv)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->tex_sv, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->tex_dual, dual, (size_t)nsv * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, stream_sync(c));
    if (P.staged) {
        const int bytes = nsv * (st + 1) * 8;
        hipError_t e = hipSuccess;
        for (int width : {8, 12, 16})   // every width, as the attribute is only ever raised (set_dyn_lds)
            tex_for_nfp(width, [&](auto w) {
                if (e == hipSuccess) e = set_dyn_lds((const void *)k_tex_yf<decltype(w)::value>, bytes);
                if (e == hipSuccess) e = set_dyn_lds((const void *)k_tex_yield_scale<decltype(w)::value>, bytes);
                if (e == hipSuccess) e = set_dyn_lds((const void *)k_tex_fgrad<decltype(w)::value>, bytes);
                if (e == hipSuccess) e = set_dyn_lds((const void *)k_tex_full_yf<decltype(w)::value>, bytes);
                if (e == hipSuccess) e = set_dyn_lds((const void *)k_tex_response<decltype(w)::value>, bytes);
            });
        HIPCHK(c, e);
    }
    c->tex = P;
    c->tex_nfp = nfp;
    c->tex_yf_launches = c->tex_ray_launches = 0;
    c->tex_fgrad_launches = c->tex_full_launches = c->tex_resp_launches = 0;
    return PLFX_OK;
}

static size_t tex_lds_bytes(const plfx_ctx *c)
{
    return c->tex.staged ? (size_t)c->tex.nsv * (tex_stride(c->tex_nfp) + 1) * 8 : 0;
}

// calc_yf(sig, tex=) of the set at n points, one launch of k_tex_yf
int plfx_tex_svc_yf(plfx_ctx *c, int n, const double *sig, int ntex, const double *tex, const int32_t *tex_id, double *yf)
{
    if (!c) return PLFX_ERR_ARG;
    if (c->tex.nsv == 0) return fail(c, PLFX_ERR_STATE, "plfx_tex_svc_yf: plfx_tex_svc_set first");
    if (n < 0 || n > INT32_MAX / 2 || (n > 0 && (!sig || !tex || !yf || ntex < 1)))
        return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_yf: bad argument");
    if (n == 0) return PLFX_OK;
    if (!tex_id && ntex != 1 && ntex != n)
        return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_yf: %d textures for %d points; without tex_id one shared texture or one per "
                    "point is expected", ntex, n);
    if (tex_id)
        for (int i = 0; i < n; i++)
            if (tex_id[i] < 0 || tex_id[i] >= ntex)
                return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_yf: tex_id[%d] = %d, the call holds %d textures", i, tex_id[i], ntex);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = n, td = c->tex.tdim;
    CallBuffers B;
    double *dsig = nullptr, *dtex = nullptr, *dyf = nullptr;
    int32_t *did = nullptr;
    if (int rc = B.put(c, &dsig, sig, 6 * N)) return rc;
    if (int rc = B.put(c, &dtex, tex, (size_t)ntex * td)) return rc;
    if (tex_id)
        if (int rc = B.put(c, &did, tex_id, N)) return rc;
    if (int rc = B.get(c, &dyf, N)) return rc;
    const int block = row16_block(c, n, TEX_BLOCK);
    const dim3 grid = row16_grid(c, n, block, 8);
    EvPair *ev;
    tim_begin(c, 0, &ev);
    tex_for_nfp(c->tex_nfp, [&](auto w) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tex_yf<decltype(w)::value>), grid, dim3(block), tex_lds_bytes(c), c->stream, c->tex,
                           (const double *)c->tex_sv, (const double *)c->tex_dual, n, (const double *)dsig, ntex,
                           (const double *)dtex, (const int32_t *)did, dyf);
    });
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    c->tex_yf_launches++;
    HIPCHK(c, hipMemcpyAsync(yf, dyf, N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

// yield_scale(su, tex=) of the set: ntex x nray rays, texture-major, one launch of k_tex_yield_scale.  x0 NULL: the search of
// ray (t, r) starts at 1 / seq_J2(su_r), the factor that brings the ray to a J2 stress of one stress unit
int plfx_tex_svc_yield_scale(plfx_ctx *c, int nray, const double *su, int ntex, const double *tex, const double *x0, double *x,
                             int32_t *status)
{
    if (!c) return PLFX_ERR_ARG;
    if (c->tex.nsv == 0) return fail(c, PLFX_ERR_STATE, "plfx_tex_svc_yield_scale: plfx_tex_svc_set first");
    if (nray < 0 || ntex < 0 || (int64_t)nray * ntex > INT32_MAX / 2)
        return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_yield_scale: bad argument");
    if (nray == 0 || ntex == 0) return PLFX_OK;
    if (!su || !tex || !x || !status) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_yield_scale: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int nq = nray * ntex;
    const size_t Q = nq, td = c->tex.tdim;
    std::vector<double> start;
    if (!x0) {
        start.resize(Q);
        for (int r = 0; r < nray; r++) {
            const double *s = su + 6 * (size_t)r;
            const double d01 = s[0] - s[1], d12 = s[1] - s[2], d20 = s[2] - s[0];
            const double sj2 = std::sqrt(0.5 * (d01 * d01 + d12 * d12 + d20 * d20) + 3. * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]));
            for (int t = 0; t < ntex; t++) start[(size_t)t * nray + r] = 1. / sj2;   // (sj2 = 0: inf, status 3)
        }
    }
    CallBuffers B;
    double *dsu = nullptr, *dtex = nullptr, *dx0 = nullptr, *dx = nullptr;
    int32_t *dst = nullptr;
    if (int rc = B.put(c, &dsu, su, 6 * (size_t)nray)) return rc;
    if (int rc = B.put(c, &dtex, tex, (size_t)ntex * td)) return rc;
    if (int rc = B.put(c, &dx0, x0 ? x0 : start.data(), Q)) return rc;
    if (int rc = B.get(c, &dx, Q)) return rc;
    if (int rc = B.get(c, &dst, Q)) return rc;
    const int block = row16_block(c, nq, TEX_BLOCK);
    const dim3 grid = row16_grid(c, nq, block, 4);
    EvPair *ev;
    tim_begin(c, 0, &ev);
    tex_for_nfp(c->tex_nfp, [&](auto w) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tex_yield_scale<decltype(w)::value>), grid, dim3(block), tex_lds_bytes(c), c->stream,
                           c->tex, (const double *)c->tex_sv, (const double *)c->tex_dual, nray, (const double *)dsu, ntex,
                           (const double *)dtex, (const double *)dx0, dx, dst);
    });
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    c->tex_ray_launches++;
    HIPCHK(c, hipMemcpyAsync(x, dx, Q * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, dst, Q * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_tex_svc_info(plfx_ctx *c, int *nsv, int *tdim, int64_t *yf_launches, int64_t *ray_launches, int *staged)
{
    if (!c) return PLFX_ERR_ARG;
    if (nsv) *nsv = c->tex.nsv;
    if (tdim) *tdim = c->tex.tdim;
    if (yf_launches) *yf_launches = c->tex_yf_launches;
    if (ray_launches) *ray_launches = c->tex_ray_launches;
    if (staged) *staged = c->tex.staged;
    return PLFX_OK;
}

// ---- flow rule and stress update of the texture SVC (kernels in plfx_texflow.hpp)
// what the three calls ask of their common arguments; 1: n = 0, nothing to do
static int tex_flow_check(plfx_ctx *c, const char *who, int n, const double *sig, int ntex, const double *tex,
                          const int32_t *tex_id, bool outs_ok)
{
    if (!c) return PLFX_ERR_ARG;
    if (c->tex.nsv == 0) return fail(c, PLFX_ERR_STATE, "%s: plfx_tex_svc_set first", who);
    if (n < 0 || n > INT32_MAX / 36 || (n > 0 && (!sig || !tex || !outs_ok || ntex < 1)))
        return fail(c, PLFX_ERR_ARG, "%s: bad argument", who);
    if (n == 0) return 1;
    if (!tex_id && ntex != 1 && ntex != n)
        return fail(c, PLFX_ERR_ARG, "%s: %d textures for %d points; without tex_id one shared texture or one per point is "
                    "expected", who, ntex, n);
    if (tex_id)
        for (int i = 0; i < n; i++)
            if (tex_id[i] < 0 || tex_id[i] >= ntex)
                return fail(c, PLFX_ERR_ARG, "%s: tex_id[%d] = %d, the call holds %d textures", who, i, tex_id[i], ntex);
    return PLFX_OK;
}

// the material record the thread-per-point kernels take seq, sy, khard and the elastic matrix from
static int tex_flow_material(plfx_ctx *c, const char *who, int mat)
{
    if (!c->dmat) return fail(c, PLFX_ERR_STATE, "%s: set_materials first", who);
    if (mat < 0 || mat >= c->nmat) return fail(c, PLFX_ERR_ARG, "%s: material %d of %d", who, mat, c->nmat);
    if (c->hmat[mat].kind != PLFX_HILL6)
        return fail(c, PLFX_ERR_UNSUPPORTED, "%s: material %d is of kind %d; the record beside a texture set is an analytic "
                    "PLFX_HILL6 one", who, mat, (int)c->hmat[mat].kind);
    return PLFX_OK;
}

// calc_fgrad(sig, tex=) of the set at n points, one launch of k_tex_fgrad
int plfx_tex_svc_fgrad(plfx_ctx *c, int n, const double *sig, int ntex, const double *tex, const int32_t *tex_id, double *grad)
{
    if (int rc = tex_flow_check(c, "plfx_tex_svc_fgrad", n, sig, ntex, tex, tex_id, grad != nullptr)) return rc > 0 ? PLFX_OK : rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = n, td = c->tex.tdim;
    CallBuffers B;
    double *dsig = nullptr, *dtex = nullptr, *dg = nullptr;
    int32_t *did = nullptr;
    if (int rc = B.put(c, &dsig, sig, 6 * N)) return rc;
    if (int rc = B.put(c, &dtex, tex, (size_t)ntex * td)) return rc;
    if (tex_id)
        if (int rc = B.put(c, &did, tex_id, N)) return rc;
    if (int rc = B.get(c, &dg, 6 * N)) return rc;
    const int block = row16_block(c, n, TEX_BLOCK);
    const dim3 grid = row16_grid(c, n, block, 8);
    EvPair *ev;
    tim_begin(c, 0, &ev);
    tex_for_nfp(c->tex_nfp, [&](auto w) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tex_fgrad<decltype(w)::value>), grid, dim3(block), tex_lds_bytes(c), c->stream, c->tex,
                           (const double *)c->tex_sv, (const double *)c->tex_dual, n, (const double *)dsig, ntex,
                           (const double *)dtex, (const int32_t *)did, dg);
    });
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    c->tex_fgrad_launches++;
    HIPCHK(c, hipMemcpyAsync(grad, dg, 6 * N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

// ML_full_yf(sig, tex=) of the set at n points beside material 0 of the context, one launch of k_tex_full_yf
int plfx_tex_svc_full_yf(plfx_ctx *c, int n, const double *sig, int ntex, const double *tex, const int32_t *tex_id, double *f,
                         int32_t *status)
{
    if (int rc = tex_flow_check(c, "plfx_tex_svc_full_yf", n, sig, ntex, tex, tex_id, f && status)) return rc > 0 ? PLFX_OK : rc;
    if (int rc = tex_flow_material(c, "plfx_tex_svc_full_yf", 0)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = n, td = c->tex.tdim;
    CallBuffers B;
    double *dsig = nullptr, *dtex = nullptr, *df = nullptr;
    int32_t *did = nullptr, *dst = nullptr;
    if (int rc = B.put(c, &dsig, sig, 6 * N)) return rc;
    if (int rc = B.put(c, &dtex, tex, (size_t)ntex * td)) return rc;
    if (tex_id)
        if (int rc = B.put(c, &did, tex_id, N)) return rc;
    if (int rc = B.get(c, &df, N)) return rc;
    if (int rc = B.get(c, &dst, N)) return rc;
    EvPair *ev;
    tim_begin(c, 0, &ev);
    tex_for_nfp(c->tex_nfp, [&](auto w) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tex_full_yf<decltype(w)::value>), dim3(grid_for(N)), dim3(BLOCK), tex_lds_bytes(c),
                           c->stream, (const MatDev *)c->dmat, c->nmat, 0, c->tex, (const double *)c->tex_sv,
                           (const double *)c->tex_dual, n, (const double *)dsig, ntex, (const double *)dtex,
                           (const int32_t *)did, df, dst);
    });
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    c->tex_full_launches++;
    HIPCHK(c, hipMemcpyAsync(f, df, N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(status, dst, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

// Material.response(..., tex=) of the set at n points beside material `mat`, one launch of k_tex_response
int plfx_tex_svc_response(plfx_ctx *c, int mat, int n, const double *sig, const double *epl, const double *deps, int ntex,
                          const double *tex, const int32_t *tex_id, int maxit, double *fy, double *sig_out, double *depl,
                          double *ct, int32_t *nsteps)
{
    if (int rc = tex_flow_check(c, "plfx_tex_svc_response", n, sig, ntex, tex, tex_id,
                                epl && deps && fy && sig_out && depl && ct && nsteps))
        return rc > 0 ? PLFX_OK : rc;
    if (maxit < 1) return fail(c, PLFX_ERR_ARG, "plfx_tex_svc_response: maxit = %d", maxit);
    if (int rc = tex_flow_material(c, "plfx_tex_svc_response", mat)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = n, td = c->tex.tdim;
    CallBuffers B;
    double *d_in = nullptr, *d_out = nullptr, *dtex = nullptr;
    int32_t *did = nullptr, *d_ns = nullptr;
    if (int rc = B.get(c, &d_in, N * 18)) return rc;
    if (int rc = B.get(c, &d_out, N * (1 + 6 + 6 + 36))) return rc;
    if (int rc = B.get(c, &d_ns, N)) return rc;
    HIPCHK(c, hipMemcpyAsync(d_in, sig, N * 48, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in + 6 * N, epl, N * 48, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in + 12 * N, deps, N * 48, hipMemcpyHostToDevice, c->stream));
    if (int rc = B.put(c, &dtex, tex, (size_t)ntex * td)) return rc;
    if (tex_id)
        if (int rc = B.put(c, &did, tex_id, N)) return rc;
    double *d_fy = d_out, *d_so = d_out + N, *d_dp = d_out + 7 * N, *d_ct = d_out + 13 * N;
    EvPair *ev;
    tim_begin(c, 0, &ev);
    tex_for_nfp(c->tex_nfp, [&](auto w) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tex_response<decltype(w)::value>), dim3(grid_for(N)), dim3(BLOCK), tex_lds_bytes(c),
                           c->stream, (const MatDev *)c->dmat, c->nmat, mat, c->tex, (const double *)c->tex_sv,
                           (const double *)c->tex_dual, n, (const double *)d_in, (const double *)(d_in + 6 * N),
                           (const double *)(d_in + 12 * N), ntex, (const double *)dtex, (const int32_t *)did, d_fy, d_so, d_dp,
                           d_ct, d_ns, maxit);
    });
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    c->tex_resp_launches++;
    HIPCHK(c, hipMemcpyAsync(fy, d_fy, N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sig_out, d_so, N * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(depl, d_dp, N * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ct, d_ct, N * 288, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nsteps, d_ns, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_tex_svc_flow_info(plfx_ctx *c, int64_t *fgrad_launches, int64_t *full_yf_launches, int64_t *response_launches)
{
    if (!c) return PLFX_ERR_ARG;
    if (fgrad_launches) *fgrad_launches = c->tex_fgrad_launches;
    if (full_yf_launches) *full_yf_launches = c->tex_full_launches;
    if (response_launches) *response_launches = c->tex_resp_launches;
    return PLFX_OK;
}

int plfx_svc_fit_batch(plfx_ctx *c, int n, int d, const double *X, const double *y, int nprob, const int32_t *off,
                       const int32_t *idx, const double *C, const double *gamma, double tol, int64_t max_iter,
                       double *alpha, double *rho, double *obj, int32_t *iters, int32_t *status)
{
    return svc_fit_batch_impl(c, n, d, X, y, nprob, off, idx, C, gamma, tol, max_iter, alpha, rho, obj, iters, status);
}

int plfx_svc_fit_wide(plfx_ctx *c, int n, int d, const double *X, const double *y, double C, double gamma, double tol,
                      int64_t max_iter, int nwg, double *alpha, double *rho, double *obj, int32_t *iters, int32_t *status)
{
    return svc_fit_wide_impl(c, n, d, X, y, C, gamma, tol, max_iter, nwg, alpha, rho, obj, iters, status);
}

int plfx_svc_decision_batch(plfx_ctx *c, int n, int d, const double *X, int nprob, const int32_t *sv_off,
                            const int32_t *sv_idx, const double *coef, const double *intercept, const double *gamma,
                            const int32_t *q_off, const int32_t *q_idx, double *dec)
{
    return svc_decision_batch_impl(c, n, d, X, nprob, sv_off, sv_idx, coef, intercept, gamma, q_off, q_idx, dec);
}

int plfx_svr_fit_batch(plfx_ctx *c, int n, int d, const double *X, int nprob, const int32_t *off, const int32_t *idx,
                       const double *t, const double *C, const double *gamma, const double *epsilon, double tol,
                       int64_t max_iter, double *coef, double *rho, double *obj, int32_t *iters, int32_t *status)
{
    return svr_fit_batch_impl(c, n, d, X, nprob, off, idx, t, C, gamma, epsilon, tol, max_iter, coef, rho, obj, iters, status);
}

int plfx_set_svr_flow(plfx_ctx *c, int mat, int l, const double *X, const double *coef, const double *intercept, double gamma,
                      const double *feat_mean, const double *feat_scale, const double *out_mean, const double *out_scale)
{
    return set_svr_flow_impl(c, mat, l, X, coef, intercept, gamma, feat_mean, feat_scale, out_mean, out_scale);
}

int plfx_svr_flow_info(plfx_ctx *c, int mat, int *rows, int64_t *launches)
{
    if (!c) return PLFX_ERR_ARG;
    if (!c->dmat) return fail(c, PLFX_ERR_STATE, "set_materials first");
    if (mat < 0 || mat >= c->nmat) return fail(c, PLFX_ERR_ARG, "plfx_svr_flow_info: material %d out of range", mat);
    if (rows) *rows = c->svr_flow[mat].l;
    if (launches) *launches = c->svr_launches[mat];
    return PLFX_OK;
}

int plfx_svr_predict_multi(plfx_ctx *c, int n, int d, const double *X, double gamma, int m, const double *coef,
                           const double *intercept, int nq, const double *Q, double *out)
{
    return svr_predict_multi_impl(c, n, d, X, gamma, m, coef, intercept, nq, Q, out);
}

int plfx_set_response_maxit(plfx_ctx *c, int maxit)
{
    if (!c) return PLFX_ERR_ARG;
    if (maxit < 1) return fail(c, PLFX_ERR_ARG, "maxit must be >= 1");
    c->resp_maxit = maxit;
    return PLFX_OK;
}

// host side of plfx_lapack3.hpp (no context, no GPU): what the device routine of the PRINC3 / SVC3 kernels computes
int plfx_eig3_host(int n, const double *sig, double *w, double *V)
{
    if (n < 0 || !sig || !w) return PLFX_ERR_ARG;
    double Vt[9];
    for (int i = 0; i < n; i++)
        if (lapack3::dgeev3(sig + 6 * (size_t)i, w + 3 * (size_t)i, V ? V + 9 * (size_t)i : Vt) != 0) return 1;
    return PLFX_OK;
}

int plfx_sig_princ_host(int n, const double *sig, double *sp)
{
    if (n < 0 || !sig || !sp) return PLFX_ERR_ARG;
    int rc = PLFX_OK;
    for (int i = 0; i < n; i++)
        if (lapack3::sig_princ_lapack3(sig + 6 * (size_t)i, sp + 3 * (size_t)i) != 0) rc = 1;
    return rc;
}

}  // extern "C"
