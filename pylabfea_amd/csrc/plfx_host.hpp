// plfx_host.hpp -- what the translation units of libplfx.so share on the host side: the context, the error / allocation /
// timing helpers and the launch macros.  Included by the four units (plfx.hip, plfx_step.hip, plfx_material.hip, plfx_solve.hip)
// and by nothing outside csrc/.  Every helper declared here is defined in exactly one unit (named at its declaration); the unit
// map and the rule that every kernel has one owning unit are in DESIGN.md sections 39 and 42.  The C-ABI is include/plfx.h.
//
// HBM layout (FP64 / int32, everything resident for the life of the mesh):
//   per owned element e (SoA, component-major [c*nel + e]): sig[6] epl[6] eps[6] res_sig[6]
//     res_depl[6] tangent (TanStore: form tag, factors[7], elstiff[21, symmetric]) M[6] (compact stiffness generator)
//     fyn max_steps cls
//   connectivity conn[nel_total*4] (global element ids), per node: block-ELL matrix
//     val[nslot][2x2][nnode], col[nslot][nnode], contrib[nslot][nq][nnode] (assembly gather lists)
//   per DOF (interleaved x,y per node = double2): u f du rhs dinv diag is_presc + PCG vectors
//     x r z q p0 p1
#pragma once
#include "../../include/plfx.h"
#include "plfx_kernels.hpp"
#include "plfx_tex.hpp"   // TexSvcPar (its kernels are templates: nothing is compiled where nothing launches them)
#include "plfx_path.hpp"  // PathArgs and the load-path kernels (templates as well)

#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#define PLFX_VERSION "0.1.0-r1"

namespace plfx {
struct MgLevDev;   // plfx_mg.hpp
namespace host {

struct EvPair {
    hipEvent_t a, b;
    int which;
    bool pending;
};

struct Timing {
    bool on = false;
    unsigned mask = 0xFFu;  // families that are timed (plfx_timing_select)
    int every = 1;          // ... every n-th launch of a family (plfx_timing_sample)
    long long seen[8] = {0};
    std::vector<EvPair> ring;
    size_t head = 0;
    double ms[8] = {0};
    int64_t n[8] = {0};
    int64_t noop[8] = {0};  // launches that returned immediately (PCG already converged)
};

// RCCL is dlopen'ed in plfx.hip; the rest of the library sees a communicator handle and these constants
typedef struct ncclComm *ncclComm_t;

constexpr int NCCL_FLOAT64 = 8;  // ncclDouble
constexpr int NCCL_INT32 = 2;    // ncclInt32
constexpr int NCCL_SUM = 0;
constexpr int NCCL_MIN = 3;

template <class T>
struct DBuf {  // device buffer
    T *p = nullptr;
    size_t n = 0;
};

}  // namespace host
}  // namespace plfx

using namespace plfx;
using namespace plfx::host;

struct plfx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    hipDeviceProp_t prop;
    int lds_doubles = 0;  // dynamic LDS budget (doubles) for SVC staging

    // materials
    int nmat = 0;
    std::vector<MatDev> hmat;
    MatDev *dmat = nullptr;
    std::vector<double *> dsv;  // owned device copies of sv/dual
    bool has_svc = false, has_svc3 = false, has_analytic = false, has_elastic = false, has_princ = false;
    bool has_barlat = false;     // Barlat material with the native normal (plfx_material.barlat_normal)
    bool has_svcwh = false;      // SVC with work-hardening features (PLFX_SVC_WH)
    SvrFlowDev svr_flow[MAXMAT] = {}; // SVR flow rule of material k (plfx_set_svr_flow); l == 0: none; X and coef are owned device memory
    unsigned svr_mask = 0;       // bit k: material k has a rule attached (its points run on k_response_svr)
    int64_t svr_launches[MAXMAT] = {0};   // response launches of k_response_svr per material since the rule was attached
    int n_noflow = 0;            // materials without a flow rule (Tresca, Barlat without the native normal)
    int64_t committee_launches = 0;   // k_committee_yf launches of this context (plfx_committee_info)
    int32_t committee_staged = 0;     // bit k: member k of the last plfx_committee_yf call had its tables staged in LDS
    // texture SVC (plfx_tex_svc_set): a table set of its own, owned by the context; plfx_set_materials leaves it alone
    TexSvcPar tex = {};               // tex.nsv == 0: no set
    double *tex_sv = nullptr, *tex_dual = nullptr;   // [nsv * tex_stride(tex_nfp)] padded vectors, [nsv] coefficients
    int tex_nfp = 0;                  // padded feature slots of the set: 8, 12 or 16
    int64_t tex_yf_launches = 0, tex_ray_launches = 0;
    int64_t tex_fgrad_launches = 0, tex_full_launches = 0, tex_resp_launches = 0;   // the flow-rule calls
    int64_t flow_launches = 0;        // k_flow_curve / k_flow_curve_analytic launches of this context (plfx_flow_info)
    int64_t path_launches = 0;        // k_path_batch / k_path_row launches of this context (plfx_load_path_info)
    int64_t path_wh_launches[2] = {0, 0};   // k_path_batch<7> / k_path_wh_wave launches (plfx_load_path_wh_info)
    // texture fields (plfx_set_svc_textures): coefficient rows of material k, a PLFX_SVC6_COLS record; coef and sabs are
    // owned device memory, ids is filled in per launch.  tex_ids / htex_ids: the row of every owned element (null / empty: row 0),
    // checked against the attached rows by tex_field_check before a sweep or calc_scf (tex_ids_ok: since the last change of either)
    TexFieldDev tex_field[MAXMAT] = {};
    int tex_field_rows[MAXMAT] = {0};
    int64_t tex_field_launches[MAXMAT] = {0};
    unsigned tex_field_mask = 0;      // bit k: material k has rows attached (its launches take the TEXF instantiations)
    int32_t *tex_ids = nullptr;
    std::vector<int32_t> htex_ids;
    bool tex_ids_ok = false;
    int svc_lds_need = 0;
    unsigned svc_row_all = 0;    // bit k: material k is a 6-feature SVC run by the row kernels (one launch per material)
    unsigned svc_row_lds = 0;    // ... of these, the ones whose tables fit the LDS of a CU (the others are read from device memory)
    unsigned svc6_mask = 0;      // bit k: material k is a 6-feature SVC
    unsigned svc_cols_mask = 0;  // bit k: material k is a PLFX_SVC6_COLS record (always among svc_row_all, never in svc6_mask)
    unsigned svcwh_mask = 0;     // bit k: material k is an SVC with work-hardening features
    int svc_wave_lds = 0;        // dynamic LDS bytes of the row kernels with their tables in LDS (k_*_row<..., true>)
    int n_svc6 = 0;              // number of 6-feature SVC materials
    int want_svc_wave = 1;       // PLFX_SVC_WAVE

    // mesh
    int nel_total = 0, nnode = 0, ndof = 0, e0 = 0, nel = 0;  // nel = owned
    int planestress = 0;
    double thick = 1.;
    int ncls = 0;
    std::vector<ClassDev> hcls;
    std::vector<int32_t> hcls_id;  // per total element
    std::vector<int32_t> hconn;
    std::vector<double> hlxy;
    ClassDev *dcls = nullptr;
    int32_t *dconn = nullptr, *dcls_id = nullptr;  // dcls_id: owned elements only
    int32_t *dcls_all = nullptr;                   // class ids of ALL elements (assembly of the replicated matrix)
    bool sharded = false;                          // owns a strict subset of the elements
    int own_n0 = 0, own_n1 = 0;                    // disjoint node ownership for the sharded SpMV rows
    int nslot = 0, nq = 0;
    int32_t *dcol = nullptr, *dcontrib = nullptr;
    std::vector<int32_t> hcol;   // host copy of the neighbour slots (empty when the pattern is the closed-form structured one)
    int pat_nx = 0, pat_ny = 0;  // > 0: structured nx x ny grid, pattern in closed form (structured_slot), hcol not kept
    double *dval = nullptr;
    int n_begin = 0, n_end = 0;  // node range touched by owned elements
    bool nonlin = false;

    // element state (owned)
    double *sig = nullptr, *epl = nullptr, *eps = nullptr, *res_sig = nullptr, *res_depl = nullptr;
    // End of a load step.  res_is_sig: the last finish exchanged sig and res_sig instead of copying one into the
    // other -- c->sig holds both fields, the res_sig buffer is scratch until the next sweep writes it.  res_fresh: a sweep wrote
    // res_sig since the last exchange.  eps_stale: the stored eps is behind u; the wanted field is class_strain(u) (ensure_eps).
    bool res_is_sig = false, res_fresh = false, eps_stale = false;
    // plfx_element_fields: the rows of the last call (grown when a call asks for more rows than any before it, else reused) and
    // the per-block minimum / maximum partials with their host mirror
    double *fld_buf = nullptr, *fld_part = nullptr;
    size_t fld_cap = 0;
    std::vector<double> fld_host;
    double *Mel = nullptr, *fyn = nullptr, *scf_hh = nullptr;
    // element tangents (TanStore, plfx_kernels.hpp): one allocation tan_buf = [21][nel] full entries (elstiff), [7][nel] factors
    // (elfac), [nel] form tags (eltag)
    double *tan_buf = nullptr, *elstiff = nullptr, *elfac = nullptr;
    uint8_t *eltag = nullptr;
    double *kh_el = nullptr;   // hardening modulus per material point (work-hardening SVC: mutable, carried from sweep to sweep)
    // work-hardening SVC, sequential carry (the reference's semantics, plfx_kernels.hpp: k_wh_entry): kh_el holds the ENTRY
    // modulus of every element, kh_out / kh_touch what its response() left, wh_carry the value each material object holds now
    int hint_nx = 0, hint_ny = 0;   // the mesh came from plfx_set_mesh_structured (numbering known, no verification scans)
    bool hint_uniform = false;
    double *colr = nullptr;         // [gx] relative column widths of a non-proportional laminate (else null), KOp::colr
    double colr_ratio = 1.;
    int wh_mode = 1;           // 1 = sequential carry (default on one GPU), 0 = one modulus per material point
    double wh_carry[16] = {0};
    double *kh_out = nullptr, *kh_new = nullptr, *wh_snap_el = nullptr, *wh_snap_M = nullptr;
    int32_t *wh_snap_ms = nullptr;   // max_steps at the start of a sequential-carry sweep
    int32_t *kh_touch = nullptr, *wh_bmax = nullptr, *wh_cnt = nullptr;
    bool kh_out_valid = false;
    int64_t n_wh_passes = 0, n_wh_sweeps = 0, n_wh_unresolved = 0;
    int32_t *max_steps = nullptr, *scf_mult = nullptr, *heavy_list = nullptr;
    // dof vectors
    double *u = nullptr, *f = nullptr, *du = nullptr, *rhs = nullptr, *dinv = nullptr, *diag = nullptr,
           *is_presc = nullptr, *dup = nullptr, *wv = nullptr, *fext = nullptr;
    double *x = nullptr, *r = nullptr, *z = nullptr, *q = nullptr, *p[2] = {nullptr, nullptr};
    // scalars / partials
    double *part = nullptr;  // [8][MAXPART]
    double *part_g = nullptr;
    CgScalars *sc = nullptr;
    int *flags = nullptr;
    int *bflags = nullptr;  // per-block result slots of the sweep kernels (post_block_flags)
    double *small = nullptr;  // [64] scratch outputs
    int32_t *idx_tmp = nullptr;
    double *val_tmp = nullptr;
    size_t tmp_cap = 0;
    bool assembled = false, bc_set = false;
    std::vector<int32_t> bc_idx;  // prescribed DOFs of the last apply_bc (the device mask is reused when unchanged)
    bool bc_valid = false;
    double *stage = nullptr;      // pinned host staging buffer, two halves used alternately
    size_t stage_cap = 0;
    hipEvent_t stage_ev[2] = {nullptr, nullptr};  // H2D copy out of half h has completed
    bool stage_busy[2] = {false, false};
    int stage_flip = 0;
    int32_t *bc_idx_dev = nullptr;  // device copy of bc_idx (idx_tmp is shared with plfx_gather)
    size_t bc_idx_cap = 0;
    int32_t *bc_rows = nullptr;     // nodes whose matrix rows touch a prescribed node (rows of K w that can be non-zero)
    int bc_nrows = 0;
    double *kw = nullptr;           // K w, zero outside bc_rows
    // Between "the boundary values are known" and the first operator pass (PLFX_BC_ROWS=0 or PLFX_REUSE=0: off;
    // never with a strip or inside a communicator).  rhs_rows_ok: the last full k_bc_finish ran with this Dirichlet set and
    // this row list and without a force vector, and nothing has made rhs dense since -- rhs is +0.0 off bc_rows and
    // k_spmv_rows rewrites it on them.  dinv_ok: c->dinv was formed from the present (diag, is_presc); cleared at every launch
    // that writes c->diag.  A plain flag, not op_epoch: the set-up pass enqueued behind a sweep's flags writes diag before
    // plfx_assemble counts it, and assemble_fine_val on behalf of plfx_get_csr never counts.
    bool bc_rows_on = true;
    bool rhs_rows_ok = false, dinv_ok = false;
    long long n_rhs_rows = 0, n_dinv_kept = 0, n_dinv_refreshed = 0, n_du_early = 0;   // plfx_bc_info
    // Passes an accepted interpolated start never needs (PLFX_SHORT_SOLVE at plfx_create, a bit mask: 1 = A, 2 = B;
    // default 3, other bits ignored, PLFX_REUSE=0: 0; never with a strip or inside a communicator).
    // A. dinv_late: the diagonal was rewritten and c->dinv NOT formed again -- its zero pattern is the present Dirichlet mask
    //    (same set, and 1/|diag| is non-zero for every finite diag), its values are those of an older diagonal.  Whoever reads
    //    VALUES calls ensure_dinv first; the kernels of an interpolated start only test dinv != 0.
    // B. pred_d_kept: pred_d holds (free ? x - pred_x : 0) of the present x, pred_x and Dirichlet set, written by k_pred_finish;
    //    cleared at every other writer of x, pred_x or pred_d.  While it stands, k_pred_diff is left out.
    int short_solve = 3;
    bool dinv_late = false, pred_d_kept = false;
    long long n_dinv_deferred = 0, n_dinv_late = 0, n_d_kept = 0;   // plfx_short_info
    // Node code (PLFX_NODE_CODE at plfx_create, a bit mask: 1 = the Dirichlet set from the code, 2 = sparse b, which
    // needs 1; default 1 -- the sparse b did not
    // show against the mask alone, DESIGN 44 -- PLFX_REUSE=0: 0).  ncode: a byte per node (padded to a multiple of 256) -- bit 0 / 1: the x / y DOF is
    // prescribed, bit 2: the node is in bc_rows.  code_ok: ncode, is_presc and bc_rows come from one bc_idx; set where apply_bc_impl
    // forms the three, cleared wherever bc_valid or bc_set is.  The kernels of an interpolated start read it in place of the zero
    // pattern of dinv / is_presc, and (bit 2, while rhs_rows_ok stands) in place of the zeros of rhs (node_code, plfx_solve.hip).
    int node_code = 1;
    uint8_t *ncode = nullptr;
    bool code_ok = false;
    long long n_code_built = 0, n_code_start = 0, n_code_bsparse = 0, n_code_vector = 0;   // plfx_code_info
    int last_heavy = -1;  // elements that needed the sub-divided corrector in the last sweep (-1: no sweep yet)
    long long n_heavy_skipped = 0, n_heavy_recovered = 0;   // sweeps that left the corrector launches out / had to add them after all
    bool x_is_du = false;  // c->x still holds the last solution on the free DOFs (0 on the prescribed ones) = the warm start
    // initial guess from the last two solutions (plfx_solve): the solution before the one in c->x, scratch for the difference,
    // whether pred_x is that vector (same mesh, same Dirichlet set, c->x untouched since), counters
    double *pred_x = nullptr, *pred_d = nullptr;
    bool pred_valid = false;
    bool predict = true;            // PLFX_PREDICT=0 (read at plfx_create) switches the two-solution initial guess off
    // the coarse levels are set up when a V-cycle is about to run, not when the tangents change (most tangent-update solves of
    // a steady workload start below the tolerance, see plfx_solve): an assembly is pending; every BC application since kept the set
    bool mg_pending = false, mg_pending_same = true;
    long long n_mg_setup = 0, n_mg_setup_skipped = 0;
    // plfx_load_step, single GPU: the set-up pass of the next stiffness iteration and the K du of the end of the load step are
    // enqueued behind k_sweep_flags with device-side predicates, before the host has read the flags
    bool spec_arm = false, spec_setup = false, spec_kdu = false, spec_was_clean = false;
    // Rewritten generators straight into the operator's snapshot (PLFX_DIRECT_SNAP at plfx_create, a bit mask: 1 = A,
    // 2 = B, which needs A; default 3, PLFX_REUSE=0: 0).  INVARIANT while M_dirty is clear: Mop[e] == Mel[e] for every element (in
    // the other layout), except that with live_owed Mel is older than Mop.
    // A. an armed plane sweep that finds the invariant intact stores a rewritten generator to Mop as well (sweep_once: direct)
    //    and no set-up pass follows it.  direct_done: that sweep reported a changed tangent and the next plfx_assemble has
    //    nothing to launch.  setup_owed: diag and mg[1].Mel are older than Mop -- ensure_setup, in front of their readers and
    //    of every other writer of Mel, launches the pass the sweep left out.
    // B. the direct sweep does not write Mel.  live_owed: Mel is older than Mop -- ensure_live_M copies it back in front of every
    //    reader or partial writer of Mel.
    int direct_snap = 3;
    bool direct_done = false, setup_owed = false, live_owed = false;
    long long n_direct_sweeps = 0, n_direct_ack = 0, n_setup_late = 0, n_live_restored = 0;   // plfx_snap_info
    // Stores nobody reads (PLFX_DEAD_STORES=0 or PLFX_REUSE=0 at plfx_create: off).  dead_arm: plfx_load_step says of
    // the sweep it is about to launch that another one follows whenever a tangent changes -- the elements whose tangent changes
    // may leave res_sig, res_depl and fyn unwritten.  res_partial: the last sweep did leave some unwritten (it ran armed and
    // reported a changed tangent); cleared by the next sweep, and until then the three fields are not to be read.  Seen from
    // outside only after plfx_load_step returned an error between two sweeps.
    // test_starts: a solve whose first test is expected to pass starts with k_cg_start_test (solve_start).
    bool dead_stores = true, test_starts = true, dead_arm = false, res_partial = false;
    long long n_dead_sweeps = 0, n_dead_tangents = 0, n_test_starts = 0, n_test_retries = 0;   // plfx_dead_store_info
    // Plane columns (PLFX_PLANE_COLS=0 or PLFX_REUSE=0 at plfx_create: off).  plane_cols: columns 3 and 4 of sig, epl,
    // res_sig, res_depl are zero-valued in memory in both buffers of the exchange, rows 4 and 5 of elfac are zero, and every
    // material is elastic or analytic Hill / J2 with the yz / zx shears uncoupled (plane_mats_ok) -- the Hill sweep and the state
    // update neither load nor store them.  Switched on by plfx_state_reset alone (which zero-fills all of these), switched off by
    // whatever could put a non-zero there (plane_off), and then off until the next reset.
    bool plane_switch = true, plane_mats_ok = false, plane_cols = false;
    int plane_off_by = PLFX_PLANE_NEVER_ON;
    long long n_plane_sweeps = 0, n_plane_updates = 0;   // plfx_plane_info
    // plfx_load_step tells the solver which of its two solves this is (site 0 predictor of the load step, 1 stiffness iteration;
    // -1 any other caller); first_test_hint[site]: the last solve of that kind was answered by the test of the plain warm start
    // -- the next one waits for that test before it enqueues the six launches of the interpolated start behind it
    bool first_test_hint[2] = {false, false};
    int spec_h0 = 0, spec_h1 = 0;
    CgScalars *spec_sc = nullptr;
    long long n_spec_setup = 0, n_spec_kdu = 0;
    int resp_maxit = MAXIT;          // plfx_set_response_maxit: sub-steps of Material.response's sub-divided increment (point entry only)
    long long n_pred = 0, n_pred_skipped = 0, n_pred_rejected = 0;   // accepted as the solution / alpha < 0.01 / failed the tolerance test
    // Unchanged inputs are not recomputed (PLFX_REUSE=0 switches this off): the generators are re-snapshotted only when a
    // sweep reported a changed tangent (or they were written from outside) since the last plfx_assemble; a registered BC
    // plan with the same segment values on the same operator is not re-applied; and a solve of the system that the previous
    // converged solve already solved returns that solution (the reference repeats the last solve of a load step as the
    // predictor and as the first stiffness iteration of the next one whenever the increments are equal).
    bool reuse = true;
    bool M_dirty = true;             // generators (or anything plfx_assemble depends on) changed since the last assembly
    unsigned long long op_epoch = 0; // counts executed assemblies
    bool bc_memo = false, bc_memo_fext = false;
    unsigned long long bc_epoch = 0;
    BcSegVals bc_last{};
    struct { bool valid = false; double rtol = 0., relres = 0.; } memo;
    int n_reuse_assemble = 0, n_reuse_bc = 0, n_reuse_solve = 0;
    long long n_sweeps = 0, n_tangents_rewritten = 0;  // plfx_sweep_info
    long long n_svc_row_launches = 0, n_svc_thread_launches = 0;  // plfx_svc_info
    // registered boundary-condition plan (plfx_set_bc_plan): calc_BC's index structure, fixed for a load history
    struct BcPlan {
        int nseg = 0;
        std::vector<int32_t> seg_of;    // segment of every entry (reference order)
        std::vector<int32_t> presc;     // ascending unique prescribed DOFs
        std::vector<int32_t> first_pos; // entry that writes du for presc[k] (first occurrence)
        std::vector<int32_t> inv;       // entry -> position in presc
        std::vector<double> first, w;   // scratch
        bool valid = false;
        int32_t *seg4 = nullptr;        // device: up to 4 segments per prescribed DOF in entry order (-1 = unused); null when
                                        // a DOF has more entries or there are more than BcSegVals::N segments
        // plfx_set_bc_sources: where each segment's value comes from, and the force-controlled segments
        std::vector<int32_t> src, k, fsrc, fk, flen, fidx;
        std::vector<double> fshare, fext;
        bool sources = false;
    } plan;
    // registered DOF set of plfx_finish_step (boundary nodes of calc_global)
    int32_t *fin_idx = nullptr;
    int fin_n = 0;
    double *fin_dev = nullptr;      // [2 n + 18] gathered u, f and the 18 element sums
    double *fin_host = nullptr;     // pinned mirror
    // deferred end-of-step results (plfx_step.defer_slot): two pinned slots, posted by the device, collected by
    // plfx_finish_fetch while the next load step is already running
    CgMbox *fin_box[2] = {nullptr, nullptr};
    double *fin_pin[2] = {nullptr, nullptr};
    unsigned long long fin_seq[2] = {0, 0};
    bool fin_pending[2] = {false, false};
    int fin_pin_n = 0;
    int fin_defer = -1;             // slot the next plfx_finish_step posts into instead of waiting
    int mg_fallbacks = 0; // solves that fell back from multigrid- to Jacobi-PCG
    int n_indefinite = 0; // solves with an indefinite tangent stiffness (PCG met negative curvature, GMRES completed them)
    std::vector<double *> gm_blk;                // GMRES: Krylov basis in blocks of GMRES_BLK vectors, allocated as a cycle grows into them
    double *gm_part = nullptr;                   //        partial sums, on first use
    double *gm_part2 = nullptr, *gm_red = nullptr, *gm_coef = nullptr;   // delayed re-orthogonalisation: partials of all columns, their sums, coefficients
    long long n_gmres_its = 0;
    int n_gmres = 0, gm_m = 0;
    bool strip_jacobi = false;  // strip-local engine during such a fall-back: the V-cycle is replaced by z = D^-1 r
    int grid_nodes = 0, grid_el = 0;

    // geometric multigrid preconditioner (structured grids, plfx_set_grid)
    struct MgLevel {
        int nx = 0, ny = 0, nnode = 0, nel = 0, nslot = 0, nq = 0, grid = 1;
        int32_t *col = nullptr, *contrib = nullptr, *cls0 = nullptr;
        double *val = nullptr, *diag = nullptr, *dinv = nullptr, *Mel = nullptr;
        double *x = nullptr, *b = nullptr, *t = nullptr, *res = nullptr;
        double *ainv = nullptr;  // dense inverse (coarsest level, small grids)
        KOp op{};                // operator descriptor (block-ELL arrays + grid/generator form)
        double rx = 1., ry = 1.; // relative size of the level's last element column / row (levels of an odd-sized mesh, KOp::rx)
        ClassDev *cls4 = nullptr; // geometry tables of its four cell shapes (interior, last column, last row, corner), when assembled
        bool matfree = false;    // applied from the generators (no assembled matrix on this level)
        bool owned = false;  // level 0 aliases the fine-grid arrays of the context
    };
    std::vector<MgLevel> mg;
    ClassDev *mg_cls = nullptr;  // geometry tables shared by all levels
    MgLevDev *mg_dev = nullptr;  // level descriptors for the single-workgroup tail kernel
    int mg_tail = -1;            // first level handled by the tail kernel (-1: none)
    int mg_tail_T = 0;           // nodes of all tail levels; > 0: the LDS-resident tail kernel is usable
    int mg_cheby = 0;            // > 0: Chebyshev steps that solve the coarsest level (no dense inverse: odd coarse sizes)
    double mg_cheby_kappa = 1.;  // assumed condition number of D^-1 K on the coarsest level
    int mg_tail_E = 0;           // elements of the tail levels without the coarsest; > 0: the matrix-free tail is usable
    size_t mg_tail_lds = 0;      // dynamic LDS of k_mg_tail_mf
    bool mg_inv_valid = false;   // the dense coarse inverse matches the current coarse matrix and Dirichlet mask
    bool mg_dinv_current = false; // the matrix-free levels' dinv was written by the last mg_assemble with the current mask
    CgMbox *mbox = nullptr;                // pinned host mailbox of the PCG convergence flag (PLFX_MAILBOX)
    unsigned long long mbox_seq = 0;
    double *mb_buf = nullptr;              // pinned result buffer of fetch_results
    int mb_cap = 0;
    hipGraph_t mg_graph = nullptr;         // captured launches of the V-cycle's coarse levels
    hipGraphExec_t mg_graph_exec = nullptr;
    int want_mg_graph = 1;                 // PLFX_MG_GRAPH
    int gx = 0, gy = 0;          // structured grid (elements) if known
    int precond = 1;             // 0 = Jacobi, 1 = multigrid when available
    double mg_omega = 0.65;  // damped Jacobi; lambda_max(D^-1 K) ~ 2.3 for Q4 elasticity (0.9 diverges)
    int mg_nu = 2;
    // matrix-free operator on structured grids with one element shape (plfx_set_grid)
    bool grid_ok = false;        // the structured, uniform grid form is available
    int want_matfree = 1;        // plfx_set_operator / PLFX_MATFREE
    double *dtab = nullptr;      // geometry table of grid_apply
    double *Mop = nullptr;       // generators as of the last plfx_assemble (the matrix-free K is a snapshot like setupK's)
    KOp op{};                    // fine-level operator
    bool val_valid = false;      // the fine block-ELL values match the current generators

    // multi-GPU
    ncclComm_t comm = nullptr;
    plfx_allreduce_fn host_ar = nullptr;  // host-staged collective transport (plfx_comm_init_callback: tests, hosts without RCCL)
    void *host_ar_user = nullptr;
    std::vector<char> host_ar_buf;
    int rank = 0, nranks = 1;
    const char *last_coll = nullptr;   // the collective enqueued last on this context's stream, and how many there have been:
    long long n_coll = 0;              // named in the error a wait for device results ends with after coll_timeout_s
    double coll_timeout_s = 300.;      // PLFX_COLL_TIMEOUT (seconds; 0 = wait for ever): a peer that never arrives must not hang the job

    // Strip-local engine (plfx_set_strip): this context holds ONE x-strip of a larger structured grid as
    // a standalone local grid -- the owned element columns [oc0, oc1) plus W halo columns on every interior side.  Three
    // things stitch the strips together: the halo refresh of a node vector (contiguous node columns, one send/recv pair per
    // neighbour), owned-only reductions followed by all-reduces of the per-block partial sums, and a replicated coarse
    // problem (`child`: levels >= Ld of the GLOBAL grid, fed by one all-reduce of the owned level-Ld residual per V-cycle).
    struct Strip {
        bool on = false;
        int oc0 = 0, oc1 = 0;            // owned element columns of the local grid
        int W = 0;                       // halo width in element columns
        int Ld = 0;                      // first level of the replicated coarse problem
        int gcol0 = 0, gnx = 0;          // global element column of local column 0, global element columns
        bool has_left = false, has_right = false;
        int own_lo = 0, own_hi = 0;      // owned node range [lo, hi): disjoint over the ranks (reductions)
        int eown_lo = 0, eown_hi = 0;    // owned element range
        plfx_ctx *child = nullptr;
        std::vector<double> hbuf;        // host staging of the callback transport
        long long n_halo = 0, n_coarse = 0, n_part = 0, n_gen = 0;
        // launches of the local levels 1 .. Ld-1 before / after the coarse hand-over, captured once and replayed
        hipGraph_t g_down = nullptr, g_up = nullptr;
        hipGraphExec_t x_down = nullptr, x_up = nullptr;
    } strip;
    bool is_child = false;               // coarse context of a strip: shares stream, sc and dtab with its parent

    Timing tim;
};

namespace plfx {
namespace host {

int fail(plfx_ctx *c, int code, const char *fmt, ...);   // plfx.hip

#define HIPCHK(c, call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(c, PLFX_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                  \
    } while (0)

template <class T>
int dalloc(plfx_ctx *c, T **p, size_t n)
{
    if (*p) {
        hipFree(*p);
        *p = nullptr;
    }
    if (n == 0) n = 1;
    HIPCHK(c, hipMalloc((void **)p, n * sizeof(T)));
    HIPCHK(c, hipMemsetAsync(*p, 0, n * sizeof(T), c->stream));
    return 0;
}

template <class T>
void dfree(T *&p)
{
    if (p) hipFree(p);
    p = nullptr;
}

// device buffers of one call, released on every exit path
struct CallBuffers {
    std::vector<void *> p;
    template <class T>
    int get(plfx_ctx *c, T **q, size_t n)
    {
        HIPCHK(c, hipMalloc((void **)q, std::max<size_t>(n, 1) * sizeof(T)));
        p.push_back(*q);
        return 0;
    }
    // get + upload of n elements on c->stream (host stays valid until the stream is synchronised)
    template <class T>
    int put(plfx_ctx *c, T **q, const T *host, size_t n)
    {
        if (int rc = get(c, q, n)) return rc;
        HIPCHK(c, hipMemcpyAsync(*q, host, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        return 0;
    }
    ~CallBuffers()
    {
        for (void *q : p) hipFree(q);
    }
};

// doubles of the tangent store of n elements: 21 entries + 7 factors + one tag byte per element
inline size_t tan_words(size_t n) { return 28 * n + (n + 7) / 8; }

inline TanStore tan_store(const plfx_ctx *c) { return TanStore{c->eltag, c->elfac, c->elstiff}; }

// blocks of the kernels that reduce the 18 element sums of calc_global (part_g): k_update_state<1> at 1024^2, same-box
// rocprofv3 averages (tools/probes/r04_sumpart_ab.sh): 1024 blocks with 18 sequential block sums 86-88 us; the 18 sums behind
// ONE barrier (block_sums_to_partials, bit-identical) 81-83; and then 2048 blocks 74, 4096 blocks 78
#ifndef PLFX_SUMPART
#define PLFX_SUMPART 2048
#endif
constexpr int SUMPART = PLFX_SUMPART;

// ---- one-line predicates: inline, so that the launch paths gain no calls
inline bool matfree(const plfx_ctx *c) { return c->grid_ok && c->want_matfree; }
inline bool comm_active(const plfx_ctx *c) { return c->comm != nullptr || c->host_ar != nullptr; }
// work-hardening SVC in the reference's sequential-carry semantics: single rank only (the chain crosses every shard)
inline bool wh_sequential(const plfx_ctx *c) { return c->has_svcwh && c->wh_mode == 1 && !comm_active(c) && !c->sharded && !c->strip.on; }

// kernels templated on the operator form: <.., 1> matrix-free grid, <.., 0> block-ELL
// (the first kernel argument is the operator: one with per-column widths takes instantiation 2)
template <class... T> static inline bool first_op_columns(const KOp &o, const T &...) { return o.colr != nullptr; }
#define LAUNCH_OP1(KERN, mf, grid, ...)                                                                        \
    do {                                                                                                       \
        if ((mf) && first_op_columns(__VA_ARGS__))                                                             \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN<2>), grid, dim3(BLOCK), 0, c->stream, __VA_ARGS__);        \
        else if (mf)                                                                                           \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN<1>), grid, dim3(BLOCK), 0, c->stream, __VA_ARGS__);        \
        else                                                                                                   \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN<0>), grid, dim3(BLOCK), 0, c->stream, __VA_ARGS__);        \
    } while (0)
// ... and on a multigrid level whose last element column / row has another size (KOp::rx, ry): instantiation 2
#define LAUNCH_OP1R(KERN, mf, op, grid, ...)                                                                   \
    do {                                                                                                       \
        if ((mf) && ((op).rx != 1. || (op).ry != 1.))                                                          \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN<2>), grid, dim3(BLOCK), 0, c->stream, __VA_ARGS__);        \
        else                                                                                                   \
            LAUNCH_OP1(KERN, mf, grid, __VA_ARGS__);                                                           \
    } while (0)
#define LAUNCH_OP2R(KERN, A, mf, op, grid, ...)                                                                \
    do {                                                                                                       \
        if ((mf) && ((op).rx != 1. || (op).ry != 1.))                                                          \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN<A, 2>), grid, dim3(BLOCK), 0, c->stream, __VA_ARGS__);     \
        else                                                                                                   \
            LAUNCH_OP2(KERN, A, mf, grid, __VA_ARGS__);                                                        \
    } while (0)
#define LAUNCH_OP2(KERN, A, mf, grid, ...)                                                                     \
    do {                                                                                                       \
        if ((mf) && first_op_columns(__VA_ARGS__))                                                             \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN<A, 2>), grid, dim3(BLOCK), 0, c->stream, __VA_ARGS__);     \
        else if (mf)                                                                                           \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN<A, 1>), grid, dim3(BLOCK), 0, c->stream, __VA_ARGS__);     \
        else                                                                                                   \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(KERN<A, 0>), grid, dim3(BLOCK), 0, c->stream, __VA_ARGS__);     \
    } while (0)

inline size_t dyn_lds_bytes(const plfx_ctx *c) { return (c->has_svc || c->has_svc3 || c->has_svcwh) ? (size_t)c->svc_lds_need * 8 : 0; }

inline int own_lo(const plfx_ctx *c) { return c->strip.on ? c->strip.own_lo : 0; }
inline int own_hi(const plfx_ctx *c) { return c->strip.on ? c->strip.own_hi : c->nnode; }

inline bool mg_active(const plfx_ctx *c) { return c->precond == 1 && c->mg.size() >= 2; }

// the level halves exactly and all its cells have one size (every level of a mesh whose sizes are multiples of 2^levels)
inline bool level_plain(const plfx_ctx::MgLevel &L) { return !(L.nx & 1) && !(L.ny & 1) && L.rx == 1. && L.ry == 1.; }

// launch a row kernel for material k: tables in LDS when they fit, else read from device memory (no dynamic LDS); a
// PLFX_SVC6_COLS material takes the per-column instantiation, and with a texture field attached the TEXF one, which
// takes the field with the rows `ids` of the elements / points as its last argument
#define LAUNCH_ROW1(c, k, ids_, kern, grid, ...)                                                                            \
    do {                                                                                                                 \
        const bool cols_ = ((c)->svc_cols_mask >> (k)) & 1u;                                                             \
        if (((c)->tex_field_mask >> (k)) & 1u) {                                                                         \
            TexFieldDev tf_ = (c)->tex_field[k];                                                                         \
            tf_.ids = (ids_);                                                                                            \
            if (((c)->svc_row_lds >> (k)) & 1u)                                                                          \
                hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<true, true, true, TexFieldDev>), grid, dim3(512), (size_t)(c)->svc_wave_lds, (c)->stream, __VA_ARGS__, tf_);  \
            else                                                                                                         \
                hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<false, true, true, TexFieldDev>), grid, dim3(512), 0, (c)->stream, __VA_ARGS__, tf_);  \
            (c)->tex_field_launches[k]++;                                                                                \
        } else if ((((c)->svc_row_lds >> (k)) & 1u) && cols_)                                                                   \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<true, true>), grid, dim3(512), (size_t)(c)->svc_wave_lds, (c)->stream, __VA_ARGS__);  \
        else if (cols_)                                                                                                  \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<false, true>), grid, dim3(512), 0, (c)->stream, __VA_ARGS__);        \
        else if (((c)->svc_row_lds >> (k)) & 1u)                                                                         \
            hipLaunchKernelGGL(kern<true>, grid, dim3(512), (size_t)(c)->svc_wave_lds, (c)->stream, __VA_ARGS__);        \
        else                                                                                                             \
            hipLaunchKernelGGL(kern<false>, grid, dim3(512), 0, (c)->stream, __VA_ARGS__);                               \
    } while (0)
#define LAUNCH_ROW2(c, k, ids_, kern, H, grid, ...)                                                                         \
    do {                                                                                                                 \
        const bool cols_ = ((c)->svc_cols_mask >> (k)) & 1u;                                                             \
        if (((c)->tex_field_mask >> (k)) & 1u) {                                                                         \
            TexFieldDev tf_ = (c)->tex_field[k];                                                                         \
            tf_.ids = (ids_);                                                                                            \
            if (((c)->svc_row_lds >> (k)) & 1u)                                                                          \
                hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<H, true, true, true, TexFieldDev>), grid, dim3(512), (size_t)(c)->svc_wave_lds, (c)->stream, __VA_ARGS__, tf_);  \
            else                                                                                                         \
                hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<H, false, true, true, TexFieldDev>), grid, dim3(512), 0, (c)->stream, __VA_ARGS__, tf_);  \
            (c)->tex_field_launches[k]++;                                                                                \
        } else if ((((c)->svc_row_lds >> (k)) & 1u) && cols_)                                                                   \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<H, true, true>), grid, dim3(512), (size_t)(c)->svc_wave_lds, (c)->stream, __VA_ARGS__);   \
        else if (cols_)                                                                                                  \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<H, false, true>), grid, dim3(512), 0, (c)->stream, __VA_ARGS__);     \
        else if (((c)->svc_row_lds >> (k)) & 1u)                                                                         \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<H, true>), grid, dim3(512), (size_t)(c)->svc_wave_lds, (c)->stream, __VA_ARGS__);   \
        else                                                                                                             \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<H, false>), grid, dim3(512), 0, (c)->stream, __VA_ARGS__);           \
    } while (0)

// (a strip or a communicator can be set up after the reset: asked at every launch)
inline bool plane_active(const plfx_ctx *c) { return c->plane_cols && !c->strip.on && !comm_active(c) && !c->sharded; }

// Block size of a kernel with 16 lanes per point whose blocks stage the tables once: the fewest points per block that still
// leave no more than a few blocks per CU, so that a short batch spreads over the device.  No result depends on the choice.
inline int row16_block(const plfx_ctx *c, int n, int cap)
{
    int block = 64;
    while (block < cap && (n + block / 16 - 1) / (block / 16) > 2 * c->prop.multiProcessorCount) block *= 2;
    return block;
}

// Grid of such a kernel: a block per block / 16 points, but no more than `rounds` blocks per CU, since every block stages the
// tables again
inline dim3 row16_grid(const plfx_ctx *c, int n, int block, int rounds)
{
    const int rpb = block / 16;
    return dim3(std::max(1, std::min((n + rpb - 1) / rpb, rounds * c->prop.multiProcessorCount)));
}
// ---- shared helpers, each defined in one unit

// plfx.hip
hipError_t set_dyn_lds(const void *fn, int bytes);
int tan_alloc(plfx_ctx *c, size_t n);
void tan_free(plfx_ctx *c);
int grid_for(size_t n, int cap = MAXPART);
int grid_xcd(size_t n);
void tim_begin(plfx_ctx *c, int which, EvPair **out);
void tim_end(plfx_ctx *c, EvPair *e);
void tim_flush(plfx_ctx *c);
hipError_t stream_sync(plfx_ctx *c);
int mbox_wait(plfx_ctx *c, unsigned long long seq, CgMbox *box = nullptr);
int fetch_results(plfx_ctx *c, const double *src_dev, int n, double *dst_host);
int ensure_tmp(plfx_ctx *c, size_t n);
int allreduce(plfx_ctx *c, void *dev, size_t count, int nccl_dtype, int nccl_op, const char *what);
int part_allreduce(plfx_ctx *c, double *p, size_t n);
int halo_refresh(plfx_ctx *c, double *v);
int strip_sync_M(plfx_ctx *c);
int sync_M(plfx_ctx *c);
void plane_off(plfx_ctx *c, int why);
KOp make_op(const plfx_ctx *c, int nnode, int nslot, const int32_t *col, const double *val, int nx, int ny, int nel,
            const double *M, double rx = 1., double ry = 1.);
void mg_graph_drop(plfx_ctx *c);
int strip_coarse(plfx_ctx *c);
void strip_free(plfx_ctx *c);
int plain_spmv(plfx_ctx *c, const double *in, double *out);
bool march_pcg(const plfx_ctx *c);
int ensure_dinv(plfx_ctx *c);
int mg_ensure(plfx_ctx *c);
int mg_vcycle_head(plfx_ctx *c);
int mg_vcycle_rest(plfx_ctx *c, double *rz_part, bool *wrote);
int mg_vcycle(plfx_ctx *c);
// ... and its kernels that the step and solve units need launched
void launch_spmv_plain(plfx_ctx *c, const double *in, double *out, CgScalars *sc);   // k_spmv MODE 0: out = K in (sc: device-side predicate or null)
void launch_jacobi_z(plfx_ctx *c);                      // k_jacobi_z: z = D^-1 r
void launch_mbox_post(plfx_ctx *c, const double *src, int n, double *dst, CgMbox *mb, unsigned long long seq);   // k_mbox_post
void launch_kdu_uf(plfx_ctx *c, CgScalars *spec);       // k_spmv MODE 3: u += du, f += K du (spec: device-side predicate or null)
void launch_spec_setup(plfx_ctx *c);                    // the set-up pass a sweep enqueues behind its flags (k_grid_setup)
int ensure_live_M(plfx_ctx *c);                         // k_restore_M if the live generators are owed
int ensure_setup(plfx_ctx *c);                          // the set-up pass a direct sweep left out, if it is owed
int before_M_write(plfx_ctx *c);                        // both, in front of whatever writes part of the live generators

// plfx_step.hip
int ensure_eps(plfx_ctx *c);
int split_res_sig(plfx_ctx *c);
int raise_step_lds(plfx_ctx *c);
void launch_response_row(plfx_ctx *c, int k, const int32_t *tex_id, int n, const int32_t *mat_id, const double *sig, const double *epl,
                         const double *deps, double *fy, double *sig_out, double *depl, double *ct, int32_t *nsteps);   // k_response_row
void launch_path_row(plfx_ctx *c, int k, const int32_t *tex_id, const PathArgs &a);   // k_path_row
void launch_tangent_expand(plfx_ctx *c, double *out, int to_full);   // k_tangent_expand over the owned elements
#ifdef PLFX_PROF_REGIONS
bool prof_regions_add_step(unsigned long long h[16]);   // h += the step unit's g_prof (probe builds; plfx_destroy prints the sums)
#endif

// plfx_material.hip
void free_materials(plfx_ctx *c);
#ifdef PLFX_PROF_REGIONS
bool prof_regions_add_material(unsigned long long h[16]);   // ... += the material unit's
#endif

// plfx_solve.hip
int solve_impl(plfx_ctx *c, double rtol, int maxit, int warm, int site, int *iters, double *relres);

}  // namespace host
}  // namespace plfx
