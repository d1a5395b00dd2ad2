// plfx.hip -- host side of libplfx.so: context, HBM residency, collectives, mesh and pattern, operator, multigrid, strip engine,
// boundary conditions, instrumentation.  The sweeps, the load step and the state access are plfx_step.hip, the material tables
// and the material-point functions plfx_material.hip, the linear solve plfx_solve.hip.  What the four units share is
// plfx_host.hpp; unit map and the rule that every kernel has one owning unit: DESIGN.md sections 39 and 42.  This unit owns the
// kernels of the three groups below.
#define PLFX_UNIT_CONTEXT
#define PLFX_UNIT_MESH
#define PLFX_UNIT_OPERATOR
#include "plfx_host.hpp"
#include "plfx_mg.hpp"

namespace plfx {
namespace host {

// minimal RCCL surface (dlopen'ed so the library loads on hosts without RCCL in the path)
typedef struct { char internal[128]; } ncclUniqueId;
typedef int (*fn_ncclGetUniqueId)(ncclUniqueId *);
typedef int (*fn_ncclCommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
typedef int (*fn_ncclAllReduce)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t);
typedef int (*fn_ncclCommDestroy)(ncclComm_t);
typedef int (*fn_ncclSend)(const void *, size_t, int, int, ncclComm_t, hipStream_t);
typedef int (*fn_ncclRecv)(void *, size_t, int, int, ncclComm_t, hipStream_t);
typedef int (*fn_ncclGroup)(void);
struct Rccl {
    void *h = nullptr;
    fn_ncclGetUniqueId GetUniqueId = nullptr;
    fn_ncclCommInitRank CommInitRank = nullptr;
    fn_ncclAllReduce AllReduce = nullptr;
    fn_ncclCommDestroy CommDestroy = nullptr;
    fn_ncclSend Send = nullptr;          // point-to-point: halo refresh of the strip-local engine
    fn_ncclRecv Recv = nullptr;
    fn_ncclGroup GroupStart = nullptr, GroupEnd = nullptr;
};
Rccl g_rccl;
bool load_rccl()
{
    if (g_rccl.h) return true;
    // prefer an RCCL that is already in the process (torch.distributed's), then the system one
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
    for (const char *n : names) {
        g_rccl.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        if (g_rccl.h) break;
    }
    if (!g_rccl.h)
        for (const char *n : names) {
            g_rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (g_rccl.h) break;
        }
    if (!g_rccl.h) return false;
    g_rccl.GetUniqueId = (fn_ncclGetUniqueId)dlsym(g_rccl.h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (fn_ncclCommInitRank)dlsym(g_rccl.h, "ncclCommInitRank");
    g_rccl.AllReduce = (fn_ncclAllReduce)dlsym(g_rccl.h, "ncclAllReduce");
    g_rccl.CommDestroy = (fn_ncclCommDestroy)dlsym(g_rccl.h, "ncclCommDestroy");
    g_rccl.Send = (fn_ncclSend)dlsym(g_rccl.h, "ncclSend");
    g_rccl.Recv = (fn_ncclRecv)dlsym(g_rccl.h, "ncclRecv");
    g_rccl.GroupStart = (fn_ncclGroup)dlsym(g_rccl.h, "ncclGroupStart");
    g_rccl.GroupEnd = (fn_ncclGroup)dlsym(g_rccl.h, "ncclGroupEnd");
    return g_rccl.GetUniqueId && g_rccl.CommInitRank && g_rccl.AllReduce && g_rccl.CommDestroy;
}
// Opt-in to > 64 KiB of dynamic LDS is a per-function attribute shared by every context of the process (several models, the
// point-evaluation context, the coarse context of a strip): only ever raise it, so that a context created later with
// smaller tables cannot shrink the limit under a context that still launches with the larger ones.
hipError_t set_dyn_lds(const void *fn, int bytes)
{
    static std::map<std::pair<int, const void *>, int> cur;
    static std::mutex mu;
    int dev = 0;
    hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    auto key = std::make_pair(dev, fn);
    auto it = cur.find(key);
    if (it != cur.end() && it->second >= bytes) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) cur[key] = bytes;
    return e;
}


int fail(plfx_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

int tan_alloc(plfx_ctx *c, size_t n)
{
    int rc = dalloc(c, &c->tan_buf, tan_words(n));
    if (rc) return rc;
    c->elstiff = c->tan_buf;
    c->elfac = c->tan_buf + 21 * n;
    c->eltag = reinterpret_cast<uint8_t *>(c->tan_buf + 28 * n);
    return 0;
}

void tan_free(plfx_ctx *c)
{
    dfree(c->tan_buf);
    c->elstiff = c->elfac = nullptr;
    c->eltag = nullptr;
}

int grid_for(size_t n, int cap)
{
    size_t g = (n + BLOCK - 1) / BLOCK;
    if (g < 1) g = 1;
    if (g > (size_t)cap) g = cap;
    return (int)g;
}

// k_grid_setup: one thread per row and group of SETUP_COLS columns, every thread exactly one walk (no partial sums: no cap)
int setup_cols(const KOp &g)
{
    static const int forced = getenv("PLFX_SETUP_COLS") ? atoi(getenv("PLFX_SETUP_COLS")) : 0;   // experiments: 1, 4, 8
    if (forced == 1 || forced == 4 || forced == 8) return forced;
    return g.nnode >= (1 << 19) ? 4 : 1;   // (level 1 of 1024^2, 513^2 nodes: 12.4 us with 1, 13.6 with 4)
}
int setup_grid(const KOp &g)
{
    return (int)((grid_setup_tasks(g.nxn, g.nyn, setup_cols(g)) + BLOCK - 1) / BLOCK);
}
// k_grid_setup<SRC, COLS> with the column walk of the level's size
#define LAUNCH_SETUP(SRC, G, ...)                                                                                             \
    do {                                                                                                                       \
        const int cols_ = setup_cols(G);                                                                                       \
        if (cols_ == 8)                                                                                                        \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grid_setup<SRC, 8>), dim3(setup_grid(G)), dim3(BLOCK), 0, c->stream, G, __VA_ARGS__); \
        else if (cols_ == 4)                                                                                                   \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grid_setup<SRC, 4>), dim3(setup_grid(G)), dim3(BLOCK), 0, c->stream, G, __VA_ARGS__); \
        else                                                                                                                   \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grid_setup<SRC, 1>), dim3(setup_grid(G)), dim3(BLOCK), 0, c->stream, G, __VA_ARGS__); \
    } while (0)

// round the grid to a multiple of 8 (XCD count) when large enough, for xcd_tile()
int grid_xcd(size_t n)
{
    int g = grid_for(n);
    if (g >= 16) g &= ~7;
    return g;
}

void tim_begin(plfx_ctx *c, int which, EvPair **out)
{
    *out = nullptr;
    Timing &t = c->tim;
    if (!t.on || !((t.mask >> which) & 1u)) return;
    // sampled (two event records per timed launch cost host time and a bubble on the stream); family 7 (collectives): every call
    if (t.every > 1 && which != 7 && (t.seen[which]++ % t.every) != 0) return;
    if (t.ring.empty()) {
        t.ring.resize(2048);
        for (auto &e : t.ring) {
            hipEventCreate(&e.a);
            hipEventCreate(&e.b);
            e.pending = false;
        }
    }
    EvPair &e = t.ring[t.head];
    if (e.pending) {  // recycle: resolve the old measurement first
        hipEventSynchronize(e.b);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e.a, e.b);
        t.ms[e.which] += ms;
        t.n[e.which]++;
        e.pending = false;
    }
    e.which = which;
    hipEventRecord(e.a, c->stream);
    *out = &e;
    t.head = (t.head + 1) % t.ring.size();
}

void tim_end(plfx_ctx *c, EvPair *e)
{
    if (!e) return;
    hipEventRecord(e->b, c->stream);
    e->pending = true;
}

void tim_flush(plfx_ctx *c)
{
    Timing &t = c->tim;
    for (auto &e : t.ring)
        if (e.pending) {
            hipEventSynchronize(e.b);
            float ms = 0.f;
            hipEventElapsedTime(&ms, e.a, e.b);
            t.ms[e.which] += ms;
            t.n[e.which]++;
            e.pending = false;
        }
}

// hipStreamSynchronize of the context's stream -- with peers, bounded like mbox_wait: a collective whose partner never arrives
// ends the call with an error that names it instead of hanging the job
hipError_t stream_sync(plfx_ctx *c)
{
    if (c->n_coll == 0 || !(c->coll_timeout_s > 0.)) return hipStreamSynchronize(c->stream);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (;;) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e != hipErrorNotReady) return e;
        __builtin_ia32_pause();
        if ((++spins & 0x3FF) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > c->coll_timeout_s) {
            fail(c, PLFX_ERR_HIP, "rank %d of %d: stream not drained after %.0f s -- stuck behind collective #%lld, the last one enqueued "
                 "being '%s'; PLFX_COLL_TIMEOUT sets the limit", c->rank, c->nranks, c->coll_timeout_s, c->n_coll, c->last_coll ? c->last_coll : "?");
            fprintf(stderr, "[plfx] %s\n", c->err.c_str());
            return hipErrorLaunchTimeOut;
        }
    }
}

// wait until a kernel has posted `seq` to the pinned mailbox (a failed launch or a hung queue must not spin forever)
int mbox_wait(plfx_ctx *c, unsigned long long seq, CgMbox *box)
{
    if (!box) box = c->mbox;
    // waits as long as the stream has work in flight (like hipStreamSynchronize would: a corrector sweep over millions
    // of SVC elements takes seconds); fails on a stream error, or when the stream has drained and the post never arrived
    unsigned spins = 0;
    int idle_seen = 0;
    std::chrono::steady_clock::time_point t0;
    bool timing = false;
    while (__atomic_load_n(&box->seq, __ATOMIC_ACQUIRE) != seq) {
        __builtin_ia32_pause();
        if ((++spins & 0xFFFFF) == 0) {
            const hipError_t e = hipStreamQuery(c->stream);
            if (e != hipSuccess && e != hipErrorNotReady)
                return fail(c, PLFX_ERR_HIP, "stream error while waiting for device results: %s", hipGetErrorString(e));
            if (e == hipSuccess && ++idle_seen > 8)
                return fail(c, PLFX_ERR_HIP, "device results were not posted although the stream has drained");
            // with peers: work that stays in flight for minutes is a collective whose partner never arrived (the longest
            // kernel of a strip, a corrector sweep over its SVC elements, takes seconds)
            if (c->n_coll > 0 && c->coll_timeout_s > 0.) {
                if (!timing) {
                    t0 = std::chrono::steady_clock::now();
                    timing = true;
                } else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > c->coll_timeout_s) {
                    return fail(c, PLFX_ERR_HIP, "rank %d of %d: no device results after %.0f s -- the stream is stuck behind collective "
                                "#%lld, the last one enqueued being '%s' (a peer that left the schedule, or a transport that never "
                                "completes); PLFX_COLL_TIMEOUT sets the limit", c->rank, c->nranks, c->coll_timeout_s, c->n_coll,
                                c->last_coll ? c->last_coll : "?");
                }
            }
        }
    }
    return 0;
}

// n doubles of device results to the host: through the pinned mailbox buffer (kernel writes host memory, host spins on
// the sequence number) or by a device->host copy + stream synchronisation
int fetch_results(plfx_ctx *c, const double *src_dev, int n, double *dst_host)
{
    if (!c->mbox || n > c->mb_cap) {
        HIPCHK(c, hipMemcpyAsync(dst_host, src_dev, (size_t)8 * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
        return 0;
    }
    const unsigned long long seq = ++c->mbox_seq;
    hipLaunchKernelGGL(k_mbox_post, dim3(1), dim3(BLOCK), 0, c->stream, src_dev, n, c->mb_buf, c->mbox, seq);
    HIPCHK(c, hipGetLastError());
    int rc = mbox_wait(c, seq);
    if (rc) return rc;
    memcpy(dst_host, c->mb_buf, (size_t)8 * n);
    return 0;
}

// Gauss point i of the Q4 element (model.py:339-346)
void gauss_point(double lx, double ly, int i, double *x, double *y)
{
    const double cpos = std::sqrt(1. / 3.);
    const double sx = ((i / 2) % 2 == 0) ? 1. : -1.;
    const double sy = (i % 2 == 0) ? 1. : -1.;
    *x = 0.5 * (1. + sx * cpos) * lx;
    *y = 0.5 * (1. + sy * cpos) * ly;
}

// shape-function derivative factors at (x,y): bx[a] = B[0][2a], by[a] = B[1][2a+1] (model.py:475-497)
void shape_b(double lx, double ly, double x, double y, double bx[4], double by[4])
{
    const double xi1 = 2. * x / lx - 1.;
    const double xi2 = 2. * y / ly - 1.;
    const double hxm = 0.125 * (1. - xi1) / ly;
    const double hym = 0.125 * (1. - xi2) / lx;
    const double hxp = 0.125 * (1. + xi1) / ly;
    const double hyp = 0.125 * (1. + xi2) / lx;
    bx[0] = -hym;
    bx[1] = -hyp;
    bx[2] = hym;
    bx[3] = hyp;
    by[0] = -hxm;
    by[1] = hxm;
    by[2] = -hxp;
    by[3] = hxp;
}

ClassDev make_class(const plfx_ctx *c, int mat, double lx, double ly)
{
    ClassDev k;
    memset(&k, 0, sizeof(k));
    k.mat = mat;
    k.lx = lx;
    k.ly = ly;
    k.vel = lx * ly * c->thick;       // model.py:316
    const double jac = 4. * k.vel;    // model.py:322, 340 (wght = 1)
    k.kappa = 0.;
    if (c->planestress) {             // model.py:498-501 with the plane-stress CV of :277-283
        const MatDev &m = c->hmat[mat];
        const double c11 = m.CV[sym_idx(0, 0)], c12 = m.CV[sym_idx(0, 1)];
        k.kappa = -m.nu * (c11 + c12) / m.E;
    }
    for (int g = 0; g < 4; g++) {
        double x, y, bx[4], by[4];
        gauss_point(lx, ly, g, &x, &y);
        shape_b(lx, ly, x, y, bx, by);
        for (int a = 0; a < 4; a++) {
            k.bxs[a] += bx[a];
            k.bys[a] += by[a];
            for (int b = 0; b < 4; b++) {
                k.Sxx[a * 4 + b] += jac * bx[a] * bx[b];
                k.Sxy[a * 4 + b] += jac * bx[a] * by[b];
                k.Syy[a * 4 + b] += jac * by[a] * by[b];
            }
        }
    }
    return k;
}

// Block-ELL pattern of the elements [e0, e1): per node the sorted neighbour list (slots) and, per
// (node, slot), the element contributions (e_local*16 + a*4 + b) in ascending element order.
// Is conn the reference's structured numbering of an nx x ny grid (model.py:893, 935-948), nx, ny >= 2?
bool structured_dims(int nel, int nnode, const int32_t *conn, int *nx_out, int *ny_out)
{
    if (nel < 4) return false;
    const int nyn = conn[2] - conn[0];   // first element: [0, 1, nyn, nyn + 1]
    if (conn[0] != 0 || conn[1] != 1 || nyn < 3 || conn[3] != nyn + 1) return false;
    const int ny = nyn - 1;
    if (nel % ny) return false;
    const int nx = nel / ny;
    if (nx < 2 || (long long)(nx + 1) * nyn != nnode) return false;
    for (int e = 0; e < nel; e++) {
        const int n1 = (e / ny) * nyn + e % ny;
        const int32_t *q = conn + 4 * (size_t)e;
        if (q[0] != n1 || q[1] != n1 + 1 || q[2] != n1 + nyn || q[3] != n1 + nyn + 1) return false;
    }
    *nx_out = nx;
    *ny_out = ny;
    return true;
}

// neighbour node in slot s of node i on the host: closed form on structured grids, the stored pattern otherwise
inline int host_col(const plfx_ctx *c, int s, int i)
{
    if (c->pat_nx > 0) {
        int32_t cj, codes[4];
        structured_slot(c->pat_nx, c->pat_ny, i, s, &cj, codes);
        return cj;
    }
    return c->hcol[(size_t)s * c->nnode + i];
}

bool build_pattern(int nnode, const int32_t *conn, int el_begin, int el_end, std::vector<int32_t> &hcol,
                   std::vector<int32_t> &hcontrib, int &nslot, int &nq, int &nb, int &ne)
{
    std::vector<int32_t> deg(nnode + 1, 0);
    for (int e = el_begin; e < el_end; e++)
        for (int a = 0; a < 4; a++) deg[conn[4 * e + a] + 1]++;
    for (int i = 0; i < nnode; i++) deg[i + 1] += deg[i];
    std::vector<int32_t> adj(deg[nnode]);  // packed (local element, local node), ascending element order
    {
        std::vector<int32_t> fill(deg.begin(), deg.end() - 1);
        for (int e = el_begin; e < el_end; e++)
            for (int a = 0; a < 4; a++) adj[fill[conn[4 * e + a]]++] = (e - el_begin) * 4 + a;
    }
    nslot = 0;
    nq = 0;
    nb = nnode;
    ne = 0;
    std::vector<int32_t> tmp;
    for (int i = 0; i < nnode; i++) {  // pass 1: sizes
        const int a0 = deg[i], a1 = deg[i + 1];
        if (a1 == a0) continue;
        nb = std::min(nb, i);
        ne = std::max(ne, i + 1);
        nq = std::max(nq, a1 - a0);
        tmp.clear();
        for (int k = a0; k < a1; k++) {
            const int e = adj[k] >> 2;
            for (int b = 0; b < 4; b++) tmp.push_back(conn[4 * (e + el_begin) + b]);
        }
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        nslot = std::max(nslot, (int)tmp.size());
    }
    if (nslot == 0) return false;
    hcol.assign((size_t)nslot * nnode, -1);
    hcontrib.assign((size_t)nslot * nq * nnode, -1);
    for (int i = 0; i < nnode; i++) {  // pass 2: fill
        const int a0 = deg[i], a1 = deg[i + 1];
        if (a1 == a0) continue;
        tmp.clear();
        for (int k = a0; k < a1; k++) {
            const int e = adj[k] >> 2;
            for (int b = 0; b < 4; b++) tmp.push_back(conn[4 * (e + el_begin) + b]);
        }
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        for (size_t s = 0; s < tmp.size(); s++) {
            hcol[s * nnode + i] = tmp[s];
            int qn = 0;
            for (int k = a0; k < a1; k++) {  // ascending element order = reference's addition order
                const int e = adj[k] >> 2, a = adj[k] & 3;
                for (int b = 0; b < 4; b++)
                    if (conn[4 * (e + el_begin) + b] == tmp[s])
                        hcontrib[((size_t)s * nq + qn++) * nnode + i] = e * 16 + a * 4 + b;
            }
        }
    }
    return true;
}

void free_mesh(plfx_ctx *c)
{
    mg_graph_drop(c);
    strip_free(c);
    dfree(c->dcls);
    dfree(c->dconn);
    dfree(c->dcls_id);
    dfree(c->dcls_all);
    dfree(c->dcol);
    dfree(c->dcontrib);
    dfree(c->dval);
    dfree(c->sig);
    dfree(c->epl);
    dfree(c->eps);
    dfree(c->res_sig);
    dfree(c->res_depl);
    dfree(c->fld_buf);
    dfree(c->fld_part);
    c->fld_cap = 0;
    tan_free(c);
    dfree(c->Mel);
    dfree(c->fyn);
    dfree(c->scf_hh);
    dfree(c->kh_el);
    dfree(c->kh_out); dfree(c->kh_new); dfree(c->wh_snap_el); dfree(c->wh_snap_M); dfree(c->wh_snap_ms);
    dfree(c->kh_touch); dfree(c->wh_bmax); dfree(c->wh_cnt);
    c->kh_out_valid = false;
    dfree(c->max_steps);
    dfree(c->scf_mult);
    dfree(c->heavy_list);
    dfree(c->u);
    dfree(c->f);
    dfree(c->du);
    dfree(c->rhs);
    dfree(c->dinv);
    dfree(c->diag);
    dfree(c->is_presc);
    dfree(c->ncode);
    dfree(c->dup);
    dfree(c->wv);
    dfree(c->fext);
    dfree(c->x);
    dfree(c->r);
    dfree(c->z);
    dfree(c->q);
    dfree(c->pred_x);
    dfree(c->pred_d);
    c->pred_valid = c->pred_d_kept = false;
    for (auto &b : c->gm_blk) dfree(b);
    c->gm_blk.clear();
    c->gm_m = 0;
    dfree(c->gm_part);
    dfree(c->gm_part2);
    dfree(c->gm_red);
    dfree(c->gm_coef);
    dfree(c->p[0]);
    dfree(c->p[1]);
    for (auto &L : c->mg) {
        if (!L.owned) continue;
        dfree(L.col);
        dfree(L.contrib);
        dfree(L.cls0);
        dfree(L.val);
        dfree(L.diag);
        dfree(L.dinv);
        dfree(L.Mel);
        dfree(L.x);
        dfree(L.b);
    }
    for (auto &L : c->mg) {
        dfree(L.t);
        dfree(L.res);
        dfree(L.ainv);
    }
    c->mg.clear();
    dfree(c->mg_cls);
    dfree(c->mg_dev);
    dfree(c->dtab);
    dfree(c->Mop);
    dfree(c->colr);
    c->grid_ok = false;
    c->val_valid = false;
    c->mg_tail = -1;
    c->gx = c->gy = 0;
    c->assembled = c->bc_set = false;
    c->M_dirty = true;
    c->x_is_du = false;
    c->bc_valid = c->code_ok = false;
    c->bc_idx.clear();
    c->plan.valid = false;
    dfree(c->fin_idx);
    dfree(c->fin_dev);
    c->fin_n = 0;
    dfree(c->kw);
    dfree(c->bc_rows);
    c->bc_nrows = 0;
    c->rhs_rows_ok = c->dinv_ok = c->dinv_late = false;
    c->direct_done = c->setup_owed = c->live_owed = false;
    dfree(c->tex_ids);
    c->htex_ids.clear();
    c->tex_ids_ok = false;
}

int ensure_tmp(plfx_ctx *c, size_t n)
{
    if (n <= c->tmp_cap) return 0;
    dfree(c->idx_tmp);
    dfree(c->val_tmp);
    int rc = dalloc(c, &c->idx_tmp, n);
    if (rc) return rc;
    rc = dalloc(c, &c->val_tmp, 4 * n);
    if (rc) return rc;
    c->tmp_cap = n;
    return 0;
}

// Marching form of the finest-grid operator kernels (grid_march): PLFX_MARCH=0 never, =1 always; default: the PCG operator
// kernel always (faster at every size measured), the three V-cycle kernels when one operator pass (112 B per node) exceeds
// 192 MiB -- three quarters of the 256 MiB Infinity Cache: a pass shares the cache with the other vectors of the cycle, and the
// gather form starts to re-fetch before the pass alone fills it (1448^2 nodes; measured cross-over between 1024^2, where the
// gather form is as fast or faster, and 2048^2, where marching wins by 20 %, tools/probes/march_probe.hip)
int march_env()
{
    static const int v = getenv("PLFX_MARCH") ? atoi(getenv("PLFX_MARCH")) : -1;
    return v;
}
bool march_pcg(const plfx_ctx *c) { return matfree(c) && march_env() != 0 && !c->op.colr; }   // (the marching kernels know one cell shape)
bool march_mg(const plfx_ctx *c)
{
    if (!matfree(c) || march_env() == 0) return false;
    return march_env() == 1 || (size_t)c->nnode * 112 > ((size_t)192 << 20);
}
// the single-workgroup tail of the V-cycle applies its levels from the generators too (needs the dense coarse inverse)
bool tail_mf(const plfx_ctx *c)
{
    return matfree(c) && c->mg_tail_T > 0 && c->mg_tail_E > 0 && c->mg_nu == 2 && !c->mg.empty() && c->mg.back().ainv;
}

void launch_spmv_plain(plfx_ctx *c, const double *in, double *out, CgScalars *sc)
{
    LAUNCH_OP2(k_spmv, 0, matfree(c), dim3(c->grid_nodes), c->op, 0, c->nnode, (const double2 *)in, nullptr, nullptr,
               (double2 *)out, nullptr, nullptr, nullptr, 0, nullptr, sc, 0, 0, 0);
}

int plain_spmv(plfx_ctx *c, const double *in, double *out)
{
    launch_spmv_plain(c, in, out, nullptr);
    HIPCHK(c, hipGetLastError());
    return 0;  // the matrix is replicated on every rank: no collective here
}

// in-place all-reduce of a device buffer on the library's stream: RCCL, or the host-staged callback transport
int allreduce(plfx_ctx *c, void *dev, size_t count, int nccl_dtype, int nccl_op, const char *what)
{
    c->last_coll = what;
    c->n_coll++;
    if (c->comm) {
        EvPair *ev;
        tim_begin(c, 7, &ev);  // family 7: collectives (time on the stream incl. the wait for the slowest peer)
        const int rcn = g_rccl.AllReduce(dev, dev, count, nccl_dtype, nccl_op, c->comm, c->stream);
        tim_end(c, ev);
        if (rcn != 0) return fail(c, PLFX_ERR_HIP, "ncclAllReduce(%s) failed", what);
        return 0;
    }
    if (c->host_ar) {
        const size_t bytes = count * (nccl_dtype == NCCL_INT32 ? 4 : 8);
        if (c->host_ar_buf.size() < bytes) c->host_ar_buf.resize(bytes);
        HIPCHK(c, hipMemcpyAsync(c->host_ar_buf.data(), dev, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
        if (c->host_ar(c->host_ar_user, c->host_ar_buf.data(), count, nccl_dtype == NCCL_INT32 ? 1 : 0,
                       nccl_op == NCCL_MIN ? 3 : 0) != 0)
            return fail(c, PLFX_ERR_HIP, "host all-reduce callback failed (%s)", what);
        HIPCHK(c, hipMemcpyAsync(dev, c->host_ar_buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, stream_sync(c));
        return 0;
    }
    return 0;
}

// Sharded runs: make the stiffness generators of the whole mesh consistent on every rank after a sweep
// changed the owned ones (own part + exact zeros elsewhere, summed by one all-reduce).
int sync_M(plfx_ctx *c)
{
    if (!comm_active(c) || !c->sharded) return 0;
    if (int rc = before_M_write(c)) return rc;   // (never owed inside a communicator: said for the rule's sake)
    if (c->strip.on) return strip_sync_M(c);  // strip-local engine: only the halo columns, from the neighbour that owns them
    hipLaunchKernelGGL(k_zero_foreign_M, dim3(grid_for((size_t)6 * c->nel_total)), dim3(BLOCK), 0, c->stream,
                       c->nel_total, c->e0, c->e0 + c->nel, c->Mel);
    HIPCHK(c, hipGetLastError());
    return allreduce(c, c->Mel, (size_t)6 * c->nel_total, NCCL_FLOAT64, NCCL_SUM, "M");
}


// ---------------------------------------------------------------------------------------------- strip-local engine
// collectives of a strip run whenever there are peers -- and with a single rank when PLFX_STRIP_FORCE_COLL=1 (exercises the
// RCCL calls of the path on a 1-rank communicator: tests)
bool strip_coll(const plfx_ctx *c)
{
    static const bool force = getenv("PLFX_STRIP_FORCE_COLL") && atoi(getenv("PLFX_STRIP_FORCE_COLL")) != 0;
    return c->nranks > 1 || (force && (c->comm || c->host_ar));
}

// all-reduce of per-block partial sums (owned-only on every rank): the consumer kernels keep summing the <= 1024 entries
// redundantly in a fixed order, so every rank takes bitwise the same decisions
int part_allreduce(plfx_ctx *c, double *p, size_t n)
{
    if (!c->strip.on || !strip_coll(c)) return 0;
    c->strip.n_part++;
    return allreduce(c, p, n, NCCL_FLOAT64, NCCL_SUM, "partial sums");
}

// Halo refresh of a node vector v (double2 per node, node id = column * nyn + row): the W node columns beyond each
// interior edge of the owned range are overwritten with the neighbour's (valid) values.  Columns are contiguous in memory,
// so a slab is one send / recv without packing:
//   to the left neighbour   my columns oc0+1 .. oc0+W      from it   columns oc0-W .. oc0-1
//   to the right neighbour  my columns oc1-W .. oc1-1      from it   columns oc1+1 .. oc1+W
// (node columns oc0 and oc1 are computed validly by both sides)
int halo_refresh(plfx_ctx *c, double *v)
{
    auto &S = c->strip;
    if (!S.on || !strip_coll(c)) return 0;
    const int nyn = c->gy + 1;
    const size_t n = (size_t)S.W * nyn * 2;
    double *sendL = v + (size_t)2 * (S.oc0 + 1) * nyn, *recvL = v + (size_t)2 * (S.oc0 - S.W) * nyn;
    double *sendR = v + (size_t)2 * (S.oc1 - S.W) * nyn, *recvR = v + (size_t)2 * (S.oc1 + 1) * nyn;
    S.n_halo++;
    c->last_coll = "halo refresh (ncclSend / ncclRecv with the strip neighbours)";
    c->n_coll++;
    if (c->comm) {
        if (!g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart || !g_rccl.GroupEnd)
            return fail(c, PLFX_ERR_UNSUPPORTED, "this RCCL has no ncclSend/ncclRecv");
        EvPair *ev;
        tim_begin(c, 7, &ev);
        int rc = g_rccl.GroupStart();
        if (!rc && S.has_left) {
            rc = g_rccl.Send(sendL, n, NCCL_FLOAT64, c->rank - 1, c->comm, c->stream);
            if (!rc) rc = g_rccl.Recv(recvL, n, NCCL_FLOAT64, c->rank - 1, c->comm, c->stream);
        }
        if (!rc && S.has_right) {
            rc = g_rccl.Send(sendR, n, NCCL_FLOAT64, c->rank + 1, c->comm, c->stream);
            if (!rc) rc = g_rccl.Recv(recvR, n, NCCL_FLOAT64, c->rank + 1, c->comm, c->stream);
        }
        const int rc2 = g_rccl.GroupEnd();
        tim_end(c, ev);
        if (rc || rc2) return fail(c, PLFX_ERR_HIP, "halo refresh (ncclSend/ncclRecv) failed: %d / %d", rc, rc2);
        return 0;
    }
    if (c->host_ar) {  // host-staged transport: [to left | to right] out, [from left | from right] back (op 100)
        S.hbuf.assign(2 * n, 0.);
        if (S.has_left) HIPCHK(c, hipMemcpyAsync(S.hbuf.data(), sendL, 8 * n, hipMemcpyDeviceToHost, c->stream));
        if (S.has_right) HIPCHK(c, hipMemcpyAsync(S.hbuf.data() + n, sendR, 8 * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, stream_sync(c));
        if (c->host_ar(c->host_ar_user, S.hbuf.data(), 2 * n, 0, 100) != 0)
            return fail(c, PLFX_ERR_HIP, "host halo-exchange callback failed");
        if (S.has_left) HIPCHK(c, hipMemcpyAsync(recvL, S.hbuf.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
        if (S.has_right) HIPCHK(c, hipMemcpyAsync(recvR, S.hbuf.data() + n, 8 * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, stream_sync(c));
    }
    return 0;
}

// Stiffness generators of the halo elements: a strip sweeps (and holds the material state of) its OWNED element columns
// only; the six generators of the W halo columns on each interior side are received from the neighbour that owns them
// whenever a sweep rewrote a tangent anywhere (plfx_sweep calls sync_M on the all-reduced flag, so every rank takes part).
// Generator k of local element e = column * ny + row sits at Mel[k * nel_total + e]: a slab of W columns is contiguous.
//   to the left neighbour   my element columns oc0 .. oc0+W-1     from it   columns oc0-W .. oc0-1
//   to the right neighbour  my element columns oc1-W .. oc1-1     from it   columns oc1 .. oc1+W-1
int strip_sync_M(plfx_ctx *c)
{
    auto &S = c->strip;
    if (!S.on || !strip_coll(c)) return 0;
    const int ny = c->gy;
    const size_t n = (size_t)S.W * ny, tot = (size_t)c->nel_total;
    double *M = c->Mel;
    const size_t sL = (size_t)S.oc0 * ny, rL = (size_t)(S.oc0 - S.W) * ny, sR = (size_t)(S.oc1 - S.W) * ny, rR = (size_t)S.oc1 * ny;
    S.n_gen++;
    c->last_coll = "stiffness generators of the halo columns (ncclSend / ncclRecv with the strip neighbours)";
    c->n_coll++;
    if (c->comm) {
        if (!g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart || !g_rccl.GroupEnd)
            return fail(c, PLFX_ERR_UNSUPPORTED, "this RCCL has no ncclSend/ncclRecv");
        EvPair *ev;
        tim_begin(c, 7, &ev);
        int rc = g_rccl.GroupStart();
        for (int k = 0; k < 6 && !rc; k++) {
            if (S.has_left) {
                rc = g_rccl.Send(M + k * tot + sL, n, NCCL_FLOAT64, c->rank - 1, c->comm, c->stream);
                if (!rc) rc = g_rccl.Recv(M + k * tot + rL, n, NCCL_FLOAT64, c->rank - 1, c->comm, c->stream);
            }
            if (!rc && S.has_right) {
                rc = g_rccl.Send(M + k * tot + sR, n, NCCL_FLOAT64, c->rank + 1, c->comm, c->stream);
                if (!rc) rc = g_rccl.Recv(M + k * tot + rR, n, NCCL_FLOAT64, c->rank + 1, c->comm, c->stream);
            }
        }
        const int rc2 = g_rccl.GroupEnd();
        tim_end(c, ev);
        if (rc || rc2) return fail(c, PLFX_ERR_HIP, "generator halo exchange (ncclSend/ncclRecv) failed: %d / %d", rc, rc2);
        return 0;
    }
    if (c->host_ar) {  // host-staged transport: [6 slabs to the left | 6 slabs to the right] out, [from left | from right] back
        S.hbuf.assign(12 * n, 0.);
        for (int k = 0; k < 6; k++) {
            if (S.has_left) HIPCHK(c, hipMemcpyAsync(S.hbuf.data() + k * n, M + k * tot + sL, 8 * n, hipMemcpyDeviceToHost, c->stream));
            if (S.has_right) HIPCHK(c, hipMemcpyAsync(S.hbuf.data() + (6 + k) * n, M + k * tot + sR, 8 * n, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, stream_sync(c));
        if (c->host_ar(c->host_ar_user, S.hbuf.data(), 12 * n, 0, 100) != 0)
            return fail(c, PLFX_ERR_HIP, "host halo-exchange callback failed (generators)");
        for (int k = 0; k < 6; k++) {
            if (S.has_left) HIPCHK(c, hipMemcpyAsync(M + k * tot + rL, S.hbuf.data() + k * n, 8 * n, hipMemcpyHostToDevice, c->stream));
            if (S.has_right) HIPCHK(c, hipMemcpyAsync(M + k * tot + rR, S.hbuf.data() + (6 + k) * n, 8 * n, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, stream_sync(c));
    }
    return 0;
}


KOp make_op(const plfx_ctx *c, int nnode, int nslot, const int32_t *col, const double *val, int nx, int ny, int nel,
            const double *M, double rx, double ry)
{
    KOp o;
    o.rx = rx;
    o.ry = ry;
    o.nnode = nnode;
    o.nslot = nslot;
    o.col = col;
    o.val = val;
    o.nxn = nx + 1;
    o.nyn = ny + 1;
    o.nel = nel;
    o.M = M;
    o.tab = c->dtab;
    return o;
}

// The fine-level dinv that apply_bc_impl left unformed (plfx_ctx::dinv_late), in front of whoever reads its VALUES:
// k_dinv as apply_bc_impl would have launched it.  INVARIANT: between an apply_bc_impl and the solve it prepares nothing writes
// c->diag, so the launch here sees the (diag, is_presc) that one saw.  The writers of diag: assemble_fine_val calls this first;
// plfx_assemble's set-up pass and the speculative one behind a sweep's flags do NOT -- they clear dinv_ok, the next
// apply_bc_impl decides again, and a late dinv that was never read is simply superseded.  A solve that follows either of them
// WITHOUT an apply_bc in between therefore gets the dinv of the new diagonal where the parent had the old one's.
int ensure_dinv(plfx_ctx *c)
{
    if (!c->dinv_late) return 0;
    if (int rc = ensure_setup(c)) return rc;   // (c->diag may be owed as well)
    hipLaunchKernelGGL(k_dinv, dim3(grid_for(c->ndof)), dim3(BLOCK), 0, c->stream, (size_t)c->ndof, c->diag, c->is_presc, c->dinv);
    HIPCHK(c, hipGetLastError());
    c->dinv_late = false;
    c->n_dinv_late++;
    return 0;
}

// fine block-ELL values on demand (matrix-free runs only need them for plfx_get_csr)
int assemble_fine_val(plfx_ctx *c)
{
    if (int rc = ensure_dinv(c)) return rc;   // (k_assemble rewrites c->diag: a late dinv belongs to the diagonal as it is now)
    if (int rc = ensure_setup(c)) return rc;  // (... and an owed set-up pass must not overwrite k_assemble's diagonal later)
    if (int rc = ensure_live_M(c)) return rc;
    hipLaunchKernelGGL(k_assemble, dim3(grid_for(c->nnode), c->nslot), dim3(BLOCK), 0, c->stream,
                       c->dcls, c->ncls, c->nnode, c->nslot, c->nq, c->nel_total, c->dcontrib, c->dcls_all,
                       (matfree(c) && c->assembled) ? c->Mop : c->Mel, c->dcol, c->dval, c->diag,
                       (matfree(c) && c->assembled) ? 1 : 0);  // the snapshot is in pair layout, the live array SoA
    HIPCHK(c, hipGetLastError());
    c->dinv_ok = false;   // (c->diag rewritten)
    c->val_valid = true;
    return 0;
}

// level l >= 1 is applied from its generators (launched matrix-free, or inside the matrix-free tail): only its diagonal is
// formed, by k_grid_setup; every other level >= 1 is assembled, diagonal included, by k_assemble
static bool level_from_generators(const plfx_ctx *c, int l)
{
    return matfree(c) && (c->mg[l].matfree || (tail_mf(c) && l < (int)c->mg.size() - 1));
}

// coarse operators: restrict M level by level and re-assemble (called after the fine assembly)
int mg_assemble(plfx_ctx *c)
{
    const bool mf = matfree(c);
    const int nl = (int)c->mg.size();
    if (int rc = ensure_setup(c)) return rc;   // (the generators of level 1 come from the fine level's pass)
    // the matrix-free levels get their Jacobi scaling with the known Dirichlet mask (taken straight from the finest grid: the
    // node lines of every level, the last one included, coincide with node lines of the finest grid)
    c->mg_dinv_current = mf && c->bc_valid;
    for (int l = 1; l < nl; l++) {
        auto &F = c->mg[l - 1];
        auto &L = c->mg[l];
        // (otherwise the parent's setup kernel has already produced this level's generators -- parents that halve exactly only)
        if (!(mf && (F.matfree || tail_mf(c))) || !level_plain(F))
            hipLaunchKernelGGL(k_mg_coarsen_M, dim3(grid_for(L.nel)), dim3(BLOCK), 0, c->stream, L.nx, L.ny, F.ny,
                               F.nel, (l == 1 && mf) ? c->mg[0].op.M : F.Mel, L.Mel, mf ? 1 : 0, mf ? 1 : 0, F.rx, F.ry);  // matrix-free mode: pair
                               // layout on every level >= 1 and in the snapshot of level 0 (the live array of level 0 is SoA)
        const bool setup_mf = level_from_generators(c, l);  // coarsest: assembled for the dense inverse
        if (setup_mf)  // only the diagonal (Jacobi smoother) is needed
            LAUNCH_SETUP(1, L.op, (double2 *)L.diag,
                               (double *)nullptr, (l + 1 < nl && level_plain(L)) ? c->mg[l + 1].Mel : (double *)nullptr,
                               (const double2 *)c->dinv, c->mg[0].ny + 1, l,
                               c->mg_dinv_current ? (double2 *)L.dinv : (double2 *)nullptr, c->mg[0].nx + 1);
        else
            hipLaunchKernelGGL(k_assemble, dim3(grid_for(L.nnode), L.nslot), dim3(BLOCK), 0, c->stream, L.cls4 ? L.cls4 : c->mg_cls,
                               L.cls4 ? 4 : 1, L.nnode, L.nslot, L.nq, L.nel, L.contrib, L.cls0, L.Mel, L.col, L.val, L.diag, mf ? 1 : 0);
    }
    HIPCHK(c, hipGetLastError());
    c->mg_inv_valid = false;
    return 0;
}

// Dirichlet masks / Jacobi scalings of the coarse levels from the fine dinv (called by apply_bc)
int mg_update_dinv(plfx_ctx *c, bool same_set)
{
    for (size_t l = 1; l < c->mg.size(); l++) {
        auto &F = c->mg[l - 1];
        auto &L = c->mg[l];
        if (same_set && c->mg_dinv_current && matfree(c) && (L.matfree || (tail_mf(c) && l + 1 < c->mg.size())))
            continue;  // written by mg_assemble already
        hipLaunchKernelGGL(k_mg_coarse_dinv, dim3(grid_for(L.nnode)), dim3(BLOCK), 0, c->stream, L.nx + 1,
                           L.ny + 1, F.ny + 1, (const double2 *)F.dinv, (const double2 *)L.diag,
                           (double2 *)L.dinv, F.nx + 1, F.rx, F.ry);
    }
    auto &Lc = c->mg.back();
    if (Lc.ainv && !(c->mg_inv_valid && same_set)) {
        const int n = 2 * Lc.nnode;
        hipLaunchKernelGGL(k_mg_coarse_invert, dim3(1), dim3(BLOCK), (size_t)n * n * sizeof(double), c->stream,
                           Lc.nnode, Lc.nslot, Lc.col, Lc.val, (const double2 *)Lc.dinv, Lc.ainv);
        c->mg_inv_valid = true;
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// smoothing sweeps of level l: mg_nu everywhere; experiment knob PLFX_MG_NU_COARSE=n: n sweeps on the launch-latency-bound
// levels >= 2 that are launched kernel by kernel (fewer launches per cycle, weaker smoothing there; not with strips, whose
// halo validity analysis assumes V(2,2))
inline int level_nu(const plfx_ctx *c, int l)
{
    static const int nc = getenv("PLFX_MG_NU_COARSE") ? atoi(getenv("PLFX_MG_NU_COARSE")) : 0;
    return (nc > 0 && l >= 2 && !c->strip.on) ? nc : c->mg_nu;
}

// z = V(nu,nu)-cycle applied to r  (level-0 x aliases z, b aliases r)
// one level of the down leg: nu pre-smoothing sweeps from a zero guess, residual, restriction to level l+1
int mg_down_level(plfx_ctx *c, int l)
{
    const double om = c->mg_omega;
    auto &L = c->mg[l];
    auto &C = c->mg[l + 1];
    const bool mf = L.matfree && matfree(c);
    const int nu = level_nu(c, l);
    EvPair *ev = nullptr;
    (void)ev;  // the head of the cycle is enqueued speculatively (may return at once): family 5 times the post-smoothing
               // launches of k_mg_smooth<1, .> only
    const bool march = l == 0 && mf && march_mg(c);
    if (nu == 2) {  // both sweeps in one pass over the operator
        if (march)
            hipLaunchKernelGGL(k_mg_smooth2_zero_march, dim3(L.grid), dim3(BLOCK), 0, c->stream, L.op, (const double2 *)L.dinv,
                               (const double2 *)L.b, (double2 *)L.x, om, c->sc);
        else if (l == 0)
            LAUNCH_OP2(k_mg_smooth2_zero, 1, mf, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                       (double2 *)L.x, om, c->sc);
        else
            LAUNCH_OP2R(k_mg_smooth2_zero, 0, mf, L.op, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                       (double2 *)L.x, om, c->sc);
    } else {
        double *src = nullptr, *dst = (nu & 1) ? L.x : L.t;
        for (int k = 0; k < nu; k++) {
            if (l == 0)
                LAUNCH_OP2(k_mg_smooth, 1, mf, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                           (const double2 *)src, (double2 *)dst, om, k == 0, c->sc);
            else
                LAUNCH_OP2R(k_mg_smooth, 0, mf, L.op, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                           (const double2 *)src, (double2 *)dst, om, k == 0, c->sc);
            src = dst;
            dst = (dst == L.x) ? L.t : L.x;
        }
    }
    if (march)
        hipLaunchKernelGGL(k_mg_residual_march, dim3(L.grid), dim3(BLOCK), 0, c->stream, L.op, (const double2 *)L.dinv,
                           (const double2 *)L.b, (const double2 *)L.x, (double2 *)L.res, c->sc);
    else if (l == 0)
        LAUNCH_OP2(k_mg_residual, 1, mf, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                   (const double2 *)L.x, (double2 *)L.res, c->sc);
    else
        LAUNCH_OP2R(k_mg_residual, 0, mf, L.op, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                   (const double2 *)L.x, (double2 *)L.res, c->sc);
    hipLaunchKernelGGL(k_mg_restrict, dim3(grid_for(C.nnode)), dim3(BLOCK), 0, c->stream, C.nx + 1, C.ny + 1,
                       L.nx + 1, L.ny + 1, (const double2 *)L.res, (const double2 *)C.dinv, (double2 *)C.b, L.rx, L.ry,
                       l == 0 ? (const CgScalars *)c->sc : (const CgScalars *)nullptr);
    return 0;
}

// one level of the up leg: prolongation from level l+1, nu post-smoothing sweeps.  rz_part (level 0, may be null): the last
// post-smoothing launch writes the r.z partials there if it can, and *wrote says whether it did
int mg_up_level(plfx_ctx *c, int l, double *rz_part, bool *wrote)
{
    const double om = c->mg_omega;
    auto &L = c->mg[l];
    auto &C = c->mg[l + 1];
    const bool mf = L.matfree && matfree(c);
    const int nu = level_nu(c, l);
    hipLaunchKernelGGL(k_mg_prolong_add, dim3(grid_for(L.nnode)), dim3(BLOCK), 0, c->stream, L.nx + 1, L.ny + 1,
                       C.ny + 1, (const double2 *)C.x, (const double2 *)L.dinv, (double2 *)L.x, L.rx, L.ry);
    double *src = L.x, *dst = L.t;
    for (int k = 0; k < nu; k++) {
        EvPair *ev = nullptr;
        if (l == 0) tim_begin(c, 5, &ev);  // family 5: fine-level smoother launches
        DotOut dot{};
        if (l == 0 && k == nu - 1 && rz_part && !(nu & 1) && L.grid <= c->grid_nodes) {  // (even nu: the last launch writes L.x = z)
            dot.part = rz_part;
            dot.nslots = c->grid_nodes;
            dot.own_lo = own_lo(c);
            dot.own_hi = own_hi(c);
            *wrote = true;  // (otherwise the caller launches k_dot_rz itself)
        }
        if (l == 0 && mf && march_mg(c))
            hipLaunchKernelGGL(k_mg_smooth_march, dim3(L.grid), dim3(BLOCK), 0, c->stream, L.op, (const double2 *)L.dinv,
                               (const double2 *)L.b, (const double2 *)src, (double2 *)dst, om, c->sc, dot);
        else if (l == 0)
            LAUNCH_OP2(k_mg_smooth, 1, mf, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                       (const double2 *)src, (double2 *)dst, om, 0, c->sc, dot);
        else
            LAUNCH_OP2R(k_mg_smooth, 0, mf, L.op, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                       (const double2 *)src, (double2 *)dst, om, 0, c->sc);
        if (l == 0) tim_end(c, ev);
        std::swap(src, dst);
    }
    if (src != L.x)  // odd nu: result sits in t
        HIPCHK(c, hipMemcpyAsync(L.x, L.t, (size_t)L.nnode * 16, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// which single-workgroup kernel runs the levels >= lt of a cycle (PLFX_MG_TAIL_*; NONE: the coarsest level alone, by a launch
// of its own).  mg_coarse_part launches by it and plfx_mg_info reports it.
int mg_tail_kernel(const plfx_ctx *c)
{
    const int nl = (int)c->mg.size();
    const int lt = (c->mg_tail > 0) ? c->mg_tail : nl - 1;
    if (!(lt < nl - 1)) return PLFX_MG_TAIL_NONE;
    if (tail_mf(c)) {
        bool ragged = false;   // some level of the tail is not "all cells alike, halving exactly" (hierarchy of an odd-sized mesh)
        for (int l = lt; l < nl - 1; l++) ragged = ragged || !level_plain(c->mg[l]);
        return ragged ? PLFX_MG_TAIL_MF_RAGGED : PLFX_MG_TAIL_MF;
    }
    if (c->mg_tail_T > 0 && c->mg_nu == 2) return PLFX_MG_TAIL_LDS;
    return PLFX_MG_TAIL_GENERIC;
}

// levels 1 .. coarsest: every kernel here is launch-latency bound (<= 513^2 nodes)
int mg_coarse_part(plfx_ctx *c)
{
    const int nl = (int)c->mg.size();
    const double om = c->mg_omega;
    const int lt = (c->mg_tail > 0) ? c->mg_tail : nl - 1;  // levels >= lt run inside one workgroup
    int rc;
    if (c->strip.on && c->want_mg_graph && lt >= 2) {
        // strip: the collective of the coarse hand-over sits in the middle of the cycle, so the latency-bound launches of the
        // local levels are replayed from two graphs, one on each side of it
        auto &S = c->strip;
        for (int leg = 0; leg < 2; leg++) {
            hipGraphExec_t &x = leg ? S.x_up : S.x_down;
            if (!x) {
                hipGraph_t &g = leg ? S.g_up : S.g_down;
                HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
                rc = 0;
                if (leg == 0)
                    for (int l = 1; l < lt && !rc; l++) rc = mg_down_level(c, l);
                else
                    for (int l = lt - 1; l >= 1 && !rc; l--) rc = mg_up_level(c, l, nullptr, nullptr);
                const hipError_t e = hipStreamEndCapture(c->stream, &g);
                if (rc) return rc;
                if (e != hipSuccess || !g) return fail(c, PLFX_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
                HIPCHK(c, hipGraphInstantiate(&x, g, nullptr, nullptr, 0));
            }
            HIPCHK(c, hipGraphLaunch(x, c->stream));
            if (leg == 0 && (rc = strip_coarse(c))) return rc;
        }
        return 0;
    }
    for (int l = 1; l < lt; l++)
        if ((rc = mg_down_level(c, l))) return rc;
    if (c->strip.on) {  // level Ld and everything below it: the replicated coarse problem of the whole grid
        if ((rc = strip_coarse(c))) return rc;
    } else {
        auto &L = c->mg[nl - 1];
        const size_t lds = (size_t)L.nnode * 4 * sizeof(double2);
        const int tail = mg_tail_kernel(c);
        if (tail == PLFX_MG_TAIL_MF_RAGGED)
            hipLaunchKernelGGL(k_mg_tail_mf<true>, dim3(1), dim3(MG_TAIL_BLOCK), c->mg_tail_lds,
                               c->stream, c->mg_dev, lt, nl, c->mg_tail_T, c->mg_tail_E, c->dtab, om, c->sc);
        else if (tail == PLFX_MG_TAIL_MF)
            hipLaunchKernelGGL(k_mg_tail_mf<false>, dim3(1), dim3(MG_TAIL_BLOCK), c->mg_tail_lds,
                               c->stream, c->mg_dev, lt, nl, c->mg_tail_T, c->mg_tail_E, c->dtab, om, c->sc);
        else if (tail == PLFX_MG_TAIL_LDS)
            hipLaunchKernelGGL(k_mg_tail_lds, dim3(1), dim3(MG_TAIL_BLOCK),
                               (size_t)c->mg_tail_T * (4 * sizeof(double2) + 9 * sizeof(int)), c->stream, c->mg_dev,
                               lt, nl, c->mg_tail_T, om, c->sc);
        else if (tail == PLFX_MG_TAIL_GENERIC)
            hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(MG_TAIL_BLOCK), lds, c->stream, c->mg_dev, lt, nl, om,
                               c->mg_nu, c->sc);
        else if (L.ainv)
            hipLaunchKernelGGL(k_mg_coarse_dense, dim3(1), dim3(BLOCK), 0, c->stream, L.nnode, L.ainv,
                               (const double2 *)L.b, (double2 *)L.x, c->sc);
        else if (c->mg_cheby > 0) {
            // eigenvalues of D^-1 K assumed in [bmax / kappa, bmax]; bmax = 3 bounds the Q4 elasticity operator with
            // room (damped Jacobi with omega = 0.9 diverges, 0.65 does not: 2.2 < lambda_max < 3.1)
            const bool mf = L.matfree && matfree(c);
            const int m = c->mg_cheby;
            const double bmax = 3.0, amin = bmax / c->mg_cheby_kappa;
            const double theta = 0.5 * (bmax + amin), delta = 0.5 * (bmax - amin), sigma = theta / delta;
            double rho = 1. / sigma;
            double *cur = (m & 1) ? L.x : L.t, *oth = (m & 1) ? L.t : L.x;  // the m-th result lands in L.x
            LAUNCH_OP1R(k_mg_cheby, mf, L.op, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                       (const double2 *)nullptr, (double2 *)cur, (double2 *)L.res, 0., 1. / theta, 1, c->sc);
            for (int k = 1; k < m; k++) {
                const double rho_new = 1. / (2. * sigma - rho);
                LAUNCH_OP1R(k_mg_cheby, mf, L.op, dim3(L.grid), L.op, (const double2 *)L.dinv, (const double2 *)L.b,
                           (const double2 *)cur, (double2 *)oth, (double2 *)L.res, rho_new * rho, 2. * rho_new / delta, 0,
                           c->sc);
                std::swap(cur, oth);
                rho = rho_new;
            }
        }
        else
            hipLaunchKernelGGL(k_mg_coarse_solve, dim3(1), dim3(BLOCK), lds, c->stream, L.nnode, L.nslot, L.col,
                               L.val, (const double2 *)L.dinv, (const double2 *)L.b, (double2 *)L.x,
                               4 * L.nnode + 20, 1.e-10, c->sc);
    }
    for (int l = lt - 1; l >= 1; l--)
        if ((rc = mg_up_level(c, l, nullptr, nullptr))) return rc;
    return 0;
}

void mg_graph_drop(plfx_ctx *c)
{
    if (c->mg_graph_exec) hipGraphExecDestroy(c->mg_graph_exec);
    if (c->mg_graph) hipGraphDestroy(c->mg_graph);
    c->mg_graph_exec = nullptr;
    c->mg_graph = nullptr;
    auto &S = c->strip;
    if (S.x_down) hipGraphExecDestroy(S.x_down);
    if (S.x_up) hipGraphExecDestroy(S.x_up);
    if (S.g_down) hipGraphDestroy(S.g_down);
    if (S.g_up) hipGraphDestroy(S.g_up);
    S.x_down = S.x_up = nullptr;
    S.g_down = S.g_up = nullptr;
}

// z = V(nu,nu)-cycle applied to r  (level-0 x aliases z, b aliases r).  The fine level is launched kernel by kernel
// (its launches are timed for the roofline); the ~35 small launches of all coarser levels are captured once into a
// hipGraph and replayed (arguments are constant for a hierarchy: pointers, omega, nu).
// The cycle in two parts so that plfx_solve can enqueue the head (fine-level pre-smoothing, residual, restriction: 60 us
// of work whose kernels return at once if the PCG flag says "converged") BEFORE it waits for that flag: the round trip
// to the host is hidden behind the head instead of idling the GPU.
// Coarse levels on demand (round 5): plfx_assemble only marks them stale when the two-solution initial guess is on -- on a
// steady workload most tangent-update solves then start below the tolerance and never apply the preconditioner, and the ~70 us of
// the coarse set-up (8 launch-bound level passes + the coarsest assembly and its dense inverse) were spent for nothing.  Whoever
// is about to run a V-cycle calls mg_ensure first.  Single GPU (a strip sets its child context up in lock-step with the others).
bool mg_lazy(const plfx_ctx *c) { return c->predict && matfree(c) && !c->strip.on && !comm_active(c); }
int mg_ensure(plfx_ctx *c)
{
    int rc = ensure_dinv(c);   // (a V-cycle follows: the smoothers and k_mg_coarse_dinv read the fine level's values)
    if (rc) return rc;
    if (!c->mg_pending) return 0;
    c->mg_pending = false;
    c->n_mg_setup++;
    rc = mg_assemble(c);
    if (rc) return rc;
    return mg_update_dinv(c, c->mg_pending_same);
}

int mg_vcycle_head(plfx_ctx *c)
{
    if (c->strip_jacobi) return 0;
    const int nl = (int)c->mg.size();
    const int lt = (c->mg_tail > 0) ? c->mg_tail : nl - 1;
    if (lt >= 1) return mg_down_level(c, 0);
    return 0;
}

// INVARIANT: only the finest level's kernels test sc->done.  The levels >= 1, the hipGraph replay and a strip's
// child context (which shares c->sc) must therefore never be enqueued speculatively or while the flag is sticky: every caller
// of mg_vcycle_rest has either seen done == 0 from cg_check_wait or has just cleared it (k_cg_setup, plfx_precond_bench).
// rz_part (may be null): where the last fine-level post-smoothing launch writes the r.z partials if it can; *wrote: whether it did
int mg_vcycle_rest(plfx_ctx *c, double *rz_part, bool *wrote)
{
    if (c->strip_jacobi) {  // Jacobi fall-back of a strip: same PCG loop, same exchanges, z = D^-1 r on the local grid
        launch_jacobi_z(c);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    const int nl = (int)c->mg.size();
    const int lt = (c->mg_tail > 0) ? c->mg_tail : nl - 1;
    int rc;
    if (lt < 1) {  // two-level hierarchy without a separate fine leg
        if ((rc = mg_coarse_part(c))) return rc;
    } else if (c->want_mg_graph && lt >= 2 && !c->strip.on) {  // (collectives inside the strip's cycle are not captured)
        if (!c->mg_graph_exec) {
            HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
            rc = mg_coarse_part(c);
            hipGraph_t g = nullptr;
            hipError_t e = hipStreamEndCapture(c->stream, &g);
            if (rc) return rc;
            if (e != hipSuccess || !g) return fail(c, PLFX_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
            c->mg_graph = g;
            HIPCHK(c, hipGraphInstantiate(&c->mg_graph_exec, g, nullptr, nullptr, 0));
        }
        HIPCHK(c, hipGraphLaunch(c->mg_graph_exec, c->stream));
    } else {
        if ((rc = mg_coarse_part(c))) return rc;
    }
    if (lt >= 1) {
        if ((rc = mg_up_level(c, 0, rz_part, wrote))) return rc;
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

int mg_vcycle(plfx_ctx *c)
{
    int rc = mg_ensure(c);
    if (rc) return rc;
    rc = mg_vcycle_head(c);
    if (rc) return rc;
    return mg_vcycle_rest(c, nullptr, nullptr);
}


// ---------------------------------------------------------------------------------------------- strip: coarse problem
// window of the local level-Ld grid inside the global one: owned node columns [jc0, jc1) (the last rank owns the closing
// column), owned element columns [ec0, ec1), global column of local column 0
struct StripWin {
    int jc0, jc1, ec0, ec1, g0;
};
StripWin strip_window(const plfx_ctx *c)
{
    const auto &S = c->strip;
    StripWin w;
    w.jc0 = S.oc0 >> S.Ld;
    w.jc1 = (S.oc1 >> S.Ld) + (S.has_right ? 0 : 1);
    w.ec0 = S.oc0 >> S.Ld;
    w.ec1 = S.oc1 >> S.Ld;
    w.g0 = S.gcol0 >> S.Ld;
    return w;
}

// z_Ld = (V-cycle of the global hierarchy below level Ld)(b_Ld): the owned part of the local level-Ld right-hand side is
// placed into the zero-filled global vector, ONE all-reduce completes it on every rank, every rank runs the same cycle
// (launch-latency-bound kernels, as on one GPU) and takes its window of the correction -- valid on ALL local columns.
int strip_coarse(plfx_ctx *c)
{
    auto &S = c->strip;
    plfx_ctx *k = S.child;
    auto &L = c->mg[S.Ld];
    const StripWin w = strip_window(c);
    const size_t nyc = L.ny + 1;
    const size_t nd = (size_t)2 * k->nnode;
    hipLaunchKernelGGL(k_strip_pack, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, 1, nd, (size_t)2 * L.nnode,
                       (size_t)2 * (w.g0 + w.jc0) * nyc, (size_t)2 * (w.jc1 - w.jc0) * nyc, (size_t)2 * w.jc0 * nyc,
                       (const double *)L.b, k->r);
    HIPCHK(c, hipGetLastError());
    if (strip_coll(c)) {
        S.n_coarse++;
        const int rc = allreduce(c, k->r, nd, NCCL_FLOAT64, NCCL_SUM, "coarse right-hand side");
        if (rc) return rc;
    }
    int rc = mg_vcycle(k);
    if (rc) {
        c->err = k->err;
        return rc;
    }
    HIPCHK(c, hipMemcpyAsync(L.x, k->z + (size_t)2 * w.g0 * nyc, (size_t)16 * L.nnode, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// generators of level Ld of the whole grid (owned columns of every rank, one all-reduce), then the coarse context's
// own "setupK": diagonal, snapshot, generators of its coarser levels
int strip_child_assemble(plfx_ctx *c)
{
    auto &S = c->strip;
    plfx_ctx *k = S.child;
    auto &L = c->mg[S.Ld];
    const StripWin w = strip_window(c);
    // pair layout on both sides: three arrays of (2 doubles per element); element columns are contiguous, so is the window
    const size_t tot = (size_t)6 * k->nel_total;
    hipLaunchKernelGGL(k_strip_pack, dim3(grid_for(tot)), dim3(BLOCK), 0, c->stream, 3, (size_t)2 * k->nel_total, (size_t)2 * L.nel,
                       (size_t)2 * (w.g0 + w.ec0) * L.ny, (size_t)2 * (w.ec1 - w.ec0) * L.ny, (size_t)2 * w.ec0 * L.ny,
                       (const double *)L.Mel, k->Mel);
    HIPCHK(c, hipGetLastError());
    if (strip_coll(c)) {
        const int rc = allreduce(c, k->Mel, tot, NCCL_FLOAT64, NCCL_SUM, "coarse generators");
        if (rc) return rc;
    }
    KOp live = k->op;
    live.M = k->Mel;
    LAUNCH_SETUP(1, live, (double2 *)k->diag, k->Mop,
                       k->mg[1].Mel, (const double2 *)nullptr, 0, 0, (double2 *)nullptr);
    HIPCHK(c, hipGetLastError());
    k->bc_valid = false;  // its Jacobi scalings / Dirichlet masks follow in strip_child_dinv (after the parent's calc_BC)
    const int rc = mg_assemble(k);
    if (rc) c->err = k->err;
    return rc;
}

// Dirichlet mask + Jacobi scaling of level Ld of the whole grid from the owned columns of every rank, then the coarser ones
int strip_child_dinv(plfx_ctx *c)
{
    auto &S = c->strip;
    plfx_ctx *k = S.child;
    auto &L = c->mg[S.Ld];
    const StripWin w = strip_window(c);
    const size_t nyc = L.ny + 1;
    const size_t nd = (size_t)2 * k->nnode;
    hipLaunchKernelGGL(k_strip_pack, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, 1, nd, (size_t)2 * L.nnode,
                       (size_t)2 * (w.g0 + w.jc0) * nyc, (size_t)2 * (w.jc1 - w.jc0) * nyc, (size_t)2 * w.jc0 * nyc,
                       (const double *)L.dinv, k->dinv);
    HIPCHK(c, hipGetLastError());
    if (strip_coll(c)) {
        const int rc = allreduce(c, k->dinv, nd, NCCL_FLOAT64, NCCL_SUM, "coarse Jacobi scaling");
        if (rc) return rc;
    }
    k->mg_inv_valid = false;
    const int rc = mg_update_dinv(k, false);
    if (rc) c->err = k->err;
    return rc;
}

void strip_free(plfx_ctx *c)
{
    mg_graph_drop(c);  // the strip's captured launches reference the levels freed below
    plfx_ctx *k = c->strip.child;
    if (k) {
        mg_graph_drop(k);
        dfree(k->Mel);
        dfree(k->Mop);
        dfree(k->diag);
        dfree(k->dinv);
        dfree(k->r);
        dfree(k->z);
        for (auto &L : k->mg) {
            if (L.owned) {
                dfree(L.col); dfree(L.contrib); dfree(L.cls0); dfree(L.val); dfree(L.diag); dfree(L.dinv);
                dfree(L.Mel); dfree(L.x); dfree(L.b);
            }
            dfree(L.t); dfree(L.res); dfree(L.ainv); dfree(L.cls4);
        }
        dfree(k->mg_cls);
        dfree(k->mg_dev);
        delete k;  // stream, sc and dtab belong to the parent
    }
    c->strip = plfx_ctx::Strip();
}

// the mode goes off and stays off until the next plfx_state_reset (the first reason is the one reported)
void plane_off(plfx_ctx *c, int why)
{
    if (c->plane_cols) c->plane_off_by = why;
    c->plane_cols = false;
}

// ---- launches of this unit's kernels on behalf of the step and solve units (one owner per kernel)
void launch_jacobi_z(plfx_ctx *c)
{
    hipLaunchKernelGGL(k_jacobi_z, dim3(grid_for(c->nnode)), dim3(BLOCK), 0, c->stream, c->nnode, (const double2 *)c->dinv,
                       (const double2 *)c->r, (double2 *)c->z, c->sc);
}

void launch_mbox_post(plfx_ctx *c, const double *src, int n, double *dst, CgMbox *mb, unsigned long long seq)
{
    hipLaunchKernelGGL(k_mbox_post, dim3(1), dim3(BLOCK), 0, c->stream, src, n, dst, mb, seq);
}

void launch_kdu_uf(plfx_ctx *c, CgScalars *spec)
{
    LAUNCH_OP2(k_spmv, 3, matfree(c), dim3(c->grid_nodes), c->op, 0, c->nnode, (const double2 *)c->du, nullptr, (double2 *)c->u,
               (double2 *)c->f, nullptr, nullptr, nullptr, 0, nullptr, spec, 0, 0, 0);
}

void launch_spec_setup(plfx_ctx *c)
{
    KOp live = c->op;
    live.M = c->Mel;
    LAUNCH_SETUP(0, live, (double2 *)c->diag,
                       c->Mop, (mg_active(c) && level_plain(c->mg[0])) ? c->mg[1].Mel : (double *)nullptr, (const double2 *)nullptr, 0, 0,
                       (double2 *)nullptr, 0x7fffffff, (const int *)(c->flags + 8));
}

// a direct sweep left its new generators in the snapshot alone; the live array gets them back in front of whoever
// reads it or writes part of it
int ensure_live_M(plfx_ctx *c)
{
    if (!c->live_owed) return 0;
    hipLaunchKernelGGL(k_restore_M, dim3(grid_for((size_t)c->nel_total, 1 << 16)), dim3(BLOCK), 0, c->stream, (size_t)c->nel_total,
                       (const double2 *)c->Mop, c->Mel);
    HIPCHK(c, hipGetLastError());
    c->live_owed = false;
    c->n_live_restored++;
    return 0;
}

// the set-up pass that a direct sweep left out, in front of whoever reads c->diag or the generators of level 1 --
// and of whoever writes part of the live array, which this pass reads (before_M_write).  The pass plfx_assemble launches, on
// generators that are what they were when it was owed: it rewrites the snapshot with equal values.
int ensure_setup(plfx_ctx *c)
{
    if (!c->setup_owed) return 0;
    if (int rc = ensure_live_M(c)) return rc;
    KOp live = c->op;
    live.M = c->Mel;
    LAUNCH_SETUP(0, live, (double2 *)c->diag,
                       c->Mop, (mg_active(c) && level_plain(c->mg[0])) ? c->mg[1].Mel : (double *)nullptr, (const double2 *)nullptr, 0, 0,
                       (double2 *)nullptr);
    HIPCHK(c, hipGetLastError());
    c->setup_owed = false;
    c->n_setup_late++;
    return 0;
}

int before_M_write(plfx_ctx *c)
{
    c->direct_done = false;   // (a sweep's changed tangents are not the last word on the generators: plfx_assemble launches its pass)
    if (int rc = ensure_setup(c)) return rc;
    return ensure_live_M(c);
}

// A call that re-shapes what plfx_assemble builds: the live generators whole, nothing owed, and the next assembly a full one
static int snap_settle(plfx_ctx *c)
{
    if (int rc = ensure_live_M(c)) return rc;
    c->direct_done = c->setup_owed = false;
    c->M_dirty = true;
    return 0;
}

}  // namespace host
}  // namespace plfx

extern "C" {

const char *plfx_version(void) { return PLFX_VERSION; }

int plfx_create(int device, plfx_ctx **out)
{
    if (!out) return PLFX_ERR_ARG;
    *out = nullptr;
    plfx_ctx *c = new plfx_ctx();
    *out = c;  // returned even on failure so that plfx_last_error works
    c->device = device;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(c, PLFX_ERR_HIP, "no HIP device available (%s); libplfx has no CPU fallback",
                    hipGetErrorString(e));
    HIPCHK(c, hipSetDevice(device));
    HIPCHK(c, hipGetDeviceProperties(&c->prop, device));
    HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (const char *e2 = getenv("PLFX_MATFREE")) c->want_matfree = atoi(e2) ? 1 : 0;
    if (const char *e3 = getenv("PLFX_SVC_WAVE")) c->want_svc_wave = atoi(e3) ? 1 : 0;
    if (const char *e4 = getenv("PLFX_COLL_TIMEOUT")) c->coll_timeout_s = atof(e4);
    if (const char *e4 = getenv("PLFX_MG_GRAPH")) c->want_mg_graph = atoi(e4) ? 1 : 0;
    if (const char *e8 = getenv("PLFX_REUSE")) c->reuse = atoi(e8) != 0;
    if (const char *e9 = getenv("PLFX_BC_ROWS")) c->bc_rows_on = atoi(e9) != 0;
    if (const char *e10 = getenv("PLFX_DEAD_STORES")) {   // 0: off, 1: on; 2 / 3: the sweeps / the starts alone (to measure them apart)
        const int v = atoi(e10);
        c->dead_stores = v == 1 || v == 2;
        c->test_starts = v == 1 || v == 3;
    }
    if (!c->reuse) c->dead_stores = c->test_starts = false;
    if (const char *e11 = getenv("PLFX_PLANE_COLS")) c->plane_switch = atoi(e11) != 0;
    if (!c->reuse) c->plane_switch = false;
    if (const char *e12 = getenv("PLFX_SHORT_SOLVE")) c->short_solve = atoi(e12) & 3;
    if (!c->reuse) c->short_solve = 0;
    if (const char *e14 = getenv("PLFX_NODE_CODE")) c->node_code = atoi(e14) & 3;
    if (!(c->node_code & 1) || !c->reuse) c->node_code = 0;   // (the sparse b needs the mask)
    if (const char *e13 = getenv("PLFX_DIRECT_SNAP")) c->direct_snap = atoi(e13) & 3;
    if (!(c->direct_snap & 1) || !c->reuse) c->direct_snap = 0;   // (B needs A)
    if (const char *e9 = getenv("PLFX_PREDICT")) c->predict = atoi(e9) != 0;
    {
        const char *e5 = getenv("PLFX_MAILBOX");
        if (!e5 || atoi(e5)) {
            if (hipHostMalloc((void **)&c->mbox, sizeof(CgMbox), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess)
                memset(c->mbox, 0, sizeof(CgMbox));
            else
                c->mbox = nullptr;
            c->mb_cap = 1 << 16;  // 512 KB of results per call (boundary gathers of meshes up to ~8000 x 8000)
            if (c->mbox && hipHostMalloc((void **)&c->mb_buf, (size_t)8 * c->mb_cap,
                                         hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
                c->mb_buf = nullptr;
                c->mb_cap = 0;
            }
        }
    }
    // 160 KiB LDS per CU on gfx950; leave room for the static material/class tables
    size_t lds = std::max((size_t)c->prop.sharedMemPerBlock, (size_t)c->prop.maxSharedMemoryPerMultiProcessor);
    lds = std::min(lds, (size_t)160 * 1024);
    const size_t reserve = sizeof(MatDev) * MAXMAT + sizeof(ClassDev) * MAXCLS + 1024;
    c->lds_doubles = lds > reserve ? (int)((lds - reserve) / 8) : 0;
    int rc;
    if ((rc = dalloc(c, &c->part, (size_t)8 * MAXPART))) return rc;
    if ((rc = dalloc(c, &c->part_g, (size_t)18 * SUMPART))) return rc;
    if ((rc = dalloc(c, &c->sc, 1))) return rc;
    if ((rc = dalloc(c, &c->flags, 16))) return rc;  // [0..3] working flags of a sweep, [4..7] its results (k_sweep_flags), [8] skip flag of the speculative set-up
    if ((rc = dalloc(c, &c->spec_sc, 1))) return rc;
    if ((rc = dalloc(c, &c->bflags, (size_t)2 * SWEEP_SLOTS))) return rc;
    if ((rc = dalloc(c, &c->small, 64))) return rc;
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

void plfx_destroy(plfx_ctx *c)
{
    if (!c) return;
    if (c->stream) stream_sync(c);
#ifdef PLFX_PROF_REGIONS
    {
        unsigned long long h[16] = {0};
        // (g_prof is a device variable per unit: the copies of the two units whose kernels hold regions)
        if (prof_regions_add_step(h) && prof_regions_add_material(h) && h[7]) {
            static const char *nm[8] = {"fgrad", "plain", "ray_sample pass", "ray_sample post", "march", "brentq", "full() in corrector", "corrector loop"};
            for (int i = 0; i < 8; i++) fprintf(stderr, "[prof] %-22s %14llu ticks  %5.1f %% of the corrector loop\n", nm[i], h[i], 100. * h[i] / h[7]);
            fprintf(stderr, "[prof] rows: ray searches %llu, direct evaluations %llu (no polynomial %llu, outside its interval %llu, inside the margin %llu), of the outside ones: below lo %llu, at brentq iterates %llu, at the start point %llu\n",
                    h[8], h[9], h[10], h[11], h[12], h[13], h[14], h[15]);
        }
    }
#endif
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    for (auto &e : c->tim.ring) {
        hipEventDestroy(e.a);
        hipEventDestroy(e.b);
    }
    free_mesh(c);
    free_materials(c);
    dfree(c->tex_sv);
    dfree(c->tex_dual);
    dfree(c->part);
    dfree(c->part_g);
    dfree(c->sc);
    dfree(c->flags);
    dfree(c->spec_sc);
    dfree(c->bflags);
    dfree(c->small);
    dfree(c->idx_tmp);
    dfree(c->val_tmp);
    if (c->stage) hipHostFree(c->stage);
    for (int h = 0; h < 2; h++)
        if (c->stage_ev[h]) hipEventDestroy(c->stage_ev[h]);
    dfree(c->bc_idx_dev);
    dfree(c->plan.seg4);
    dfree(c->bc_rows);
    dfree(c->kw);
    dfree(c->fin_idx);
    dfree(c->fin_dev);
    if (c->fin_host) hipHostFree(c->fin_host);
    for (int q = 0; q < 2; q++) {
        if (c->fin_pin[q]) hipHostFree(c->fin_pin[q]);
        if (c->fin_box[q]) hipHostFree(c->fin_box[q]);
    }
    if (c->mbox) hipHostFree(c->mbox);
    if (c->mb_buf) hipHostFree(c->mb_buf);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char *plfx_last_error(plfx_ctx *c) { return c ? c->err.c_str() : "null context"; }

int plfx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int plfx_device_info(plfx_ctx *c, char *name, int len, int *cus, int64_t *hbm)
{
    if (!c || !c->stream) return PLFX_ERR_STATE;
    if (name && len > 0) {
        snprintf(name, len, "%s (%s)", c->prop.name, c->prop.gcnArchName);
    }
    if (cus) *cus = c->prop.multiProcessorCount;
    if (hbm) *hbm = (int64_t)c->prop.totalGlobalMem;
    return PLFX_OK;
}

void *plfx_stream(plfx_ctx *c) { return c ? (void *)c->stream : nullptr; }

int plfx_sync(plfx_ctx *c)
{
    if (!c || !c->stream) return PLFX_ERR_STATE;
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ mesh
// hint: the caller (plfx_set_mesh_structured) wrote the arrays itself from an NX x NY grid description -- the scans that verify
// what it already knows (index ranges, the structured numbering, uniform element sizes) are skipped
struct StructHint {
    int nx, ny;
    bool uniform;
};
static int set_mesh_impl(plfx_ctx *c, int nel, int nnode, const int32_t *conn, const int32_t *mat_id,
                         const double *lxy, double thick, int planestress, int el_begin, int el_end, const StructHint *hint)
{
    if (!c || !c->dmat) return c ? fail(c, PLFX_ERR_STATE, "set_materials first") : PLFX_ERR_STATE;
    if (nel < 1 || nnode < 4 || !conn || !mat_id || !lxy) return fail(c, PLFX_ERR_ARG, "bad mesh arguments");
    if (el_begin < 0 || el_end > nel || el_begin >= el_end) return fail(c, PLFX_ERR_ARG, "bad owned element range");
    free_mesh(c);
    c->nel_total = nel;
    c->nnode = nnode;
    c->ndof = 2 * nnode;
    c->e0 = el_begin;
    c->nel = el_end - el_begin;
    c->thick = thick;
    c->planestress = planestress ? 1 : 0;
    c->hint_nx = hint ? hint->nx : 0;
    c->hint_ny = hint ? hint->ny : 0;
    c->hint_uniform = hint && hint->uniform;
    for (int e = 0; e < nel && !hint; e++) {
        if (mat_id[e] < 0 || mat_id[e] >= c->nmat) return fail(c, PLFX_ERR_ARG, "mat_id[%d] out of range", e);
        for (int a = 0; a < 4; a++)
            if (conn[4 * e + a] < 0 || conn[4 * e + a] >= nnode)
                return fail(c, PLFX_ERR_ARG, "conn[%d][%d] out of range", e, a);
    }
    c->hconn.assign(conn, conn + (size_t)4 * nel);
    c->hlxy.assign(lxy, lxy + (size_t)2 * nel);
    // element classes (material, lx, ly)
    c->hcls.clear();
    c->hcls_id.resize(nel);
    {
        int last = -1;
        for (int e = 0; e < nel; e++) {
            const double lx = lxy[2 * e], ly = lxy[2 * e + 1];
            int found = -1;
            if (last >= 0 && c->hcls[last].mat == mat_id[e] && c->hcls[last].lx == lx && c->hcls[last].ly == ly)
                found = last;
            else
                for (size_t k = 0; k < c->hcls.size(); k++)
                    if (c->hcls[k].mat == mat_id[e] && c->hcls[k].lx == lx && c->hcls[k].ly == ly) {
                        found = (int)k;
                        break;
                    }
            if (found < 0) {
                if ((int)c->hcls.size() >= MAXCLS)
                    return fail(c, PLFX_ERR_UNSUPPORTED, "more than %d (material, lx, ly) element classes", MAXCLS);
                c->hcls.push_back(make_class(c, mat_id[e], lx, ly));
                found = (int)c->hcls.size() - 1;
            }
            c->hcls_id[e] = found;
            last = found;
        }
    }
    c->ncls = (int)c->hcls.size();

    // node -> owned elements adjacency, neighbour slots, assembly gather lists
    const int nown = c->nel;
    std::vector<int32_t> hcontrib;
    int nslot = 0, nq = 0;
    // The matrix (and its multigrid hierarchy) is assembled for the WHOLE mesh on every rank; a sharded
    // rank owns the material state of its x-strip only and the rows [own_n0, own_n1) of the CG SpMV.
    c->sharded = (nown != nel);
    // structured grids (every mesh of the reference's Model.mesh): slots and gather codes in closed form, written by a kernel
    // below -- the generic derivation sorts the neighbourhood of every node on the host and uploads 180 B per node (0.4 of
    // the 0.6 s of plfx_set_mesh at 2048^2)
    static const bool closed_form = !(getenv("PLFX_PATTERN_CLOSED_FORM") && atoi(getenv("PLFX_PATTERN_CLOSED_FORM")) == 0);
    c->pat_nx = c->pat_ny = 0;
    c->hcol.clear();
    c->hcol.shrink_to_fit();
    if (closed_form && hint && hint->nx >= 2 && hint->ny >= 2 && nel >= 4) {
        c->pat_nx = hint->nx;
        c->pat_ny = hint->ny;
        nslot = 9;
        nq = 4;
        c->n_begin = 0;
        c->n_end = nnode;
    } else if (closed_form && structured_dims(nel, nnode, conn, &c->pat_nx, &c->pat_ny)) {
        nslot = 9;
        nq = 4;
        c->n_begin = 0;
        c->n_end = nnode;
    } else {
        c->pat_nx = c->pat_ny = 0;
        if (!build_pattern(nnode, conn, 0, nel, c->hcol, hcontrib, nslot, nq, c->n_begin, c->n_end))
            return fail(c, PLFX_ERR_ARG, "empty mesh");
    }
    if (hint) {   // first node of an element = (e / ny) * (ny + 1) + e % ny, increasing with e
        const int ny = hint->ny, nyn = hint->ny + 1;
        c->own_n0 = (el_begin == 0) ? 0 : (el_begin / ny) * nyn + el_begin % ny;
        c->own_n1 = (el_end == nel) ? nnode : (el_end / ny) * nyn + el_end % ny;
    } else {
        int lo = nnode, nxt = nnode;
        for (int e = el_begin; e < el_end; e++)
            for (int a = 0; a < 4; a++) lo = std::min(lo, (int)conn[4 * (size_t)e + a]);
        for (int e = el_end; e < nel; e++)
            for (int a = 0; a < 4; a++) nxt = std::min(nxt, (int)conn[4 * (size_t)e + a]);
        c->own_n0 = (el_begin == 0) ? 0 : lo;   // the node column shared with the left neighbour is ours,
        c->own_n1 = (el_end == nel) ? nnode : nxt;  // the one shared with the right neighbour is theirs
    }
    c->nslot = nslot;
    c->nq = nq;
    if ((size_t)nel * 16 > 0x7fffffffULL) return fail(c, PLFX_ERR_UNSUPPORTED, "too many elements for int32 gather codes");

    int rc;
#define ALLOC(ptr, n) if ((rc = dalloc(c, &(ptr), (size_t)(n)))) return rc
    ALLOC(c->dcls, c->ncls);
    ALLOC(c->dconn, (size_t)4 * nel);
    ALLOC(c->dcls_id, nown);
    ALLOC(c->dcls_all, nel);
    ALLOC(c->dcol, (size_t)nslot * nnode);
    ALLOC(c->dcontrib, (size_t)nslot * nq * nnode);
    ALLOC(c->dval, (size_t)nslot * 4 * nnode);
    ALLOC(c->sig, (size_t)6 * nown);
    ALLOC(c->epl, (size_t)6 * nown);
    ALLOC(c->eps, (size_t)6 * nown);
    ALLOC(c->res_sig, (size_t)6 * nown);
    ALLOC(c->res_depl, (size_t)6 * nown);
    if ((rc = tan_alloc(c, nown))) return rc;
    ALLOC(c->Mel, (size_t)6 * nel);  // whole mesh (global element ids)
    ALLOC(c->fyn, nown);
    ALLOC(c->scf_hh, nown);
    ALLOC(c->kh_el, nown);
    ALLOC(c->max_steps, nown);
    ALLOC(c->scf_mult, nown);
    ALLOC(c->heavy_list, nown);
    const size_t nd = c->ndof;
    ALLOC(c->u, nd);
    ALLOC(c->f, nd);
    ALLOC(c->du, nd);
    ALLOC(c->rhs, nd);
    ALLOC(c->dinv, nd);
    ALLOC(c->diag, nd);
    ALLOC(c->is_presc, nd);
    ALLOC(c->ncode, ((size_t)nnode + 255) / 256 * 256);
    ALLOC(c->dup, nd);
    ALLOC(c->wv, nd);
    ALLOC(c->fext, nd);
    ALLOC(c->x, nd);
    ALLOC(c->r, nd);
    ALLOC(c->z, nd);
    ALLOC(c->q, nd);
    ALLOC(c->p[0], nd);
    ALLOC(c->p[1], nd);
#undef ALLOC
    HIPCHK(c, hipMemcpyAsync(c->dcls, c->hcls.data(), sizeof(ClassDev) * c->ncls, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dconn, conn, (size_t)16 * nel, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dcls_id, c->hcls_id.data() + el_begin, (size_t)4 * nown, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dcls_all, c->hcls_id.data(), (size_t)4 * nel, hipMemcpyHostToDevice, c->stream));
    if (c->pat_nx > 0) {
        hipLaunchKernelGGL(k_structured_pattern, dim3(grid_for(nnode)), dim3(256), 0, c->stream, c->pat_nx, c->pat_ny, c->dcol,
                           c->dcontrib);
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemcpyAsync(c->dcol, c->hcol.data(), c->hcol.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->dcontrib, hcontrib.data(), hcontrib.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, stream_sync(c));
    c->grid_nodes = grid_xcd(nnode);
    c->grid_el = grid_xcd(nown);
    // PLFX_SWEEP_BLOCKS=<n> (tests): at most n blocks in the grid of the sweeps and of calc_scf, so that a small mesh runs several passes of the
    // sweep's tile loop (read per mesh, not once per process)
    if (const char *cap = getenv("PLFX_SWEEP_BLOCKS"))
        if (atoi(cap) > 0 && c->grid_el > atoi(cap)) c->grid_el = atoi(cap);
    c->grid_ok = false;
    c->val_valid = false;
    c->op = make_op(c, nnode, nslot, c->dcol, c->dval, 0, 0, nel, c->Mel);
    return plfx_state_reset(c);
}

int plfx_set_mesh(plfx_ctx *c, int nel, int nnode, const int32_t *conn, const int32_t *mat_id,
                  const double *lxy, double thick, int planestress, int el_begin, int el_end)
{
    return set_mesh_impl(c, nel, nnode, conn, mat_id, lxy, thick, planestress, el_begin, el_end, nullptr);
}

// Model.mesh of the reference (model.py:758-952) produces nothing but structured grids: node j * (NY + 1) + k, element j * NY + k,
// connectivity [n1, n1 + 1, n1 + NY + 1, n1 + NY + 2] (:893, :935-948), one element width per column (laminate sections, :847) and
// one height.  This entry point takes that description -- NX column widths, material numbers per column or per element -- and
// writes the index arrays itself (round 3 built them with NumPy in the facade: 155 ms of the 0.35 s between mesh() and the first
// load step at 1024^2); everything else is plfx_set_mesh.
int plfx_set_mesh_structured(plfx_ctx *c, int NX, int NY, const int32_t *mat_col, const int32_t *mat_el, const double *dx_col, double dy,
                             double thick, int planestress, int el_begin, int el_end)
{
    if (!c) return PLFX_ERR_STATE;
    if (NX < 1 || NY < 1 || (!mat_col && !mat_el) || !dx_col || (int64_t)(NX + 1) * (NY + 1) > INT32_MAX)
        return fail(c, PLFX_ERR_ARG, "bad structured mesh description");
    const int nel = NX * NY, nyn = NY + 1;
    std::vector<int32_t> conn((size_t)4 * nel), mid((size_t)nel);
    std::vector<double> lxy((size_t)2 * nel);
    bool uniform = true;
    for (int j = 0; j < NX; j++) {
        const double dx = dx_col[j];
        if (std::fabs(dx - dx_col[0]) > 1e-12 * std::fabs(dx_col[0])) uniform = false;   // (one element height by construction)
        const int32_t mc = mat_col ? mat_col[j] : 0;
        if (mat_col && (mc < 0 || mc >= c->nmat)) return fail(c, PLFX_ERR_ARG, "mat_col[%d] out of range", j);
        int32_t *q = conn.data() + (size_t)4 * j * NY;
        double *l = lxy.data() + (size_t)2 * j * NY;
        int32_t *m = mid.data() + (size_t)j * NY;
        const int32_t *me = mat_el ? mat_el + (size_t)j * NY : nullptr;
        const int n0 = j * nyn;
        for (int k = 0; k < NY; k++) {
            const int n1 = n0 + k;
            q[4 * k] = n1;
            q[4 * k + 1] = n1 + 1;
            q[4 * k + 2] = n1 + nyn;
            q[4 * k + 3] = n1 + nyn + 1;
            l[2 * k] = dx;
            l[2 * k + 1] = dy;
            m[k] = me ? me[k] : mc;
            if (me && (me[k] < 0 || me[k] >= c->nmat)) return fail(c, PLFX_ERR_ARG, "mat_el[%d] out of range", j * NY + k);
        }
    }
    const StructHint hint{NX, NY, uniform};
    return set_mesh_impl(c, nel, (NX + 1) * nyn, conn.data(), mid.data(), lxy.data(), thick, planestress, el_begin, el_end, &hint);
}

int plfx_get_bmat(plfx_ctx *c, int e, double *B)
{
    if (!c || c->hcls.empty()) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (e < 0 || e >= c->nel_total || !B) return fail(c, PLFX_ERR_ARG, "bad argument");
    const ClassDev &k = c->hcls[c->hcls_id[e]];
    for (int g = 0; g < 4; g++) {
        double x, y, bx[4], by[4];
        gauss_point(k.lx, k.ly, g, &x, &y);
        shape_b(k.lx, k.ly, x, y, bx, by);
        double *Bg = B + 48 * g;
        for (int i = 0; i < 48; i++) Bg[i] = 0.;
        for (int a = 0; a < 4; a++) {
            Bg[0 * 8 + 2 * a] = bx[a];
            Bg[1 * 8 + 2 * a + 1] = by[a];
            Bg[5 * 8 + 2 * a] = by[a];
            Bg[5 * 8 + 2 * a + 1] = bx[a];
            Bg[2 * 8 + 2 * a] = k.kappa * bx[a];
            Bg[2 * 8 + 2 * a + 1] = k.kappa * by[a];
        }
    }
    return PLFX_OK;
}

int plfx_get_kel(plfx_ctx *c, int e, double *Kel)
{
    if (!c || !c->Mel) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (e < c->e0 || e >= c->e0 + c->nel || !Kel) return fail(c, PLFX_ERR_ARG, "element not owned");
    if (c->live_owed) {
        if (int rc = ensure_live_M(c)) return rc;
        HIPCHK(c, stream_sync(c));   // (the copies below run on the null stream)
    }
    double M[6];
    for (int k = 0; k < 6; k++)
        HIPCHK(c, hipMemcpy(&M[k], c->Mel + (size_t)k * c->nel_total + e, 8, hipMemcpyDeviceToHost));
    const ClassDev &k = c->hcls[c->hcls_id[e]];
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) {
            const double sxx = k.Sxx[a * 4 + b], sxy = k.Sxy[a * 4 + b], syx = k.Sxy[b * 4 + a], syy = k.Syy[a * 4 + b];
            Kel[(2 * a) * 8 + 2 * b] = M[0] * sxx + M[2] * (sxy + syx) + M[5] * syy;
            Kel[(2 * a) * 8 + 2 * b + 1] = M[1] * sxy + M[2] * sxx + M[4] * syy + M[5] * syx;
            Kel[(2 * a + 1) * 8 + 2 * b] = M[1] * syx + M[4] * syy + M[2] * sxx + M[5] * sxy;
            Kel[(2 * a + 1) * 8 + 2 * b + 1] = M[3] * syy + M[4] * (syx + sxy) + M[5] * sxx;
        }
    return PLFX_OK;
}

// Multigrid hierarchy of the nx x ny element grid of context c (level 0 aliases the context's fine-grid arrays): level
// dimensions, block-ELL patterns of the coarse levels, single-workgroup tail, coarse solver.  Shared by plfx_set_grid and
// by the coarse context of a strip (strip_create_child).
static int build_hierarchy(plfx_ctx *c, int nx, int ny, const ClassDev &geom)
{
    int rc;
    std::vector<std::pair<int, int>> dims;
    dims.push_back({nx, ny});
    // coarsening goes on to 2 x 2 elements (9 nodes, 18 DOFs, dense inverse).  Stopping at 4 x 4 (PLFX_MG_COARSEST_ELEMS=16:
    // 50 DOFs, one level of six workgroup-barrier phases less) saves 4.5 us of the 259 us of a cycle at 1024^2 -- and made four
    // GMRES solves of config 5 at 2048^2 stall at 1e-6 in load step 16 (130 000 mildly indefinite elements by then;
    // profiles/r04d_config5_coarsest_level.txt -- with partial pivoting in the 50 x 50 inverse the numbers are identical, so it
    // is the truncated hierarchy on that indefinite operator, not the inversion).  Measured, not adopted.
    static const long long coarsest = getenv("PLFX_MG_COARSEST_ELEMS") ? atoll(getenv("PLFX_MG_COARSEST_ELEMS")) : 4;
    // Meshes with an odd number of elements in a direction (round 5) used to have no hierarchy at all (Jacobi-PCG, ~8 NX
    // iterations per cold solve).  Now, if the FINEST grid is odd and large, every level covers exactly the fine grid with cells
    // of one size except the last column / row, whose relative size r stays in [1, 2): n cells are paired; an odd n ALWAYS puts
    // three children (1, 1, r) into the last coarse cell -- mg_coarse_cells / mg_coarse_ratio / mg_odd_triple under the default
    // PLFX_MG_ODD_RULE=1.  (The area-scaled smoothing diagonal of k_grid_setup is a stable Jacobi scaling only while no cell is
    // narrower than its neighbours, i.e. r >= 1: compiling with PLFX_MG_ODD_RULE=0 restores the round-5-v3 rule r in [1/2, 3/2)
    // with lone narrow cells AND the true-diagonal scaling that goes with it -- the two belong together.)
    // The stiffness integrals of the last cells scale with their shape (KOp::rx, ry), the transfers take the position-dependent
    // weights of bilinear interpolation (mg_tr1d), the coarse generators are area-weighted means of the children, the last node
    // line of every level is the edge of the grid (Dirichlet masks as before): the coarse spaces are nested in the fine one and
    // the re-discretised coarse operators are the Galerkin ones of a homogeneous field, as on grids that halve exactly
    // (elastic cold solves: 11-12 PCG iterations on 512 x 511 / 511 x 512 / 512 x 512 alike).  Two earlier versions, measured:
    // a zero-stiffness ghost element beyond the edge (exact behind free edges, ~10x the iterations of the homogeneous plastic
    // workload behind a Dirichlet edge); lone narrow cells only (1025 cells: r = 1/2, 1/4, 1/8 ... slivers, 795 iterations).
    // PLFX_MG_ODD=0: never (exact halving only, Chebyshev / Jacobi below an odd level), 1 (default since the area-scaled smoothing
    // diagonal): every level that cannot be halved and is too large for the dense coarse solve is coarsened this way --
    // also the odd coarse levels of even meshes (1000^2 -> 125^2: 6.0 -> 2.5 ms per load step of the config-3 workload instead of a
    // Chebyshev solve there), 2: only hierarchies whose FINEST grid is odd and large (the default until then).
    const int odd_mode = getenv("PLFX_MG_ODD") ? atoi(getenv("PLFX_MG_ODD")) : 1;   // (read per hierarchy: tests switch it)
    const bool finest_odd = ((nx | ny) & 1) && (long long)(nx + 1) * (ny + 1) > 150000 && c->want_matfree;
    std::vector<std::pair<double, double>> ratio;
    ratio.push_back({1., 1.});
    for (;;) {
        const int fx = dims.back().first, fy = dims.back().second;
        const double rx = ratio.back().first, ry = ratio.back().second;
        const long long ne = (long long)fx * fy;
        const bool plain = fx % 2 == 0 && fy % 2 == 0 && rx == 1. && ry == 1.;
        const bool big = (long long)(fx + 1) * (fy + 1) > MG_COARSE_MAX;
        if (!(ne > 4 && (ne > coarsest || dims.size() < 2))) break;   // (at least two levels)
        if (!plain && !((odd_mode == 1 || (odd_mode == 2 && finest_odd)) && (big || rx != 1. || ry != 1.) && fx >= 2 && fy >= 2)) break;
        if (plain) {
            ratio.push_back({1., 1.});
            dims.push_back({fx / 2, fy / 2});
        } else {
            ratio.push_back({mg_coarse_ratio(fx, rx), mg_coarse_ratio(fy, ry)});
            dims.push_back({mg_coarse_cells(fx, rx), mg_coarse_cells(fy, ry)});
        }
    }
    if (dims.size() < 2) return PLFX_OK;
    if (!c->mg_cls) {
        if ((rc = dalloc(c, &c->mg_cls, 1))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->mg_cls, &geom, sizeof(ClassDev), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, stream_sync(c));
    }
    c->mg.resize(dims.size());
    for (size_t l = 0; l < dims.size(); l++) {
        auto &L = c->mg[l];
        L.nx = dims[l].first;
        L.ny = dims[l].second;
        L.rx = ratio[l].first;
        L.ry = ratio[l].second;
        L.nnode = (L.nx + 1) * (L.ny + 1);
        L.nel = L.nx * L.ny;
        L.grid = grid_xcd(L.nnode);
        if ((rc = dalloc(c, &L.t, (size_t)2 * L.nnode))) return rc;
        if ((rc = dalloc(c, &L.res, (size_t)2 * L.nnode))) return rc;
        if (l == 0) {
            L.owned = false;
            L.nslot = c->nslot;
            L.nq = c->nq;
            L.col = c->dcol;
            L.val = c->dval;
            L.diag = c->diag;
            L.dinv = c->dinv;
            L.Mel = c->Mel;
            L.nel = c->nel_total;
            L.x = c->z;
            L.b = c->r;
            continue;
        }
        L.owned = true;
        std::vector<int32_t> conn, hcol, hcontrib;
        const bool closed = L.nx >= 2 && L.ny >= 2 && !(getenv("PLFX_PATTERN_CLOSED_FORM") && atoi(getenv("PLFX_PATTERN_CLOSED_FORM")) == 0);
        if (closed) {   // the levels are structured grids by construction: pattern in closed form, written on the device
            L.nslot = 9;
            L.nq = 4;
        } else {
            conn.resize((size_t)4 * L.nel);
            const int nr = L.ny + 1;
            for (int e = 0; e < L.nel; e++) {
                const int n1 = (e / L.ny) * nr + e % L.ny;
                conn[4 * (size_t)e] = n1;
                conn[4 * (size_t)e + 1] = n1 + 1;
                conn[4 * (size_t)e + 2] = n1 + nr;
                conn[4 * (size_t)e + 3] = n1 + nr + 1;
            }
            int nb, ne;
            if (!build_pattern(L.nnode, conn.data(), 0, L.nel, hcol, hcontrib, L.nslot, L.nq, nb, ne))
                return fail(c, PLFX_ERR_ARG, "empty multigrid level");
        }
        if ((rc = dalloc(c, &L.col, (size_t)L.nslot * L.nnode))) return rc;
        if ((rc = dalloc(c, &L.contrib, (size_t)L.nslot * L.nq * L.nnode))) return rc;
        if ((rc = dalloc(c, &L.cls0, (size_t)L.nel))) return rc;
        if ((rc = dalloc(c, &L.val, (size_t)L.nslot * 4 * L.nnode))) return rc;
        if ((rc = dalloc(c, &L.diag, (size_t)2 * L.nnode))) return rc;
        if ((rc = dalloc(c, &L.dinv, (size_t)2 * L.nnode))) return rc;
        if ((rc = dalloc(c, &L.Mel, (size_t)6 * L.nel))) return rc;
        if ((rc = dalloc(c, &L.x, (size_t)2 * L.nnode))) return rc;
        if ((rc = dalloc(c, &L.b, (size_t)2 * L.nnode))) return rc;
        if (L.rx != 1. || L.ry != 1.) {
            // assembled form of such a level (coarsest level: dense inverse; tail levels when the matrix-free tail is not in use):
            // four cell shapes, class id = (odd column, mg_odd_cell) + 2 (odd row); Sxx ~ ly / lx, Syy ~ lx / ly, Sxy independent of the size
            ClassDev h4[4];
            for (int q = 0; q < 4; q++) {
                h4[q] = geom;
                const double sx = (q & 1) ? L.rx : 1., sy = (q & 2) ? L.ry : 1.;
                for (int t = 0; t < 16; t++) {
                    h4[q].Sxx[t] *= sy / sx;
                    h4[q].Syy[t] *= sx / sy;
                }
            }
            if ((rc = dalloc(c, &L.cls4, 4))) return rc;
            HIPCHK(c, hipMemcpyAsync(L.cls4, h4, sizeof(h4), hipMemcpyHostToDevice, c->stream));
            std::vector<int32_t> hc((size_t)L.nel);
            for (int e = 0; e < L.nel; e++) hc[e] = ((e / L.ny == mg_odd_cell(L.nx)) ? 1 : 0) + ((e % L.ny == mg_odd_cell(L.ny)) ? 2 : 0);
            HIPCHK(c, hipMemcpyAsync(L.cls0, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, stream_sync(c));
        }
        if (closed) {
            hipLaunchKernelGGL(k_structured_pattern, dim3(grid_for(L.nnode)), dim3(256), 0, c->stream, L.nx, L.ny, L.col, L.contrib);
            HIPCHK(c, hipGetLastError());
        } else {
            HIPCHK(c, hipMemcpyAsync(L.col, hcol.data(), hcol.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(L.contrib, hcontrib.data(), hcontrib.size() * 4, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, stream_sync(c));
    }
    {
        auto &Lc = c->mg.back();
        const int n = 2 * Lc.nnode;
        if (n <= MG_DENSE_MAX) {
            if ((rc = dalloc(c, &Lc.ainv, (size_t)n * n))) return rc;
            HIPCHK(c, set_dyn_lds((const void *)k_mg_coarse_invert, n * n * (int)sizeof(double)));
        }
    }
    c->mg_cheby = 0;
    const bool small_coarsest = c->mg.back().nnode <= MG_COARSE_MAX;
    if (small_coarsest) {
        const int lds = c->mg.back().nnode * 4 * (int)sizeof(double2);
        HIPCHK(c, set_dyn_lds((const void *)k_mg_coarse_solve, lds));
        HIPCHK(c, set_dyn_lds((const void *)k_mg_tail, lds));
    }
    {   // levels small enough for the single-workgroup tail (never level 0)
        std::vector<MgLevDev> hd(c->mg.size());
        c->mg_tail = -1;
        for (size_t l = 0; l < c->mg.size(); l++) {
            auto &L = c->mg[l];
            if (c->mg_tail < 0 && l > 0 && L.nnode <= MG_TAIL_NODES) c->mg_tail = (int)l;
            int off = 0;
            if (c->mg_tail >= 0)
                for (size_t m = c->mg_tail; m < l; m++) off += c->mg[m].nnode;
            int eoff = 0;
            if (c->mg_tail >= 0)
                for (size_t m = c->mg_tail; m < l; m++) eoff += c->mg[m].nel;
            hd[l] = MgLevDev{L.nx, L.ny, L.nnode, L.nslot, L.ainv, off, 0, L.col, L.val, (const double2 *)L.dinv,
                             (double2 *)L.x, (double2 *)L.b, (double2 *)L.t, (double2 *)L.res, L.Mel, L.nel, eoff, L.rx, L.ry};
        }
        c->mg_tail_T = 0;
        if (c->mg_tail >= 0 && c->mg.back().ainv && c->mg_nu == 2) {
            int T = 0;
            bool ok = true;
            for (size_t m = c->mg_tail; m < c->mg.size(); m++) {
                T += c->mg[m].nnode;
                ok = ok && c->mg[m].nslot <= 9;
            }
            const size_t bytes = (size_t)T * (4 * sizeof(double2) + 9 * sizeof(int));
            if (ok && bytes <= 150 * 1024) {
                c->mg_tail_T = T;
                HIPCHK(c, set_dyn_lds((const void *)k_mg_tail_lds, (int)bytes));
            }
            // matrix-free tail: generators of the tail levels (coarsest excluded) in LDS instead of neighbour tables
            int E = 0;
            for (size_t m = c->mg_tail; m + 1 < c->mg.size(); m++) E += c->mg[m].nel;
            const size_t bytes_mf = (size_t)T * 3 * sizeof(double2) + (size_t)E * 6 * sizeof(double);
            c->mg_tail_lds = bytes_mf;
            c->mg_tail_E = 0;
            if (c->grid_ok && bytes_mf <= 154 * 1024 && E > 0 && c->mg.size() <= 16) {  // + 2 KB static LDS (level table)
                c->mg_tail_E = E;
                HIPCHK(c, set_dyn_lds((const void *)k_mg_tail_mf<false>, (int)bytes_mf));
                HIPCHK(c, set_dyn_lds((const void *)k_mg_tail_mf<true>, (int)bytes_mf));
            }
        }
        {   // levels above the tail are applied matrix-free; the tail and the coarsest level keep assembled matrices
            const int nl = (int)c->mg.size();
            const int lt = (c->mg_tail > 0) ? c->mg_tail : nl - 1;
            // coarsest level without a dense inverse (odd coarse sizes such as 25 x 25 or 125 x 125 elements) and not
            // inside a multi-level tail: solved by a fixed number of Jacobi-preconditioned Chebyshev steps
            c->mg_cheby = 0;
            if (!c->mg.back().ainv && lt == nl - 1) {
                const int n = std::max(c->mg.back().nx, c->mg.back().ny);
                c->mg_cheby = std::min(std::max(n, 16), 160);
                c->mg_cheby_kappa = std::max(4., 0.5 * (double)n * n);
                if (const char *e6 = getenv("PLFX_MG_CHEBY")) c->mg_cheby = std::max(0, atoi(e6));
                if (const char *e7 = getenv("PLFX_MG_CHEBY_KAPPA")) c->mg_cheby_kappa = std::max(1.5, atof(e7));
            }
            for (int l = 0; l < nl; l++) {
                auto &L = c->mg[l];
                L.op = make_op(c, L.nnode, L.nslot, L.col, L.val, L.nx, L.ny, L.nel, l == 0 ? c->Mop : L.Mel, L.rx, L.ry);
                L.matfree = l < lt || (c->mg_cheby > 0 && l == nl - 1);
            }
            if (c->mg_cheby == 0 && c->mg.back().nnode > MG_COARSE_MAX) c->precond = 0;  // no usable coarse solver
        }
        dfree(c->mg_dev);
        if ((rc = dalloc(c, &c->mg_dev, hd.size()))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->mg_dev, hd.data(), hd.size() * sizeof(MgLevDev), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, stream_sync(c));
    }
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ structured grid / multigrid
int plfx_set_grid(plfx_ctx *c, int nx, int ny)
{
    if (!c || !c->dval) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (nx < 1 || ny < 1 || (long long)nx * ny != c->nel_total || (long long)(nx + 1) * (ny + 1) != c->nnode)
        return fail(c, PLFX_ERR_ARG, "grid %dx%d does not match the mesh", nx, ny);
    if (c->strip.on)  // the hierarchy, halo analysis and coarse child context of a strip belong to the grid they were set up for
        return fail(c, PLFX_ERR_STATE, "plfx_set_grid after plfx_set_strip: call plfx_set_mesh again");
    if (int rcs = snap_settle(c)) return rcs;
    const int nrow = ny + 1;
    const bool known = c->hint_nx == nx && c->hint_ny == ny;   // written by plfx_set_mesh_structured: nothing to verify
    for (int e = 0; e < c->nel_total && !known; e++) {  // model.py:935-948
        const int n1 = (e / ny) * nrow + e % ny;
        const int32_t *q = &c->hconn[4 * (size_t)e];
        if (q[0] != n1 || q[1] != n1 + 1 || q[2] != n1 + nrow || q[3] != n1 + nrow + 1)
            return fail(c, PLFX_ERR_ARG, "connectivity of element %d is not the structured numbering", e);
    }
    c->gx = nx;
    c->gy = ny;
    c->code_ok = false;   // (built again with the next Dirichlet set)
    mg_graph_drop(c);
    for (auto &L : c->mg) {  // drop a previous hierarchy
        if (L.owned) {
            dfree(L.col); dfree(L.contrib); dfree(L.cls0); dfree(L.val); dfree(L.diag); dfree(L.dinv);
            dfree(L.Mel); dfree(L.x); dfree(L.b);
        }
        dfree(L.t); dfree(L.res); dfree(L.ainv); dfree(L.cls4);
    }
    c->mg.clear();
    c->grid_ok = false;
    c->op = make_op(c, c->nnode, c->nslot, c->dcol, c->dval, 0, 0, c->nel_total, c->Mel);
    // coarse re-assembly and the matrix-free operator need one element shape.  Laminate meshes compute dx = LS[i]/nes[i]
    // per section (model.py:847), so nominally uniform sections can differ by an ulp: compare with a relative tolerance and
    // use element 0's shape for the operator tables (the strain operator keeps each class's own lx, ly).
    // Non-proportional laminates (round 5): nes[i] = round(NX LS[i] / lenx) elements per section leave the
    // sections with slightly different dx (relative deviation <= 1 / (2 nes[i])), constant within a column; dy is one value.
    // The KRYLOV operator of such a mesh is exact -- the matrix-free form with the width of every column relative to column 0
    // (KOp::colr, instantiation 2 of the kernels; or the block-ELL matrix) -- while the V-cycle is the one of the UNIFORM grid
    // with column 0's cell shape on the same generators: a symmetric positive definite preconditioner of a spectrally
    // equivalent operator (element matrices within [1/r, r] of each other, r = widest / narrowest column), instead of no
    // hierarchy at all (Jacobi-PCG: ~8 NX iterations per cold solve).  r <= 1.5 is accepted (larger ratios need sections of one or two elements: meshes too small to need a hierarchy).
    dfree(c->colr);
    c->colr = nullptr;
    bool uniform = known && c->hint_uniform;
    if (!uniform) {
        uniform = true;
        bool columns = true;
        std::vector<double> cr(nx, 1.);
        const double lx0 = c->hlxy[0], ly0 = c->hlxy[1];
        double rmin = 1., rmax = 1.;
        for (int e = 0; e < c->nel_total && columns; e++) {
            const double lx = c->hlxy[2 * (size_t)e], ly = c->hlxy[2 * (size_t)e + 1];
            const int j = e / ny;
            if (std::fabs(ly - ly0) > 1e-12 * std::fabs(ly0)) columns = false;
            if (e % ny == 0) {
                cr[j] = (std::fabs(lx - lx0) > 1e-12 * std::fabs(lx0)) ? lx / lx0 : 1.;
                if (cr[j] != 1.) uniform = false;
                rmin = std::min(rmin, cr[j]);
                rmax = std::max(rmax, cr[j]);
            } else if (std::fabs(lx - c->hlxy[2 * (size_t)(j * ny)]) > 1e-12 * std::fabs(lx0))
                columns = false;
        }
        if (!columns) return PLFX_OK;
        if (!uniform) {
            if (!(rmin > 0.) || rmax / rmin > 1.5) return PLFX_OK;
            int rc0;
            if ((rc0 = dalloc(c, &c->colr, (size_t)nx))) return rc0;
            HIPCHK(c, hipMemcpyAsync(c->colr, cr.data(), (size_t)8 * nx, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, stream_sync(c));
            c->colr_ratio = rmax / rmin;
        }
    }
    int rc;
    {   // geometry table of grid_apply: position p = pj*2+pk <-> element (j-1+pj, k-1+pk), in which node (j,k) has the
        // local number a = (1-pj)*2 + (1-pk) (connectivity order model.py:936-948)
        double tab[64];
        const ClassDev &g = c->hcls[0];
        for (int pj = 0; pj < 2; pj++)
            for (int pk = 0; pk < 2; pk++) {
                const int a = (1 - pj) * 2 + (1 - pk), p = pj * 2 + pk;
                for (int b = 0; b < 4; b++) {
                    tab[p * 16 + b * 4 + 0] = g.Sxx[a * 4 + b];
                    tab[p * 16 + b * 4 + 1] = g.Syy[a * 4 + b];
                    tab[p * 16 + b * 4 + 2] = g.Sxy[a * 4 + b];
                    tab[p * 16 + b * 4 + 3] = g.Sxy[b * 4 + a];
                }
            }
        if (!c->dtab && (rc = dalloc(c, &c->dtab, 64))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->dtab, tab, sizeof(tab), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, stream_sync(c));
        if ((rc = dalloc(c, &c->Mop, (size_t)6 * c->nel_total))) return rc;
        c->op = make_op(c, c->nnode, c->nslot, c->dcol, c->dval, nx, ny, c->nel_total, c->Mop);
        c->op.colr = c->colr;
        c->grid_ok = true;
    }
    if ((rc = build_hierarchy(c, nx, ny, c->hcls[0]))) return rc;
    c->assembled = false, c->M_dirty = true;
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ strip-local engine
int plfx_set_strip(plfx_ctx *c, int own_col0, int own_col1, int global_col0, int global_nx, int coarse_level)
{
    if (!c || !c->dval) return c ? fail(c, PLFX_ERR_STATE, "set_mesh / set_grid first") : PLFX_ERR_STATE;
    if (!c->grid_ok || !c->want_matfree || c->mg.size() < 2)
        return fail(c, PLFX_ERR_UNSUPPORTED, "a strip needs the uniform structured grid (matrix-free operator + multigrid)");
    if (c->colr) return fail(c, PLFX_ERR_UNSUPPORTED, "a strip needs element columns of one width");
    if (int rcs = snap_settle(c)) return rcs;
    const int nx = c->gx, ny = c->gy, Ld = coarse_level;
    // material state and sweeps: either the whole local mesh (halo elements swept redundantly) or exactly the owned columns
    // (el_begin / el_end of plfx_set_mesh; the generators of the halo columns then come from the neighbours: strip_sync_M)
    if (c->sharded && (c->e0 != own_col0 * ny || c->nel != (own_col1 - own_col0) * ny))
        return fail(c, PLFX_ERR_STATE, "the owned element range of plfx_set_mesh must be the owned columns of the strip (or the whole local mesh)");
    if (Ld < 1 || Ld >= (int)c->mg.size())
        return fail(c, PLFX_ERR_ARG, "coarse level %d outside 1..%d of the local hierarchy", Ld, (int)c->mg.size() - 1);
    const int al = 1 << Ld;
    if (own_col0 < 0 || own_col1 > nx || own_col0 >= own_col1) return fail(c, PLFX_ERR_ARG, "bad owned column range");
    const bool hl = own_col0 > 0, hr = own_col1 < nx;
    const int W = hl ? own_col0 : (hr ? nx - own_col1 : 0);
    if ((hl && own_col0 != W) || (hr && nx - own_col1 != W)) return fail(c, PLFX_ERR_ARG, "halo widths of the two sides differ");
    if ((own_col0 | own_col1 | global_col0 | global_nx | ny | W | nx) & (al - 1))
        return fail(c, PLFX_ERR_ARG, "columns, halo and NY must be multiples of 2^level = %d", al);
    if (global_col0 < 0 || global_col0 + nx > global_nx) return fail(c, PLFX_ERR_ARG, "local grid outside the global one");
    if ((hl != (global_col0 + own_col0 > 0)) || (hr != (global_col0 + own_col1 < global_nx)))
        return fail(c, PLFX_ERR_ARG, "a halo is needed exactly on the interior sides of the strip");
    if ((hl || hr) && own_col1 - own_col0 < W) return fail(c, PLFX_ERR_ARG, "owned width %d below the halo width %d", own_col1 - own_col0, W);
    if ((hl || hr) && c->nranks < 2) return fail(c, PLFX_ERR_STATE, "interior strip edges need a communicator (plfx_comm_init*)");
    if (c->mg_nu != 2) return fail(c, PLFX_ERR_UNSUPPORTED, "the validity widths of a strip are worked out for V(2,2)");
    if (hl || hr) {
        // Validity widths (columns beyond the owned range on which a quantity equals the single-GPU one).  The operator row
        // and the Jacobi scaling of the outermost local column E are wrong (elements beyond the artificial edge are missing)
        // and every operator application moves that error one column inwards.  Down: b valid v -> first sweep a = min(v, E-1),
        // second a-1, residual a-2, full-weighting restriction (a-3)/2.  Up: x of the down leg a-1, prolongated correction
        // 2 g', two post-smoothing sweeps -2.  Needed: b of level Ld valid on the owned columns (v >= 0) and z valid on
        // owned + 1 (g >= 1; then p, K p and r stay valid on the owned columns without further exchange).
        std::vector<int> a(Ld + 1);
        int v = W;
        for (int l = 0; l < Ld; l++) {
            a[l] = std::min(v, (W >> l) - 1);
            v = (a[l] - 3) >= 0 ? (a[l] - 3) / 2 : -1;
        }
        int g = W >> Ld;  // the coarse correction is valid on every local column
        for (int l = Ld - 1; l >= 0 && v >= 0; l--) g = std::min(a[l] - 1, 2 * g) - 2;
        if (v < 0 || g < 1)
            return fail(c, PLFX_ERR_ARG, "halo of %d columns is too narrow for coarse level %d (need 4 * 2^level: 32 for level 3, 64 for level 4)", W, Ld);
    }
    mg_graph_drop(c);
    strip_free(c);
    auto &S = c->strip;
    // the local hierarchy ends at level Ld (kept for its vectors, generators and Jacobi scaling: the hand-over level)
    for (size_t l = Ld + 1; l < c->mg.size(); l++) {
        auto &L = c->mg[l];
        if (L.owned) {
            dfree(L.col); dfree(L.contrib); dfree(L.cls0); dfree(L.val); dfree(L.diag); dfree(L.dinv);
            dfree(L.Mel); dfree(L.x); dfree(L.b);
        }
        dfree(L.t); dfree(L.res); dfree(L.ainv); dfree(L.cls4);
    }
    c->mg.resize(Ld + 1);
    dfree(c->mg.back().ainv);
    c->mg_tail = -1;
    c->mg_tail_T = c->mg_tail_E = 0;
    c->mg_cheby = 0;
    c->precond = 1;
    for (auto &L : c->mg) L.matfree = true;
    S.oc0 = own_col0;
    S.oc1 = own_col1;
    S.W = W;
    S.Ld = Ld;
    S.gcol0 = global_col0;
    S.gnx = global_nx;
    S.has_left = hl;
    S.has_right = hr;
    const int nyn = ny + 1;
    S.own_lo = own_col0 * nyn;
    S.own_hi = (hr ? own_col1 : nx + 1) * nyn;
    S.eown_lo = c->sharded ? 0 : own_col0 * ny;  // in the numbering of the state arrays
    S.eown_hi = c->sharded ? c->nel : own_col1 * ny;
    // replicated coarse problem: levels >= Ld of the global grid
    plfx_ctx *k = new plfx_ctx();
    S.child = k;
    k->is_child = true;
    k->device = c->device;
    k->stream = c->stream;
    k->prop = c->prop;
    k->sc = c->sc;
    k->dtab = c->dtab;
    k->want_matfree = 1;
    k->want_mg_graph = c->want_mg_graph;
    k->mg_omega = c->mg_omega;
    k->mg_nu = c->mg_nu;
    k->gx = global_nx >> Ld;
    k->gy = ny >> Ld;
    k->nel_total = k->nel = k->gx * k->gy;
    k->nnode = (k->gx + 1) * (k->gy + 1);
    k->ndof = 2 * k->nnode;
    int rc;
#define KALLOC(ptr, n)                               \
    if ((rc = dalloc(c, &(ptr), (size_t)(n)))) {     \
        strip_free(c);                               \
        return rc;                                   \
    }
    KALLOC(k->Mel, (size_t)6 * k->nel_total);
    KALLOC(k->Mop, (size_t)6 * k->nel_total);
    KALLOC(k->diag, k->ndof);
    KALLOC(k->dinv, k->ndof);
    KALLOC(k->r, k->ndof);
    KALLOC(k->z, k->ndof);
#undef KALLOC
    k->grid_ok = true;
    k->grid_nodes = grid_xcd(k->nnode);
    k->op = make_op(k, k->nnode, 0, nullptr, nullptr, k->gx, k->gy, k->nel_total, k->Mop);
    rc = build_hierarchy(k, k->gx, k->gy, c->hcls[0]);
    if (rc || !mg_active(k)) {
        if (!rc) rc = fail(c, PLFX_ERR_UNSUPPORTED, "the global coarse grid %d x %d has no usable hierarchy", k->gx, k->gy);
        else c->err = k->err;
        strip_free(c);
        return rc;
    }
    S.on = true;
    // the per-block partial sums are all-reduced element-wise: every rank must produce (and consume) the same number of them
    c->grid_nodes = MAXPART;
    c->assembled = false, c->M_dirty = true;
    c->bc_set = false;
    c->bc_valid = c->code_ok = false;
    c->rhs_rows_ok = c->dinv_ok = false;
    c->dinv_late = c->pred_d_kept = false;   // (a strip never defers: the full k_bc_finish of its first apply_bc writes dinv)
    c->x_is_du = false;
    c->memo.valid = false;
    return PLFX_OK;
}

int plfx_strip_info(plfx_ctx *c, int *active, int *halo, int *coarse_level, int *coarse_levels, int64_t *halo_refreshes,
                    int64_t *coarse_gathers, int64_t *partial_allreduces, int64_t *generator_exchanges)
{
    if (!c) return PLFX_ERR_ARG;
    const auto &S = c->strip;
    if (active) *active = S.on ? 1 : 0;
    if (halo) *halo = S.W;
    if (coarse_level) *coarse_level = S.Ld;
    if (coarse_levels) *coarse_levels = S.child ? (int)S.child->mg.size() : 0;
    if (halo_refreshes) *halo_refreshes = S.n_halo;
    if (coarse_gathers) *coarse_gathers = S.n_coarse;
    if (partial_allreduces) *partial_allreduces = S.n_part;
    if (generator_exchanges) *generator_exchanges = S.n_gen;
    return PLFX_OK;
}

int plfx_allreduce_host(plfx_ctx *c, double *buf, int n, int op)
{
    if (!c || !c->small) return PLFX_ERR_STATE;
    if (!buf || n < 0 || n > 32 || (op != 0 && op != 3)) return fail(c, PLFX_ERR_ARG, "n must be in 0..32, op 0 (sum) or 3 (min)");
    if (n == 0 || !comm_active(c)) return PLFX_OK;
    HIPCHK(c, hipMemcpyAsync(c->small, buf, (size_t)8 * n, hipMemcpyHostToDevice, c->stream));
    const int rc = allreduce(c, c->small, n, NCCL_FLOAT64, op == 3 ? NCCL_MIN : NCCL_SUM, "host scalars");
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(buf, c->small, (size_t)8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_set_operator(plfx_ctx *c, int kind)
{
    if (!c) return PLFX_ERR_ARG;
    if (kind != 0 && kind != 1) return fail(c, PLFX_ERR_ARG, "operator kind must be 0 (assembled) or 1 (matrix-free)");
    if (c->strip.on && kind != 1) return fail(c, PLFX_ERR_UNSUPPORTED, "a strip (plfx_set_strip) runs the matrix-free operator only");
    if (kind != c->want_matfree) {
        if (int rcs = snap_settle(c)) return rcs;
        mg_graph_drop(c);
        c->want_matfree = kind;
        c->assembled = false, c->M_dirty = true;  // diagonal / matrix values of the other form have to be rebuilt
        c->bc_set = c->code_ok = false;
    }
    return PLFX_OK;
}

int plfx_operator_info(plfx_ctx *c, int *matrix_free, int *levels_matrix_free)
{
    if (!c) return PLFX_ERR_ARG;
    if (matrix_free) *matrix_free = matfree(c) ? 1 : 0;
    if (levels_matrix_free) {
        int n = 0;
        if (matfree(c))
            for (auto &L : c->mg) n += L.matfree ? 1 : 0;
        *levels_matrix_free = n;
    }
    return PLFX_OK;
}

int plfx_sweep_info(plfx_ctx *c, int64_t *sweeps, int64_t *tangents_rewritten)
{
    if (!c) return PLFX_ERR_ARG;
    if (sweeps) *sweeps = c->n_sweeps;
    if (tangents_rewritten) *tangents_rewritten = c->n_tangents_rewritten;
    return PLFX_OK;
}

int plfx_bc_info(plfx_ctx *c, int64_t *rhs_rows_only, int64_t *dinv_kept, int64_t *dinv_refreshed, int64_t *du_early)
{
    if (!c) return PLFX_ERR_ARG;
    if (rhs_rows_only) *rhs_rows_only = c->n_rhs_rows;
    if (dinv_kept) *dinv_kept = c->n_dinv_kept;
    if (dinv_refreshed) *dinv_refreshed = c->n_dinv_refreshed;
    if (du_early) *du_early = c->n_du_early;
    return PLFX_OK;
}

int plfx_short_info(plfx_ctx *c, int64_t *dinv_deferred, int64_t *dinv_formed_late, int64_t *d_kept, int64_t *spec_merged)
{
    if (!c) return PLFX_ERR_ARG;
    if (dinv_deferred) *dinv_deferred = c->n_dinv_deferred;
    if (dinv_formed_late) *dinv_formed_late = c->n_dinv_late;
    if (d_kept) *d_kept = c->n_d_kept;
    if (spec_merged) *spec_merged = 0;   // (no merged launch behind a sweep's flags in this library: DESIGN 38 C)
    return PLFX_OK;
}

int plfx_code_info(plfx_ctx *c, int64_t *built, int64_t *start_launches, int64_t *b_sparse_launches, int64_t *vector_launches)
{
    if (!c) return PLFX_ERR_ARG;
    if (built) *built = c->n_code_built;
    if (start_launches) *start_launches = c->n_code_start;
    if (b_sparse_launches) *b_sparse_launches = c->n_code_bsparse;
    if (vector_launches) *vector_launches = c->n_code_vector;
    return PLFX_OK;
}

int plfx_code_get(plfx_ctx *c, uint8_t *out)
{
    if (!c || !c->ncode) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (!out) return fail(c, PLFX_ERR_ARG, "bad argument");
    if (!c->code_ok) return fail(c, PLFX_ERR_STATE, "no node code: apply_bc first");
    HIPCHK(c, hipMemcpyAsync(out, c->ncode, (size_t)c->nnode, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_snap_info(plfx_ctx *c, int64_t *direct_sweeps, int64_t *direct_acknowledged, int64_t *setup_formed_late, int64_t *live_restored)
{
    if (!c) return PLFX_ERR_STATE;
    if (direct_sweeps) *direct_sweeps = c->n_direct_sweeps;
    if (direct_acknowledged) *direct_acknowledged = c->n_direct_ack;
    if (setup_formed_late) *setup_formed_late = c->n_setup_late;
    if (live_restored) *live_restored = c->n_live_restored;
    return PLFX_OK;
}

int plfx_dead_store_info(plfx_ctx *c, int64_t *armed_sweeps, int64_t *tangents_rewritten_in_armed_sweeps, int64_t *test_only_starts,
                         int64_t *test_only_retries)
{
    if (!c) return PLFX_ERR_ARG;
    if (armed_sweeps) *armed_sweeps = c->n_dead_sweeps;
    if (tangents_rewritten_in_armed_sweeps) *tangents_rewritten_in_armed_sweeps = c->n_dead_tangents;
    if (test_only_starts) *test_only_starts = c->n_test_starts;
    if (test_only_retries) *test_only_retries = c->n_test_retries;
    return PLFX_OK;
}

int plfx_plane_info(plfx_ctx *c, int *mode_on, int64_t *plane_sweeps, int64_t *plane_updates, int *switched_off_by)
{
    if (!c) return PLFX_ERR_ARG;
    const bool on = plane_active(c);
    if (mode_on) *mode_on = on ? 1 : 0;
    if (plane_sweeps) *plane_sweeps = c->n_plane_sweeps;
    if (plane_updates) *plane_updates = c->n_plane_updates;
    if (switched_off_by) *switched_off_by = on ? PLFX_PLANE_ON : c->plane_cols ? PLFX_PLANE_SHARDED : c->plane_off_by;
    return PLFX_OK;
}

int plfx_mg_info(plfx_ctx *c, int max_levels, int *levels, int *dims, double *ratios, int *matfree_level, int *tail_level,
                 int *tail_kernel, int *coarse_solver, int *cheby_steps, double *cheby_kappa, int *march)
{
    if (!c) return PLFX_ERR_ARG;
    const int nl = mg_active(c) ? (int)c->mg.size() : 0;
    if (levels) *levels = nl;
    for (int l = 0; l < nl && l < max_levels; l++) {
        const auto &L = c->mg[l];
        if (dims) dims[2 * l] = L.nx, dims[2 * l + 1] = L.ny;
        if (ratios) ratios[2 * l] = L.rx, ratios[2 * l + 1] = L.ry;
        if (matfree_level) matfree_level[l] = (l == 0 ? matfree(c) : level_from_generators(c, l)) ? 1 : 0;
    }
    const int tail = (nl && !c->strip.on) ? mg_tail_kernel(c) : PLFX_MG_TAIL_NONE;
    if (tail_kernel) *tail_kernel = tail;
    if (tail_level) *tail_level = tail != PLFX_MG_TAIL_NONE ? c->mg_tail : -1;
    // (what mg_coarse_part does with the coarsest level: the LDS-resident tails require the dense inverse)
    const bool dense = nl && c->mg.back().ainv;
    const bool cheby = nl && !dense && tail == PLFX_MG_TAIL_NONE && c->mg_cheby > 0;
    if (coarse_solver) *coarse_solver = dense ? PLFX_MG_COARSE_DENSE : cheby ? PLFX_MG_COARSE_CHEBY : PLFX_MG_COARSE_PCG;
    if (cheby_steps) *cheby_steps = cheby ? c->mg_cheby : 0;
    if (cheby_kappa) *cheby_kappa = cheby ? c->mg_cheby_kappa : 0.;
    if (march) *march = (nl && c->mg[0].matfree && march_mg(c)) ? 1 : 0;
    return PLFX_OK;
}

int plfx_sweep_launch_info(plfx_ctx *c, int64_t *heavy_skipped, int64_t *heavy_recovered)
{
    if (!c) return PLFX_ERR_ARG;
    if (heavy_skipped) *heavy_skipped = c->n_heavy_skipped;
    if (heavy_recovered) *heavy_recovered = c->n_heavy_recovered;
    return PLFX_OK;
}

int plfx_svc_info(plfx_ctx *c, int *row_materials, int *thread_materials, int64_t *row_launches, int64_t *thread_launches)
{
    if (!c) return PLFX_ERR_ARG;
    if (row_materials) *row_materials = (int)c->svc_row_all;
    if (thread_materials) *thread_materials = (int)(c->svc6_mask & ~c->svc_row_all);
    if (row_launches) *row_launches = c->n_svc_row_launches;
    if (thread_launches) *thread_launches = c->n_svc_thread_launches;
    return PLFX_OK;
}

int plfx_reuse_info(plfx_ctx *c, int *assemblies, int *bc_applications, int *solves)
{
    if (!c) return PLFX_ERR_ARG;
    if (assemblies) *assemblies = c->n_reuse_assemble;
    if (bc_applications) *bc_applications = c->n_reuse_bc;
    if (solves) *solves = c->n_reuse_solve;
    return PLFX_OK;
}

int plfx_gen_structured(int NX, int NY, int32_t *conn, int32_t *noleft, int32_t *noright, int32_t *nobot, int32_t *notop)
{
    if (NX < 1 || NY < 1 || (int64_t)(NX + 1) * (NY + 1) > INT32_MAX) return PLFX_ERR_ARG;
    const int nyn = NY + 1;
    if (conn)
        for (int ih = 0; ih < NX * NY; ih++) {
            const int n1 = (ih / NY) * nyn + ih % NY;
            conn[4 * (size_t)ih + 0] = n1;
            conn[4 * (size_t)ih + 1] = n1 + 1;
            conn[4 * (size_t)ih + 2] = n1 + nyn;
            conn[4 * (size_t)ih + 3] = n1 + nyn + 1;
        }
    for (int k = 0; k <= NY; k++) {
        if (noleft) noleft[k] = k;
        if (noright) noright[k] = NX * nyn + k;
    }
    for (int j = 0; j <= NX; j++) {
        if (nobot) nobot[j] = j * nyn;
        if (notop) notop[j] = j * nyn + NY;
    }
    return PLFX_OK;
}

int plfx_pattern_selftest(int nx, int ny)
{
    // closed-form pattern of a structured grid (structured_slot) against the generic derivation from the connectivity
    if (nx < 2 || ny < 2 || (int64_t)(nx + 1) * (ny + 1) > (1 << 24)) return PLFX_ERR_ARG;
    const int nel = nx * ny, nnode = (nx + 1) * (ny + 1), nyn = ny + 1;
    std::vector<int32_t> conn((size_t)4 * nel), hcol, hcontrib;
    for (int e = 0; e < nel; e++) {
        const int n1 = (e / ny) * nyn + e % ny;
        conn[4 * (size_t)e] = n1;
        conn[4 * (size_t)e + 1] = n1 + 1;
        conn[4 * (size_t)e + 2] = n1 + nyn;
        conn[4 * (size_t)e + 3] = n1 + nyn + 1;
    }
    int gx = 0, gy = 0;
    if (!structured_dims(nel, nnode, conn.data(), &gx, &gy) || gx != nx || gy != ny) return 1;
    int nslot = 0, nq = 0, nb = 0, ne = 0;
    if (!build_pattern(nnode, conn.data(), 0, nel, hcol, hcontrib, nslot, nq, nb, ne)) return 2;
    if (nslot != 9 || nq != 4 || nb != 0 || ne != nnode) return 3;
    for (int i = 0; i < nnode; i++)
        for (int s = 0; s < 9; s++) {
            int32_t cj, codes[4];
            structured_slot(nx, ny, i, s, &cj, codes);
            if (cj != hcol[(size_t)s * nnode + i]) return 4;
            for (int q = 0; q < 4; q++)
                if (codes[q] != hcontrib[((size_t)s * 4 + q) * nnode + i]) return 5;
        }
    std::swap(conn[4], conn[5]);  // any other numbering is not "structured"
    if (structured_dims(nel, nnode, conn.data(), &gx, &gy)) return 6;
    return PLFX_OK;
}

int plfx_set_precond(plfx_ctx *c, int kind, double omega, int nu)
{
    if (!c) return PLFX_ERR_STATE;
    if (kind != 0 && kind != 1) return fail(c, PLFX_ERR_ARG, "precond kind must be 0 (Jacobi) or 1 (multigrid)");
    if (c->strip.on) {
        // the halo validity widths were worked out for V(2,2) and the replicated coarse context copied omega / nu at
        // plfx_set_strip: only a call that changes nothing is accepted afterwards
        if (kind != 1 || (nu > 0 && nu != c->mg_nu) || (omega > 0. && omega != c->mg_omega))
            return fail(c, PLFX_ERR_UNSUPPORTED, "plfx_set_precond after plfx_set_strip: a strip runs multigrid V(2,2) with the "
                        "smoother chosen before plfx_set_strip");
        return PLFX_OK;
    }
    if (int rcs = snap_settle(c)) return rcs;
    c->precond = kind;
    if (omega > 0.) c->mg_omega = omega;
    if (nu > 0) c->mg_nu = nu;
    mg_graph_drop(c);  // the captured launches carry omega / nu
    c->M_dirty = true;  // the next plfx_assemble (re)builds what this preconditioner needs
    return PLFX_OK;
}

int plfx_precond_info(plfx_ctx *c, int *kind, int *levels)
{
    if (!c) return PLFX_ERR_STATE;
    if (kind) *kind = mg_active(c) ? 1 : 0;
    if (levels) *levels = (int)c->mg.size();
    return PLFX_OK;
}

// measurement hook: `reps` applications of the preconditioner (z = M^-1 r on whatever r holds) back to back, timed with one
// pair of HIP events; *us_coarse = the same with the fine level's launches left out (levels >= 1 only: the restriction to
// level 1, the launch-latency-bound levels, the single-workgroup tail, the prolongation to level 0).
int plfx_precond_apply(plfx_ctx *c, const double *r, double *z)
{
    if (!c || !mg_active(c) || c->strip.on || !c->assembled || !r || !z)
        return c ? fail(c, PLFX_ERR_STATE, "needs the multigrid hierarchy of a single-GPU solve, assembled") : PLFX_ERR_STATE;
    HIPCHK(c, hipMemsetAsync(&c->sc->done, 0, sizeof(int), c->stream));  // the fine-level kernels are no-ops while it is set
    HIPCHK(c, hipMemcpyAsync(c->r, r, (size_t)8 * c->ndof, hipMemcpyHostToDevice, c->stream));
    const int rc = mg_vcycle(c);   // (mg_ensure in it forms a late fine-level dinv first)
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(z, c->z, (size_t)8 * c->ndof, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    c->memo.valid = false;   // (the work vectors of the last solve are gone)
    return PLFX_OK;
}

int plfx_precond_bench(plfx_ctx *c, int reps, double *us_per_cycle, double *us_coarse)
{
    if (!c || !mg_active(c) || c->strip.on) return c ? fail(c, PLFX_ERR_STATE, "needs the multigrid hierarchy of a single-GPU solve") : PLFX_ERR_STATE;
    if (reps < 1) reps = 1;
    {   // (the coarse levels are set up on demand: a window whose solves never needed a V-cycle leaves them stale)
        const int e = mg_ensure(c);
        if (e) return e;
    }
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0));
    HIPCHK(c, hipEventCreate(&e1));
    HIPCHK(c, hipMemsetAsync(&c->sc->done, 0, sizeof(int), c->stream));  // the fine-level kernels are no-ops while it is set
    int rc = 0;
    float ms = 0.f;
    for (int w = 0; w < 3 && !rc; w++) rc = mg_vcycle(c);
    HIPCHK(c, hipEventRecord(e0, c->stream));
    for (int k = 0; k < reps && !rc; k++) {
        rc = mg_vcycle(c);
        if ((k & 63) == 63) HIPCHK(c, stream_sync(c));  // bounded queue depth (one drain per ~17 ms of cycles: < 0.2 %)
    }
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipEventSynchronize(e1));
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    if (us_per_cycle) *us_per_cycle = 1e3 * ms / reps;
    if (us_coarse && !rc) {
        const int nl = (int)c->mg.size();
        const int lt = (c->mg_tail > 0) ? c->mg_tail : nl - 1;
        auto coarse_only = [&]() -> int {
            if (lt < 2 || !c->want_mg_graph) return mg_coarse_part(c);
            if (!c->mg_graph_exec) return mg_vcycle_rest(c, nullptr, nullptr);  // (captures the graph; not reached after the cycles above)
            return hipGraphLaunch(c->mg_graph_exec, c->stream) == hipSuccess ? 0 : PLFX_ERR_HIP;
        };
        auto &L = c->mg[0];
        auto &C1 = c->mg[1];
        HIPCHK(c, hipEventRecord(e0, c->stream));
        for (int k = 0; k < reps && !rc; k++) {
            hipLaunchKernelGGL(k_mg_restrict, dim3(grid_for(C1.nnode)), dim3(BLOCK), 0, c->stream, C1.nx + 1, C1.ny + 1, L.nx + 1, L.ny + 1,
                               (const double2 *)L.res, (const double2 *)C1.dinv, (double2 *)C1.b);
            rc = coarse_only();
            hipLaunchKernelGGL(k_mg_prolong_add, dim3(grid_for(L.nnode)), dim3(BLOCK), 0, c->stream, L.nx + 1, L.ny + 1, C1.ny + 1,
                               (const double2 *)C1.x, (const double2 *)L.dinv, (double2 *)L.x);
        }
        HIPCHK(c, hipEventRecord(e1, c->stream));
        HIPCHK(c, hipEventSynchronize(e1));
        HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
        *us_coarse = 1e3 * ms / reps;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    c->x_is_du = c->x_is_du && true;  // (c->x untouched: z and the level vectors are scratch outside a solve)
    return rc;
}

int plfx_assemble(plfx_ctx *c)
{
    if (!c || !c->dval) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    // (the set-up pass may have run already, behind the flags of the sweep that changed the tangents: sweep_once)
    // (... or have been left out, where that sweep wrote its generators into the snapshot itself: DESIGN 43)
    const bool direct = c->direct_done && matfree(c) && c->M_dirty;
    const bool setup_done = (c->spec_setup && c->spec_was_clean && c->spec_h0 != 0 && matfree(c)) || direct;
    c->spec_setup = c->spec_kdu = c->direct_done = false;
    if (c->reuse && c->assembled && !c->M_dirty) {  // no tangent changed since the last assembly: K is what it was
        c->n_reuse_assemble++;
        return PLFX_OK;
    }
    EvPair *ev;
    tim_begin(c, 3, &ev);
    if (matfree(c)) {  // operators are applied from the generators: only the diagonal is formed
        KOp live = c->op;
        live.M = c->Mel;  // diagonal + snapshot of the generators (+ generators of multigrid level 1) in one pass
        if (direct) {   // diag and the generators of level 1 are owed to their first reader (ensure_setup)
            c->n_direct_ack++;
            c->setup_owed = true;
        } else if (setup_done)
            c->n_spec_setup++;
        else {
            if (int rc = ensure_live_M(c)) return rc;
            LAUNCH_SETUP(0, live, (double2 *)c->diag,
                               c->Mop, (mg_active(c) && level_plain(c->mg[0])) ? c->mg[1].Mel : (double *)nullptr, (const double2 *)nullptr, 0, 0,
                               (double2 *)nullptr);
            c->setup_owed = false;   // (superseded)
        }
        c->dinv_ok = false;   // (c->diag rewritten, here or by the pass behind the sweep's flags)
        c->val_valid = false;
    } else {
        int rc = assemble_fine_val(c);
        if (rc) return rc;
    }
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    if (mg_active(c)) {
        if (mg_lazy(c)) {   // (an older pending set-up is superseded: only the newest generators matter)
            if (c->mg_pending) c->n_mg_setup_skipped++;
            else c->mg_pending_same = true;
            c->mg_pending = true;
        } else {
            int rc = mg_assemble(c);
            if (rc) return rc;
        }
    }
    if (c->strip.on) {
        int rc = strip_child_assemble(c);
        if (rc) return rc;
    }
    c->assembled = true;
    c->M_dirty = false;
    c->op_epoch++;
    c->memo.valid = false;
    return PLFX_OK;
}

int plfx_get_csr(plfx_ctx *c, int64_t *nnz, int32_t *rowptr, int32_t *colidx, double *val)
{
    if (!c || !c->assembled) return c ? fail(c, PLFX_ERR_STATE, "assemble first") : PLFX_ERR_STATE;
    const int nn = c->nnode, ns = c->nslot;
    int64_t cnt = 0;
    for (int i = 0; i < nn; i++) {
        int k = 0;
        for (int s = 0; s < ns; s++)
            if (host_col(c, s, i) >= 0) k++;
        cnt += 4 * (int64_t)k;
    }
    if (nnz) *nnz = cnt;
    if (!rowptr || !colidx || !val) return PLFX_OK;
    if (!c->val_valid) {
        int rc = assemble_fine_val(c);
        if (rc) return rc;
    }
    std::vector<double> hv((size_t)ns * 4 * nn);
    HIPCHK(c, hipMemcpyAsync(hv.data(), c->dval, hv.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    int64_t pos = 0;
    for (int i = 0; i < nn; i++)
        for (int rr = 0; rr < 2; rr++) {
            rowptr[2 * i + rr] = (int32_t)pos;
            for (int s = 0; s < ns; s++) {
                const int j = host_col(c, s, i);
                if (j < 0) continue;
                for (int cc = 0; cc < 2; cc++) {
                    colidx[pos] = 2 * j + cc;
                    val[pos] = hv[((size_t)s * 4 + rr * 2 + cc) * nn + i];
                    pos++;
                }
            }
        }
    rowptr[2 * nn] = (int32_t)pos;
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ BC (the solve: plfx_solve.hip)
namespace {
// calc_BC on the device.  Values of the prescribed DOFs come either from host arrays (du_presc, w: one staged copy) or,
// for a registered plan, from the per-segment values passed as kernel arguments (seg4 != null: no copy at all).
int apply_bc_impl(plfx_ctx *c, int n, const int32_t *idx, const double *du_presc, const double *w, const double *fext,
                  const int32_t *seg4, const BcSegVals *segv)
{
    const size_t nd = c->ndof;
    int rc = ensure_tmp(c, std::max(n, 1));
    if (rc) return rc;
    // The set of prescribed DOFs rarely changes between calls (same BC flags, new values): keep the mask
    // and only overwrite the values then.  Values travel through one pinned staging buffer = one copy.
    const bool same_set = c->bc_valid && (int)c->bc_idx.size() == n &&
                          (n == 0 || memcmp(c->bc_idx.data(), idx, (size_t)4 * n) == 0);
    if (!same_set) {
        c->code_ok = false;
        c->x_is_du = false;  // another Dirichlet mask: x0 has to be rebuilt from du
        c->pred_d_kept = false;   // (and pred_d was masked with the old one)
        HIPCHK(c, hipMemsetAsync(c->is_presc, 0, 8 * nd, c->stream));
        HIPCHK(c, hipMemsetAsync(c->dup, 0, 8 * nd, c->stream));
        HIPCHK(c, hipMemsetAsync(c->wv, 0, 8 * nd, c->stream));
        c->bc_idx.assign(idx, idx + n);
        if ((size_t)n > c->bc_idx_cap) {
            dfree(c->bc_idx_dev);
            if ((rc = dalloc(c, &c->bc_idx_dev, (size_t)n))) return rc;
            c->bc_idx_cap = n;
        }
        if (n > 0) {
            HIPCHK(c, hipMemcpyAsync(c->bc_idx_dev, c->bc_idx.data(), (size_t)4 * n, hipMemcpyHostToDevice, c->stream));
        }
        // rows of K that see a prescribed DOF: the neighbours (in the block-ELL pattern) of the prescribed nodes
        {
            std::vector<char> mark(c->nnode, 0);
            const int nn = c->nnode;
            for (int k = 0; k < n; k++) {
                const int i = idx[k] >> 1;
                for (int s2 = 0; s2 < c->nslot; s2++) {
                    const int j = host_col(c, s2, i);
                    if (j >= 0) mark[j] = 1;  // the pattern is symmetric: j has i as a neighbour
                }
            }
            std::vector<int32_t> rows;
            for (int i = 0; i < nn; i++)
                if (mark[i]) rows.push_back(i);
            c->bc_nrows = (int)rows.size();
            dfree(c->bc_rows);
            if ((rc = dalloc(c, &c->bc_rows, rows.size()))) return rc;
            if (!rows.empty())
                HIPCHK(c, hipMemcpyAsync(c->bc_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, c->stream));
            if (!c->kw && (rc = dalloc(c, &c->kw, nd))) return rc;
            HIPCHK(c, hipMemsetAsync(c->kw, 0, 8 * nd, c->stream));
            c->rhs_rows_ok = false;   // another row list, kw rebuilt: rhs needs one full pass
            // the node code of the same idx and the same mark: the mask as is_presc will hold it, the rows as bc_rows does
            std::vector<uint8_t> code(((size_t)nn + 255) / 256 * 256, 0);
            for (int i = 0; i < nn; i++)
                if (mark[i]) code[i] = 4;
            for (int k = 0; k < n; k++) code[idx[k] >> 1] |= (uint8_t)(1 << (idx[k] & 1));
            HIPCHK(c, hipMemcpyAsync(c->ncode, code.data(), code.size(), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, stream_sync(c));  // `rows` and `code` go out of scope
            c->code_ok = true;
            c->n_code_built++;
        }
        c->bc_valid = true;
        c->rhs_rows_ok = c->dinv_ok = false;   // (another mask: dinv and the zeros of rhs belong to the old one)
    }
    if (c->reuse && seg4 && same_set && c->bc_set && c->bc_memo && c->bc_epoch == c->op_epoch && !fext && !c->bc_memo_fext &&
        memcmp(&c->bc_last, segv, sizeof(BcSegVals)) == 0) {
        c->n_reuse_bc++;  // same plan, same values, same operator: rhs, prescribed values and masks are what they were
        return PLFX_OK;
    }
    c->memo.valid = false;  // another system
    c->bc_memo = seg4 != nullptr;
    if (seg4) {
        c->bc_last = *segv;
        c->bc_epoch = c->op_epoch;
        c->bc_memo_fext = fext != nullptr;
    }
    if (n > 0 && seg4) {
        hipLaunchKernelGGL(k_scatter_bc_plan, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, n, c->bc_idx_dev,
                           seg4, *segv, c->dup, c->wv, c->is_presc, same_set ? 0 : 1);
        HIPCHK(c, hipGetLastError());
    } else if (n > 0) {
        if ((size_t)n > c->stage_cap) {
            HIPCHK(c, stream_sync(c));
            if (c->stage) hipHostFree(c->stage);
            c->stage = nullptr;
            HIPCHK(c, hipHostMalloc((void **)&c->stage, (size_t)32 * n));
            c->stage_cap = n;
            c->stage_busy[0] = c->stage_busy[1] = false;
        }
        // no stream-wide sync: only wait until the copy that last read this half has finished
        const int h = c->stage_flip;
        c->stage_flip ^= 1;
        if (!c->stage_ev[h]) HIPCHK(c, hipEventCreateWithFlags(&c->stage_ev[h], hipEventDisableTiming));
        if (c->stage_busy[h]) HIPCHK(c, hipEventSynchronize(c->stage_ev[h]));
        double *st = c->stage + (size_t)h * 2 * c->stage_cap;
        memcpy(st, du_presc, (size_t)8 * n);
        memcpy(st + n, w, (size_t)8 * n);
        HIPCHK(c, hipMemcpyAsync(c->val_tmp, st, (size_t)16 * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->stage_ev[h], c->stream));
        c->stage_busy[h] = true;
        hipLaunchKernelGGL(k_scatter_bc, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, n, c->bc_idx_dev,
                           c->val_tmp, c->val_tmp + n, c->dup, c->wv, c->is_presc, same_set ? 0 : 1);
        HIPCHK(c, hipGetLastError());
    }
    if (fext) HIPCHK(c, hipMemcpyAsync(c->fext, fext, 8 * nd, hipMemcpyHostToDevice, c->stream));
    // rhs = fext - K w and dinv.  Without a force vector rhs can differ from what it was on bc_rows only, and dinv is a function
    // of (diag, is_presc): with the set and the row list of the last full pass, k_spmv_rows writes rhs on its rows and dinv is
    // formed again only if the diagonal was rewritten since.  One GPU, no strip; the full pass otherwise.
    const bool rows_only = c->bc_rows_on && c->reuse && !c->strip.on && !comm_active(c) && c->rhs_rows_ok && same_set && !fext &&
                           c->bc_nrows > 0;
    const double2 *rm = rows_only ? (const double2 *)c->is_presc : nullptr;
    double2 *rr = rows_only ? (double2 *)c->rhs : nullptr;
    if (c->bc_nrows > 0)  // K w on the few rows where it can be non-zero
    {
        if (matfree(c) && c->op.colr)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_rows<2>), dim3((c->bc_nrows + BLOCK - 1) / BLOCK), dim3(BLOCK), 0,
                               c->stream, c->bc_nrows, c->bc_rows, c->op, (const double2 *)c->wv, (double2 *)c->kw, rm, rr);
        else if (matfree(c))
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_rows<1>), dim3((c->bc_nrows + BLOCK - 1) / BLOCK), dim3(BLOCK), 0,
                               c->stream, c->bc_nrows, c->bc_rows, c->op, (const double2 *)c->wv, (double2 *)c->kw, rm, rr);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spmv_rows<0>), dim3((c->bc_nrows + BLOCK - 1) / BLOCK), dim3(BLOCK), 0,
                               c->stream, c->bc_nrows, c->bc_rows, c->op, (const double2 *)c->wv, (double2 *)c->kw, rm, rr);
    }
    if (rows_only) {
        c->n_rhs_rows++;
        if (c->dinv_ok)
            c->n_dinv_kept++;   // (dinv_late stands as it is: still the mask of this set, still unformed)
        else if ((c->short_solve & 1) && mg_lazy(c) && mg_active(c) && c->mg_pending) {
            // The coarse levels wait for the first V-cycle, and so does the fine level's dinv: until then its readers
            // only test dinv != 0, and the old dinv answers that test as the new one would -- same_set holds on this branch, and
            // free ? 1/|diag| : 0 is non-zero on every free DOF whatever the diagonal.  PRECONDITION: diag is finite (1/inf = 0
            // would take a DOF out of the pattern; k_dinv maps 0, denormals and NaN to non-zero values).
            c->dinv_late = true;
            c->n_dinv_refreshed++;   // (rows_only = kept + refreshed as before; n_dinv_deferred says how many of these were left open)
            c->n_dinv_deferred++;
        } else {
            if ((rc = ensure_setup(c))) return rc;
            hipLaunchKernelGGL(k_dinv, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->diag, c->is_presc, c->dinv);
            c->n_dinv_refreshed++;
            c->dinv_late = false;
        }
    } else {
        if ((rc = ensure_setup(c))) return rc;
        hipLaunchKernelGGL(k_bc_finish, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd,
                           fext ? c->fext : nullptr, c->kw, c->diag, c->is_presc, c->rhs, c->dinv);
        c->rhs_rows_ok = !fext;
        c->dinv_late = false;   // (written for every DOF)
    }
    c->dinv_ok = true;
    HIPCHK(c, hipGetLastError());
    if (fext) HIPCHK(c, stream_sync(c));
    if (mg_active(c)) {
        if (c->mg_pending)
            c->mg_pending_same = c->mg_pending_same && same_set;
        else {
            rc = mg_update_dinv(c, same_set);
            if (rc) return rc;
        }
    }
    if (c->strip.on && (rc = strip_child_dinv(c))) return rc;
    c->bc_set = true;
    return PLFX_OK;
}
}  // namespace

int plfx_apply_bc(plfx_ctx *c, int n, const int32_t *idx, const double *du_presc, const double *w,
                  const double *fext)
{
    if (!c || !c->assembled) return c ? fail(c, PLFX_ERR_STATE, "assemble first") : PLFX_ERR_STATE;
    if (n < 0 || (n > 0 && (!idx || !du_presc || !w))) return fail(c, PLFX_ERR_ARG, "bad argument");
    for (int k = 0; k < n; k++)
        if (idx[k] < 0 || idx[k] >= c->ndof) return fail(c, PLFX_ERR_ARG, "presc_idx[%d] out of range", k);
    return apply_bc_impl(c, n, idx, du_presc, w, fext, nullptr, nullptr);
}

int plfx_set_bc_plan(plfx_ctx *c, int nseg, const int32_t *seg_len, const int32_t *idx)
{
    if (!c || !c->u) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    if (nseg < 0 || (nseg > 0 && (!seg_len || !idx))) return fail(c, PLFX_ERR_ARG, "bad argument");
    auto &P = c->plan;
    P.valid = false;
    c->bc_memo = false;  // values are compared per segment: another plan, another meaning
    c->memo.valid = false;
    P.nseg = nseg;
    P.seg_of.clear();
    std::vector<int32_t> all;
    for (int s2 = 0, o = 0; s2 < nseg; s2++) {
        if (seg_len[s2] < 0) return fail(c, PLFX_ERR_ARG, "negative segment length");
        for (int k = 0; k < seg_len[s2]; k++, o++) {
            if (idx[o] < 0 || idx[o] >= c->ndof) return fail(c, PLFX_ERR_ARG, "plan index %d out of range", o);
            all.push_back(idx[o]);
            P.seg_of.push_back(s2);
        }
    }
    // ascending unique DOFs, first occurrence and inverse map (what numpy.unique(return_index, return_inverse) gives)
    const int n = (int)all.size();
    std::vector<int32_t> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a2, int b2) { return all[a2] < all[b2]; });
    P.presc.clear();
    P.first_pos.clear();
    P.inv.assign(n, 0);
    for (int q2 = 0; q2 < n; q2++) {
        const int i = order[q2];
        if (q2 == 0 || all[i] != all[order[q2 - 1]]) {
            P.presc.push_back(all[i]);
            P.first_pos.push_back(i);  // stable sort: the first entry of a run is the first occurrence
        }
        P.inv[i] = (int32_t)P.presc.size() - 1;
    }
    P.first.assign(P.presc.size(), 0.);
    P.w.assign(P.presc.size(), 0.);
    dfree(P.seg4);
    if (nseg <= BcSegVals::N && !P.presc.empty()) {  // entries of every DOF in entry order (= the host's summation order)
        const size_t np = P.presc.size();
        std::vector<int32_t> t(4 * np, -1);
        std::vector<int> cnt(np, 0);
        bool ok = true;
        for (int i = 0; i < n && ok; i++) {
            const int k = P.inv[i];
            if (cnt[k] == 4)
                ok = false;
            else
                t[4 * (size_t)k + cnt[k]++] = P.seg_of[i];
        }
        if (ok) {
            int rc = dalloc(c, &P.seg4, t.size());
            if (rc) return rc;
            HIPCHK(c, hipMemcpyAsync(P.seg4, t.data(), t.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, stream_sync(c));
        }
    }
    P.valid = true;
    return PLFX_OK;
}

int plfx_apply_bc_plan(plfx_ctx *c, const double *seg_val, const double *fext, int *inconsistent_entry)
{
    if (!c || !c->plan.valid) return c ? fail(c, PLFX_ERR_STATE, "set_bc_plan first") : PLFX_ERR_STATE;
    auto &P = c->plan;
    if (P.nseg > 0 && !seg_val) return fail(c, PLFX_ERR_ARG, "segment values required");
    const int n = (int)P.seg_of.size(), np = (int)P.presc.size();
    for (int k = 0; k < np; k++) {
        P.first[k] = seg_val[P.seg_of[P.first_pos[k]]];
        P.w[k] = 0.;
    }
    int bad = -1;
    for (int i = 0; i < n; i++) {  // multiplicity-weighted value (a DOF on two edges enters the rhs twice, model.py:1115-1122)
        const double v = seg_val[P.seg_of[i]];
        P.w[P.inv[i]] += v;
        if (bad < 0 && v != P.first[P.inv[i]]) bad = i;
    }
    if (inconsistent_entry) *inconsistent_entry = bad;
    if (P.seg4) {  // first = value of the first entry, w = sum over the entries: formed on the device from the segment values
        if (!c->assembled) return fail(c, PLFX_ERR_STATE, "assemble first");
        BcSegVals sv;
        for (int i = 0; i < BcSegVals::N; i++) sv.v[i] = i < P.nseg ? seg_val[i] : 0.;
        return apply_bc_impl(c, np, P.presc.data(), nullptr, nullptr, fext, P.seg4, &sv);
    }
    return plfx_apply_bc(c, np, P.presc.data(), P.first.data(), P.w.data(), fext);
}

int plfx_set_bc_sources(plfx_ctx *c, int nseg, const int32_t *src, const int32_t *k, int nf, const int32_t *fsrc,
                        const int32_t *fk, const int32_t *flen, const int32_t *fidx, const double *fshare)
{
    if (!c || !c->plan.valid) return c ? fail(c, PLFX_ERR_STATE, "set_bc_plan first") : PLFX_ERR_STATE;
    auto &P = c->plan;
    P.sources = false;
    if (nseg != P.nseg || nf < 0) return fail(c, PLFX_ERR_ARG, "segment count differs from the registered plan");
    for (int i = 0; i < nseg; i++)
        if (src[i] < 0 || src[i] > 4 || k[i] < 0 || k[i] > 1) return fail(c, PLFX_ERR_ARG, "bad segment source");
    P.src.assign(src, src + nseg);
    P.k.assign(k, k + nseg);
    P.fsrc.assign(fsrc, fsrc + nf);
    P.fk.assign(fk, fk + nf);
    P.flen.assign(flen, flen + nf);
    size_t tot = 0;
    for (int i = 0; i < nf; i++) {
        if (fsrc[i] < 2 || fsrc[i] > 4 || fk[i] < 0 || fk[i] > 1 || flen[i] < 0)
            return fail(c, PLFX_ERR_ARG, "bad force segment");
        tot += flen[i];
    }
    for (size_t q = 0; q < tot; q++)
        if (fidx[q] < 0 || fidx[q] >= c->ndof) return fail(c, PLFX_ERR_ARG, "force DOF out of range");
    P.fidx.assign(fidx, fidx + tot);
    P.fshare.assign(fshare, fshare + tot);
    P.sources = true;
    return PLFX_OK;
}

int plfx_matvec(plfx_ctx *c, const double *x, double *y)
{
    if (!c || !c->assembled) return c ? fail(c, PLFX_ERR_STATE, "assemble first") : PLFX_ERR_STATE;
    if (!x || !y) return fail(c, PLFX_ERR_ARG, "null argument");
    const size_t nd = c->ndof;
    // p[0] / q are free between solves (plfx_solve re-initialises both)
    HIPCHK(c, hipMemcpyAsync(c->p[0], x, 8 * nd, hipMemcpyHostToDevice, c->stream));
    int rc = plain_spmv(c, c->p[0], c->q);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(y, c->q, 8 * nd, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    return PLFX_OK;
}

int plfx_comm_info(plfx_ctx *c, int *rank, int *nranks, int *device_collectives)
{
    if (!c) return PLFX_ERR_ARG;
    if (rank) *rank = c->rank;
    if (nranks) *nranks = c->nranks;
    if (device_collectives) *device_collectives = comm_active(c) ? 1 : 0;
    return PLFX_OK;
}

int plfx_comm_unique_id(char id[128])
{
    if (!id) return PLFX_ERR_ARG;
    if (!load_rccl()) return PLFX_ERR_UNSUPPORTED;
    ncclUniqueId u;
    if (g_rccl.GetUniqueId(&u) != 0) return PLFX_ERR_HIP;
    memcpy(id, u.internal, 128);
    return PLFX_OK;
}

int plfx_comm_init(plfx_ctx *c, const char id[128], int rank, int nranks)
{
    if (!c || !c->stream) return PLFX_ERR_STATE;
    if (!id || rank < 0 || rank >= nranks) return fail(c, PLFX_ERR_ARG, "bad rank/nranks");
    if (!load_rccl()) return fail(c, PLFX_ERR_UNSUPPORTED, "librccl.so not found");
    ncclUniqueId u;
    memcpy(u.internal, id, 128);
    HIPCHK(c, hipSetDevice(c->device));
    int nrc = g_rccl.CommInitRank(&c->comm, nranks, u, rank);
    // a communicator without peers can be retried safely (the bootstrap of RCCL occasionally fails right after another
    // process on the box released its sockets); with peers a retry on one rank would dead-lock the others
    for (int attempt = 0; nrc != 0 && nranks == 1 && attempt < 3; attempt++) {
        std::this_thread::sleep_for(std::chrono::milliseconds(300));
        ncclUniqueId u2;
        if (g_rccl.GetUniqueId(&u2) != 0) break;
        nrc = g_rccl.CommInitRank(&c->comm, 1, u2, 0);
    }
    if (nrc != 0) return fail(c, PLFX_ERR_HIP, "ncclCommInitRank failed (RCCL result %d)", nrc);
    c->rank = rank;
    c->nranks = nranks;
    return PLFX_OK;
}

// ncclSend / ncclRecv of this rank to itself inside one group, and an all-reduce, on scratch buffers: checks the entry points
// bound by dlsym (signatures, the data-type and reduction constants) on hardware where no second GPU is at hand
int plfx_comm_selftest(plfx_ctx *c)
{
    if (!c || !c->stream) return PLFX_ERR_STATE;
    if (!c->comm) return fail(c, PLFX_ERR_STATE, "no RCCL communicator (plfx_comm_init first)");
    if (!g_rccl.Send || !g_rccl.Recv || !g_rccl.GroupStart || !g_rccl.GroupEnd)
        return fail(c, PLFX_ERR_UNSUPPORTED, "this RCCL has no ncclSend/ncclRecv");
    const int n = 4096;
    double *buf = nullptr;
    int rc = dalloc(c, &buf, (size_t)3 * n);
    if (rc) return rc;
    std::vector<double> h(n), back(n), red(n);
    for (int i = 0; i < n; i++) h[i] = 1.5 * i - 7. + c->rank;
    HIPCHK(c, hipMemcpyAsync(buf, h.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(buf + 2 * n, h.data(), 8 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(buf + n, 0, 8 * n, c->stream));
    int r1 = g_rccl.GroupStart();
    if (!r1) r1 = g_rccl.Send(buf, n, NCCL_FLOAT64, c->rank, c->comm, c->stream);
    if (!r1) r1 = g_rccl.Recv(buf + n, n, NCCL_FLOAT64, c->rank, c->comm, c->stream);
    const int r2 = g_rccl.GroupEnd();
    const int r3 = g_rccl.AllReduce(buf + 2 * n, buf + 2 * n, n, NCCL_FLOAT64, NCCL_SUM, c->comm, c->stream);
    HIPCHK(c, hipMemcpyAsync(back.data(), buf + n, 8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(red.data(), buf + 2 * n, 8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_sync(c));
    dfree(buf);
    if (r1 || r2 || r3) return fail(c, PLFX_ERR_HIP, "RCCL self test: send/recv %d, group end %d, all-reduce %d", r1, r2, r3);
    for (int i = 0; i < n; i++)
        if (back[i] != h[i]) return fail(c, PLFX_ERR_HIP, "RCCL self test: received %g instead of %g at %d", back[i], h[i], i);
    if (c->nranks == 1)
        for (int i = 0; i < n; i++)
            if (red[i] != h[i]) return fail(c, PLFX_ERR_HIP, "RCCL self test: all-reduce over one rank changed entry %d", i);
    return PLFX_OK;
}

int plfx_comm_init_callback(plfx_ctx *c, int rank, int nranks, plfx_allreduce_fn fn, void *user)
{
    if (!c || !c->stream) return PLFX_ERR_STATE;
    if (!fn || rank < 0 || rank >= nranks) return fail(c, PLFX_ERR_ARG, "bad rank/nranks/callback");
    if (c->comm) return fail(c, PLFX_ERR_STATE, "an RCCL communicator is already active");
    c->host_ar = fn;
    c->host_ar_user = user;
    c->rank = rank;
    c->nranks = nranks;
    return PLFX_OK;
}

// ------------------------------------------------------------------------------ instrumentation
int plfx_timing_enable(plfx_ctx *c, int on)
{
    if (!c) return PLFX_ERR_STATE;
    c->tim.on = on != 0;
    if (c->tim.on && c->tim.ring.empty()) {  // create the event ring now, not inside the first timed launch
        c->tim.ring.resize(2048);
        for (auto &e : c->tim.ring) {
            hipEventCreate(&e.a);
            hipEventCreate(&e.b);
            e.pending = false;
        }
        // first use of an event makes the runtime allocate its completion signal (pool growth costs milliseconds when
        // it happens in the middle of a timed region): touch every event once now
        for (auto &e : c->tim.ring) {
            hipEventRecord(e.a, c->stream);
            hipEventRecord(e.b, c->stream);
        }
        stream_sync(c);
    }
    return PLFX_OK;
}

int plfx_timing_select(plfx_ctx *c, unsigned mask)
{
    if (!c) return PLFX_ERR_STATE;
    c->tim.mask = mask;
    return PLFX_OK;
}

int plfx_timing_sample(plfx_ctx *c, int every)
{
    if (!c) return PLFX_ERR_STATE;
    c->tim.every = every < 1 ? 1 : every;
    return PLFX_OK;
}

int plfx_timing_reset(plfx_ctx *c)
{
    if (!c) return PLFX_ERR_STATE;
    tim_flush(c);
    for (int i = 0; i < 8; i++) {
        c->tim.ms[i] = 0.;
        c->tim.n[i] = 0;
        c->tim.noop[i] = 0;
        c->tim.seen[i] = 0;
    }
    return PLFX_OK;
}

int plfx_timing_get(plfx_ctx *c, int which, double *ms, int64_t *launches)
{
    if (!c || which < 0 || which >= 8) return PLFX_ERR_ARG;
    tim_flush(c);
    if (ms) *ms = c->tim.ms[which];
    // no-op launches (PCG already converged) are counted for every launch, timed ones only for the sampled share
    if (launches) *launches = c->tim.n[which] - (c->tim.noop[which] + c->tim.every / 2) / c->tim.every;
    return PLFX_OK;
}

}  // extern "C"
