// plfx.hip -- host side of libplfx.so: context, HBM residency, C-ABI (include/plfx.h) -- all but the sweeps, the load step and the
// state access, which are plfx_step.hip.  What the two units share is plfx_host.hpp; unit map and the rule that every kernel has
// one owning unit: DESIGN.md section 39.  This unit owns the kernels of all the groups below but PLFX_UNIT_STEP.
#define PLFX_UNIT_CONTEXT
#define PLFX_UNIT_MATERIALS
#define PLFX_UNIT_MESH
#define PLFX_UNIT_OPERATOR
#define PLFX_UNIT_SOLVE
#include "plfx_host.hpp"
#include "plfx_mg.hpp"
#include "plfx_texflow.hpp"
#include "plfx_flow.hpp"

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

}  // namespace host
}  // namespace plfx

namespace plfx {
namespace host {

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
    c->bc_valid = false;
    c->bc_idx.clear();
    c->plan.valid = false;
    dfree(c->fin_idx);
    dfree(c->fin_dev);
    c->fin_n = 0;
    dfree(c->kw);
    dfree(c->bc_rows);
    c->bc_nrows = 0;
    c->rhs_rows_ok = c->dinv_ok = c->dinv_late = false;
    dfree(c->tex_ids);
    c->htex_ids.clear();
    c->tex_ids_ok = false;
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

int plain_spmv(plfx_ctx *c, const double *in, double *out)
{
    LAUNCH_OP2(k_spmv, 0, matfree(c), dim3(c->grid_nodes), c->op, 0, c->nnode, (const double2 *)in, nullptr, nullptr,
               (double2 *)out, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 0);
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
        hipLaunchKernelGGL(k_jacobi_z, dim3(grid_for(c->nnode)), dim3(BLOCK), 0, c->stream, c->nnode, (const double2 *)c->dinv,
                           (const double2 *)c->r, (double2 *)c->z, c->sc);
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

// ---- launches of this unit's kernels on behalf of the step unit (one owner per kernel)
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

}  // namespace host
}  // namespace plfx

#include "plfx_svm.hpp"

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
        unsigned long long h[16];
        // (g_prof is a device variable per unit: this unit's copy plus the step unit's, whose kernels hold most of the regions)
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_prof), sizeof(h)) == hipSuccess && prof_regions_add(h) && h[7]) {
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
int plfx_load_path(plfx_ctx *c, int mat, int n, int K, const double *dload, int shared, const int32_t *control,
                   const double *sig0, const double *epl0, const int32_t *tex_id, int maxit, int newton, double stol,
                   double eps_cap, double *sig, double *epl, double *deps, double *fy, int32_t *nsteps, int32_t *newton_out,
                   int32_t *ksteps, int32_t *status, double *ct)
{
    if (!c || !c->dmat) return c ? fail(c, PLFX_ERR_STATE, "set_materials first") : PLFX_ERR_STATE;
    if (mat < 0 || mat >= c->nmat) return fail(c, PLFX_ERR_ARG, "load_path: material %d, the context holds %d", mat, c->nmat);
    const MatDev &hm = c->hmat[mat];
    const bool row = (hm.kind == PLFX_SVC6 || hm.kind == PLFX_SVC6_COLS) && ((c->svc_row_all >> mat) & 1u);
    int kind = 0;   // instantiation of k_path_batch
    if (hm.kind == PLFX_ELASTIC || hm.kind == PLFX_HILL6)
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
    if (n == 0) return PLFX_OK;
    if (!ksteps || !status || (K > 0 && (!dload || !sig || !epl || !deps || !fy || !nsteps || !newton_out)))
        return fail(c, PLFX_ERR_ARG, "load_path: null argument");
    const size_t N = n, KK = K, nd = shared ? 1 : N;
    if (KK * N * 19 > (size_t)INT32_MAX) return fail(c, PLFX_ERR_ARG, "load_path: K n 19 = %zu exceeds INT32_MAX", KK * N * 19);
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
    // one buffer in: dload | sig0 | epl0 | control, tex_id (int32)
    const size_t o_s0 = KK * nd * 6, o_e0 = o_s0 + (sig0 ? 6 * N : 0), o_int = o_e0 + (epl0 ? 6 * N : 0);
    const size_t n_int = (control ? N : 0) + (field ? N : 0), in_words = o_int + (n_int + 1) / 2;
    const std::unique_ptr<double[]> hin(new double[std::max<size_t>(in_words, 1)]);   // (not zeroed: every word sent is written)
    memcpy(hin.get(), dload, o_s0 * 8);
    if (sig0) memcpy(hin.get() + o_s0, sig0, N * 48);
    if (epl0) memcpy(hin.get() + o_e0, epl0, N * 48);
    int32_t *hint = (int32_t *)(hin.get() + o_int);
    if (n_int & 1) hint[n_int] = 0;
    if (control) memcpy(hint, control, N * 4);
    if (field) memcpy(hint + (control ? N : 0), tex_id, N * 4);
    // one buffer out: sig | epl | deps | fy | ct | nsteps, newton, ksteps, status (int32)
    const size_t KN = KK * N, o_ct = 19 * KN, o_oi = o_ct + (ct ? 36 * N : 0), out_words = o_oi + KN + N;
    CallBuffers B;
    double *d_in = nullptr, *d_out = nullptr;
    if (int rc = B.put(c, &d_in, (const double *)hin.get(), in_words)) return rc;
    if (int rc = B.get(c, &d_out, out_words)) return rc;
    const int32_t *d_int = (const int32_t *)(d_in + o_int);
    int32_t *d_oi = (int32_t *)(d_out + o_oi);
    PathArgs a;
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
    EvPair *ev;
    tim_begin(c, 0, &ev);
    if (row)
        launch_path_row(c, mat, field ? d_int + (control ? N : 0) : nullptr, a);
    else if (kind == 1)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_batch<1>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, mat, a);
    else if (kind == 2)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_batch<2>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, mat, a);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_batch<5>), dim3(grid_for(N)), dim3(BLOCK), 0, c->stream, c->dmat, c->nmat, mat, a);
    tim_end(c, ev);
    HIPCHK(c, hipGetLastError());
    c->path_launches++;
    // one copy out: straight into the caller's arrays where they lie in one block in the order of the device buffer (the Python
    // binding's do), else through a staging block
    const bool packed = epl == sig + 6 * KN && deps == sig + 12 * KN && fy == sig + 18 * KN && (!ct || ct == sig + o_ct) &&
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
    if (ct) memcpy(ct, hout.get() + o_ct, N * 288);
    const int32_t *hoi = (const int32_t *)(hout.get() + o_oi);
    memcpy(nsteps, hoi, KN * 4);
    memcpy(newton_out, hoi + KN, KN * 4);
    memcpy(ksteps, hoi + 2 * KN, N * 4);
    memcpy(status, hoi + 2 * KN + N, N * 4);
    return PLFX_OK;
}

int plfx_load_path_info(plfx_ctx *c, int64_t *launches)
{
    if (!c) return PLFX_ERR_ARG;
    if (launches) *launches = c->path_launches;
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
    c->bc_valid = false;
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
        mg_graph_drop(c);
        c->want_matfree = kind;
        c->assembled = false, c->M_dirty = true;  // diagonal / matrix values of the other form have to be rebuilt
        c->bc_set = false;
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

int plfx_predict_info(plfx_ctx *c, int64_t *applied, int64_t *skipped, int64_t *rejected)
{
    if (!c) return PLFX_ERR_ARG;
    if (applied) *applied = c->n_pred;
    if (skipped) *skipped = c->n_pred_skipped;
    if (rejected) *rejected = c->n_pred_rejected;
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

int plfx_solve_fallbacks(plfx_ctx *c, int64_t *count)
{
    if (!c || !count) return PLFX_ERR_ARG;
    *count = (int64_t)c->mg_fallbacks + c->n_indefinite;
    return PLFX_OK;
}

int plfx_assemble(plfx_ctx *c)
{
    if (!c || !c->dval) return c ? fail(c, PLFX_ERR_STATE, "set_mesh first") : PLFX_ERR_STATE;
    // (the set-up pass may have run already, behind the flags of the sweep that changed the tangents: sweep_once)
    const bool setup_done = c->spec_setup && c->spec_was_clean && c->spec_h0 != 0 && matfree(c);
    c->spec_setup = c->spec_kdu = false;
    if (c->reuse && c->assembled && !c->M_dirty) {  // no tangent changed since the last assembly: K is what it was
        c->n_reuse_assemble++;
        return PLFX_OK;
    }
    EvPair *ev;
    tim_begin(c, 3, &ev);
    if (matfree(c)) {  // operators are applied from the generators: only the diagonal is formed
        KOp live = c->op;
        live.M = c->Mel;  // diagonal + snapshot of the generators (+ generators of multigrid level 1) in one pass
        if (setup_done)
            c->n_spec_setup++;
        else
            LAUNCH_SETUP(0, live, (double2 *)c->diag,
                               c->Mop, (mg_active(c) && level_plain(c->mg[0])) ? c->mg[1].Mel : (double *)nullptr, (const double2 *)nullptr, 0, 0,
                               (double2 *)nullptr);
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

// ------------------------------------------------------------------------------ BC + solve
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
            HIPCHK(c, stream_sync(c));  // `rows` goes out of scope
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
            hipLaunchKernelGGL(k_dinv, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->diag, c->is_presc, c->dinv);
            c->n_dinv_refreshed++;
            c->dinv_late = false;
        }
    } else {
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

}  // extern "C"

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
        hipLaunchKernelGGL(k_jacobi_z, dim3(grid_for(nn)), dim3(BLOCK), 0, c->stream, nn, (const double2 *)c->dinv,
                           (const double2 *)c->r, (double2 *)c->z, c->sc);
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
int compose_du(plfx_ctx *c)
{
    int rc;
    if (c->strip.on && (rc = halo_refresh(c, c->x))) return rc;
    hipLaunchKernelGGL(k_compose_du, dim3(grid_for(c->ndof)), dim3(BLOCK), 0, c->stream, c->ndof, c->x, c->dup, c->is_presc, c->du);
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
        hipLaunchKernelGGL(k_cg_start_pred, dim3(gn), dim3(BLOCK), 0, c->stream, c->op, nn, (const double2 *)c->x, (const double2 *)c->pred_d,
                           (const double2 *)c->rhs, (const double2 *)c->dinv, (double2 *)c->r, (double2 *)c->p[0], s.P_rr[1], s.P_bb);
    } else if (c->test_starts && s.mg && wait_first_on() && s.pred_active && site >= 0 && c->first_test_hint[site] && !c->strip.on &&
               !comm_active(c) && matfree(c)) {
        // solve_first_test will wait for the first test before it enqueues anything that reads r or z, and expects it to pass:
        // the sums of that test alone.  If it fails, k_cg_start follows there.
#define TEST_START(G)                                                                                                          \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cg_start_test<G>), dim3(gn), dim3(BLOCK), 0, c->stream, c->op, nn, 1, (const double2 *)c->x, \
                       (const double2 *)c->rhs, (const double2 *)c->dinv, s.P_rr[1], s.P_bb, s.olo, s.ohi)
        if (c->op.colr) TEST_START(2); else TEST_START(1);   // (the matrix-free instantiations, as LAUNCH_OP1 picks them)
#undef TEST_START
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
            hipLaunchKernelGGL(k_compose_du, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, c->x, c->dup, c->is_presc, c->du,
                               (const CgScalars *)c->sc);
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
            LAUNCH_OP2(k_spmv, 0, matfree(c), dim3(gn), c->op, 0, nn, (const double2 *)c->pred_d, nullptr, nullptr, (double2 *)c->p[0],
                       nullptr, nullptr, nullptr, 0, nullptr, c->sc, 0, 0, 0);
        }
        const int gp = MAXPART;   // (one size on every rank: the all-reduce of the partial sums pairs up)
        hipLaunchKernelGGL(k_pred_dots, dim3(gp), dim3(BLOCK), 0, c->stream, (size_t)2 * olo, (size_t)2 * ohi, c->dinv, c->r, c->p[0],
                           c->part, c->sc);
        HIPCHK(c, hipGetLastError());
        if (c->strip.on && (rc = part_allreduce(c, c->part, (size_t)2 * MAXPART))) return rc;
        hipLaunchKernelGGL(k_pred_try, dim3(gn), dim3(BLOCK), 0, c->stream, nn, c->sc, (const double *)c->part, gp, (const double2 *)c->r,
                           (const double2 *)c->p[0], (const double2 *)c->dinv, s.P_rr[0], olo, ohi);
        HIPCHK(c, hipGetLastError());
        if (c->strip.on && (rc = part_allreduce(c, s.P_rr[0], gn))) return rc;
        seq = cg_check_post(c, s.P_rr[0], gn, -2);   // (iters = -2 marks "converged by the interpolated start")
        if (!c->strip.on)   // x, du and the history in one pass -- behind the test, before the host has seen it (no-op unless accepted)
            hipLaunchKernelGGL(k_pred_finish, dim3(grid_for(nd)), dim3(BLOCK), 0, c->stream, nd, (const CgScalars *)c->sc, c->x,
                               c->pred_d, c->pred_x, (const double *)c->dup, (const double *)c->is_presc, c->du,
                               ((c->short_solve & 2) && !comm_active(c)) ? 1 : 0);
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
    if (!s.pred_finished && !s.du_early && (rc = compose_du(c))) return rc;
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

int plfx_solve(plfx_ctx *c, double rtol, int maxit, int warm, int *iters, double *relres)
{
    if (!c || !c->bc_set) return c ? fail(c, PLFX_ERR_STATE, "apply_bc first") : PLFX_ERR_STATE;
    return solve_impl(c, rtol, maxit, warm, -1, iters, relres);
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
