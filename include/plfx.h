/*
 * plfx.h — C-ABI of libplfx.so, the MI355X (gfx950) engine for pyLabFEA's hot path.
 *
 * The reference (pyLabFEA v4.4.2, pure Python) has no FFI: its boundary is the Python object
 * API Model.solve() -> Element.* -> Material.response().  Every entry point below replaces the
 * reference function cited next to it (paths relative to /root/reference/src/pylabfea) and is
 * what a ctypes binding inside the reference would call (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; all host arrays are caller-owned, C-contiguous,
 *     `double` / `int32_t`, and are not retained after the call returns (copied to HBM).
 *   - Voigt order (11,22,33,23,13,12), engineering shear strains; 6x6 matrices row-major [36].
 *   - host-side per-point arrays are AoS ([n*6], [n*36]) exactly like the NumPy arrays of the
 *     reference; the SoA layout in HBM is private to the library (DESIGN.md "Data layout").
 *   - every function returns 0 on success, <0 on error (plfx_last_error gives the text);
 *     soft failures of the reference (warnings.warn) are returned as counters/flags.
 *   - one context per host thread; a context is bound to one GPU and one HIP stream.
 */
#ifndef PLFX_H
#define PLFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plfx_ctx plfx_ctx;

/* yield-function kinds */
enum {
    PLFX_ELASTIC = 0, /* Material.sy is None: no response() call (model.py:1341) */
    PLFX_HILL6 = 1,   /* analytic Hill-6p on the full Voigt stress, J2 = all ones (material.py:650-661) */
    PLFX_PRINC3 = 2,  /* sdim=3: Hill-3p/J2 on principal stresses in sig_princ's axis-tracking order
                         (material.py:662-670, basic.py:107-179); exact for plane stress states */
    PLFX_SVC6 = 3,    /* RBF-SVC yield function on 6 stress features (material.py:398-405, 765-807) */
    PLFX_TRESCA = 4,  /* Tresca equivalent stress (material.py:630-632): calc_seq only, the reference has
                         no flow rule for it (calc_fgrad raises, material.py:824) */
    PLFX_BARLAT = 5,  /* Barlat Yld2004-18p equivalent stress (material.py:678-702): calc_seq only (:822) unless
                         plfx_material.barlat_normal is set (native normal, extension) */
    PLFX_SVC3 = 6,    /* sdim=3 ML material: RBF-SVC on 2 features (seq_J2/scale - 1, polar angle/pi) of the
                         principal stresses, gradient through the Jacobian (material.py:779-807, 2331-2333) */
    PLFX_SVC_WH = 7,  /* RBF-SVC with work-hardening features (material.py:2342-2346): 15 features = 6 stress features, the
                         plastic strain / scale_wh (6), accumulated strain, max. stress / scale_seq, flag (the last three are
                         zero on the path); the hardening modulus is read off the gradient (material.py:808-814) */
    PLFX_SVC6_COLS = 8 /* RBF-SVC on 6 features with ONE SCALE PER STRESS COLUMN, x_j = s_j / scale_j (plfx_set_svc_cols), and
                         the gradient of a dev_only set projected onto the deviator: a texture SVC bound to one texture
                         (DESIGN section 34).  Fields of a PLFX_SVC6 record.  Runs on the 16-lane row kernels only: sweeps,
                         calc_scf, plfx_response_batch, plfx_full_yf_batch; every other point function is
                         PLFX_ERR_UNSUPPORTED for it */
};

/* error codes */
enum {
    PLFX_OK = 0,
    PLFX_ERR_HIP = -1,      /* HIP runtime failure (no device, OOM, launch error) */
    PLFX_ERR_ARG = -2,      /* invalid argument */
    PLFX_ERR_STATE = -3,    /* call order violated (e.g. solve before set_mesh) */
    PLFX_ERR_UNSUPPORTED = -4
};

/* One material as seen by an element: mirrors Material.elasticity/plasticity (material.py:2401-2594)
 * plus the trained SVC parameters (svm_yf.support_vectors_, dual_coef_, intercept_, gam_yf, scale_seq). */
typedef struct plfx_material {
    int32_t kind;      /* PLFX_* */
    int32_t sdim;      /* 6, or 3 for PLFX_PRINC3 */
    double CV[36];     /* ELEMENT elastic matrix, i.e. after the plane-stress/strain choice of
                          Element.__init__ (model.py:272-303); must be symmetric */
    double E, nu;      /* used by the plane-stress B-matrix row (model.py:498-501) */
    double sy, khard;  /* material.py:2512-2513 */
    double hill[6];    /* material.py:2573 */
    double drucker;    /* material.py:2514 (d0 = ones*drucker) */
    int32_t nsv;       /* SVC: number of support vectors */
    int32_t nfeat;     /* SVC: features per support vector (6, or 2 for PLFX_SVC3) */
    int32_t dev_only;  /* SVC: deviatoric features (material.py:2336) */
    int32_t _pad;
    double gamma, intercept, scale_seq;
    const double *sv;   /* [nsv*nfeat] row-major */
    const double *dual; /* [nsv] */
    double barlat[18];  /* Yld2004-18p coefficients c'_12.. (material.py:2578-2591) */
    double barlat_exp;  /* exponent a */
    int32_t barlat_normal; /* PLFX_BARLAT only.  0: like the reference, the material has an equivalent stress but no flow rule
                            * (calc_fgrad raises, material.py:822-825) -- plfx_fgrad_batch / plfx_response_batch / plfx_sweep
                            * refuse it.  1 (EXTENSION, north star "Barlat ... with their normals"): the analytic normal
                            * d seq / d sigma of Yld2004-18p through the eigen-decompositions of the two transformed deviators,
                            * associated flow rule like the Hill materials.  NO REFERENCE VALUE EXISTS for this branch: the
                            * reference raises for Barlat normals (material.py:822-825), so its parity is "unpinned" in the sense
                            * of DESIGN.md 4 -- it is held by central finite differences of the pinned calc_seqB, Euler's theorem
                            * (a . sigma = seq) and the identity "unit coefficients, a = 2" == J2 (tests/test_barlat_normal.py). */
    int32_t _pad2;
    double scale_wh;    /* PLFX_SVC_WH: scaling of the plastic-strain features (Material.scale_wh, material.py:1165-1172) */
} plfx_material;

/* ---------------------------------------------------------------- context */
int plfx_create(int device, plfx_ctx **out);
void plfx_destroy(plfx_ctx *ctx);
const char *plfx_last_error(plfx_ctx *ctx);
const char *plfx_version(void);
/* number of GPUs visible to the process (0 when there is none or the HIP runtime cannot start); needs no context */
int plfx_device_count(void);
/* name[<=len], number of CUs, bytes of HBM */
int plfx_device_info(plfx_ctx *ctx, char *name, int len, int *cus, int64_t *hbm_bytes);
/* HIP stream the library launches on (for hipEvent timing by the caller) */
void *plfx_stream(plfx_ctx *ctx);
int plfx_sync(plfx_ctx *ctx);

/* ---------------------------------------------------------------- materials */
/* replaces the parameter set-up consumed by Material.response (material.py:2401-2594) */
int plfx_set_materials(plfx_ctx *ctx, int nmat, const plfx_material *mats);

/* ---------------------------------------------------------------- batched point evaluations
 * Material.calc_seq (material.py:576), calc_fgrad (:704), calc_yf (:348), ML_full_yf (:414),
 * response (:207) on N points; also the kernel-level parity entry points. */
int plfx_seq_batch(plfx_ctx *ctx, int mat, int n, const double *sig, double *seq);
int plfx_fgrad_batch(plfx_ctx *ctx, int mat, int n, const double *sig, double *fgrad);
/* calc_fgrad(sig, seq=seq) of an analytic Hill material (PLFX_HILL6 / PLFX_PRINC3), material.py:834-847: the deviator of the
 * Voigt components over 2 seq[i] with the equivalent stress handed in -- the reference's `seq` argument, and the form its
 * point function takes for a (6,) stress of a principal-stress (sdim = 3) material: seq in sig_princ's order, deviator of
 * the Voigt normals, no shear rows (plfx_fgrad_batch returns the principal-space normal epl_dot / C_tan use, :1044-1047). */
int plfx_fgrad_seq_batch(plfx_ctx *ctx, int mat, int n, const double *sig, const double *seq, double *fgrad);
int plfx_yf_batch(plfx_ctx *ctx, int mat, int n, const double *sig, const double *epl, double *yf);
/* ld: NULL or one loading direction [6] shared by all points (model.py:1052); status[n]: 0 ok,
 * 1 bracket failure, 2 root not accepted (both fall back to seq-0.85*sflow as the reference) */
int plfx_full_yf_batch(plfx_ctx *ctx, int mat, int n, const double *sig, const double *epl,
                       const double *ld, double *yf, int32_t *status);
int plfx_response_batch(plfx_ctx *ctx, int n, const int32_t *mat_id, const double *sig,
                        const double *epl, const double *deps, double *fy, double *sig_out,
                        double *depl, double *ct /* [n*36] */, int32_t *nsteps);
/* The `maxit` argument of Material.response (material.py:207, 288-291: an increment whose trial step ends outside the yield
 * locus is sub-divided into maxit sub-steps; nsteps = maxit - 1 then) for the point entries plfx_response_batch(_kh) of this
 * context; default 50, the reference's default and what the load-step loop always uses (model.py:1346 passes none). */
int plfx_set_response_maxit(plfx_ctx *ctx, int maxit);
/* basic.sig_princ (basic.py:107-179) on n Voigt stresses, computed on the HOST by the routine the PRINC3 / SVC3 kernels run on
 * states with out-of-plane shear: np.linalg.eig's eigenpair ORDER (LAPACK dgeev replayed for symmetric 3 x 3 matrices,
 * csrc/plfx_lapack3.hpp) and the reference's row-argmax re-ordering.  No context, no GPU.  sp[n*3].  plfx_eig3_host returns the
 * eigenvalues w[n*3] in dgeev's order and (V != NULL) the unit eigenvectors V[n*9], V[i*3+k] = component i of eigenvector k.
 * Return 1 if a matrix did not converge / gave a complex pair (numpy would, too). */
int plfx_sig_princ_host(int n, const double *sig, double *sp);
int plfx_eig3_host(int n, const double *sig, double *w, double *V);
/* Work-hardening-aware SVC materials (PLFX_SVC_WH).  The reference keeps the hardening modulus in ONE mutable attribute of
 * the Material object: every calc_fgrad call overwrites it (khard = max(0, -sum dK/dx[wh] scale_seq/scale_wh),
 * material.py:808-814), every get_sflow / epl_dot / C_tan reads it, and it is carried from call to call.  Here it is an
 * explicit input and output per point: khard_in[n] (NULL: the material's khard) is what Material.khard holds when
 * response() is entered, khard_out[n] what it holds on return.
 * Inside the load-step loop (plfx_sweep / plfx_load_step) the reference hands ONE value from element to element in index order
 * (model.py:1340-1359): reproduced exactly by default, see plfx_set_wh_mode below (round 4; rounds 2-3 carried one modulus
 * per material point, which remains available and is the only form on several GPUs). */
int plfx_response_batch_kh(plfx_ctx *ctx, int n, const int32_t *mat_id, const double *sig, const double *epl,
                           const double *deps, const double *khard_in, double *fy, double *sig_out, double *depl,
                           double *ct, int32_t *nsteps, double *khard_out);
/* calc_fgrad(sig, epl) of a PLFX_SVC_WH material on n points: gradient w.r.t. the stress and, per point, the raw value
 * -sum_k dK/dx[6+k] * scale_seq / scale_wh whose mean over the points, clipped at 0, the reference stores in khard */
int plfx_fgrad_batch_wh(plfx_ctx *ctx, int mat, int n, const double *sig, const double *epl, double *fgrad, double *khard_raw);
/* Material.calc_hessian (material.py:860-972) of an SVC material on n points: the 6x6 block of the feature-space
 * Hessian of the decision function w.r.t. the stress features, hess[n*36] row-major, symmetric.  epl: NULL or [n*6]
 * (PLFX_SVC_WH only; NULL = zeros).  The scaling to stress units is the caller's (the reference divides by
 * scale_seq ONCE, :962).  PLFX_ERR_UNSUPPORTED for every other kind (the reference raises for Hill / Tresca /
 * Barlat :965-970, NotImplementedError for sdim = 3 :950). */
int plfx_hessian_batch(plfx_ctx *ctx, int mat, int n, const double *sig, const double *epl, double *hess);
/* Material.yield_scale: the factor x[n] with calc_yf(x su, epl) = 0 along n unit stresses su[n*6] -- the root search behind
 * the reference's polar_plot_yl (material.py:3290-3293), kept on the device ray by ray.  epl: NULL or [n*6]; x0: NULL or [n]
 * start values, default sflow(epl) / seq_J2(su).
 * SVC kinds: the root that the marching bracket of ML_full_yf (material.py:468-486) isolates, made symmetric: from x0 down by
 * factors 0.98 while f >= 0 (to 0.01 x0), else up by factors 1.02 while f < 0 (to 5 x0); the bracket f(lo) < 0 <= f(hi) is
 * bisected until lo and hi are neighbouring doubles.  Analytic kinds (homogeneous of degree one): sflow(epl) / seq(su); the
 * value of x0 is not used there, but a given x0 that is <= 0 or not finite makes the ray degenerate as for the SVC kinds.
 * Rays of the principal-stress kinds (PLFX_PRINC3, PLFX_SVC3) with out-of-plane shear are reduced to their principal stresses
 * on the host (plfx_sig_princ_host).  PLFX_ERR_ARG for an elastic material.
 * status[n]: 0 root found; 1 no bracket in [0.01 x0, 5 x0]; 2 refinement cap reached; 3 degenerate ray (su = 0, seq(su) = 0
 * where x follows from it -- analytic kinds, or no x0 given --, a non-finite input, x0 <= 0).  x is NaN unless status is 0. */
int plfx_yield_scale(plfx_ctx *ctx, int mat, int n, const double *su, const double *epl, const double *x0, double *x,
                     int32_t *status);
/* Material.flow_curve: n flow curves along the unit stresses su[n*6] (of unit J2 stress), the loop of
 * plot_sig_eps in the reference's examples/train_hardening.py:83-133 with whole chains on the device, ONE launch per call
 * whatever n and max_steps.  Per curve, with epl = epl0 (NULL: zeros): x_0 is the point of the yield locus along su at epl;
 * then, while eps_eq(epl) + depl <= epl_max and k < max_steps: peeq = eps_eq(epl) + depl,
 * a = calc_fgrad(su (x_k + peeq predictor), epl), epl += a depl / eps_eq(a), x_{k+1} the point of the locus at the new epl.
 * The point of the locus: PLFX_SVC6 / PLFX_SVC_WH the root of plfx_yield_scale started at the previous root (x_0: at sy), with
 * its bits; PLFX_HILL6 sflow(epl) / seq(su).  epl_max = inf runs exactly max_steps steps.
 * Outputs, curve-major, NaN past a curve's last recorded point: x[n*(max_steps+1)], epl[n*(max_steps+1)*6],
 * yf[n*(max_steps+1)] the yield function at the recorded point (the decision function at the root; seq - sflow for
 * PLFX_HILL6), hk (NULL or [n*max_steps]) the raw hardening value of every gradient evaluation as plfx_fgrad_batch_wh
 * returns it (NaN for kinds without work-hardening features; the material's khard is neither read for it nor changed),
 * nsteps[n] completed steps, status[n]: 0 complete; 1 / 2 the status of the root search at the step where the curve ended;
 * 3 degenerate direction (su = 0, seq(su) <= 0 for PLFX_HILL6, a non-finite input); 4 eps_eq(a) zero or not finite.
 * n = 0 is PLFX_OK with nothing launched.  PLFX_ERR_ARG for depl <= 0 or not finite, max_steps < 0, a predictor that is not
 * finite, an epl_max that is NaN, an elastic material and every kind not named above. */
int plfx_flow_curve(plfx_ctx *ctx, int mat, int n, const double *su, const double *epl0, int max_steps, double depl,
                    double epl_max, double predictor, double *x, double *epl, double *yf, double *hk, int32_t *nsteps,
                    int32_t *status);
/* launches of the flow-curve kernels by this context */
int plfx_flow_info(plfx_ctx *ctx, int64_t *launches);

/* Material.load_path: n points of material `mat` driven along load paths of K increments, each step
 * starting from the state the last one left, every path in ONE launch with one copy in and one copy out.
 * dload[K][n][6], or [K][6] with shared != 0 (one path for all points).  control: NULL (every component strain-controlled) or
 * int32[n], bit c set = component c of dload is a stress increment, clear = a strain increment; constant along a path.
 * sig0, epl0: [n][6] or NULL (zeros).  tex_id: [n] rows of a texture field or NULL (row 0), as plfx_response_batch_tid.
 * With S the strain- and F the stress-controlled components, the stress target is t_k[F] = t_{k-1}[F] + dload[k][F],
 * t_{-1} = sig0[F] (one rounded add per step).  One step, from (sig, epl) and the tangent Ct of the last accepted step (the
 * material's CV before the first): deps[S] = dload[k][S]; deps[F] solves Ct_FF deps_F = (t_k - sig)_F - Ct_FS deps_S; the
 * trial is Material.response(sig, epl, deps, CV, maxit), accepted when F is empty or max |sig'[F] - t_k[F]| <= stol; else
 * deps[F] -= Ct'_FF^-1 (sig'[F] - t_k[F]) and the trial is repeated from the same state, at most `newton` corrections.  On
 * acceptance sig = sig', epl = epl + depl (one rounded add), Ct = Ct'.  An elastic material's trial is sig + CV deps.
 * The masked tangent is factored as L D L^T without pivoting.  No trial is evaluated on a deps that is not finite or has
 * max |deps| > eps_cap: the path ends instead.
 * Out, step-major: sig, epl, deps [K][n][6] (state after step k, increment taken; on S the bits of dload), fy[K][n],
 * nsteps[K][n] (Material.response's value and sub-step count of the accepted trial), newton_out[K][n] corrections taken,
 * ksteps[n] steps completed, status[n]: 0 complete, 1 stol not reached within `newton` corrections, 2 a pivot of the masked
 * tangent zero or not finite, 3 deps not finite or beyond eps_cap.  Steps from ksteps[i] on hold NaN (-1 in the int arrays);
 * the completed steps are exactly those of the same path cut to ksteps[i] steps.  ct: NULL or [n][36], the tangent after the
 * last completed step.  With F empty the results have the bits of K plfx_response_batch calls with epl += depl in between.
 * Kinds: PLFX_ELASTIC, PLFX_HILL6, PLFX_PRINC3, PLFX_BARLAT with barlat_normal, and PLFX_SVC6 / PLFX_SVC6_COLS on the row
 * kernels (texture fields included); every other kind is PLFX_ERR_UNSUPPORTED.  PLFX_ERR_ARG, with nothing launched: mat out
 * of range, n or K < 0, maxit < 1, newton < 0, stol or eps_cap not finite or <= 0, a dload, sig0 or epl0 that is not finite,
 * a strain-controlled |dload| > eps_cap, a control outside 0..63, a tex_id outside the attached rows, K n 19 > INT32_MAX.
 * n = 0 or K = 0 is PLFX_OK with nothing launched (K = 0: ksteps = status = 0 and ct = CV). */
int plfx_load_path(plfx_ctx *ctx, int mat, int n, int K, const double *dload, int shared, const int32_t *control,
                   const double *sig0, const double *epl0, const int32_t *tex_id, int maxit, int newton, double stol,
                   double eps_cap, double *sig, double *epl, double *deps, double *fy, int32_t *nsteps, int32_t *newton_out,
                   int32_t *ksteps, int32_t *status, double *ct);
/* launches of the load-path kernels by this context */
int plfx_load_path_info(plfx_ctx *ctx, int64_t *launches);

/* Load paths of a material with work-hardening features (PLFX_SVC_WH): plfx_load_path with the hardening
 * modulus as state of each path.  khard0[n]: the modulus at the start of every path, finite and >= 0 -- the material record's
 * khard is neither read nor written.  Every trial of a step enters with the step's modulus (as a plfx_response_batch_kh call
 * with khard_in); on acceptance the modulus is the accepted trial's khard_out, unchanged where that trial evaluated no
 * gradient.  khard[K][n]: the modulus after each completed step, NaN from ksteps[i] on.  Every other argument and output is
 * plfx_load_path's (there is no tex_id: no texture field lies on this kind).
 * form: 1 one thread per path (k_path_batch<7>): with strain control alone sig, epl, fy, nsteps, khard and ct have the bits of K
 * plfx_response_batch_kh calls with epl += depl and the modulus carried in between; 2 one wave per path (k_path_wh_wave): the
 * support-vector sums are split over 64 lanes, so results differ from form 1 by the order of those sums; 0 the faster
 * form by n: form 2 at every n, by the measurement of DESIGN section 45.  One launch per call.
 * PLFX_ERR_UNSUPPORTED, with nothing launched: a material of another kind, or one with an SVR flow rule attached.
 * PLFX_ERR_ARG, with nothing launched: every case of plfx_load_path, a form other than 0, 1, 2, khard0 NULL, not finite or
 * negative, K n 20 > INT32_MAX.  n = 0 or K = 0 is PLFX_OK with nothing launched, as in plfx_load_path. */
int plfx_load_path_wh(plfx_ctx *ctx, int mat, int n, int K, const double *dload, int shared, const int32_t *control,
                      const double *sig0, const double *epl0, const double *khard0, int form, int maxit, int newton, double stol,
                      double eps_cap, double *sig, double *epl, double *deps, double *fy, double *khard, int32_t *nsteps,
                      int32_t *newton_out, int32_t *ksteps, int32_t *status, double *ct);
/* launches of k_path_batch<7> and of k_path_wh_wave by this context (plfx_load_path_info does not count them) */
int plfx_load_path_wh_info(plfx_ctx *ctx, int64_t *launches_thread, int64_t *launches_wave);

/* A committee of SVC yield functions on n shared unit stresses su[n*6] (query by committee): member k is
 * material mats[k] of the context, 1 <= nmem <= 16, duplicates allowed, each a 6-feature SVC on Voigt stresses (PLFX_SVC6,
 * dev_only or not), with its own stress scale scale[k] (finite, > 0).  One launch of k_committee_yf, whatever nmem is:
 *   yf[nmem*n]  member-major: y[k, i] = calc_yf(su_i * scale[k]) of member k -- create_scaled_input and decision_function
 *               of the reference (material.py:398-405, 2336-2339), roundings in its order: su * scale, (deviator), / scale_seq
 *   mean[n]     (sum_k y[k, i]) / nmem, summed in member order
 *   var[n]      (sum_k (y[k, i] - mean_i)^2) / nmem, summed in member order (np.var, ddof = 0, as a fixed two-pass formula)
 *   best        index of the largest variance, best_var its value: NaN variances are skipped, equal variances resolve to the
 *               smaller index; -1 and NaN when no point has a variance that is not NaN
 * yf, mean, var, best and best_var may each be NULL.  A non-finite component of su_i makes y[:, i], mean_i and var_i NaN and
 * nothing else.  A member's row of yf does not depend on n, the place of the point, or the other members.
 * PLFX_ERR_UNSUPPORTED for a member of any other kind (the message names it); PLFX_ERR_ARG for nmem out of range, a material
 * index out of range, a scale that is not finite or <= 0; n = 0 is PLFX_OK with nothing launched. */
int plfx_committee_yf(plfx_ctx *ctx, int nmem, const int32_t *mats, const double *scale, int n, const double *su, double *yf,
                      double *mean, double *var, int32_t *best, double *best_var);
/* launches: k_committee_yf launches of this context so far (one per plfx_committee_yf call with n > 0); staged_members: bit k
 * set when member k of the last such call had its tables staged in LDS (clear: read from device memory) */
int plfx_committee_info(plfx_ctx *ctx, int64_t *launches, int32_t *staged_members);

/* The texture-dependent SVC yield function (train_SVC on a txdat material, material.py:1186-1196,
 * 2347-2361): an RBF C-SVC on 6 + tdim features [Voigt stress | texture descriptor], every column standardised,
 * f_j = (x_j - mean[j]) / scale[j], the stress taken as its deviator first when dev_only.  A table set of its own, owned by the
 * context: plfx_set_materials leaves it alone, a second call replaces it, nsv = 0 releases it, plfx_destroy frees it.
 * sv[nsv*(6+tdim)] row-major, dual[nsv].  PLFX_ERR_ARG for tdim outside 1..10, a scale that is <= 0 or not finite,
 * gamma <= 0, a non-finite table entry. */
int plfx_tex_svc_set(plfx_ctx *ctx, int nsv, int tdim, const double *sv, const double *dual, double intercept, double gamma,
                     const double *mean, const double *scale, int dev_only);
/* yf[n] = calc_yf(sig_i, tex=) at n stresses sig[n*6] in one launch; tex[ntex*tdim] row-major.  The texture of point i is row
 * tex_id[i] (each in 0..ntex-1); with tex_id NULL it is row 0 (ntex == 1, shared) or row i (ntex == n), anything else is
 * PLFX_ERR_ARG.  A point's value does not depend on n, its place, or how its texture was addressed; a non-finite stress or
 * texture component makes that point NaN and nothing else.  n = 0 is PLFX_OK with nothing launched; PLFX_ERR_STATE before
 * plfx_tex_svc_set. */
int plfx_tex_svc_yf(plfx_ctx *ctx, int n, const double *sig, int ntex, const double *tex, const int32_t *tex_id, double *yf);
/* Yield loci over textures: x[t*nray + r] with calc_yf(x su_r, tex_t) = 0 for nray unit stresses su[nray*6] and ntex textures
 * tex[ntex*tdim], all ntex * nray rays in ONE launch, output texture-major.  x0: NULL or [ntex*nray] start values; NULL starts
 * ray (t, r) at 1 / seq_J2(su_r), a J2 stress of one stress unit, so callers that know the yield strength pass x0.  The search
 * and the status values are exactly those of plfx_yield_scale: march by 0.98 / 1.02 from x0 (caps 240 / 90), bisection to
 * neighbouring doubles (cap 80); status 0 root found, 1 no bracket in [0.01 x0, 5 x0], 2 refinement cap reached, 3 degenerate
 * ray (su = 0, a non-finite input, x0 <= 0 or not finite); x is NaN unless status is 0.  nray = 0 or ntex = 0 is PLFX_OK with
 * nothing launched; PLFX_ERR_STATE before plfx_tex_svc_set. */
int plfx_tex_svc_yield_scale(plfx_ctx *ctx, int nray, const double *su, int ntex, const double *tex, const double *x0, double *x,
                             int32_t *status);
/* the set (nsv = 0: none), launches of k_tex_yf / k_tex_yield_scale since it was set, and whether its tables are staged in LDS
 * (0: read from device memory) */
int plfx_tex_svc_info(plfx_ctx *ctx, int *nsv, int *tdim, int64_t *yf_launches, int64_t *ray_launches, int *staged);
/* Flow rule and stress update of the texture SVC (the reference has none that run).  sig, tex, tex_id, ntex
 * and their conventions are those of plfx_tex_svc_yf: n = 0 is PLFX_OK with nothing launched, PLFX_ERR_STATE before
 * plfx_tex_svc_set, PLFX_ERR_ARG for ntex not in {1, n} without tex_id and for a tex_id outside 0..ntex-1.
 * grad[n*6] = d calc_yf(sig_i, tex=) / d sig: with f the standardised features, v_k the vectors and K_k the kernel values,
 * g_j = -2 gamma sum_k dual_k K_k (f_j - v_kj) and a_j = g_j / scale[j] for j < 6; for a dev_only set (a_0 + a_1 + a_2) / 3
 * is then taken off a_0..a_2 (the chain rule through the deviator).  With equal scales and zero means on the six stress columns
 * this is the gradient of a PLFX_SVC6 material (plfx_fgrad_batch) up to rounding -- for a dev_only set as far as the vectors
 * are deviators, since that gradient is not projected.  A point's six values do not depend on n, its place, or how its
 * texture was addressed; a non-finite stress or texture component makes them NaN and nothing else. */
int plfx_tex_svc_fgrad(plfx_ctx *ctx, int n, const double *sig, int ntex, const double *tex, const int32_t *tex_id, double *grad);
/* ML_full_yf(sig_i, tex=) (material.py:414-516 as plfx_full_yf_batch runs it for a PLFX_SVC6 material, without loading
 * direction and with epl = 0): the decision function is the texture one at the point's texture; seq and the flow stress sy
 * come from material 0 of the context, which must be a PLFX_HILL6 record (PLFX_ERR_STATE without materials,
 * PLFX_ERR_UNSUPPORTED for another kind).  f[n], status[n]: 0 root found, 1 no bracket, 2 search not converged (1 and 2: the
 * conservative estimate seq - 0.85 sy).  A non-finite stress or texture component: NaN and status 1. */
int plfx_tex_svc_full_yf(plfx_ctx *ctx, int n, const double *sig, int ntex, const double *tex, const int32_t *tex_id, double *f,
                         int32_t *status);
/* Material.response (material.py:207-346) on n points with the texture SVC as yield function: the update of
 * plfx_response_batch with calc_yf, ML_full_yf and calc_fgrad replaced by the texture forms above at the point's texture.
 * `mat`: a PLFX_HILL6 record among the context's materials, which gives the elastic matrix, sy, khard (flow stress
 * sy + khard peeq, hardening modulus khard) and the Hill form of seq; any other kind is PLFX_ERR_UNSUPPORTED.  maxit: the
 * sub-steps of a sub-divided increment (PLFX_ERR_ARG below 1).  Outputs as plfx_response_batch: fy[n], sig_out[n*6],
 * depl[n*6], ct[n*36], nsteps[n].  A point with a non-finite sig, epl, deps or texture component: all outputs NaN and
 * nsteps = -1, nothing else changes. */
int plfx_tex_svc_response(plfx_ctx *ctx, int mat, int n, const double *sig, const double *epl, const double *deps, int ntex,
                          const double *tex, const int32_t *tex_id, int maxit, double *fy, double *sig_out, double *depl,
                          double *ct, int32_t *nsteps);
/* launches of k_tex_fgrad / k_tex_full_yf / k_tex_response since the set was installed (each pointer may be NULL) */
int plfx_tex_svc_flow_info(plfx_ctx *ctx, int64_t *fgrad_launches, int64_t *full_yf_launches, int64_t *response_launches);

/* Index products of Model.mesh for the reference's structured NX x NY grid, computed on the host (no context, no GPU):
 * conn[NX*NY*4] = [n1, n1+1, n1+NnodeY, n1+NnodeY+1] with n1 = (ih / NY) * NnodeY + ih % NY for element ih = j*NY + k
 * (model.py:935-948); node sets noleft (j = 0), noright (j = NX), nobot (k = 0), notop (k = NY) in ascending node order
 * (model.py:897-911), each [NY+1] or [NX+1] long.  Any output pointer may be NULL.  Integer work: bit-exact. */
int plfx_gen_structured(int NX, int NY, int32_t *conn, int32_t *noleft, int32_t *noright, int32_t *nobot, int32_t *notop);

/* ---------------------------------------------------------------- mesh (Model.mesh products, model.py:758-952)
 * conn[nel*4]: Q4 connectivity in the reference's node order; mat_id[nel]; lxy[nel*2] element
 * sizes (Lelx, Lely).  Elements are rectangles aligned with the axes (model.py:262).
 * The element range [el_begin, el_end) is the part owned by this rank (x-strip shard);
 * pass 0, nel for a single GPU. */
int plfx_set_mesh(plfx_ctx *ctx, int nel, int nnode, const int32_t *conn, const int32_t *mat_id,
                  const double *lxy, double thick, int planestress, int el_begin, int el_end);
/* The same for the structured grids Model.mesh produces (model.py:758-952): node j * (NY + 1) + k, element j * NY + k,
 * connectivity [n1, n1 + 1, n1 + NY + 1, n1 + NY + 2] (:893, :935-948) written by the library; dx_col[NX] = element width of every
 * column (laminate sections, :847), dy the element height; material numbers per column (mat_col[NX]) or per element
 * (mat_el[NX * NY], the `elmts` form of Model.mesh); exactly one of the two non-NULL. */
int plfx_set_mesh_structured(plfx_ctx *ctx, int NX, int NY, const int32_t *mat_col, const int32_t *mat_el, const double *dx_col,
                             double dy, double thick, int planestress, int el_begin, int el_end);
/* Host-only self-test (no GPU needed): the closed-form block-ELL pattern that plfx_set_mesh / plfx_set_grid write for the
 * reference's structured numbering equals the one derived generically from the connectivity (slots, gather codes, order).
 * 0 = identical. */
int plfx_pattern_selftest(int nx, int ny);
/* Declare that the mesh is the reference's structured NX x NY grid (node j*(NY+1)+k, element j*NY+k,
 * model.py:893, 935); verified against conn.  Enables the geometric-multigrid preconditioner of
 * plfx_solve when all elements have one shape and NX, NY halve down to a small grid. */
int plfx_set_grid(plfx_ctx *ctx, int nx, int ny);
/* preconditioner of plfx_solve: kind 0 = Jacobi, 1 = multigrid V(nu,nu) with damped-Jacobi smoothing
 * (falls back to Jacobi when no hierarchy exists); omega <= 0 / nu <= 0 keep the defaults (0.65, 2) */
int plfx_set_precond(plfx_ctx *ctx, int kind, double omega, int nu);
int plfx_precond_info(plfx_ctx *ctx, int *kind_in_use, int *levels);
/* z = B r: one application of the preconditioner of plfx_solve (the multigrid V-cycle) to a host vector [ndof], for tests of
 * its symmetry / of what it does to a given field (single GPU, after plfx_assemble + plfx_apply_bc). */
int plfx_precond_apply(plfx_ctx *ctx, const double *r, double *z);
/* measurement hook (bench.py: `vcycle`): `reps` applications of the multigrid preconditioner back to back on the current
 * residual vector, one pair of HIP events around them -> microseconds per V-cycle; us_coarse (may be NULL): the part of a cycle
 * below the fine level (transfers to / from level 1, the launch-latency-bound levels, the single-workgroup tail).  Only scratch
 * vectors are written.  Single-GPU hierarchies (no strip). */
int plfx_precond_bench(plfx_ctx *ctx, int reps, double *us_per_cycle, double *us_coarse);
/* number of plfx_solve calls so far that PCG could not finish: a direction of negative curvature was met (the tangents of
 * Material.response are not always positive semi-definite, material.py:324-338) and right-preconditioned GMRES completed
 * the solve from the last iterate -- the reference's LU does not need definiteness either -- or multigrid-PCG did not
 * converge within 300 iterations and Jacobi-PCG took over */
int plfx_solve_fallbacks(plfx_ctx *ctx, int64_t *count);
/* The solves with an indefinite tangent stiffness among them (p.Kp <= 0 met by PCG): how many there were and how many GMRES
 * completed.  by_minres_surrogate, surrogates_built and elements_shifted are always 0: they counted the MINRES solver on an
 * SPD surrogate operator, which was removed; the signature is kept.  Any pointer may be NULL. */
int plfx_indefinite_info(plfx_ctx *ctx, int64_t *solves, int64_t *by_minres_surrogate, int64_t *by_gmres,
                         int64_t *surrogates_built, int64_t *elements_shifted);
/* Form of the stiffness operator in plfx_solve / plfx_update_state / plfx_apply_bc: kind 1 (default) applies
 * K matrix-free from the element stiffness generators (Element.calc_Kel never materialised, Model.setupK reduced to
 * the diagonal) wherever plfx_set_grid found a structured grid with one element shape; kind 0 always assembles the
 * block-ELL matrix (Model.setupK, model.py:954-977).  plfx_get_csr assembles on demand in both cases.
 * Environment override of the default: PLFX_MATFREE=0|1. */
int plfx_set_operator(plfx_ctx *ctx, int kind);
/* y = K x over all DOFs with the current operator (the product of model.py:1384, `K @ du`); host arrays [ndof] */
int plfx_matvec(plfx_ctx *ctx, const double *x, double *y);
int plfx_operator_info(plfx_ctx *ctx, int *matrix_free, int *levels_matrix_free);
/* Unchanged inputs are not recomputed (environment PLFX_REUSE=0 switches it off): plfx_assemble returns at once when no
 * sweep reported a changed tangent and nothing was written into the tangents since the last assembly (Model.setupK of an
 * unchanged model, model.py:1333); plfx_apply_bc_plan with the values of the previous call on the same operator keeps the
 * right-hand side; plfx_solve(warm=1) of the system the previous converged solve solved returns that solution with 0
 * iterations (the reference repeats the last solve of a load step as predictor and first stiffness iteration of the next,
 * model.py:1291/1335).  Counters of the three cases since plfx_create. */
int plfx_reuse_info(plfx_ctx *ctx, int *assemblies, int *bc_applications, int *solves);
/* Initial guess of a warm-started solve from the last two solutions (environment PLFX_PREDICT=0 at plfx_create switches it off):
 * with x the previous solution, d its difference to the one before and alpha in [0, 1] of smallest residual
 * | P (b - K (x + alpha d)) |, plfx_solve(warm=1) returns x + alpha d when -- and only when -- it satisfies the tolerance as it is
 * (0 iterations); otherwise the solve iterates from x exactly as with PLFX_PREDICT=0 (bit-identical).  Tried on multigrid-PCG
 * solves of meshes of >= 16384 nodes (strips: of the whole grid; the sums are all-reduced).  d is taken to the last solution that
 * differed from x (repeated solves of one system keep the history).  x itself is never rescaled.
 * applied (accepted as the solution) / skipped (alpha < 0.01) / rejected (failed the tolerance test) since plfx_create. */
int plfx_predict_info(plfx_ctx *ctx, int64_t *applied, int64_t *skipped, int64_t *rejected);
/* Sweeps since plfx_create and the number of element tangents they rewrote (model.py:1346-1355: a tangent is stored, and
 * Kel refreshed, only where it changed by more than 1e-3) -- whole mesh in sharded runs.  A sweep moves 412 B per element
 * plus 216 B per rewritten tangent. */
int plfx_sweep_info(plfx_ctx *ctx, int64_t *sweeps, int64_t *tangents_rewritten);
/* Single GPU with the mailbox: a sweep that follows one whose list of sub-stepped elements was empty leaves the corrector
 * launches out (heavy_skipped counts such sweeps); if its own list is not empty after all, the launches and a second flags
 * kernel follow after one more round trip (heavy_recovered).  Results are the same either way. */
int plfx_sweep_launch_info(plfx_ctx *ctx, int64_t *heavy_skipped, int64_t *heavy_recovered);
/* Between the boundary values and the first operator pass (one GPU, no strip; PLFX_BC_ROWS=0 or
 * PLFX_REUSE=0 at plfx_create: all four stay 0).  apply_bc calls that rewrote rhs on the rows next to prescribed nodes only
 * (same Dirichlet set, no force vector) instead of passing over all DOFs (rhs_rows_only); those among them that kept the
 * Jacobi scaling because the diagonal had not been rewritten (dinv_kept) / had it to form again on its own (dinv_refreshed:
 * at once, or in front of its first reader of values, plfx_short_info);
 * solves whose du was composed behind the first convergence test, under the host's wait for it (du_early).  Results are
 * the same bit for bit either way. */
int plfx_bc_info(plfx_ctx *ctx, int64_t *rhs_rows_only, int64_t *dinv_kept, int64_t *dinv_refreshed, int64_t *du_early);
/* Passes an accepted interpolated start never needs (one GPU, no strip, no communicator; PLFX_SHORT_SOLVE
 * at plfx_create is a bit mask -- 1: the fine level's dinv waits for its first reader of values, like the coarse set-up; 2:
 * k_pred_finish leaves the d of the next interpolated start behind, k_pred_diff is left out -- default 3, other bits ignored,
 * 0 or PLFX_REUSE=0: the launches as they were, all counters stay 0).  apply_bc calls that left dinv unformed although the
 * diagonal had been rewritten (dinv_deferred; they count in plfx_bc_info's dinv_refreshed too); k_dinv launches that made up
 * for one in front of a reader of values (dinv_formed_late; the rest were superseded unread); solves that left k_pred_diff out
 * (d_kept).  spec_merged: always 0 (one launch behind a sweep's flags instead of two was built and not kept).
 * Results are the same bit for bit either way -- for every solve that follows an apply_bc of the present diagonal, which is
 * every solve of plfx_load_step; plfx_solve called after plfx_assemble or a tangent-changing sweep WITHOUT an apply_bc in
 * between is preconditioned with the dinv of the new diagonal where it used to get the old one's. */
int plfx_short_info(plfx_ctx *ctx, int64_t *dinv_deferred, int64_t *dinv_formed_late, int64_t *d_kept, int64_t *spec_merged);
/* Rewritten generators straight into the operator's snapshot (one GPU, plane Hill sweep, matrix-free grid
 * of one column width, no strip, no communicator; PLFX_DIRECT_SNAP at plfx_create is a bit mask -- 1: a sweep of plfx_load_step
 * that is certain to be followed by plfx_assemble if it changes a tangent stores each rewritten generator into the snapshot as
 * well, and the set-up pass behind its flags is left out; 2 (needs 1): into the snapshot alone, the live array follows in
 * front of its next reader -- default 3, 0 or PLFX_REUSE=0: the launches as they were, all counters stay 0).  Such sweeps
 * (direct_sweeps); plfx_assemble calls that found the snapshot taken and launched nothing (direct_acknowledged); set-up passes
 * launched after all in front of a reader of the fine diagonal or of the level-1 generators (setup_formed_late; the rest were
 * superseded unread); copies of the snapshot back into the live array (live_restored).  Results are the same bit for bit. */
int plfx_snap_info(plfx_ctx *ctx, int64_t *direct_sweeps, int64_t *direct_acknowledged, int64_t *setup_formed_late, int64_t *live_restored);
/* Node code (one GPU, matrix-free grid of one column width, no strip, no communicator; PLFX_NODE_CODE at
 * plfx_create is a bit mask -- 1: the kernels of an interpolated start read the Dirichlet set from a byte per node instead of
 * the doubles of dinv / is_presc; 2 (needs 1): the two start kernels load rhs on the rows next to prescribed nodes alone while
 * it is zero elsewhere (no force vector) -- default 1, 0 or PLFX_REUSE=0: the launches as they were, the last three counters
 * stay 0).  Codes formed (built: one per apply_bc with another Dirichlet set); k_cg_start_test / k_cg_start_pred launches that
 * read the code (start_launches) and those among them with the sparse rhs (b_sparse_launches); k_pred_dots, k_pred_try,
 * k_pred_finish and k_compose_du launches that read it (vector_launches).  Results are the same bit for bit either way. */
int plfx_code_info(plfx_ctx *ctx, int64_t *built, int64_t *start_launches, int64_t *b_sparse_launches, int64_t *vector_launches);
/* The node code of the last apply_bc, a byte per node -- bit 0 / 1: the x / y DOF is prescribed, bit 2: a row of K next to a
 * prescribed node (rhs can be non-zero there without a force vector).  out: nnode bytes.  PLFX_ERR_STATE before the first apply_bc. */
int plfx_code_get(plfx_ctx *ctx, uint8_t *out);
/* Stores that nothing reads (one GPU, no strip; PLFX_DEAD_STORES=0 or PLFX_REUSE=0 at plfx_create: all
 * four stay 0).  Sweeps of plfx_load_step that were certain to be repeated if they changed a tangent, and in which the
 * elements whose tangent changed therefore left res_sig, res_depl and fyn to the next sweep (armed_sweeps; the tangents they
 * rewrote: tangents_rewritten_in_armed_sweeps, 104 B not stored for each of those the streaming kernel rewrote); solves that
 * started with the sums of the first tolerance test alone, without r, z and r.z (test_only_starts), and those among them
 * whose test failed, so that the full start followed (test_only_retries: one operator pass each).  Results are the same bit
 * for bit either way.  plfx_sweep called from outside plfx_load_step always stores every element. */
int plfx_dead_store_info(plfx_ctx *ctx, int64_t *armed_sweeps, int64_t *tangents_rewritten_in_armed_sweeps,
                         int64_t *test_only_starts, int64_t *test_only_retries);
/* Plane columns (one GPU, no strip, no communicator; PLFX_PLANE_COLS=0 or PLFX_REUSE=0 at plfx_create:
 * off).  Every model here is a plane model: the yz / zx shears (Voigt columns 3 and 4) of sig, epl, res_sig, res_depl are zero,
 * and elastic and analytic Hill / J2 materials whose CV does not couple those shears to the rest keep them zero.  While that
 * holds (*mode_on = 1) the Hill sweep and the state update neither load nor store these columns (plane_sweeps, plane_updates:
 * launches of the plane kernels since plfx_create).  The mode is switched on by plfx_state_reset / plfx_set_mesh alone and goes
 * off, until the next reset, for the reason in *switched_off_by (PLFX_PLANE_*).  Results are the same bit for bit either way,
 * but for the sign of zeros in columns 3 and 4 of res_depl. */
enum {
    PLFX_PLANE_ON = 0,          /* not switched off */
    PLFX_PLANE_NEVER_ON = 1,    /* no state reset yet */
    PLFX_PLANE_SWITCH = 2,      /* PLFX_PLANE_COLS=0 or PLFX_REUSE=0 */
    PLFX_PLANE_SHARDED = 3,     /* the context owns a part of the mesh / strip / communicator */
    PLFX_PLANE_MATERIALS = 4,   /* a material is not elastic / Hill6, couples the shears, or has a non-finite parameter */
    PLFX_PLANE_STATE_SET = 5,   /* plfx_state_set delivered a non-zero in column 3 or 4 of sig, epl, res_sig or res_depl */
    PLFX_PLANE_TANGENT_SET = 6  /* plfx_state_set of the tangents */
};
int plfx_plane_info(plfx_ctx *ctx, int *mode_on, int64_t *plane_sweeps, int64_t *plane_updates, int *switched_off_by);
/* Which form of the multigrid V-cycle the next cycle of this context runs (read-only, tests assert the
 * path they were written for).  *levels = levels of the hierarchy (0: none).  The first min(*levels, max_levels) entries of
 * the per-level arrays (any of them may be null): dims[2l], dims[2l+1] = nx, ny elements; ratios[2l], ratios[2l+1] = rx, ry,
 * the size of the last element column / row relative to the others; matfree[l] = 1 where the level's operator is applied from
 * the stiffness generators (its smoothing diagonal comes from the generators too: area-scaled on a level with rx or ry != 1),
 * 0 where it is an assembled block-ELL matrix with the true diagonal.  *tail_level = first level of the single-workgroup tail
 * (-1: no tail kernel; the coarsest level is then solved by a launch of its own), *tail_kernel = PLFX_MG_TAIL_*,
 * *coarse_solver = PLFX_MG_COARSE_* with *cheby_steps and *cheby_kappa (0 unless Chebyshev), *march = 1 where the fine-level
 * kernels of the cycle run in marching form. */
enum {
    PLFX_MG_TAIL_NONE = 0,       /* every level is launched kernel by kernel */
    PLFX_MG_TAIL_GENERIC = 1,    /* k_mg_tail: vectors in global memory, any number of sweeps, any coarsest solver */
    PLFX_MG_TAIL_LDS = 2,        /* k_mg_tail_lds: assembled levels, vectors and neighbour tables in LDS */
    PLFX_MG_TAIL_MF = 3,         /* k_mg_tail_mf<false>: matrix-free, every tail level halves exactly */
    PLFX_MG_TAIL_MF_RAGGED = 4   /* k_mg_tail_mf<true>: matrix-free, a tail level has a last column / row of another size */
};
enum {
    PLFX_MG_COARSE_DENSE = 0,    /* dense inverse (unpivoted Gauss-Jordan, once per set of boundary conditions) */
    PLFX_MG_COARSE_CHEBY = 1,    /* fixed number of Jacobi-preconditioned Chebyshev steps */
    PLFX_MG_COARSE_PCG = 2       /* Jacobi-PCG inside one workgroup, vectors in LDS, to 1e-10 */
};
int plfx_mg_info(plfx_ctx *ctx, int max_levels, int *levels, int *dims, double *ratios, int *matfree, int *tail_level,
                 int *tail_kernel, int *coarse_solver, int *cheby_steps, double *cheby_kappa, int *march);
/* Which kernels run the 6-feature SVC materials (Material.response with an ML yield function, material.py:398-405 evaluates
 * any trained svm_yf): bit k of *row_materials = material k runs with 16 lanes per element / point (one launch per material
 * and sweep phase), its support-vector tables staged in LDS when they fit the 160 KB of a CU (up to ~2200 vectors) and read
 * from device memory otherwise -- no limit on the number of 6-feature SVC materials or of their support vectors;
 * bit k of *thread_materials = material k runs one thread per element / point (only when the row kernels are switched off
 * by PLFX_SVC_WAVE).  A PLFX_SVC6_COLS material is always among the row materials and never among the thread ones.  Launch counters of the sweep kernels of either form since plfx_create. */
int plfx_svc_info(plfx_ctx *ctx, int *row_materials, int *thread_materials, int64_t *row_launches, int64_t *thread_launches);
/* B matrices of element e at its 4 Gauss points, [4*6*8] (Element.calc_Bmat, model.py:439) */
int plfx_get_bmat(plfx_ctx *ctx, int e, double *B);
/* element stiffness of element e from its current tangent (Element.calc_Kel, model.py:365), [64] */
int plfx_get_kel(plfx_ctx *ctx, int e, double *Kel);

/* ---------------------------------------------------------------- state (el.sig/eps/epl/elstiff, Model.u/f/du)
 * which: 0 sig, 1 eps, 2 epl, 3 res_sig, 4 res_depl  -> [nel_owned*6];  5 elstiff -> [nel_owned*36];
 *        6 u, 7 f, 8 du -> [ndof];  9 fyn (fy/sflow of the last sweep) -> [nel_owned];
 *        10 max_steps (stat_nlin) -> [nel_owned] as double;  11 hardening modulus of every material point (PLFX_SVC_WH
 *        materials: carried from sweep to sweep; others: the material's khard) -> [nel_owned] */
int plfx_state_get(plfx_ctx *ctx, int which, double *out);
int plfx_state_set(plfx_ctx *ctx, int which, const double *in);
/* solve() first-call initialisation (model.py:1212-1234): zero u,f,sig,eps,epl; elstiff = CV */
int plfx_state_reset(plfx_ctx *ctx);
/* gather entries of u (which=6), f (7) or du (8) at idx[n] */
int plfx_gather(plfx_ctx *ctx, int which, int n, const int32_t *idx, double *out);

/* Element result fields: per owned element the value the closures of Model.plot compute (model.py:1591-1677).
 * STRAIN* = eps[0], eps[1], eps[5] times 100; STRESS* = sig[0], sig[1], sig[5]; PLASTIC* = epl[0], epl[1], epl[5] times 100;
 * SEQ = calc_seq of the element's own material (material.py:576-676); SEQJ2 = sig_eq_j2(sig); PEEQ / ETOT = eps_eq(epl) /
 * eps_eq(eps) times 100; UX / UY = mean of the four nodal displacements (summed in the order of the element's nodes).
 * The reference's sixteenth field, the material number, is the caller's own map and no selector of the library. */
enum {
    PLFX_FIELD_STRAIN1 = 0,
    PLFX_FIELD_STRAIN2 = 1,
    PLFX_FIELD_STRAIN12 = 2,
    PLFX_FIELD_STRESS1 = 3,
    PLFX_FIELD_STRESS2 = 4,
    PLFX_FIELD_STRESS12 = 5,
    PLFX_FIELD_PLASTIC1 = 6,
    PLFX_FIELD_PLASTIC2 = 7,
    PLFX_FIELD_PLASTIC12 = 8,
    PLFX_FIELD_SEQ = 9,
    PLFX_FIELD_SEQJ2 = 10,
    PLFX_FIELD_PEEQ = 11,
    PLFX_FIELD_ETOT = 12,
    PLFX_FIELD_UX = 13,
    PLFX_FIELD_UY = 14
};
/* nsel selectors sel[] (any order, repeats allowed) in one device pass; columns several selectors share are read once.
 * out: [nsel * nel_owned], selector-major (row k = selector sel[k]), or NULL; range: [2 * nsel], minimum and maximum of
 * every row, reduced on the device (both NaN when the row holds a NaN), or NULL.  The call reads the state and changes
 * neither it nor its flags: the stress is the current one also right after a load step, and the strain selectors are
 * formed from u whenever the stored eps is behind it, without writing the stored field.  The device rows live in a buffer
 * of the context that later calls reuse.  Unknown selector: PLFX_ERR_ARG; before set_mesh: PLFX_ERR_STATE; nsel = 0: PLFX_OK. */
int plfx_element_fields(plfx_ctx *ctx, int nsel, const int32_t *sel, double *out, double *range);

/* ---------------------------------------------------------------- assembly (Model.setupK, model.py:954-977) */
int plfx_assemble(plfx_ctx *ctx);
/* export the assembled matrix as CSR (scalar rows, sorted columns).  Call with NULL arrays to get nnz. */
int plfx_get_csr(plfx_ctx *ctx, int64_t *nnz, int32_t *rowptr, int32_t *colidx, double *val);

/* ---------------------------------------------------------------- boundary conditions + solve
 * calc_BC (model.py:1070-1206) reduced to data: presc_idx[n] DOFs with displacement BC (ascending or
 * not), du_presc[n] the value written to du (first application), w[n] the multiplicity-weighted
 * value that enters the right-hand side (the reference re-applies a DOF shared by two edges),
 * fext[ndof] consistent nodal forces (or NULL).  Builds rhs = P (fext - K w) and the free mask. */
int plfx_apply_bc(plfx_ctx *ctx, int n, const int32_t *presc_idx, const double *du_presc,
                  const double *w, const double *fext);
/* calc_BC's index structure registered once (it only depends on the BC flags, model.py:1070-1206): nseg segments of
 * prescribed DOFs in the reference's order (left, bottom, right, top, node set; x before y), seg_len[nseg] entries each,
 * idx = their DOF numbers concatenated.  plfx_apply_bc_plan then takes ONE value per segment and forms, exactly like
 * plfx_apply_bc fed by the host: the ascending unique DOF set, the value written to du (first occurrence) and the
 * multiplicity-weighted right-hand-side value (a DOF shared by two edges is applied twice, :1115-1122).
 * inconsistent_entry: first entry whose value differs from the first one on its DOF (the reference's warning), -1 if none. */
int plfx_set_bc_plan(plfx_ctx *ctx, int nseg, const int32_t *seg_len, const int32_t *idx);
int plfx_apply_bc_plan(plfx_ctx *ctx, const double *seg_val, const double *fext, int *inconsistent_entry);
/* Kred + np.linalg.solve (model.py:1028-1033, 1291, 1335) as an iterative solve on the free DOFs: PCG with the multigrid
 * V-cycle (uniform structured grids) or the Jacobi scaling as preconditioner, stopped at |P(b - K du)| <= rtol |P b|.
 * Systems PCG cannot finish are completed from its last iterate: tangent stiffness that is not positive definite (a
 * direction with p.Kp <= 0 was met) by right-preconditioned GMRES(400), stalled multigrid (300 iterations) by Jacobi-PCG;
 * plfx_solve_fallbacks counts them.  warm != 0 starts from the previous du on the free DOFs.  Result in du (state 8);
 * returns 1 when maxit iterations did not reach rtol (iters / relres report what was reached). */
int plfx_solve(plfx_ctx *ctx, double rtol, int maxit, int warm, int *iters, double *relres);

/* ---------------------------------------------------------------- non-linear driver pieces */
/* material sweep (model.py:1340-1359) over owned elements with the current du:
 * response + |elstiff - Ct|_F > 1e-3 test + tangent refresh (averaging when nit >= 15).
 * changed: any tangent updated; conv: all fy/sflow <= yf_tolerance*1.0001 */
int plfx_sweep(plfx_ctx *ctx, int nit, int *changed, int *conv);
/* Work-hardening SVC materials (PLFX_SVC_WH) inside the load-step loop.  The reference keeps the hardening modulus in ONE
 * mutable attribute of the Material object: every calc_fgrad overwrites it (material.py:808-814), get_sflow / epl_dot / C_tan
 * read it, and the element loop of Model.solve (model.py:1340-1359) hands it from element to element in index order.
 *   sequential = 1 (default; one GPU, no shard): exactly that.  plfx_sweep resolves the chain as a fixed point -- sweep with
 *       guessed entry moduli, derive the entry moduli that sweep implies (exit modulus of the last element before e, same
 *       material, whose call evaluated a gradient; else the value the material held when the sweep began), repeat while any
 *       entry changed; tangents / generators are restored before every repetition.  plfx_wh_info counts sweeps and passes.
 *       State 11 then returns the EXIT modulus of every element's last call; plfx_wh_carry reads / sets the value a material
 *       object holds now (what Material.khard is after / before Model.solve in the reference).
 *   sequential = 0: one modulus per material point, carried from sweep to sweep (state 11) -- the data-parallel contract of
 *       rounds 2-3, the only form on several GPUs (the chain would cross every shard); deviates from the reference by ~1e-4
 *       on its 4 x 4 trace (tests/test_workhard_svc.py). */
int plfx_set_wh_mode(plfx_ctx *ctx, int sequential);
int plfx_wh_info(plfx_ctx *ctx, int *sequential_in_use, int64_t *sweeps, int64_t *passes,
                 int64_t *unresolved /* sweeps whose chain had not settled after 64 passes (accepted as they were; never observed) */);
int plfx_wh_carry(plfx_ctx *ctx, int mat, const double *set, double *get);
/* calc_scf statistics (model.py:1036-1067): sum of entries, sum of squares about the mean, min, count.
 * sld[6] loading direction for SVC materials. */
int plfx_scf_stats(plfx_ctx *ctx, const double *sld, double *sum, double *sumsq_c, double *minv,
                   int64_t *count, double mean_in, int pass);
/* both passes of calc_scf's statistics in one call (single GPU: the mean of pass 0 stays on the device) */
int plfx_scf_all(plfx_ctx *ctx, const double *sld, int64_t *count, double *minv, double *sum, double *sumsq_c);
/* end-of-load-step update (model.py:1383-1392): u += du, f += K du, sig/epl/eps update */
int plfx_update_state(plfx_ctx *ctx);
/* End of a load step in one call and one host synchronisation: plfx_update_state, then u and f at the registered DOFs
 * (the boundary nodes calc_global averages, model.py:1452-1471) and the 18 element sums of plfx_global_sums. */
int plfx_set_finish_set(plfx_ctx *ctx, int n, const int32_t *idx);
int plfx_finish_step(plfx_ctx *ctx, double *u_at /* [n] */, double *f_at /* [n] */, double *sums18);
/* calc_global element sums (model.py:1500-1511): out[18] = sum(sig*Vel), sum(eps*Vel), sum(epl*Vel) */
int plfx_global_sums(plfx_ctx *ctx, double *out18);

/* ---------------------------------------------------------------- one load step of Model.solve (model.py:1262-1392)
 * The whole body of the reference's load-step loop as ONE call: elastic predictor with the stiffness of the previous
 * step (:1290-1291), load-step scaling calc_scf while il < 10 (:1296), the stiffness iterations
 * [halving of the increment while il < 6 (:1308-1330) -> setupK -> calc_BC -> solve -> material sweep] until no tangent
 * changed and the yield function converged or 16 iterations (:1306-1381), state update (:1383-1392) and the data of
 * calc_global (= plfx_finish_step).  The host keeps the loop over load steps and its bookkeeping.
 * Needs plfx_set_bc_plan (with the segment sources below) and plfx_set_finish_set.
 * Segment source codes: 0 left (value bcl0[k]), 1 bottom (bcb0[k]), 2 right (dbcr[k]), 3 top (dbct[k]), 4 node set (dbcn[k]). */
typedef struct plfx_step {
    /* in */
    int32_t il, nonlin, has_nodeset, warm, maxit;
    int32_t defer_slot; /* 0: the call returns the end-of-step data; 1 or 2: it returns as soon as the end-of-step kernels are
                         * enqueued, the data are collected later with plfx_finish_fetch(slot - 1) -- the caller's bookkeeping
                         * and the predictor of the next step overlap the state update of this one */
    double rtol;
    double bcl0[2], bcb0[2];
    double max_dbcr[2], max_dbct[2], max_dbcn[2]; /* increments planned for this step (max_dbcn is updated like the reference's alias, :1285) */
    double bcr[2], bct[2], bcn[2];                /* target totals */
    double bcr0[2], bct0[2], bcn0[2];             /* reached before this step */
    double sld[6];                                /* loading direction for calc_scf (:1245-1258) */
    /* out */
    double dbcr[2], dbct[2], dbcn[2];             /* increments applied in the end */
    double scale_bc;
    int32_t nit, nconv, nsweeps, nsolves, soft_fail, inconsistent_entry;
    int32_t its[40];
    double relres[40];
} plfx_step;
/* which segments of the registered BC plan take which value, and the force-controlled segments (edge force split
 * over the nodes, model.py:1145-1151): src/k per segment; nf force segments with flen[nf] DOFs each, fidx / fshare
 * concatenated */
int plfx_set_bc_sources(plfx_ctx *ctx, int nseg, const int32_t *src, const int32_t *k, int nf, const int32_t *fsrc,
                        const int32_t *fk, const int32_t *flen, const int32_t *fidx, const double *fshare);
int plfx_load_step(plfx_ctx *ctx, plfx_step *step, double *u_at, double *f_at, double *sums18);
int plfx_finish_fetch(plfx_ctx *ctx, int slot, double *u_at, double *f_at, double *sums18);

/* ---------------------------------------------------------------- strip-local engine
 * Multi-GPU form of the whole path for the reference's structured grids: the global NX x NY grid (node j*(NY+1)+k, element
 * j*NY+k, model.py:893, 935) is cut into x-strips of whole element columns; every rank holds ONE strip as a standalone local
 * mesh (plfx_set_mesh with el_begin = 0, el_end = nel; plfx_set_grid with its local column count) made of its owned columns
 * [own_col0, own_col1) of the local grid plus `halo` columns on each interior side.  Nothing is replicated except the
 * coarse problem; per PCG iteration the ranks exchange one halo slab of the residual (contiguous node columns, ncclSend /
 * ncclRecv), one all-reduce of the owned level-`coarse_level` residual into the replicated global coarse grid, and three
 * all-reduces of <= 8 KB of partial sums.  The V-cycle is arithmetically the one a single GPU runs on the global grid
 * (validity widths in DESIGN.md section 6), so iteration counts do not depend on the number of strips.  Material state and
 * sweep: when plfx_set_mesh was given exactly the owned columns as its owned element range [el_begin, el_end), the strip
 * holds and sweeps only those, and the six stiffness generators of the halo columns arrive from the neighbour that owns
 * them after every sweep that rewrote a tangent anywhere (6 * halo * NY doubles per side); with el_begin = 0, el_end = nel
 * the sweep runs on the halo elements too (state recomputed from the exchanged displacement increment, nothing else sent).
 * global_col0 = global element column of local column 0; halo (derived) must be at least 4 * 2^coarse_level (32 for level 3, 64 for
 * level 4); all column numbers and NY must be multiples of 2^coarse_level.  Needs the matrix-free operator and, for more
 * than one strip, a communicator (plfx_comm_init / plfx_comm_init_callback) created BEFORE this call.
 * plfx_sweep flags, plfx_scf_all statistics and plfx_finish_step element sums then refer to the whole grid; u_at / f_at of
 * plfx_finish_step and the nodal arrays are local (owned + halo columns); element state arrays hold the owned element range. */
int plfx_set_strip(plfx_ctx *ctx, int own_col0, int own_col1, int global_col0, int global_nx, int coarse_level);
/* diagnostic: one ncclSend / ncclRecv pair of this rank with itself inside a group plus one all-reduce on scratch buffers,
 * results checked on the host (the entry points the library binds by dlsym, on whatever hardware is at hand) */
int plfx_comm_selftest(plfx_ctx *ctx);
int plfx_strip_info(plfx_ctx *ctx, int *active, int *halo, int *coarse_level, int *coarse_levels, int64_t *halo_refreshes,
                    int64_t *coarse_gathers, int64_t *partial_allreduces, int64_t *generator_exchanges);
/* in-place all-reduce of n <= 32 host doubles over the context's communicator (op 0 = sum, 3 = min): the boundary sums of
 * calc_global (model.py:1452-1471) over the strips.  No-op without a communicator. */
int plfx_allreduce_host(plfx_ctx *ctx, double *buf, int n, int op);

/* Host-staged transport for the same collectives (tests on a single GPU, hosts without RCCL): every in-place all-reduce
 * the library needs is staged through host memory and handed to `fn` (dtype 0 = double, 1 = int32; op 0 = sum, 3 = min;
 * return 0 on success).  op 100 = halo exchange of a strip: buf holds [slab for the left neighbour | slab for the right
 * neighbour] (count / 2 doubles each) and must come back as [slab from the left | slab from the right]; every rank calls.  Slow by construction -- the product transport is plfx_comm_init (RCCL). */
typedef int (*plfx_allreduce_fn)(void *user, void *buf, size_t count, int dtype, int op);
int plfx_comm_init_callback(plfx_ctx *ctx, int rank, int nranks, plfx_allreduce_fn fn, void *user);
/* device_collectives = 1: this context shards the elements over an RCCL communicator; plfx_sweep (flags),
 * plfx_scf_all (statistics) and plfx_finish_step (element sums) then return values of the WHOLE mesh (all-reduced on
 * the device, on the library's stream) and the caller needs no collective of its own. */
int plfx_comm_info(plfx_ctx *ctx, int *rank, int *nranks, int *device_collectives);
/* ---------------------------------------------------------------- multi-GPU
 * RCCL communicator for the per-CG-step all-reduce of the global vector.  id is the 128-byte
 * ncclUniqueId created on rank 0 by plfx_comm_unique_id and broadcast by the caller. */
int plfx_comm_unique_id(char id[128]);
int plfx_comm_init(plfx_ctx *ctx, const char id[128], int rank, int nranks);

/* ---------------------------------------------------------------- SVC training (Material.train_SVC, material.py:1596-1640)
 * Binary RBF C-SVC fits by libsvm's non-shrinking SMO, many problems in one call (grid search: one per (C, gamma, fold)).
 * X [n*d] row-major features shared by all problems (1 <= d <= 16), y [n] labels -1 / +1; problem p trains on the rows
 * idx[off[p] .. off[p+1]) of X with C[p] > 0, gamma[p] > 0; tol: stopping tolerance of m(a) - M(a) (scikit-learn's 1e-3);
 * max_iter <= 0: max(10^7, 100 n_p).  Out: alpha[off[nprob]] in the order of idx (0 <= alpha <= C), rho[nprob] with
 * decision(x) = sum_k y_k alpha_k exp(-gamma |x - x_k|^2) - rho (scikit-learn: dual_coef_ = y alpha over alpha > 0,
 * intercept_ = -rho), obj[nprob] (NULL allowed) the dual objective, iters[nprob] SMO iterations, status[nprob] 0 converged,
 * 1 max_iter reached (libsvm's warning).  Rejects C or gamma <= 0, labels other than -1 / +1, d > 16, one-class problems. */
int plfx_svc_fit_batch(plfx_ctx *ctx, int n, int d, const double *X, const double *y, int nprob, const int32_t *off,
                       const int32_t *idx, const double *C, const double *gamma, double tol, int64_t max_iter,
                       double *alpha, double *rho, double *obj, int32_t *iters, int32_t *status);
/* One fit over ALL rows of X (same problem, arithmetic and outputs as plfx_svc_fit_batch with nprob = 1 and idx = 0 .. n-1,
 * bit for bit) spread over nwg workgroups that exchange the two selections of every SMO iteration grid-wide (k_smo_wide,
 * DESIGN.md §14).  nwg = 0: automatic (grows with n); a problem too large for the register-resident rows of one workgroup
 * per CU then runs on the plfx_svc_fit_batch solver.  A forced nwg must not exceed the CUs.  A grid-wide exchange that
 * does not complete within its time bound ends the fit with PLFX_ERR_HIP. */
int plfx_svc_fit_wide(plfx_ctx *ctx, int n, int d, const double *X, const double *y, double C, double gamma, double tol,
                      int64_t max_iter, int nwg, double *alpha, double *rho, double *obj, int32_t *iters, int32_t *status);
/* Decision values of nprob RBF-SVC models on rows of the shared X: problem p has the support vectors
 * X[sv_idx[sv_off[p] .. sv_off[p+1])] with coefficients coef[...] (dual_coef_), intercept[p] and gamma[p], and is evaluated
 * on the rows q_idx[q_off[p] .. q_off[p+1]) of X: dec[k] = sum_s coef_s exp(-gamma |x_q - x_s|^2) + intercept[p], summed in
 * the order given (libsvm's predict sums in support-vector order). */
int plfx_svc_decision_batch(plfx_ctx *ctx, int n, int d, const double *X, int nprob, const int32_t *sv_off,
                            const int32_t *sv_idx, const double *coef, const double *intercept, const double *gamma,
                            const int32_t *q_off, const int32_t *q_idx, double *dec);

/* ---------------------------------------------------------------- SVR flow rule (Material.setup_fgrad_SVM, material.py:2058-2131)
 * RBF epsilon-SVR fits by libsvm's non-shrinking SMO (solve_epsilon_svr), many problems in one call.  X [n*d] row-major
 * features shared by all problems (1 <= d <= 16); problem p trains on the rows idx[off[p] .. off[p+1]) of X, in that order,
 * with the targets t[off[p] .. off[p+1]) (one per entry of idx), C[p] > 0, gamma[p] > 0 and epsilon[p] >= 0; tol: stopping
 * tolerance (scikit-learn's SVR default 1e-3); max_iter <= 0: max(10^7, 200 l_p).  Out: coef[off[nprob]] in the order of
 * idx (alpha - alpha*, |coef| <= C; scikit-learn's dual_coef_ over coef != 0), rho[nprob] with prediction(x) =
 * sum_k coef_k exp(-gamma |x - x_k|^2) - rho (intercept_ = -rho), obj[nprob] (NULL allowed) the dual objective,
 * iters[nprob], status[nprob] 0 converged, 1 max_iter reached.  Rejects C or gamma <= 0, epsilon < 0 and d > 16. */
int plfx_svr_fit_batch(plfx_ctx *ctx, int n, int d, const double *X, int nprob, const int32_t *off, const int32_t *idx,
                       const double *t, const double *C, const double *gamma, const double *epsilon, double tol,
                       int64_t max_iter, double *coef, double *rho, double *obj, int32_t *iters, int32_t *status);
/* Predictions of m <= 8 RBF models that share the training rows X [n*d] and gamma, on nq points Q [nq*d] in one pass:
 * out[q*m + k] = sum_r coef[r*m + k] exp(-gamma |Q_q - X_r|^2) + intercept[k], every kernel value computed once and
 * the rows summed in order; coef [n*m] holds 0 where row r is no support vector of model k (an exact zero term leaves
 * the sum as it is, so a column is the sum over its support vectors in their order). */
int plfx_svr_predict_multi(plfx_ctx *ctx, int n, int d, const double *X, double gamma, int m, const double *coef,
                           const double *intercept, int nq, const double *Q, double *out);

/* SVR flow rule of Material.response (material.py:207-346 with ML_grad set; opt-in).  Attaches to material `mat` of the
 * loaded set -- a work-hardening SVC material (PLFX_SVC_WH), anything else is PLFX_ERR_UNSUPPORTED -- the seven models of
 * setup_fgrad_SVM: X [l*12] the standardised training rows, coef [l*7] as plfx_svr_predict_multi takes it (0 where a row
 * is no support vector of a model), intercept[7], gamma, the feature scaler feat_mean[12] / feat_scale[12] and the output
 * scaler out_mean[7] / out_scale[7] (six gradient components, then the hardening rate).  plfx_response_batch(_kh) then
 * runs the points of this material with every gradient evaluation taken from the SVRs: a = predictions 0-5 * out_scale +
 * out_mean (not normalised), and the point's hardening modulus is REPLACED by prediction 6 * out_scale[6] + out_mean[6] (not
 * clipped), as calc_fgrad overwrites Material.khard (:752-764); the predictions are those of plfx_svr_predict_multi on
 * ([sig | epl] - feat_mean) / feat_scale, bit for bit.  Sweeps and solves do not follow the rule.  l = 0 detaches;
 * plfx_set_materials detaches every rule.  The tables are copied to device memory owned by the context. */
int plfx_set_svr_flow(plfx_ctx *ctx, int mat, int l, const double *X, const double *coef, const double *intercept,
                      double gamma, const double *feat_mean, const double *feat_scale, const double *out_mean,
                      const double *out_scale);
/* The six column scales of material `mat`, a PLFX_SVC6_COLS record (any other kind: PLFX_ERR_UNSUPPORTED; without materials:
 * PLFX_ERR_STATE): its features are x_j = s_j / scale[j].  plfx_set_materials sets every one to the record's scale_seq; the
 * scales given here hold until the next plfx_set_materials.  A scale that is not finite or <= 0 is PLFX_ERR_ARG. */
int plfx_set_svc_cols(plfx_ctx *ctx, int mat, const double scale[6]);
/* rows of the rule attached to material `mat` (0: none) and the response launches that took the SVR kernel for it since
 * it was attached (either pointer may be NULL) */
int plfx_svr_flow_info(plfx_ctx *ctx, int mat, int *rows, int64_t *launches);
/* A texture field on material `mat`, a PLFX_SVC6_COLS record: coef[ntex * nsv], row-major, holds one row of
 * dual coefficients per texture (Material.fold_textures); an element or point with texture row t runs with row t in place of
 * the record's dual and with sum |coef[t][.]| (fabs in index order, as plfx_set_materials sums the record's) in the error bound
 * of the sampled ray.  Vectors, column scales, gamma and intercept are the record's.  The rows are copied to device memory
 * owned by the context, padded with zeros to the width of the row tables.  ntex = 0 detaches: the material is the plain
 * record again.  plfx_set_materials detaches every field; plfx_destroy frees them.  Another kind: PLFX_ERR_UNSUPPORTED; without
 * materials: PLFX_ERR_STATE; a coefficient that is not finite, ntex < 0 or ntex * (padded width) > INT32_MAX: PLFX_ERR_ARG. */
int plfx_set_svc_textures(plfx_ctx *ctx, int mat, int ntex, const double *coef);
/* The texture row of every element, tex_id[nel] in element order (after the mesh; every rank-owned element of a single-GPU
 * mesh).  NULL, or a new mesh, clears it: every element has row 0.  Entries of elements whose material carries no field are
 * ignored; the others are checked on the host against the attached rows when a sweep or calc_scf is set up, and an entry
 * outside 0..ntex-1 is PLFX_ERR_ARG there, before anything is launched.  A strip, a shard or a communicator with a field
 * material in the model is PLFX_ERR_UNSUPPORTED. */
int plfx_set_element_textures(plfx_ctx *ctx, const int32_t *tex_id);
/* plfx_full_yf_batch / plfx_response_batch with the texture row of every point, tex_id[n] (NULL: row 0).  Points of materials
 * without a field ignore their entry; the others are checked on the host (PLFX_ERR_ARG, nothing launched). */
int plfx_full_yf_batch_tid(plfx_ctx *ctx, int mat, int n, const double *sig, const double *epl,
                           const double *ld, double *yf, int32_t *status, const int32_t *tex_id);
int plfx_response_batch_tid(plfx_ctx *ctx, int n, const int32_t *mat_id, const double *sig,
                            const double *epl, const double *deps, double *fy, double *sig_out,
                            double *depl, double *ct /* [n*36] */, int32_t *nsteps, const int32_t *tex_id);
/* rows attached to material `mat` (0: none), whether they are staged in LDS (0: the kernels read them from device memory),
 * and the launches that took a texture-field instantiation for it since the rows were attached (any pointer may be NULL) */
int plfx_svc_textures_info(plfx_ctx *ctx, int mat, int *rows, int *staged, int64_t *launches);

/* ---------------------------------------------------------------- instrumentation */
/* accumulated HIP-event time (ms) and launch count of a named kernel family since the last reset:
 * which: 0 streaming phase of the material sweep (k_sweep_light / k_sweep_svc_row<0>); also the kernels of the batched point
 *          functions (plfx_response_batch, plfx_seq / fgrad / yf / full_yf_batch, plfx_hessian_batch, plfx_yield_scale, plfx_flow_curve, plfx_committee_yf, plfx_tex_svc_yf, plfx_tex_svc_yield_scale, plfx_tex_svc_fgrad / full_yf / response, plfx_svr_predict_multi), 1 spmv(+dot), 2 cg vector
 *        update, 3 assemble, 4 multigrid V-cycle (whole cycle), 5 fine-level multigrid smoother launches,
 *        6 sub-stepping phase of the material sweep (k_sweep_heavy / k_sweep_svc_row<1>),
 *        7 collectives on the library's stream (RCCL all-reduces, halo and generator exchanges; every call is timed, the time
 *          includes the wait for the slowest peer) */
int plfx_timing_get(plfx_ctx *ctx, int which, double *ms, int64_t *launches);
int plfx_timing_reset(plfx_ctx *ctx);
int plfx_timing_enable(plfx_ctx *ctx, int on);
/* Bit f of mask = time family f (default: all).  Every timed launch costs two hipEventRecord calls (about 4 us of host time
 * each and a bubble on the stream); bench.py times only the two kernels its roofline objects need. */
int plfx_timing_select(plfx_ctx *ctx, unsigned mask);
/* time only every n-th launch of a selected family (n >= 1; the averages stay representative, the host cost drops n-fold) */
int plfx_timing_sample(plfx_ctx *ctx, int every);

#ifdef __cplusplus
}
#endif
#endif /* PLFX_H */
