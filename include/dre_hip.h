/* libdre_hip — C ABI of the MI355X-native low-rank Rosenbrock/ADI engine.
 *
 * Drop-in boundary for the hot path of mpimd-csc/DifferentialRiccatiEquations.jl v0.5.5
 *   solve(GDREProblem{<:LDLᵀ}, Ros1/Ros2(ADI(...)))  and everything below it.
 * The reference has no FFI of its own (pure Julia, multiple dispatch); each entry point cites the
 * reference method it replaces (paths relative to the reference tree).  The Julia shim that binds
 * these symbols with `ccall` is differentialriccatiequations.jl_amd/julia/DREHip.jl; the ctypes
 * binding used by the tests is differentialriccatiequations.jl_amd/_lib.py.  See INTEGRATION.md.
 *
 * Conventions
 *  - every function returns an int32 status: 0 ok, <0 error (dre_last_error(ctx) has the text);
 *    no exception crosses the boundary;
 *  - dense matrices are column-major Float64 (Julia `Matrix{Float64}`), sparse matrices are passed
 *    as the three arrays of a Julia `SparseMatrixCSC{Float64,Int64}` (colptr, rowval, nzval; 1-based
 *    with index_base = 1) — CSC of M is byte-for-byte CSR of M', which is what every product on
 *    the path needs (E'V, A'L, (A'+pE')\R);
 *  - host buffers belong to the caller, device objects to the context; every object has a *_free;
 *  - one context per GPU / host thread; all work of a context is ordered on its private HIP stream;
 *  - there is NO CPU fallback: without a usable HIP device dre_ctx_create fails with DRE_ERR_NODEVICE.
 */
#ifndef DRE_HIP_H
#define DRE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRE_OK 0
#define DRE_ERR_INVALID (-1)
#define DRE_ERR_HIP (-2)
#define DRE_ERR_ALLOC (-3)
#define DRE_ERR_SINGULAR (-4)
#define DRE_ERR_INTERNAL (-5)
#define DRE_ERR_NODEVICE (-6)
#define DRE_ERR_NOT_STABLE (-7)   /* dense path: (F, E) is not c-stable, the sign iteration did not reach -E; dense GARE: the Hamiltonian has eigenvalues on or near the imaginary axis */
#define DRE_ERR_STEP (-8)         /* adaptive dense path: a step was rejected at dt_min, or more than max_steps trial steps were needed */

/* hard limits of the engine */
#define DRE_ADI_MAX_ITERS 100000      /* largest dre_adi_options.maxiters (the device keeps the norm history as a ring that the host empties per chunk) */
#define DRE_SMW_MAX_RANK 32           /* columns of the low-rank factors U, V of F = cA*A + cE*E + inv(alpha)*U*V */

/* warning bits reported by ADI (AdiResult.warnings) */
#define DRE_WARN_NOT_CONVERGED 1      /* src/lyapunov/adi.jl:125-126 */
#define DRE_WARN_ZERO_INCREMENT 2     /* src/lyapunov/adi.jl:134-137,200-204: a complex pair's solve returned V = 0 exactly; the increment is zero,
                                         X and the residual are left alone and the iteration stops with the pair's two shifts counted */
#define DRE_WARN_RITZ_DISCARDED 4     /* src/shifts/helpers.jl:133 */
#define DRE_WARN_RITZ_FLIPPED 8       /* src/shifts/helpers.jl:136 */
#define DRE_WARN_PIVOT_GROWTH 16      /* the pivot-free sparse LU met multipliers above "pivot_growth_warn" (default 1e8); the convergence claim of
                                         this solve was re-checked against the residual evaluated from scratch (see dre_shift_factor) */

typedef struct dre_ctx dre_ctx;
typedef struct dre_dense dre_dense;
typedef struct dre_pencil dre_pencil;
typedef struct dre_factor dre_factor;
typedef struct dre_ldlt dre_ldlt;
typedef struct dre_adi_result dre_adi_result;
typedef struct dre_gdre_result dre_gdre_result;

/* ---- context ------------------------------------------------------------------------------ */
int dre_version(void);
int dre_ctx_create(int device, dre_ctx** out);
int dre_ctx_destroy(dre_ctx* ctx);
const char* dre_last_error(dre_ctx* ctx);
int dre_ctx_sync(dre_ctx* ctx);
int dre_ctx_info(dre_ctx* ctx, int64_t* info /* [0]=CUs [1]=pool bytes */);
/* Tunables of the engine (no counterpart in the reference; they select between device code paths that compute the same result):
 *   "dense_inverse_max_n"  real ADI shifts on pencils with n <= value apply a cached dense inverse of A' + mu E' by MFMA GEMM
 *                          instead of the multifrontal triangular sweeps (default 1536, or env DRE_DENSE_INV_MAX_N; 0 disables).
 *   compress! (LDLt.jl:204-225) without a QR of the factor — the band reduction runs in the natural coordinates:
 *   "compress_direct_max_n"     n <= value and columns >= n / compress_direct_ratio: S = L D L' (n x n) is formed directly
 *                               (default 2560; n <= 512 always);  "compress_direct_ratio" (default 8)
 *   "compress_factor_min_n"     n >= value: band reduction in factor form, reflectors applied to L, randomized termination estimate
 *                               (default 2561; a huge value disables);  "compress_factor_min_cols" (default 96) fewer columns: QR path
 *   "compress_sketch"           wide factors (columns >= "compress_sketch_min_cols", default 320, and >= "compress_sketch_ratio", default 1.25, x the sketch width) of sums without
 *                               cancellation: randomized range finder, three GEMM passes over the factor; sketch width = rank of the previous
 *                               compression of this kind + "compress_sketch_extra" (48); rejected sketches fall back (default 1, 0 disables)
 *   "compress_sketch_sparse"    1 (default): the test matrix of the sketch is a structured sparse sign matrix (8 entries +-1/sqrt(8) per row), applied
 *                               in one pass over the factor; 0: Gaussian (dense GEMM).  The acceptance test uses 16 independent Gaussian probe
 *                               columns either way; two probe rejections at an order n switch that order to the Gaussian matrix
 *   "compress_sketch_cholqr"    1 (default): the sketch is orthonormalised in 64-column blocks by block Gram-Schmidt + Cholesky QR, both twice
 *                               (GEMMs and a 64 x 64 Cholesky kernel); a block with cond > ~3e6 is detected on the device and the compression
 *                               redone, after two such events at an order n Householder/TSQR panels are used (0: always)
 *   (env: DRE_COMPRESS_DIRECT_MAX_N, DRE_COMPRESS_DIRECT_RATIO, DRE_COMPRESS_FACTOR_MIN_N, DRE_COMPRESS_FACTOR_MIN_COLS, DRE_COMPRESS_SKETCH*)
 *   "mf_subtree"                1: the multifrontal sweeps below the dense top run as one workgroup per subtree (default 0: one launch per level)
 *   "setup_streams"             helper streams for the factorisations / dense inverses of the shifts of a Cyclic list (default 5; 0, 1: none)
 *   "top_inverse_max_rows"      multifrontal solves with a real factor that keeps being reused (third multi-column solve on): the top
 *                               levels of the elimination tree with at most this many pivot variables are applied as ONE dense inverse
 *                               of their Schur complement (MFMA GEMM) instead of level-by-level sweeps (default 1536, 0 disables;
 *                               env DRE_TOP_INVERSE_MAX_ROWS)
 *   "pivot_growth_warn" / "pivot_growth_fail"   thresholds on the largest multiplier of the pivot-free sparse LU (defaults 1e8 / 1e13), see dre_shift_factor
 *   "dense_x_max_n"            Ros1 without save_state, real Cyclic shifts, n <= value (default 1536): X is carried as a dense symmetric n x n matrix
 *                               between the time steps and converted to LDL' form once at the end (env DRE_DENSE_X_MAX_N; 0 disables)
 *   "x_side_stream"             Ros1, n <= 1536, no save_state: X is carried as "compressed warm start + ADI increments" and its
 *                               compression (adi.jl:78-80) runs on a second stream beside the next time step (default 1; env
 *                               DRE_X_SIDE_STREAM);  "x_compress_every" = s (default 1) with x_side_stream = 0: single stream,
 *                               X compressed every s-th step only
 *   "dense_gj_panel"            dense path: the pivoting panel of the Gauss-Jordan inversions.  0 (default) auto: the register panel for
 *                               n <= 4096, the tournament panel above; 1 the register panel only (n > 4096 is DRE_ERR_INVALID); 2 the
 *                               tournament panel at every n.  Other values are DRE_ERR_INVALID
 *   "sym_eig_method"            the symmetric eigensolver behind the rank-revealing compressions (FactoredSign, compress!, the projection's Gram
 *                               eigenproblem).  0 (default) Householder tridiagonalisation + implicit QL (dre_sym_eig); 1 block Jacobi on the
 *                               whole device (dre_sym_eig_jacobi).  Other values are DRE_ERR_INVALID
 *   "gemm_swizzle"              workgroup -> tile order of the split-K GEMM.  1 (default): XCD-aware where the larger operand does not fit the
 *                               Infinity Cache; 0: launch order; 2 (diagnostic): XCD-aware in every launch, whatever its size.  Same results */
int dre_ctx_set_option(dre_ctx* ctx, const char* name, double value);
/* the current value of an option of dre_ctx_set_option (tests snapshot and restore what they change; no reference counterpart: the reference's
 * tunables are keyword arguments) */
int dre_ctx_get_option(dre_ctx* ctx, const char* name, double* value);
/* per-kernel-class timing with HIP events on the library stream (replaces TimerOutputs.@timeit_debug,
 * src/DifferentialRiccatiEquations.jl:22 and the sections listed in SURVEY.md §5) */
int dre_prof_enable(dre_ctx* ctx, int on);
int dre_prof_reset(dre_ctx* ctx);
int dre_prof_count(dre_ctx* ctx, int* n);
int dre_prof_get(dre_ctx* ctx, int i, char* name, int name_len, double* ms, int64_t* launches, double* bytes, double* flops);

/* ---- dense matrices (array backend: similar/adapt/copyto!) ------------------- */
int dre_dense_upload(dre_ctx* ctx, int rows, int cols, const double* host, int ld, dre_dense** out);
int dre_dense_create(dre_ctx* ctx, int rows, int cols, dre_dense** out);            /* zero-filled */
int dre_dense_download(dre_ctx* ctx, const dre_dense* a, double* host, int ld);
/* device-to-device interop with buffers the caller owns (the exchange buffers of the multi-GPU layer, e.g. a torch tensor's data_ptr):
 * column-major with leading dimension ld; both synchronise the context's stream */
int dre_dense_from_device(dre_ctx* ctx, int rows, int cols, const double* src_dev, int ld, dre_dense** out);
int dre_dense_to_device(dre_ctx* ctx, const dre_dense* a, double* dst_dev, int ld);
int dre_dense_shape(const dre_dense* a, int* rows, int* cols);
int dre_dense_free(dre_ctx* ctx, dre_dense* a);

/* ---- the pencil (E, A): union pattern, nested-dissection ordering, symbolic multifrontal analysis,
 *      done once per problem because the pattern of A' + pE' never changes
 *      (replaces the per-step `factorize` analysis of src/blocklinear/backslash.jl:13) --------- */
int dre_pencil_create(dre_ctx* ctx, int n, const int64_t* E_colptr, const int64_t* E_rowval, const double* E_nzval,
                      const int64_t* A_colptr, const int64_t* A_rowval, const double* A_nzval, int index_base,
                      int leaf_size, dre_pencil** out);
/* host-only variant (no GPU touched): symbolic analysis for inspection / CPU tests */
int dre_pencil_create_host(int n, const int64_t* E_colptr, const int64_t* E_rowval, const double* E_nzval,
                           const int64_t* A_colptr, const int64_t* A_rowval, const double* A_nzval, int index_base,
                           int leaf_size, dre_pencil** out);
int dre_pencil_free(dre_pencil* p);
/* info: [0]=n [1]=nnz(union) [2]=tree nodes [3]=levels [4]=max front [5]=max separator [6]=factor nnz [7]=fronts slab entries */
int dre_pencil_info(const dre_pencil* p, int64_t* info);
/* integer arrays of the symbolic structure by name ("perm","iperm","ptr","idx","first","size","parent","level",
 * "child_ptr","child_idx","bptr","bidx","cmap_ptr","cmap","front_off","inv_off","upd_off","asm_dest","lvl_ptr","lvl_nodes") */
int dre_pencil_get_array(const dre_pencil* p, const char* name, int64_t* out, int64_t cap, int64_t* len);
int dre_pencil_get_values(const dre_pencil* p, int which /*0 = E', 1 = A'*/, double* out, int64_t cap);

/* ---- kernels exposed one by one (extension points of SURVEY.md §8b; parity tests call these) -- */
/* C = alpha*op(A)*op(B) + beta*C on the f64 MFMA path (LinearAlgebra.mul!) */
int dre_gemm(dre_ctx* ctx, int transA, int transB, double alpha, const dre_dense* A, const dre_dense* B, double beta, dre_dense* C);
/* Y = alpha*M'*X + beta*Y, M = E (which=0) or A (which=1): mul!(R, E', V, a, b) src/lyapunov/adi.jl:171,217 */
int dre_spmm(dre_ctx* ctx, const dre_pencil* p, int which, double alpha, const dre_dense* X, double beta, dre_dense* Y);
/* orthf(L) -> Q, R  (src/LDLt.jl:237-245) */
int dre_orthf(dre_ctx* ctx, const dre_dense* L, dre_dense** Q, dre_dense** R);
/* The reference's EXTENSION POINT `DifferentialRiccatiEquations.orthf(L) -> (Q, R)` (src/LDLt.jl:227-245; test/cuda.jl:32-37 substitutes an SVD):
 * a user-supplied orthogonalisation for this context.  L is n x c (device, column-major, leading dimension ldl); the callback fills Q (n x p,
 * orthonormal columns) and R (p x c) with p = min(n, c) and L = Q R, and returns 0.  It is called with the context's stream idle and must return
 * when its own work is complete.  Honoured wherever the engine runs the reference's arithmetic: the literal compression (ADI option
 * compress_exact, dre_ldlt_compress: src/LDLt.jl:211) and dre_ldlt_norm (src/LDLt.jl:84).  fn = NULL restores the library's Householder QR. */
typedef int (*dre_orthf_fn)(void* user, int n, int c, const double* L, int ldl, double* Q, int ldq, double* R, int ldr);
int dre_ctx_set_orthf(dre_ctx* ctx, dre_orthf_fn fn, void* user);
/* eigen(Symmetric(S)) with early-terminating tridiagonalisation (src/LDLt.jl:214); returns the j computed
 * eigenpairs (all those above tolfac*eps*||S||_F in magnitude), values ascending */
int dre_sym_eig(dre_ctx* ctx, const dre_dense* S, double tolfac, dre_dense** values, dre_dense** vectors);
/* Test and diagnostic surface of that solver (dre_version >= 114): ONE run of its chain with the arguments the library's own callers pass, and
 * every intermediate result.  The reduction stops at the first j with ||S22||_F^2 + 2 e_(j-1)^2 <= tol^2, where S22 is the trailing block not
 * yet reduced and tol = tolfac eps ||S||_F;  abs_tol > 0 replaces tol (floor_mode = 0) or is its lower limit (floor_mode = 1: tol =
 * max(tolfac eps ||S||_F, abs_tol)).  deflate: an off-diagonal entry of T_j at or below deflate eps ||S||_F counts as zero in the QL iteration
 * for jdim > 128; at jdim <= 128 the constant is 1e-3 whatever deflate says.  S is left untouched; the context option "sym_eig_method" does
 * not reroute the call.
 * ii (3): [0] jdim, the order of the kept tridiagonal matrix [1] nref, the reflectors generated [2] q;  *snorm = ||S||_F.
 * *d (jdim x 1), *e (max(jdim - 1, 0) x 1): T_j;  *tau (q x 1, zero from nref on);  *V (q x q): column i holds reflector i, H_i = I - tau_i v v',
 * v(i + 1) = 1, zero above, zero columns from nref on.  want_eig != 0 and jdim > 0: *w (jdim x 1) the eigenvalues of T_j, UNSORTED, and *Z
 * (jdim x jdim), column i the eigenvector of w(i); otherwise both are NULL.
 * ids (nids entries of [0, jdim), any order, repeats allowed): *B (q x nids) = H_0 ... H_(nref-1) [Z(:, ids); 0], with want_eig = 0 the same
 * with the unit vectors e_ids in the place of Z's columns; nids < 0: every column 0 .. jdim - 1 (ids is not read); no column: *B is NULL.
 * Every output pointer but ii may be NULL (B only with nids = 0).
 * DRE_ERR_INVALID before any launch for a matrix that is not square or of an order above 8192; after the reduction, before anything else is
 * launched, for a non-finite S (or one whose squares overflow) and for an entry of ids outside [0, jdim).  The context stays usable. */
int dre_sym_eig_probe(dre_ctx* ctx, const dre_dense* S, double tolfac, int want_eig, double abs_tol, int floor_mode, double deflate, const int32_t* ids,
                      int nids, int64_t* ii /* 3 */, double* snorm, dre_dense** d, dre_dense** e, dre_dense** tau, dre_dense** V, dre_dense** w,
                      dre_dense** Z, dre_dense** B);
/* Test and diagnostic surface of the dense-inverse ADI chain (dre_version >= 116): the entry points adi_fast_build, adi_fast_pack_r, adi_fast_iter,
 * adi_group_pack and adi_group_iter (csrc/dense.hip) on caller-supplied operands, driven by exactly the pipeline of the engine's fast branch and of
 * the dense-X time loop's group branch (Gram matrix of iteration j riding on launch j + 1, norm and decision on launch j + 2, two flush launches).
 * No kernel of its own.  Every array is HOST memory, column-major, without padding; every output array may be NULL.
 * kind 0 (DRE_ADI_PROBE_FAST): build, pack R0, nit iterations, two flushes.  kind 2 (DRE_ADI_PROBE_BUILD): build only.
 *   stacks: nstack matrices [N; E'N; U'N] of (2n + m) x n;  wks: nstack matrices of 2n x m (NULL with m = 0);  wks_null (nstack flags or NULL):
 *   1 = that shift is built WITHOUT a correction (null pointer: the whole build then takes the scalar kernel);  packs: nstack packed effective
 *   stacks of 2 nstrip kst 64 doubles, nstrip = ceil(n / 16), kst = ceil(n / 4): entry (row 16 s + (lane & 15), column 4 t + (lane >> 4)) of half h
 *   (0: top, 1: bottom) at ((h nstrip + s) kst + t) 64 + lane, zero padded.
 * kind 1 (DRE_ADI_PROBE_GROUP): pack, then launches L = 0 .. nit / g + 1 of g iterations each.  stacks: nstack = ncyc / g matrices
 *   [Om_0 .. Om_(g-1); Pi_1 .. Pi_g] of (2 g n) x n, one per start position of the cycle;  packs: nstack x 2 g nstrip kst 64 doubles (same order,
 *   block b in the place of half h).  m, wks, tdiag, mode and nt are not read.
 * cycle (ncyc entries of [0, nstack), kinds 0 and 2 only) names the stack of every position of the cycle, mu (ncyc) its shift; iteration j
 * (1-based) uses position (j - 1) mod ncyc.  R0: n x k;  T: k x k (tdiag = 1 promises that it is diagonal);  the control block starts with
 * iters = base_it, done = 0, the given abstol and maxiters, and NaN in every norm.
 * mode / nt: -1 = adi_fast_pick (both must then be -1), otherwise mode 0 (K-split tiles) or 1 (LDS-staged strips) and nt 1, 2 or 4.
 * Outputs.  V, R: ld x k (nit + 1), prefilled with NaN: V_j / R_j (after iteration j = 1 .. nit) in rows [0, n) of columns [(j - 1) k, j k);  rows
 * from n on and the last k columns are never written.  Rp: nit + 1 slots of 4 nstrip ceil(k / 16) 64 doubles, prefilled with NaN: slot 0 the packed
 * R0, slot j the packed R_j as the launch that produced it left it — element (row 4 t + (lane >> 4), column 16 c + (lane & 15)) at
 * (t ceil(k / 16) + c) 64 + lane, zero padded; all NaN with mode 1, which does not use it.  The first packed residual lives in an allocation of exactly
 * one slot, the others in one of nit + 1 slots whose first is unused, as in the time loop.  G: the Gram matrices R_j' R_j still held when the chain
 * ends, prefilled with NaN — kinds 0: 2 slots of k x k, slot (j & 1);  kind 1: 2 g slots, slot (L & 1) g + i for residual i of launch L - 1.
 * state_i (4): iters, done, mode used, nt used;  state_d (514): res_norm, abstol, norms[512] (index = shifts consumed & 511).
 * DRE_ERR_INVALID before any launch: n < 1, k < 1, k > 512 (kind 1: k > 256), m < 0, nit < 1 or > 480 (kind 1: not a multiple of g), g outside
 * 2 .. 6, ncyc not a multiple of g or nstack != ncyc / g, g ceil(k / 16) ceil(ceil(k / 16) / 4) > 1031, mode outside {0, 1}, nt outside {1, 2, 4},
 * ld < n + 2, an entry of cycle outside [0, nstack), base_it < 0, a missing input. */
enum { DRE_ADI_PROBE_FAST = 0, DRE_ADI_PROBE_GROUP = 1, DRE_ADI_PROBE_BUILD = 2 };
typedef struct dre_adi_chain_probe_args {
    int32_t kind, n, m, k;
    int32_t nstack, ncyc, g, nit;
    int32_t base_it, maxiters, tdiag, mode;
    int32_t nt, ld;
    double alpha, abstol;
    const double* stacks; const double* wks; const int32_t* wks_null; const int32_t* cycle; const double* mu; const double* R0; const double* T;
    double* V; double* R; double* packs; double* Rp; double* G;
    int32_t* state_i; double* state_d;
} dre_adi_chain_probe_args;
int dre_adi_chain_probe(dre_ctx* ctx, const dre_adi_chain_probe_args* args);
/* Test and diagnostic surface of the warm-started compression (dre_version >= 120; csrc/warm.hip, DESIGN.md "warm probe"): ONE call of an entry
 * point of that file on caller-supplied operands, in buffers shaped like those of the library's own callers (the basis buffer [Om | Q | Z], the
 * right-hand block [Y_p, Y_f, W, Z, W_2], the slab of nslab 256 + nstrip + 256 doubles with C behind the shares, the context's block of four
 * arrival counters, zeroed once per context).  No kernel of its own.  Every array is HOST memory, column-major, without padding; every output may
 * be NULL; every output is prefilled with NaN on the device, so what a kernel never wrote comes back as NaN.  Matrices of n rows live in
 * allocations of n + ldpad rows (the library's callers: ldpad = 0) and their OUTPUTS come back with all n + ldpad rows.
 * stage 0 PROJECT (warm_project):  Q (n x q), Yf (n x 16), Pf (q x 16)  ->  Z1_out ((n + ldpad) x 16), Cw_out (16 x 16), slab (nslab x 256 shares of
 *   Z_1'Z_1, share (i, j) of workgroup b at 256 b + i + 16 j;  nslab = ceil(n / rows), rows = 16 up to 256 strips of 16 rows, else 16 ceil(strips / 256)).
 * stage 1 Z (warm_z, n <= 1024):  Z1 (n x 16), Cw, Res (n x n)  ->  Zb, Zy, W2 ((n + ldpad) x 16 each).   stage 2 ZAPPLY (warm_zapply): Z1, Cw -> Zb, Zy.
 *   q only places the views inside the two buffers.
 * stage 3 SMALL (warm_small; mode 0: the Jacobi form, mode 1: stops behind the whitening):  Cc (m x (64 + q)) = [P_p | . | B'W | B'Z | B'W_2], parts
 *   (nparts, or NULL with 0), reltol, abstol, frac, budget_frac, kl, qn  ->  tols (12), Uc (m x qn), T (kl x kl), Cp (m x 16), mode 1: Mout, LTout (m x m).
 * stage 4 EIG (warm_eig):  S (m x m)  ->  U (m x m).
 * stage 5 FINISH (warm_finish):  Q = B (n x q, q <= 80), Wk (q x kl), Yp (n x 16), Pp (q x 16), tols_in (12: [1], [5], [7] are read)  ->  R ((n + ldpad) x
 *   16 ceil(kl / 16)), tols (12), slab (ceil(n / 16) shares of the probe).
 * stage 6 CHAIN (the launch sequence of the dense-X time loop's compression, Jacobi form, n <= 1024):  Res (n x n), basis (n x (32 + q): [Om_p, Om_f, Q]),
 *   parts / nparts, reltol, abstol, frac, budget_frac, kl, qn (at most 64)  ->  R ((n + ldpad) x qn: the next basis, its first kl columns the chain's R),
 *   basis_out ((n + ldpad) x (32 + q + 16): with Z in the last 16 columns), T, tols, Uc ((q + 16) x qn), Cp ((q + 16) x 16).
 * ticket (2): the arrival counters of warm_project and of warm_small / warm_finish after the call.
 * DRE_ERR_INVALID before any launch: an unknown stage, n < 1, q outside 1 .. 64 (FINISH: 1 .. 80), m not q or q + 16, m > 80, qn outside 1 .. m, kl
 * outside 1 .. qn (FINISH: 1 .. 80), n > 1024 for Z and CHAIN, mode outside {0, 1}, nparts without parts, a missing input.  The context stays usable. */
enum { DRE_WARM_PROBE_PROJECT = 0, DRE_WARM_PROBE_Z = 1, DRE_WARM_PROBE_ZAPPLY = 2, DRE_WARM_PROBE_SMALL = 3, DRE_WARM_PROBE_EIG = 4, DRE_WARM_PROBE_FINISH = 5,
       DRE_WARM_PROBE_CHAIN = 6 };
typedef struct dre_warm_probe_args {
    int32_t stage, n, q, m;
    int32_t kl, qn, nparts, mode;
    int32_t ldpad, reserved;
    double reltol, abstol, frac, budget_frac;
    const double* Q; const double* Yf; const double* Pf; const double* Z1; const double* Cw; const double* Res; const double* Cc; const double* parts;
    const double* S; const double* Wk; const double* Yp; const double* Pp; const double* tols_in; const double* basis;
    double* Z1_out; double* Cw_out; double* slab; double* Zb; double* Zy; double* W2; double* tols; double* Uc; double* T; double* Cp; double* Mout;
    double* LTout; double* U; double* R; double* basis_out;
    int32_t* ticket;
} dre_warm_probe_args;
int dre_warm_probe(dre_ctx* ctx, const dre_warm_probe_args* args);
/* eigen(Symmetric(S)) by two-sided cyclic block Jacobi on the whole device (blocks of 16, round-robin ordering, both products of the update on
 * v_mfma_f64_16x16x4_f64): all q eigenpairs, values ascending, S untouched (full symmetric storage; indefinite, rank-deficient and clustered
 * spectra are fine).  Converged when off(A) <= tol ||A||_F; tol <= 0: q eps.  stats (may be NULL): [0] block sweeps, [1] rounds.
 * DRE_ERR_INVALID for a non-finite S, DRE_ERR_INTERNAL after 30 sweeps.  The context option "sym_eig_method" = 1 puts this solver behind
 * every rank-revealing compression of the library instead of the Householder + QL solver of dre_sym_eig. */
int dre_sym_eig_jacobi(dre_ctx* ctx, const dre_dense* S, double tol, dre_dense** values, dre_dense** vectors, int64_t* stats);
/* factorize(cA*A' + (cE_re + i cE_im)*E')  (src/blocklinear/backslash.jl:8-15); complex iff cE_im != 0.
 * The multifrontal LU does NOT pivot (the reference's UMFPACK / CHOLMOD do): it is exact-arithmetic safe for the pencils of the path
 * (-(A + pE) symmetric positive definite for real p < 0, complex symmetric with definite parts otherwise) and for diagonally dominant
 * ones.  For anything else the largest multiplier |l_ik| is tracked: above "pivot_growth_fail" (default 1e13; dre_ctx_set_option) the
 * factorisation is rejected with DRE_ERR_SINGULAR, above "pivot_growth_warn" (default 1e8) ADI results carry DRE_WARN_PIVOT_GROWTH and
 * their convergence claim is verified against the true residual.  Pencils that need pivoting take a user block solver
 * (dre_adi_options.inner_solve). */
int dre_shift_factor(dre_ctx* ctx, const dre_pencil* p, double cA, double cE_re, double cE_im, dre_factor** out);
/* X = F \ B  (src/blocklinear/backslash.jl:17-21); X_im may be NULL for a real factor */
int dre_shift_solve(dre_ctx* ctx, const dre_factor* f, const dre_dense* B, dre_dense** X_re, dre_dense** X_im);
/* X = (M + inv(alpha) * Vt * U') \ B  with M the factorised sparse matrix: ShermanMorrisonWoodbury(Backslash) applied to
 * BlockLinearProblem(LowRankUpdate(M, alpha, Vt, U'), B)  (src/blocklinear/sherman-morrison-woodbury.jl:10-45, src/LowRankUpdate.jl:61-64).
 * U and Vt are n x m (m <= DRE_SMW_MAX_RANK); complex iff the factor is. */
int dre_shift_solve_smw(dre_ctx* ctx, const dre_factor* f, double alpha, const dre_dense* U, const dre_dense* Vt, const dre_dense* B,
                        dre_dense** X_re, dre_dense** X_im);
int dre_factor_growth(dre_ctx* ctx, const dre_factor* f, double* growth);   /* largest multiplier met by the LU */
/* Static pivoting (the reference's factorize pivots: UMFPACK / CHOLMOD, src/blocklinear/backslash.jl:13): pivots below
 * pivot_static * max|entry| (option "pivot_static", default sqrt(eps); 0 = plain pivot-free LU) are replaced by that value, which bounds
 * the multipliers by 1 / pivot_static; solves with a factor that has replaced pivots run "pivot_refine_steps" (default 3) steps of
 * fixed-point refinement against the true operator (real shifts; a complex factor with replaced pivots is refused: user block solver).
 * count = number of replaced pivots of this factor. */
int dre_factor_perturbed(dre_ctx* ctx, const dre_factor* f, int64_t* count);
int dre_factor_free(dre_ctx* ctx, dre_factor* f);

/* ---- LDLᵀ objects (src/LDLt.jl) ------------------------------------------------------------ */
/* lowrank(L, D) scaled by alpha; rows are permuted to the pencil's ordering when p != NULL */
int dre_ldlt_create(dre_ctx* ctx, const dre_pencil* p, const dre_dense* L, const dre_dense* D, double alpha, dre_ldlt** out);
int dre_ldlt_zero(dre_ctx* ctx, const dre_pencil* p, int n, dre_ldlt** out);
int dre_ldlt_free(dre_ctx* ctx, dre_ldlt* x);
int dre_ldlt_info(const dre_ldlt* x, int* n, int* rank, int* nblocks);
int dre_ldlt_add(dre_ctx* ctx, const dre_ldlt* a, const dre_ldlt* b, dre_ldlt** out);          /* LDLt.jl:131-148 */
int dre_ldlt_scale(dre_ctx* ctx, const dre_ldlt* a, double alpha, dre_ldlt** out);             /* LDLt.jl:156-159 */
int dre_ldlt_concatenate(dre_ctx* ctx, dre_ldlt* x);                                           /* LDLt.jl:174-191 */
int dre_ldlt_compress(dre_ctx* ctx, dre_ldlt* x);                                              /* LDLt.jl:204-225 */
/* compress! with an ABSOLUTE truncation tolerance (Frobenius norm of what may be dropped) instead of the relative one: used where the
 * caller only compares norm(x) with a tolerance (Riccati / Lyapunov residuals near convergence are pure cancellation noise relative to
 * their own size, so a relative criterion keeps all of it).  abs_tol <= 0 behaves like dre_ldlt_compress_fast. */
int dre_ldlt_compress_tol(dre_ctx* ctx, dre_ldlt* x, double abs_tol);
/* The engine's own compression (what the ADI and Rosenbrock loops use between the API boundaries): early-terminating band reduction — on
 * S = L D L', in factor form, or through a randomized range finder for wide factors — truncated at 4 eps ||X||_F; the result has an
 * orthonormal factor and a band matrix D instead of diag(eigenvalues).  Same X up to that tolerance. */
int dre_ldlt_compress_fast(dre_ctx* ctx, dre_ldlt* x);
int dre_ldlt_norm(dre_ctx* ctx, dre_ldlt* x, double* out);                                     /* LDLt.jl:77-89 */
/* bring an engine result to the reference's canonical form: one component, D = diag(eigenvalues), |lambda| >= 100 eps max|lambda| */
int dre_ldlt_canonicalize(dre_ctx* ctx, dre_ldlt* x);
/* dot(X1, X2) = <X1, X2>_F (LDLt.jl:91-108): Gram products and the two small congruences on the device; both operands on the same pencil */
int dre_ldlt_dot(dre_ctx* ctx, const dre_ldlt* a, const dre_ldlt* b, double* out);
/* alpha, L, D = X  (LDLt.jl:54-60; compresses when more than one component); pass NULL buffers to query sizes */
int dre_ldlt_destructure(dre_ctx* ctx, dre_ldlt* x, double* alpha, double* L_host, int ldl, double* D_host, int ldd);

/* ---- GALE / ADI (src/lyapunov/types.jl:10-32, adi.jl:29-225) --------------------------------- */
/* Pluggable inner solver (src/blocklinear/types.jl:15-62; src/lyapunov/types.jl:26 `inner_alg`; example test/cuda.jl:23-30,74):
 * a user-supplied solver of the SPARSE shifted system
 *      (cA*A' + (cE_re + i*cE_im)*E') X = B,        B real n x nrhs, column-major, leading dimension n,
 * i.e. the ALG of inner_alg = ShermanMorrisonWoodbury(ALG, Backslash): the engine keeps doing the rank-m Sherman-Morrison-Woodbury
 * correction for F = Fs + inv(alpha) U V around it.  All pointers are DEVICE pointers in the caller's row ordering; X_im is NULL for a
 * real system.  The engine synchronises its stream before the call; the callback must have completed its own device work when it
 * returns.  Return 0 on success (anything else aborts the solve with DRE_ERR_INTERNAL).  With a user solver the engine neither caches
 * factorisations nor takes the dense-inverse fast paths. */
typedef int (*dre_block_solver_fn)(void* user, int n, int nrhs, double cA, double cE_re, double cE_im, const double* B, double* X_re, double* X_im);

/* User-defined shift strategy: the reference's extension point  Shifts.init(strategy, prob) / Shifts.update!(shifts, X, R, Vs...) /
 * Shifts.take!(shifts)  (src/Shifts.jl:79-116; a strategy that produces batches implements take_many! behind a BufferedIterator,
 * src/shifts/helpers.jl:60-89; example: the Dummy strategy of test/Shifts.jl:133-163).  With shift_kind = 3 the engine calls shift_fn whenever
 * its buffer of shifts is empty:
 *     restart   1 on the first call of a Lyapunov solve (= init), 0 afterwards
 *     hist      DEVICE pointer, n x hist_cols column-major (leading dimension ldh), rows in the CALLER's ordering: what update! has handed over — the residual factor R at the
 *               start of a solve, afterwards the last n_history increments V (a conjugate pair contributes its two real blocks), oldest first
 *     capacity  room in re / im (HOST arrays); write *count >= 1 shifts, in the order in which they are to be used
 * Every shift must have a negative real part; a complex shift mu is followed by conj(mu) — the pair is handled by ONE double step and the
 * second take! is checked against the first (adi.jl:181-225, :190).  The engine synchronises its stream before the call.  Return 0 on success (anything else aborts the solve with DRE_ERR_INTERNAL). */
typedef int (*dre_shift_fn)(void* user, int restart, int n, int hist_cols, const double* hist, int ldh, int capacity, double* re, double* im, int* count);

typedef struct dre_adi_options {
    int32_t maxiters;              /* 100 */
    double reltol;                 /* < 0 = nothing -> n*eps */
    double abstol;                 /* < 0 = nothing -> reltol*norm(C) */
    int32_t ignore_initial_guess;  /* 0 */
    int32_t compression_interval;  /* 10 */
    int32_t compression;           /* 1 */
    int32_t shift_kind;            /* 0 = Cyclic(values), 1 = Projection(n_history), 2 = Cyclic(Heuristic(nshifts, kplus, kminus)) recomputed
                                      on the device from (E, F) at the start of every Lyapunov solve (adi.jl:54, heuristic.jl:39-66),
                                      3 = user-defined strategy: shift_fn below (n_history = number of increments it is shown) */
    int32_t n_history;             /* 2 */
    int32_t nshifts;               /* Cyclic: number of values (conjugate pairs adjacent); Heuristic: number of shifts to select */
    const double* shifts_re;
    const double* shifts_im;       /* may be NULL (all real) */
    double compress_tolfac;        /* <= 0 -> 4: the engine's compressions drop what lies below tolfac*eps*||S||_F */
    int32_t compress_exact;        /* 1: eigen-decomposition + 100*eps*max|lambda| threshold at every compression (reference arithmetic);
                                      0 (default): Krylov-truncated compression, D stays tridiagonal inside the engine */
    int32_t heuristic_kplus;       /* shift_kind 2: Arnoldi steps with E^-1 F */
    int32_t heuristic_kminus;      /* shift_kind 2: Arnoldi steps with F^-1 E */
    dre_block_solver_fn inner_solve; /* NULL (default): inner_alg = Backslash() on the library's multifrontal LU (src/blocklinear/backslash.jl) */
    void* inner_user;              /* passed back to inner_solve */
    dre_shift_fn shift_fn;         /* shift_kind 3 only */
    void* shift_user;              /* passed back to shift_fn */
} dre_adi_options;
int dre_adi_default_options(dre_adi_options* opt);

/* solve(GALEProblem(E, F, C), ADI(...); initial_guess) with F = cA*A + cE*E + inv(lr_alpha)*U*V
 * (LowRankUpdate, src/LowRankUpdate.jl:18-39).  U is n x m, Vt = V' is n x m; both NULL for a plain sparse F. */
int dre_gale_solve(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U,
                   const dre_dense* Vt, dre_ldlt* C, const dre_ldlt* X0, const dre_adi_options* opt, dre_adi_result** out);
/* The same solve as the reference's stepwise protocol on the solver object (ADICache, src/lyapunov/adi.jl:5-21):
 *   dre_adi_init   = CommonSolve.init(::GALEProblem, ::ADI; initial_guess)   adi.jl:29-69   (residual, tolerances, shift oracle)
 *   dre_adi_step   = step!(cache)          adi.jl:97-128  — ONE shift, or one conjugate pair (counts two, adi.jl:181-225), then the
 *                                                           residual norm and the convergence test (adi.jl:115-123)
 *   dre_adi_isdone = isdone(cache)         adi.jl:130-141
 *   dre_adi_solve  = solve!(cache)         adi.jl:71-76   — steps until done (whole chunks are enqueued speculatively)
 *   dre_adi_finish = the tail of solve!    adi.jl:78-89   — final compression, observe_gale_done! payload; call once
 * Stepping to the end and solving in one go run the same kernels in the same order: the results are identical bit for bit
 * (test/tiny_random.jl:48-57).  dre_gale_solve = init + solve + finish. */
typedef struct dre_adi_solver dre_adi_solver;
int dre_adi_init(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                 dre_ldlt* C, const dre_ldlt* X0, const dre_adi_options* opt, dre_adi_solver** out);
int dre_adi_step(dre_ctx* ctx, dre_adi_solver* s);
int dre_adi_solve(dre_ctx* ctx, dre_adi_solver* s);
int dre_adi_isdone(const dre_adi_solver* s, int* done);
int dre_adi_state(const dre_adi_solver* s, int64_t* iters, double* res_norm, double* abstol);     /* shifts consumed, last residual norm, abstol */
/* observe_gale_step!(observer, i, X, residual, residual_norm) (src/lyapunov/adi.jl:119, src/Callbacks.jl:97-107): the iterate X and the
 * residual object of the solver's CURRENT iteration as LDLᵀ handles (either pointer may be NULL).  X shares its factors with the solver
 * (lazy list of increments, LDLt.jl:131-148); the residual factor is a copy (the iteration updates it in place, adi.jl:171). */
int dre_adi_snapshot(dre_ctx* ctx, dre_adi_solver* s, dre_ldlt** X, dre_ldlt** residual);
/* observe_gale_metadata!(observer, "ADI shifts", mu) (adi.jl:103,192) while stepping: the shifts of the accepted iterations from `from`
 * (0-based) on; re/im may be NULL to ask for the count only (they must hold *count doubles otherwise). */
int dre_adi_shifts(const dre_adi_solver* s, int64_t from, int64_t* count, double* re, double* im);
int dre_adi_finish(dre_ctx* ctx, dre_adi_solver* s, dre_adi_result** out);
int dre_adi_free(dre_adi_solver* s);
/* Penzl's heuristic, device part (src/shifts/heuristic.jl:39-66,103-130): Ritz values of E^-1 F (kplus Arnoldi steps) and of F^-1 E
 * (kminus steps), both from ones(n), for F = cA*A + cE*E + inv(lr_alpha)*U*V (products and solves see the low-rank part, the solves
 * through Sherman-Morrison-Woodbury like heuristic.jl:51-60).  Outputs: kplus + kminus complex numbers, raw (unsorted, unstabilised);
 * the selection `heuristic(R, nshifts)` (heuristic.jl:22-37,82-101) is host logic of the shim. */
int dre_heuristic_ritz(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                       int kplus, int kminus, double* plus_re, double* plus_im, double* minus_re, double* minus_im);
/* residual(GALEProblem, X)  (src/lyapunov/residual.jl:3-31) */
int dre_gale_residual(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U,
                      const dre_dense* Vt, dre_ldlt* C, dre_ldlt* X, dre_ldlt** out);
/* LyapunovOperator(E, F) * X = F'XE + E'XF as an LDL' object with factor [E'L, F'L] (src/lyapunov/gmres.jl:108-120); F as in dre_gale_solve */
/* residual(::GAREProblem, ::LDLt) = gamma C'SC + A'XE + E'XA - beta^2 E'XB Rinv B'XE as one LDL' object [C', A'L, E'L] T [...]'
 * (src/riccati/residual.jl:5-52), and the feedback K' = E'XB (newton.jl:104-112), both formed from the device factors of X */
int dre_gare_residual(dre_ctx* ctx, const dre_pencil* p, dre_ldlt* X, const dre_dense* Ct, const dre_dense* S, double gamma, const dre_dense* B,
                      const dre_dense* Rinv, double beta, dre_ldlt** out);
int dre_ldlt_feedback(dre_ctx* ctx, const dre_pencil* p, dre_ldlt* X, const dre_dense* B, dre_dense** Kt);
int dre_gale_apply(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                   const dre_ldlt* X, dre_ldlt** out);
/* info: [0]=iters [1]=converged [2]=warnings [3]=number of recorded norms [4]=rhs columns;  dinfo: [0]=res_norm [1]=abstol [2]=initial norm */
int dre_adi_result_info(const dre_adi_result* r, int64_t* info, double* dinfo);
int dre_adi_result_history(const dre_adi_result* r, double* norms, int32_t* norm_iters, double* shifts_re, double* shifts_im);
int dre_adi_result_take_x(dre_adi_result* r, dre_ldlt** X);            /* observe_gale_done!(…, X, …) */
int dre_adi_result_take_residual(dre_adi_result* r, dre_ldlt** R);
int dre_adi_result_free(dre_adi_result* r);

/* ---- multi-GPU: RCCL over xGMI inside the library (SURVEY.md section 8b `dre_comm_init`, 8e) ----
 * One process per GPU, one context per process.  Rank 0 makes the 128-byte unique id (ncclGetUniqueId), the host program hands it to
 * the other ranks (torch.distributed / MPI / a file), every rank calls dre_comm_init(ctx, nranks, rank, id): the communicator belongs
 * to the context and its collectives are enqueued on the context's stream (no host synchronisation, no staging copies).
 * With a communicator of more than one rank attached, every solve entered through this ABI (dre_gdre_solve, dre_gale_solve,
 * dre_adi_*) runs the SAME device-resident loop on every rank with the shifted solves of the ADI iteration
 * (perform_single_step!, src/lyapunov/adi.jl:149-179; the multifrontal sweeps + SMW of src/blocklinear) sharded:
 *  - Cyclic real shifts (fan groups: g consecutive iterations from g INDEPENDENT solves with the same right-hand side): BY SHIFT — rank r
 *    solves the group positions s = r (mod P), so it only ever factorises the shifts it owns (src/blocklinear/backslash.jl:13 once per
 *    owned shift and run), and ONE in-place all-gather per GROUP of g iterations completes the panel [W_1 .. W_g] on every rank;
 *  - any other real-shift step: BY COLUMN — rank r solves its 16-column tiles of the residual block, one all-gather per ADI step;
 * residual update, norm, compression, shifts and the feedback K(t) are replicated and bit-identical on all ranks (the reference has
 * no multi-device path; test/cuda.jl runs one GPU).  librccl is loaded lazily by the first dre_comm_* call.
 * option "shard_min_cols" (default 32): narrower residual blocks are solved replicated; option "shard_emulate" = P: one process plays
 * P ranks one after the other (tests). */
int dre_comm_unique_id(dre_ctx* ctx, void* id128);
int dre_comm_init(dre_ctx* ctx, int nranks, int rank, const void* id128);      /* id128 may be NULL for nranks == 1 (no RCCL object) */
/* The same communicator over a HOST transport: the collectives are staged through pinned host memory and handed to the caller's callbacks
 * (MPI, gloo, ... — hosts without RCCL, and the two-rank tests of the sharded solve on ONE GPU: RCCL refuses two ranks on one device).
 * allgather(user, send, recv, bytes_per_rank): recv holds nranks blocks, send points at this rank's block inside recv (in place);
 * allreduce(user, buf, count): sum of `count` doubles in place.  Both return 0 on success; they are called from the thread that drives
 * the solve, between two stream synchronisations. */
typedef int (*dre_comm_allgather_fn)(void* user, const void* send, void* recv, size_t bytes_per_rank);
typedef int (*dre_comm_allreduce_fn)(void* user, void* buf, size_t count);
int dre_comm_init_host(dre_ctx* ctx, int nranks, int rank, dre_comm_allgather_fn allgather, dre_comm_allreduce_fn allreduce, void* user);
int dre_comm_free(dre_ctx* ctx);
/* info: [0]=nranks [1]=rank [2]=collective calls [3]=bytes received by all-gathers [4]=bytes reduced [5]=emulated ranks */
int dre_comm_info(dre_ctx* ctx, int64_t* info);
/* generic collectives on device buffers of doubles (the K(t) gather of independent replicas uses them: recv holds nranks blocks of count) */
int dre_comm_allgather(dre_ctx* ctx, const void* send_dev, void* recv_dev, size_t count);
int dre_comm_allreduce_sum(dre_ctx* ctx, void* buf_dev, size_t count);

/* ---- GDRE (src/riccati/lowrank_ros1.jl:3-66, lowrank_ros2.jl:3-89) ---------------------------- */
/* solve(GDREProblem(E, A, B, C, X0, (t0, tf)), Ros<order>(ADI(opt)); dt, save_state).  B is n x m, C is q x n. */
int dre_gdre_solve(dre_ctx* ctx, const dre_pencil* p, const dre_dense* B, const dre_dense* C, dre_ldlt* X0, double t0,
                   double tf, double dt, int order, int save_state, const dre_adi_options* opt, dre_gdre_result** out);
/* info: [0]=time points [1]=stored states [2]=total ADI iterations [3]=sparse factorisations [4]=Lyapunov solves [5]=m [6]=n */
int dre_gdre_result_info(const dre_gdre_result* r, int64_t* info);
int dre_gdre_result_times(const dre_gdre_result* r, double* t);
int dre_gdre_result_K(dre_ctx* ctx, const dre_gdre_result* r, int i, double* K_host /* m x n */, int ld);
/* whole trajectory K(t_0..t_end) as nt consecutive m x n column-major blocks written to DEVICE memory owned by the
 * caller (e.g. a torch tensor's data_ptr) so that it can be handed to RCCL without a host round trip */
int dre_gdre_result_K_device(dre_ctx* ctx, const dre_gdre_result* r, double* K_dev);
/* the same nt blocks written to HOST memory (nt * m * n doubles): one export launch and one copy instead of nt calls of dre_gdre_result_K
 * (sol.K of DRESolution, src/riccati/lowrank_ros1.jl:65) */
int dre_gdre_result_K_all(dre_ctx* ctx, const dre_gdre_result* r, double* K_host);
/* shares the factors (sol.X[1] === prob.X0).  A Ros1 run without save_state that ends on the dense-X path keeps its last X as a dense matrix
 * (context option final_x_lazy, default 1): the first call for that X runs the conversion to LDL' on the stream of the context the solve ran
 * on and caches the factors in the result; later calls return the same factors.  The result therefore refers to its context: free every
 * result (dre_gdre_result_free) before the context it was made on (dre_ctx_destroy).  On failure the message goes to that context. */
int dre_gdre_result_X(const dre_gdre_result* r, int i, dre_ldlt** X);
/* per Lyapunov solve j: iinfo [0]=iters [1]=converged [2]=warnings [3]=rhs columns; dinfo [0]=res_norm [1]=abstol */
int dre_gdre_result_gale(const dre_gdre_result* r, int j, int64_t* iinfo, double* dinfo);
/* per-iteration record of Lyapunov solve j for the observer replay (observe_gale_step! / observe_gale_metadata!, src/lyapunov/adi.jl:65,103,119,192):
 * counts [0]=number of recorded norms (index 0 = initial residual) [1]=shifts consumed; pass NULL arrays to query the counts */
int dre_gdre_result_gale_history(const dre_gdre_result* r, int j, int64_t* counts, double* norms, int32_t* norm_iters, double* shifts_re, double* shifts_im);
/* every Lyapunov solve of the result at once: iinfo 6 per solve ([0..3] as dre_gdre_result_gale, [4]=recorded norms, [5]=shifts consumed), dinfo 2 per
 * solve; the histories concatenated in solve order.  Call with NULL history arrays first to size them from iinfo. */
int dre_gdre_result_gales_all(const dre_gdre_result* r, int64_t* iinfo, double* dinfo, double* norms, int32_t* norm_iters, double* shifts_re,
                              double* shifts_im);
int dre_gdre_result_free(dre_gdre_result* r);

/* ---- dense path (GDREProblem{<:Matrix}: src/riccati/dense_ros{1,2,3,4}.jl, src/lyapunov/bartels-stewart.jl) ------------------------
 * Every dense operand is n x n (B n x m, C q x n), n <= 46340: the index limit of the device kernels (every int element index inside an
 * n x n operand stays below 2^31); below it the device memory decides.  The Gauss-Jordan inversions use the register pivoting panel for
 * n <= 4096 and the multi-workgroup tournament panel above (option "dense_gj_panel").  The Lyapunov solver is the generalized matrix-sign-function iteration
 * (Benner & Quintana-Orti 1999) on the device in place of the reference's Bartels-Stewart: it requires a c-stable pencil (F, E) and fails
 * with DRE_ERR_NOT_STABLE otherwise; a singular E or F is DRE_ERR_SINGULAR.  maxiters: sign iterations per pencil; tol <= 0 selects
 * 10 n eps (stop when ||Z + E||_F <= tol ||E||_F); max_refine: refinement steps by replay while the relative residual exceeds 100 n eps.
 * Device memory of about (maxiters + 26) n^2 doubles (+ n^2 per saved state) is checked up front (DRE_ERR_ALLOC). */
/* solve(GALEProblem(E, F, R), MatrixSign()):  F'XE + E'XF = -R   (bartels-stewart.jl:3-12, lyapc replaced)
   iinfo: [0] sign iterations [1] refinement steps;  dinfo: [0] relative residual before refinement [1] after */
int dre_dense_gale_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* F, const dre_dense* R, int maxiters, double tol, int max_refine,
                         dre_dense** X, int64_t* iinfo, double* dinfo);
/* solve(GDREProblem{<:Matrix}, Ros<order>(MatrixSign()); dt, save_state), order 1..4 (dense_ros{1,2,3,4}.jl).  The result is a
 * dre_gdre_result: _info ([2], [3] = 0; [4] = Lyapunov solves), _times, _K, _K_all, _K_device and _free work as for the low-rank path;
 * dre_gdre_result_X and the _gale* accessors return DRE_ERR_INVALID on it. */
int dre_dense_gdre_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X0,
                         double t0, double tf, double dt, int order, int save_state, int maxiters, double tol, int max_refine,
                         dre_gdre_result** out);
/* solve(GDREProblem{<:Matrix}, Ros2(MatrixSign()); dt = dt0, adaptive = StepControl(...)) (dre_version >= 107): Ros2 with step-size control by
 * its embedded first-order solution.  One trial step of size tau from (t, X): Xnew as a Ros2 step of dre_dense_gdre_solve, D = Xnew - (X + tau K1),
 * err = sqrt(mean_ij (D_ij / (atol + rtol max(|X_ij|, |Xnew_ij|)))^2); accepted iff err <= 1; the next size is tau * clamp(0.9 err^(-1/2), 0.2, 5)
 * (5 when err == 0; 0.2 and a rejection when err is not finite; at most 1 on the trial right after a rejection), clamped to [dt_min, dt_max].
 * tf and the ntstops values of tstops (strictly between t0 and tf, strictly monotone in the direction of integration) are hit exactly: with d the
 * distance to the next of them, a step is d when d <= 1.1 |h| and d/2 when d < 2 |h|.  dt0: the first step, of the sign of tf - t0.  The
 * step tau is |h| in either direction of integration.
 * The result is an ordinary dense dre_gdre_result over the ACCEPTED steps (_info, _times, _K, _K_all, _K_device, _X_dense, _dense_stats, _free;
 * info[4] and _dense_stats count the Lyapunov solves of every trial, two per trial); dre_gdre_result_step_stats adds the counts and errors.
 * Errors: DRE_ERR_INVALID for order != 2, rtol <= 0, atol <= 0, dt0 zero or of the wrong sign, dt_min < 0 or dt_min > dt_max, max_steps < 1,
 * tstops outside the open span or not monotone; DRE_ERR_STEP for a rejection at a step <= dt_min or more than max_steps trial steps (rejected
 * ones included); DRE_ERR_NOT_STABLE / DRE_ERR_SINGULAR of a factorisation are passed up, not turned into rejections; DRE_ERR_ALLOC when the
 * fixed part, (maxiters + 28) n^2 doubles, does not fit (checked before any kernel) or when the result, which grows in chunks of 64 K(t) and
 * of 8 saved states, cannot grow (the message names the step).  The context stays usable after every one of them. */
int dre_dense_gdre_solve_adaptive(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X0,
                                  double t0, double tf, double dt0, int order, double rtol, double atol, double dt_min, double dt_max, int64_t max_steps,
                                  const double* tstops, int ntstops, int save_state, int maxiters, double tol, int max_refine, dre_gdre_result** out);
/* of an adaptive result (DRE_ERR_INVALID on any other): accepted_rejected[0], [1] trial steps accepted / rejected; err[i] the error measure of
   accepted step i (accepted_rejected[0] = info[0] - 1 values); either array may be NULL */
int dre_gdre_result_step_stats(const dre_gdre_result* r, int64_t* accepted_rejected /* 2 */, double* err /* per accepted step */);
/* A <- inv(A) in place with the configured pivoting panel (n x n, n <= 46340); piv (n entries, or NULL): the row interchanges, LAPACK
 * style with 0-based indices (row j was swapped with row piv[j] >= j); logabsdet (or NULL): log |det A|.  A singular A (an exactly zero or
 * non-finite pivot) is DRE_ERR_SINGULAR and leaves A undefined. */
int dre_dense_invert(dre_ctx* ctx, dre_dense* A, int32_t* piv, double* logabsdet);
/* solve(GAREProblem(E, A, G, Q), MatrixSign(maxiters, tol, max_refine)): the dense stabilizing solution X of
 *     Q + A'XE + E'XA - E'XGXE = 0,   G = B Rinv B',  Q = Ct S Ct'
 * (riccati/types.jl:41-52, riccati/newton.jl:3-147 for dense data; the reference has no dense GARE solver).  Rinv (m x m) and S (q x q) may be
 * NULL: identity; the scalars of the LDL' objects are folded into them by the caller.  E, A n x n with 2n <= 46340 (the Hamiltonian is 2n x 2n).
 * Generalized sign iteration of the Hamiltonian pencil (H, diag(E, E')) with determinantal scaling and Byers' structure averaging; tol <= 0
 * selects 10 (2n) eps (stop when ||Z_{k+1} - Z_k||_F <= tol ||Z_{k+1}||_F); X from a Householder QR of [Z12; Z22 + E'] and then up to
 * max_refine Newton-Kleinman steps (each a MatrixSign GALE solve on the closed loop (A - GXE, E)) while the scaled residual
 * ||R(X)||_F / (||Q||_F + 2 ||A'XE||_F + ||E'XGXE||_F) exceeds 100 n eps and decreases.
 * Errors: DRE_ERR_NOT_STABLE when the sign iteration stagnates, produces non-finite values or does not converge in maxiters (Hamiltonian
 * eigenvalues on or near the imaginary axis: (A, B, E) not stabilizable or (A, C, E) not detectable), and when a refinement step finds the
 * closed loop not c-stable; DRE_ERR_SINGULAR for a singular E, a singular Z_k or a rank-deficient [Z12; Z22 + E'].  Device memory of about
 * 24 n^2 doubles, plus (maxiters + 12) n^2 when max_refine > 0, is checked up front (DRE_ERR_ALLOC, before any kernel runs).
 * iinfo: [0] sign iterations [1] refinement steps;  dinfo: [0] scaled residual after extraction [1] final */
int dre_dense_gare_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                         const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo);
/* Both Riccati solutions of LQG design from ONE Hamiltonian sign iteration (dre_version >= 113): *X as dre_dense_gare_solve returns it for the
 * same arguments, bit for bit, and *Y, the stabilizing solution of the filter equation
 *     G + A Y E' + E Y A' - E Y Q Y E' = 0.
 * The filter's Hamiltonian pencil is the transpose (H', K') of the regulator's, and the sign iteration commutes with transposition, so Y is
 * extracted from the transposed blocks of the same Z_inf: [Z21'; Z22' + E] Yr = -[Z11' + E'; Z12'], Y = sym(Yr E^-T).  Its Newton-Kleinman steps
 * run on the dual closed loop (A - E Y Q, E) with the dual replay of the refinement's sign solver, while the scaled residual
 * ||R_f(Y)||_F / (||G||_F + 2 ||A Y E'||_F + ||E Y Q Y E'||_F) exceeds 100 n eps and decreases.
 * Arguments, limits and errors are those of dre_dense_gare_solve, checked before any kernel runs; a failure of the shared iteration fails the
 * call, one that concerns a single solution (a rank-deficient extraction operand: DRE_ERR_SINGULAR; a refinement whose closed loop is not
 * c-stable: DRE_ERR_NOT_STABLE) names it in the message ("regulator", "filter").  Device memory of about 25 n^2 doubles (the single call's
 * 24 n^2 and Y; the dual extraction works in the iteration's own buffers), plus (maxiters + 12) n^2 when max_refine > 0, is checked up front.
 * iinfo (4): [0] sign iterations [1] refinement steps of X, [2] sign iterations (the same count: there is one iteration) [3] refinement steps of Y;
 * dinfo (4): [0] [1] scaled residual of X after extraction and final, [2] [3] the same for Y */
int dre_dense_gare_solve_pair(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                              const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, dre_dense** Y, int64_t* iinfo /* 4 */,
                              double* dinfo /* 4 */);
/* residual(::GAREProblem, X) for a dense X (riccati/residual.jl:54-66): Res = Q + A'XE + E'XA - E'XGXE (symmetrised) as a new n x n matrix,
 * *norm = ||Res||_F.  G, Q as for dre_dense_gare_solve. */
int dre_dense_gare_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                            const dre_dense* S, const dre_dense* X, dre_dense** Res, double* norm);
/* Discrete-time dense solvers by doubling (dre_version >= 118; csrc/dense_doubling.hip).
 * Generalized Stein equation  A'XA - E'XE = -Q  (dual != 0:  A X A' - E X E' = -Q)  by the squared Smith iteration on M = E^-1 A:
 * H_{k+1} = H_k + sym(M_k' H_k M_k), M_{k+1} = M_k^2, H_0 = sym(Q), X = sym(E^-T H E^-1); one Gauss-Jordan inversion (of E) in the whole call.
 * E, A, Q n x n, n <= 46340; *X a new n x n matrix, symmetric bit for bit.  The iteration ends when the relative step ||dH||_F / ||H||_F is at
 * most tol (tol <= 0: 10 n eps) AND ||M_k||_F < 1.  Errors: DRE_ERR_NOT_STABLE when it produces non-finite values or does not converge in
 * maxiters (E^-1 A has eigenvalues on or outside the unit circle); DRE_ERR_SINGULAR for a singular E; DRE_ERR_ALLOC from the up-front check of
 * 7 n^2 doubles; DRE_ERR_INVALID for shapes and maxiters outside 1 .. 1000, before any kernel.
 * iinfo: [0] doubling iterations [1] 0;  dinfo: [0] [1] the last relative step */
int dre_dense_stein_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* Q, int dual, int maxiters, double tol, dre_dense** X,
                          int64_t* iinfo, double* dinfo);
/* Res = sym(Q + A'XA - E'XE) (dual != 0: Q + A X A' - E X E') as a new n x n matrix; *norm = ||Res||_F, *scaled = ||Res||_F / (||Q||_F + ||A'XA||_F +
 * ||E'XE||_F); either may be NULL */
int dre_dense_stein_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* Q, const dre_dense* X, int dual, dre_dense** Res,
                             double* norm, double* scaled);
/* Generalized discrete-time algebraic Riccati equation
 *     Q + A'X (I + G X)^-1 A - E'XE = 0      (= A'XA - E'XE - A'XB (R + B'XB)^-1 B'XA + Q),      G = B Rinv B', Q = Ct S Ct',
 * by the structure-preserving doubling algorithm on (E^-1 A, E^-1 G E^-T, Q): per iteration one Gauss-Jordan inversion of order n (of
 * I + G_k H_k) with one Newton-Schulz correction, nine products and one fused update; X = sym(E^-T H_inf E^-1).  Arguments and the NULL-means-identity convention of Rinv and S
 * as for dre_dense_gare_solve; any n <= 46340.  Then up to max_refine Newton (Hewer) steps  A_c' D A_c - E'DE = -R(X), X <- X + D  on the
 * closed loop A_c = (I + G X)^-1 A with the Stein solver above, while the scaled residual
 * ||R(X)||_F / (||Q||_F + ||A'X (I + G X)^-1 A||_F + ||E'XE||_F) exceeds 100 n eps and decreases.
 * Errors: DRE_ERR_NOT_STABLE when the doubling produces non-finite values or does not converge in maxiters (symplectic pencil with
 * eigenvalues on or near the unit circle: (A, B, E) not d-stabilizable or (A, C, E) not d-detectable) and when a refinement's closed loop is
 * not d-stable; DRE_ERR_SINGULAR for a singular E, I + G_k H_k or I + G X.  Device memory of 17 n^2 doubles is checked up front (DRE_ERR_ALLOC).
 * iinfo: [0] doubling iterations [1] refinement steps;  dinfo: [0] scaled residual after the doubling [1] final */
int dre_dense_dare_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                         const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo);
/* Both solutions from ONE doubling: *X as dre_dense_dare_solve returns it for the same arguments, bit for bit, and *Y = G_inf, the
 * stabilizing solution of the filter equation  G + A Y (I + Q Y)^-1 A' - E Y E' = 0  (no back-transformation), refined by the dual Stein
 * solve on A (I + Y Q)^-1.  Arguments, limits and errors of dre_dense_dare_solve (18 n^2 doubles); a failure that concerns one solution names
 * it ("regulator", "filter").  iinfo (4) and dinfo (4) as for dre_dense_gare_solve_pair. */
int dre_dense_dare_solve_pair(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                              const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, dre_dense** Y, int64_t* iinfo /* 4 */,
                              double* dinfo /* 4 */);
/* Res = sym(Q + A'X (I + G X)^-1 A - E'XE) as a new n x n matrix; *norm = ||Res||_F, *scaled the scaled norm above; either may be NULL.
 * DRE_ERR_SINGULAR for a singular I + G X. */
int dre_dense_dare_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                            const dre_dense* S, const dre_dense* X, dre_dense** Res, double* norm, double* scaled);
/* Dense generalized Sylvester solver by the coupled sign iteration (dre_version >= 119; csrc/dense_sylvester.hip).
 *     A X F + E X B = -C      (transposed != 0:  A'X F' + E'X B' = -C),      A, E n x n;  B, F m x m;  C, X n x m;  n, m <= 46340.
 * E or F NULL means the identity.  Both pencils (A, E) and (B, F) must be c-stable.  Per iteration: L_k = E A_k^-1, R_k = B_k^-1 F (two
 * Gauss-Jordan inversions), A_{k+1} = A_k/(2c) + (c/2) L_k E, B_{k+1} = B_k/(2c) + (c/2) F R_k, C_{k+1} = C_k/(2c) + (c/2) L_k C_k R_k with ONE
 * scaling factor c_k = exp((log|det A_k| + log|det B_k| - log|det E| - log|det F|) / (n + m)) for both sides (c = 1 once both distances are
 * below 1e-2); X = E^-1 C_inf F^-1 / 2.  The iteration ends when ||A_k + E||_F / ||E||_F and ||B_k + F||_F / ||F||_F are both at most tol
 * (tol <= 0: 10 max(n, m) eps).  Then up to max_refine refinement steps replay the residual through the kept sequence while the relative
 * residual ||C + A X F + E X B||_F / ||C||_F exceeds 100 max(n, m) eps.  C = 0 returns X = 0 exactly.
 * Errors: DRE_ERR_NOT_STABLE when a side stagnates away from -E resp. -F, produces non-finite values or does not converge in maxiters (the
 * message names the pencil: "left pencil (A, E)" or "right pencil (B, F)"); DRE_ERR_SINGULAR for a singular E, F, A_k or B_k (named);
 * DRE_ERR_INVALID, before any kernel, for shapes and maxiters outside 1 .. 1000, and for a C with non-finite entries; DRE_ERR_ALLOC from the
 * up-front check of (maxiters + 5)(n^2 + m^2) + 8 n m doubles.
 * iinfo: [0] sign iterations [1] refinement steps;  dinfo: [0] relative residual before the refinement [1] final [2] C's last relative step */
int dre_dense_sylvester_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, const dre_dense* C,
                              int transposed, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo /* 2 */, double* dinfo /* 3 */);
/* Res = C + A X F + E X B (transposed != 0: C + A'X F' + E'X B') as a new n x m matrix; *norm = ||Res||_F, *scaled = ||Res||_F / (||C||_F +
 * ||A X F||_F + ||E X B||_F); either may be NULL.  E or F NULL: the identity. */
int dre_dense_sylvester_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, const dre_dense* C,
                                 const dre_dense* X, int transposed, dre_dense** Res, double* norm, double* scaled);
/* A kept coupled sign iteration of the two pencils (the Sylvester twin of dre_sign_create): every right-hand side, in either direction, costs
 * only the recursion of C.  E, F NULL: the identity; the handle keeps its own copies.  Errors as dre_dense_sylvester_solve; device memory of
 * (maxiters + 5)(n^2 + m^2) + 7 n m doubles is checked before any kernel. */
typedef struct dre_sylvester dre_sylvester;
int dre_sylvester_create(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, int maxiters, double tol,
                         dre_sylvester** out);
/* A X F + E X B = -C (transposed != 0: A'X F' + E'X B' = -C) for an n x m C on the kept sequence, refined as in dre_dense_sylvester_solve; the
 * untransposed *X is bit for bit what dre_dense_sylvester_solve returns for the same operands.  iinfo, dinfo as there; the kept state is not
 * changed. */
int dre_sylvester_solve(dre_ctx* ctx, dre_sylvester* s, const dre_dense* C, int transposed, int max_refine, dre_dense** X, int64_t* iinfo /* 2 */,
                        double* dinfo /* 3 */);
/* *n_iters: sign iterations of the kept sequence */
int dre_sylvester_iters(const dre_sylvester* s, int64_t* n_iters);
int dre_sylvester_destroy(dre_ctx* ctx, dre_sylvester* s);
/* stored state i of a dense result as a new n x n matrix (sol.X[i]; index 0 is X0) */
int dre_gdre_result_X_dense(dre_ctx* ctx, const dre_gdre_result* r, int i, dre_dense** X);
/* per Lyapunov solve j (info[4] of them): iters[j] sign iterations, refinements[j], residuals[2j], residuals[2j+1] relative residual before /
   after refinement; any array may be NULL */
int dre_gdre_result_dense_stats(const dre_gdre_result* r, int64_t* iters, int64_t* refinements, double* residuals /* 2 per solve */);

/* ---- batched dense path: `batch` independent problems of one order n <= 4096 (the register panel) side by side on the device ---------
 * Members come as ordinary dre_dense handles (arrays of `batch` pointers); the library packs them into strided stacks and unpacks the
 * results.  Every launch carries member b on a grid axis, with per-member control words: a member's result is a function of that member's
 * data only, bit for bit the same whatever the other members are, however many there are and wherever it sits in the batch (no atomics, no
 * split-K, per-member grids independent of `batch`).  The return value is DRE_OK whenever the batch was processed; per-member outcomes are in
 * status[b]: 0, DRE_ERR_SINGULAR or DRE_ERR_NOT_STABLE, dre_last_error names the first failed member and dre_batch_member_error(ctx, b)
 * gives the message of member b of the context's last batched call.  A failed member is dropped from the following launches; the others go
 * on.  Argument errors are the call's own DRE_ERR_INVALID (batch < 1, mismatched shapes, n > 4096, order 3 or 4); DRE_ERR_ALLOC comes from
 * the up-front memory check (batch times the single call's count plus the stacks), before any kernel runs. */
/* A[b] <- inv(A[b]) in place; piv: batch * n interchanges (or NULL), logabsdet: batch values (or NULL); a singular member: DRE_ERR_SINGULAR
 * in status[b], its A[b] is left as it came */
int dre_dense_invert_batched(dre_ctx* ctx, int batch, dre_dense* const* A, int32_t* piv /* batch*n */, double* logabsdet /* batch */,
                             int32_t* status /* batch */);
/* dre_dense_gale_solve per member: X[b] is a new n x n matrix (NULL for a failed member); iinfo, dinfo as there, 2 per member */
int dre_dense_gale_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* F, const dre_dense* const* R,
                                 int maxiters, double tol, int max_refine, dre_dense** X /* batch */, int64_t* iinfo /* 2*batch */,
                                 double* dinfo /* 2*batch */, int32_t* status /* batch */);
/* dre_dense_gdre_solve per member, order 1 or 2 (Ros1, Ros2; orders 3 and 4 are DRE_ERR_INVALID here: they run through the single call).
 * The members share n, m, q, the time grid, order, save_state and the sign parameters and differ in E, A, B, C and X0.  out[b] is an
 * ordinary dense dre_gdre_result (all its accessors work unchanged); for a member that failed at step i it holds the steps completed before. */
int dre_dense_gdre_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                                 const dre_dense* const* C, const dre_dense* const* X0, double t0, double tf, double dt, int order,
                                 int save_state, int maxiters, double tol, int max_refine, dre_gdre_result** out /* batch */,
                                 int32_t* status /* batch */);
/* dre_dense_gare_solve per member (dre_version >= 106): the members share n, m, q (2n <= 4096: the Hamiltonian of order 2n goes through the
 * register panel) and the sign parameters and differ in E, A, B, Ct and the inner matrices.  Rinv and S: the array may be NULL (identity for
 * every member) and so may single entries (identity for that member).  X[b] is a new n x n matrix, NULL for a failed member;
 * iters_refinements[2b], [2b+1] and res0_res[2b], [2b+1] as iinfo and dinfo of dre_dense_gare_solve.  status[b]: 0, DRE_ERR_SINGULAR (singular
 * E_b, singular Z_k, rank-deficient extraction) or DRE_ERR_NOT_STABLE (stagnation, non-finite values, maxiters exhausted, a refinement whose
 * closed loop is not c-stable).  The return value is the first failed member's code (DRE_OK when none failed); every surviving member's X
 * is delivered all the same, and dre_last_error / dre_batch_member_error work as above.  DRE_ERR_INVALID: batch < 1, mismatched shapes,
 * 2n > 4096, maxiters outside 1 .. 1000, max_refine < 0.  DRE_ERR_ALLOC: batch * ((26 + (max_refine > 0 ? maxiters + 12 : 0)) n^2 +
 * n (m + q) + m^2 + q^2 + the panel's work stacks) doubles do not fit; checked before any kernel, nothing is allocated. */
int dre_dense_gare_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                                 const dre_dense* const* Rinv /* array or entries may be NULL */, const dre_dense* const* Ct,
                                 const dre_dense* const* S /* likewise */, int maxiters, double tol, int max_refine,
                                 dre_dense** X /* batch, NULL for a failed member */, int64_t* iters_refinements /* 2*batch */,
                                 double* res0_res /* 2*batch */, int32_t* status /* batch */);
/* message of member b of the context's last batched call ("" when it did not fail or b is out of range) */
const char* dre_batch_member_error(dre_ctx* ctx, int b);

/* ---- factored sign-function Lyapunov solver (dense pencil, LDL' right-hand side in, LDL' solution out; no ADI shifts) -----------------
 * A kept sign factorisation of one pencil (F, E): several right-hand sides share it (the two stages of Ros2, lowrank_ros2.jl:41-69).
 * Plain dre_dense operands in the caller's row order; no dre_pencil, no dre_ldlt. */
typedef struct dre_sign dre_sign;
/* runs the generalized sign iteration on (F, E) and keeps its (P_k, c_k) sequence; replaces the shift selection + factorisations of an ADI
 * solve (lyapunov/adi.jl:37-72).  maxiters, tol as for dre_dense_gale_solve.  Errors: DRE_ERR_NOT_STABLE (pencil not c-stable), DRE_ERR_SINGULAR,
 * DRE_ERR_ALLOC when (maxiters + 7) n^2 doubles do not fit (checked before any kernel). */
int dre_sign_create(dre_ctx* ctx, const dre_dense* E, const dre_dense* F, int maxiters, double tol, dre_sign** out);
/* *n_iters: sign iterations the factorisation took */
int dre_sign_info(const dre_sign* s, int64_t* n_iters);
/* solve(GALEProblem(E, F, C::LDLt), FactoredSign()):  F'XE + E'XF = -G S G'  with G n x r, S r x r symmetric (indefinite allowed);
 * X = L D L' with *L n x rank and *D rank x rank diagonal (replaces solve(::GALEProblem{LDLt}, ::ADI), lyapunov/adi.jl:3-147).  The kept
 * sequence is applied to the factor, L_{k+1} = [L_k, P_k'L_k], with a compression (QR, eigenvalues, |lambda| > rtol max|lambda| kept, the
 * rule of compress!, LDLt.jl:237-245) whenever the width exceeds max_width and once at the end; up to max_refine corrections by replaying the
 * compressed residual factor while the relative residual exceeds 100 n eps + 10 rtol.
 * rtol in (0, 1), max(r, 1) <= max_width <= 4096, max_refine >= 0: DRE_ERR_INVALID otherwise.  r = 0 returns rank 0.  Device memory of
 * 5 n (2 max_width) + 6 (2 max_width)^2 doubles is checked before any kernel (DRE_ERR_ALLOC).
 * ii: [0] rank [1] peak width [2] compressions [3] refinements;  dd: [0] relative residual before refinement [1] after.  Either may be NULL. */
int dre_sign_solve_lr(dre_ctx* ctx, dre_sign* s, const dre_dense* G, const dre_dense* S, double rtol, int max_width, int max_refine,
                      dre_dense** L, dre_dense** D, int64_t* ii, double* dd);
/* F'XE + E'XF = -R for a dense symmetric R on the kept factorisation (what dre_dense_gale_solve does after its own sign iteration);
 * iinfo / dinfo as there.  The three n x n work matrices of this replay are allocated by the first call. */
int dre_sign_solve_dense(dre_ctx* ctx, dre_sign* s, const dre_dense* R, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo);
/* The dual equation of the kept pencil (dre_version >= 109):  F Y E' + E Y F' = -R  (the controllability Gramian next to the observability
 * Gramian, the filter equation next to the regulator equation) from the SAME factorisation: no second dre_sign_create on (F', E').
 * Arguments, info arrays, refinement rule and errors as dre_sign_solve_dense; the kept state is not changed. */
int dre_sign_solve_dense_t(dre_ctx* ctx, dre_sign* s, const dre_dense* R, int max_refine, dre_dense** Y, int64_t* iinfo, double* dinfo);
/* The factored dual (dre_version >= 109):  F Y E' + E Y F' = -G S G',  Y = L D L', with L_0 = E^-1 G and L_{k+1} = [L_k, P_k L_k].  Arguments,
 * info arrays, cap, compression, refinement threshold and errors as dre_sign_solve_lr; the memory check adds n (r + 2 max_width) doubles
 * (the E^-1 G block and the residual's F L and E L blocks). */
int dre_sign_solve_lr_t(dre_ctx* ctx, dre_sign* s, const dre_dense* G, const dre_dense* S, double rtol, int max_width, int max_refine,
                        dre_dense** L, dre_dense** D, int64_t* ii, double* dd);
int dre_sign_free(dre_ctx* ctx, dre_sign* s);

/* ---- device SVD and balanced truncation (dre_version >= 110) ---------------------------------------------------------------------------
 * svd(A) by one-sided (Hestenes) cyclic block Jacobi on the device (column blocks of 16, round-robin ordering, one launch per round, the Gram
 * and update products on v_mfma_f64_16x16x4_f64): A (m x w, untouched) ~ U diag(S) V' with k = min(m, w), *U m x k, *S k x 1 descending and
 * non-negative, *V w x k.  Accuracy is norm-wise, like a LAPACK driver: errors of order eps sigma_1; there is NO claim of high relative
 * accuracy for tiny singular values (the Gram matrices are formed explicitly).  tol <= 0: sqrt(max(m, w)) eps; two columns count as orthogonal
 * when |g_r'g_c| <= tol ||g_r|| ||g_c||.  The columns of U (of V for a wide input, m < w) that belong to sigma <= tol ||A||_F are zero columns; their number
 * defines the numerical rank.  stats (may be NULL): [0] block sweeps, [1] rounds, [2] numerical rank.
 * DRE_ERR_INVALID for a non-finite A, min(m, w) > 4096 or max(m, w) > 46340 (before any launch); DRE_ERR_ALLOC from the memory check (before
 * any launch); DRE_ERR_INTERNAL after 60 sweeps. */
int dre_svd_jacobi(dre_ctx* ctx, const dre_dense* A, double tol, dre_dense** U, dre_dense** S, dre_dense** V, int64_t* stats /* 3, may be NULL */);
/* Square-root balanced truncation of  E x' = A x + B u,  y = C x  from its Gramians in the form dre_sign_solve_lr_t and dre_sign_solve_lr return
 * them:  P = Lc Dc Lc' from A P E' + E P A' = -B B'  and  Q = Lo Do Lo' from A'Q E + E'Q A = -C'C  (Dc, Do: a diagonal matrix or a vector; entries
 * that are not positive are left out with their columns).  With Z = L sqrt(D) and Zo'E Zc = U Sigma V' (dre_svd_jacobi):  *hsv the Hankel singular
 * values (min(r_o, r_c) x 1),  *W = Zo U_r Sigma_r^-1/2 and *T = Zc V_r Sigma_r^-1/2 (n x r, W'E T = I),  *Ar = W'A T, *Br = W'B, *Cr = C T.
 * order > 0: r = order (above the numerical rank of Zo'E Zc: DRE_ERR_INVALID); order = 0: the smallest r with 2 sum_{i > r} sigma_i <= tol sigma_1,
 * at most the numerical rank.
 * ii (6, may be NULL): [0] r [1] numerical rank [2] r_c [3] r_o [4] entries of Dc and Do left out [5] sweeps of the SVD;
 * dd (3, may be NULL): [0] ||W'E T - I||_F [1] the a-priori bound 2 sum_{i > r} sigma_i on max_w ||H(iw) - H_r(iw)||_2 [2] largest |d| left out.
 * Shape and argument errors are DRE_ERR_INVALID before any launch; the context stays usable after every error. */
int dre_balance_lr(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* Lc, const dre_dense* Dc,
                   const dre_dense* Lo, const dre_dense* Do, int order, double tol, dre_dense** hsv, dre_dense** T, dre_dense** W, dre_dense** Ar,
                   dre_dense** Br, dre_dense** Cr, int64_t* ii /* 6 */, double* dd /* 3 */);
/* LQG balanced truncation (dre_version >= 113) of  E x' = A x + B u,  y = C x,  which need not be c-stable: X and Y are the dense stabilizing
 * solutions of the regulator and the filter Riccati equations (dre_dense_gare_solve_pair).  Both are factored by the eigensolver of dre_sym_eig
 * (eigenvalues that are not positive are left out) and the steps of dre_balance_lr run with the factor of X in the place of the observability
 * Gramian's and the factor of Y in the place of the controllability Gramian's:  *mu the LQG characteristic values (the singular values of
 * Zo'E Zc, descending),  *T, *W (n x r, W'E T = I),  *Ar = W'A T, *Br = W'B, *Cr = C T, which satisfy both reduced Riccati equations with
 * diag(mu_1 .. mu_r), and the reduced-order LQG controller  x_c' = Ac x_c + Lr y,  u = -Kr x_c:  *Kr = Br' Sigma_r (m x r),
 * *Lr = Sigma_r Cr' (r x q),  *Ac = Ar - Br Kr - Lr Cr.
 * order > 0: r = order (above the numerical rank: DRE_ERR_INVALID); order = 0: the smallest r with 2 sum_{i > r} nu_i <= tol,
 * nu_i = mu_i / sqrt(1 + mu_i^2) (absolute: the normalised coprime factors have norm 1), at most the numerical rank.  n <= 8192, m, q >= 1.
 * ii (6, may be NULL): as dre_balance_lr;  dd (3, may be NULL): [0] ||W'E T - I||_F [1] the bound 2 sum_{i > r} nu_i on the error of the
 * normalised right coprime factors, max_w ||[N; M](iw) - [N_r; M_r](iw)||_2 [2] largest |eigenvalue| left out.
 * Shape and argument errors are DRE_ERR_INVALID before any launch; the context stays usable after every error. */
int dre_lqg_balance(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X, const dre_dense* Y,
                    int order, double tol, dre_dense** mu, dre_dense** T, dre_dense** W, dre_dense** Ar, dre_dense** Br, dre_dense** Cr, dre_dense** Kr,
                    dre_dense** Lr, dre_dense** Ac, int64_t* ii /* 6 */, double* dd /* 3 */);

/* ---- batched block Jacobi and ensemble balanced truncation (dre_version >= 111) -----------------------------------------------------------
 * The eigensolver of dre_sym_eig_jacobi, the SVD of dre_svd_jacobi and dre_balance_lr for `batch` members of one shape in shared launches
 * (member b on a grid axis, one control block per member).  Every output of a member is bit for bit what the single call returns for that
 * member alone, whatever the other members are; a member that is finished, non-finite or out of sweeps drops out of the following launches
 * and the others go on.  Conventions of the other *_batched entries: the return value is DRE_OK when the batch was processed; status[b] is 0
 * or the member's error code (DRE_ERR_INVALID for a non-finite member, DRE_ERR_INTERNAL without convergence), the outputs of a failed member
 * are NULL, dre_last_error names the first failed member and dre_batch_member_error(ctx, b) gives member b's message.  DRE_ERR_INVALID of the
 * call itself, before any launch: batch < 1 or > 65535, a NULL array or member, members of different shapes, a shape beyond the single call's
 * limits; DRE_ERR_ALLOC from the memory check, before any launch.
 * values[b] (q x 1, ascending), vectors[b] (q x q) in the output format of dre_sym_eig_jacobi; stats (2 * batch, may be NULL): [2b] block
 * sweeps, [2b + 1] rounds. */
int dre_sym_eig_jacobi_batched(dre_ctx* ctx, int batch, const dre_dense* const* S, double tol, dre_dense** values, dre_dense** vectors,
                               int64_t* stats /* 2 * batch */, int32_t* status);
/* U[b], S[b], V[b] as dre_svd_jacobi returns them (handles into stacks shared by the batch: the memory goes back when the last of them is
 * freed); stats (3 * batch, may be NULL): [3b] block sweeps, [3b + 1] rounds, [3b + 2] numerical rank. */
int dre_svd_jacobi_batched(dre_ctx* ctx, int batch, const dre_dense* const* A, double tol, dre_dense** U, dre_dense** S, dre_dense** V,
                           int64_t* stats /* 3 * batch */, int32_t* status);
/* dre_balance_lr for members that share (n, m, q); the Gramian factors' ranks may differ.  Every Zo'E Zc is written into a zero-filled stack
 * of the common shape (max_b r_o) x (max_b r_c) and one batched SVD diagonalises the stack.  Contract: a member's result is a bitwise function
 * of its own data and of that padded shape only (a batch of one member is bitwise dre_balance_lr).  An order above a member's numerical rank
 * is that member's DRE_ERR_INVALID in status[b], not the call's.  ii (6 * batch, may be NULL) and dd (3 * batch, may be NULL): per member the
 * entries of dre_balance_lr. */
int dre_balance_lr_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                           const dre_dense* const* C, const dre_dense* const* Lc, const dre_dense* const* Dc, const dre_dense* const* Lo,
                           const dre_dense* const* Do, int order, double tol, dre_dense** hsv, dre_dense** T, dre_dense** W, dre_dense** Ar,
                           dre_dense** Br, dre_dense** Cr, int64_t* ii /* 6 * batch */, double* dd /* 3 * batch */, int32_t* status);

/* ---- frequency response of dense descriptor systems, batched by frequency (dre_version >= 112) -------------------------------------------
 * H(i w_k) = C (i w_k E - A)^-1 B for K frequencies in shared launches, the frequency on the member axis of the batched dense path.  Per
 * member the real form [[-A, -w E], [w E, -A]] of i w E - A (order 2n) is assembled, inverted in place with the register panel (so
 * 2n <= 4096) and multiplied out, with one refinement step whose residual is formed from E and A (the real form is not kept): 16 n^3 flops
 * per frequency; the result is as accurate as a complex LU solve.  The n x n Schur form A + w^2 E A^-1 E would be 8 x cheaper, but it squares the condition number and needs a regular A.  E may be
 * singular (descriptor systems): nothing here inverts E.
 * H_re, H_im: q*m*K doubles each, member k at k*q*m, q x m column-major.  status[k]: 0, or DRE_ERR_SINGULAR for a frequency at which
 * i w E - A has an exactly zero or non-finite pivot (w on a pole, a NaN in the system): its H is NaN, the other frequencies go on.  The sweep
 * runs in chunks of `chunk` members (0: as many as fit the free device memory, at most 65535); a member's result is bit for bit the same
 * whatever the other members are and whatever chunk it falls in.  info (2, may be NULL): [0] members per chunk, [1] chunks.
 * Conventions of the other *_batched entries: DRE_OK when the sweep was processed, dre_last_error names the first failed member and
 * dre_batch_member_error(ctx, k) gives member k's message.  The call's own DRE_ERR_INVALID, before any launch: a NULL argument, K < 1, a
 * non-finite frequency, mismatched shapes, 2n > 4096, chunk < 0 or > 65535; DRE_ERR_ALLOC, before any launch: the chunk does not fit. */
int dre_freq_response(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int K, const double* omega,
                      int chunk, double* H_re /* q*m*K */, double* H_im /* q*m*K */, int32_t* status /* K */, int64_t* info /* 2, may be NULL */);
/* the same for nsys systems of one (n, m, q) at the same K frequencies: member s*K + k is system s at w_k */
int dre_freq_response_batched(dre_ctx* ctx, int nsys, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                              const dre_dense* const* C, int K, const double* omega, int chunk, double* H_re /* q*m*K*nsys */,
                              double* H_im /* q*m*K*nsys */, int32_t* status /* K*nsys */, int64_t* info /* 2, may be NULL */);

/* ---- complex inversion and the transfer function at complex points (dre_version >= 115) --------------------------------------------------
 * A complex matrix is two dre_dense planes of one shape, its real and its imaginary part.  The complex Gauss-Jordan inversion runs on the
 * register panel in both planes (n <= 4096), pivots by |re| + |im| and does its trailing update as one real product per panel:
 * 8 n^3 real flops, 2 n^2 doubles per member.
 * Are[b] + i Aim[b] <- its inverse, in place on both planes; piv: batch * n interchanges (or NULL); logabsdet: batch values log|det| (or
 * NULL; the phase of the determinant is not returned).  The conventions of dre_dense_invert_batched: a singular member (exactly zero or
 * non-finite pivot) gets DRE_ERR_SINGULAR in status[b] and its planes are left as they came; batch < 1, mismatched shapes and n > 4096 are the
 * call's DRE_ERR_INVALID before any launch. */
int dre_dense_invert_complex_batched(dre_ctx* ctx, int batch, dre_dense* const* Are, dre_dense* const* Aim, int32_t* piv /* batch*n */,
                                     double* logabsdet /* batch */, int32_t* status /* batch */);
/* H(s_k) = C (s_k E - A)^-1 B at K complex points s_k = s_re[k] + i s_im[k], the point on the member axis: per member the planes of s E - A
 * are assembled, inverted in place with the complex register panel (n <= 4096) and multiplied out, with one refinement step whose residual is
 * formed from E and A.  8 n^3 flops per point, half of dre_freq_response's, which it reproduces at s = i w to rounding.  Arguments, layouts
 * (H_re, H_im: q*m*K doubles, member k at k*q*m, q x m column-major), status, chunk, info and error rules are those of dre_freq_response, with
 * the two point arrays in place of omega: DRE_ERR_SINGULAR in status[k] for a point on a pole (or a NaN in the system), its H is NaN; the
 * call's own DRE_ERR_INVALID, before any launch: a NULL argument, K < 1, a non-finite s_re or s_im, mismatched shapes, n > 4096, chunk < 0
 * or > 65535; DRE_ERR_ALLOC, before any launch: the chunk does not fit. */
int dre_transfer_eval(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int K, const double* s_re,
                      const double* s_im, int chunk, double* H_re /* q*m*K */, double* H_im /* q*m*K */, int32_t* status /* K */,
                      int64_t* info /* 2, may be NULL */);
/* the same for nsys systems of one (n, m, q) at the same K points: member s*K + k is system s at s_k */
int dre_transfer_eval_batched(dre_ctx* ctx, int nsys, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                              const dre_dense* const* C, int K, const double* s_re, const double* s_im, int chunk, double* H_re /* q*m*K*nsys */,
                              double* H_im /* q*m*K*nsys */, int32_t* status /* K*nsys */, int64_t* info /* 2, may be NULL */);

/* ---- time response of dense descriptor systems: step, impulse, simulate (dre_version >= 117) ----------------------------------------------
 * E x' = A x + B u, y = C x on the uniform grid t_k = k dt, k = 0 .. K, by one of two one-step schemes x_{k+1} = M x_k + N w_k:
 *   method 0, tustin (order 2, A-stable):          P = E - (dt/2) A, M = 2 P^-1 E - I, N = (dt/2) P^-1 B, w_k = u_k + u_{k+1};
 *   method 1, backward Euler (order 1, L-stable):  P = E - dt A,     M = P^-1 E,       N = dt P^-1 B,     w_k = u_{k+1}.
 * kind 0, step response: y_k[:, c] for a unit step on input channel c from x_0 = 0, every channel;  kind 1, impulse response: the free
 * response y_k = C M^k E^-1 B from x(0+) = E^-1 B (E must be regular; no feedthrough term);  kind 2, simulate: the outputs for S input
 * signals ("scenarios") and initial states.  A feedthrough D u_k is the caller's to add.  The pencil need not be stable.  E may be singular
 * for kinds 0 and 2; under tustin the algebraic part then has the eigenvalue -1 in M, and backward Euler is the method to use.
 * The outputs are formed from the Markov sequence G_j = C M^j, which is built by doubling ([G_0 .. G_{2J-1}] = [O_J; O_J M^J]) up to the
 * block length L and then L samples per GEMM: log2 L + ceil((K+1)/L) large GEMMs in place of K dependent thin ones.  block: L, a power of
 * two (one beyond the power of two >= K + 1 is cut to it); 0: the smallest power of two at which the ceil(L q / 64) ceil(n / 64) output
 * tiles of one such GEMM number 256, cut to the power of two >= K + 1 and halved while the stack would hold over 5/4 (K + 1) sample rows; 1: plain
 * sequential stepping.
 * U (kind 2; NULL otherwise): (K+1) m x S doubles on the host, u_k[c] of scenario s at s*(K+1)*m + k*m + c.  X0 (kind 2, may be NULL: zero):
 * n x S doubles on the host, column-major.  S is read under kind 2 only.
 * Y (host): kinds 0 and 1: (K+1)*q*m doubles, sample k at k*q*m, q x m column-major;  kind 2: S*(K+1)*q doubles, scenario s at s*(K+1)*q,
 * sample k at k*q.  info (4, may be NULL): [0] L in force, [1] blocks = ceil((K+1)/L), [2] squarings of M, [3] launches (kernels, GEMM calls
 * and inversions enqueued, a GEMM and an inversion counted as one each).  A call is bit for bit repeatable.
 * DRE_ERR_INVALID, before any launch: a NULL argument, K < 1, dt not finite or <= 0, an unknown method or kind, mismatched shapes, S < 1 or
 * U NULL under kind 2 (U or X0 given under another kind), a block that is negative or not a power of two, a stack of (K + 1 rounded up to L)
 * q n elements beyond 2^31 - 1, and under kind 2 q > 256 or q m > 2048.  DRE_ERR_ALLOC, before any launch: the stack ((K + 1 rounded up to L)
 * q n doubles), 4 n^2 and the thin operands do not fit the free device memory (there is no chunking over time).  DRE_ERR_SINGULAR: P has an
 * exactly zero or non-finite pivot (dt on a pole of the scheme, a NaN in E or A), or E has one under kind 1; Y is not written. */
int dre_time_response(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int method, double dt, int K,
                      int kind, const double* U /* (K+1)*m*S or NULL */, int S, const double* X0 /* n*S or NULL */, int block,
                      double* Y, int64_t* info /* 4, may be NULL */);

/* ---- test and diagnostic surface: the internal GEMM entry points one by one (dre_version >= 108) ----------------------------------------
 * dre_gemm_probe calls ONE entry point of the f64 MFMA GEMM family with arguments a public caller cannot form: operands that are views into
 * larger buffers, member masks, device-side counts, the `done` flag of an ADI control block.  It has no wrapper beyond the ctypes prototype
 * and no counterpart in the reference; tests/test_gpu_gemm_family.py is its user.
 * A view is rows x cols, column-major with leading dimension ld, beginning `offset` elements into the buffer `buf`.  Before any launch every
 * view (every member of a stack, every product of a list) is checked to lie inside its buffer, every rowmap entry to lie inside C's rows, and
 * the shapes to agree; DRE_ERR_INVALID otherwise, and for whatever the entry point itself refuses.  The call synchronises. */
typedef struct dre_gemm_view { const dre_dense* buf; int64_t offset; int32_t ld, rows, cols; } dre_gemm_view;
typedef struct dre_gemm_product { dre_gemm_view A, B, C, copy_dst; double alpha; } dre_gemm_product;   /* C = alpha A B; copy_dst.buf NULL: no copy, else
                                                                                                          M x K with ld = ldcopy */
#define DRE_PROBE_GEMM 0            /* gemm: C = alpha op(A) op(B) + beta C; done, tile_sumsq */
#define DRE_PROBE_GEMM_THIN 1       /* gemm_thin: C = alpha op(A) B + beta C; done */
#define DRE_PROBE_GEMM_STRIDED 2    /* gemm_strided: batch members at offset + b * stride_*; member_on, coef */
#define DRE_PROBE_GEMM_BATCHED 3    /* gemm_batched on prod[0 .. nprod): the arguments A, B, C, alpha, beta are not read; count */
#define DRE_PROBE_GEMM_ROWS 4       /* gemm_partials + gemm_reduce_rows: C[rowmap[i], :] = (op(A) op(B))[i, :]; rowmap needed; done, count */
#define DRE_PROBE_GEMM_Z 5          /* gemm_partials_z + gemm_reduce_z: batch = nz products A_z, B_z at stride_a, stride_b into C + z * cz; rowmap optional; done */
#define DRE_PROBE_GEMM_SYM 6        /* gemm_sym_update: C <- sym(C + A B') for A, B of n x K; count */
typedef struct dre_gemm_probe_options {
    int32_t batch;                          /* members (strided) or nz (z); 0 counts as 1 */
    int64_t stride_a, stride_b, stride_c;   /* member strides in elements */
    const int32_t* member_on;               /* strided: batch entries, 0 = the member is masked out (a device BatchCtl with `fail` set); NULL: all on */
    const double* coef; int64_t coef_stride;/* strided: member b takes alpha = coef[b * coef_stride], beta = coef[b * coef_stride + 1] (uploaded); NULL: the arguments */
    const int32_t* rowmap;                  /* rows, z: M entries in [0, C.rows) (uploaded) */
    int64_t cz;                             /* z: member stride of C */
    int32_t nprod; const dre_gemm_product* prod;   /* batched */
    int32_t use_done, done;                 /* use_done != 0: a device AdiState with this `done` goes to every kernel that takes one */
    int32_t use_count, iters, base, nmax, per;     /* use_count != 0: DevCount {AdiState with this `iters`, base, nmax, per} */
    dre_dense* tile_sumsq;                  /* gemm: receives one sum of squares per 64 x 64 tile, entry bx + ceil(M / 64) * by (at least that many elements); NULL: none */
} dre_gemm_probe_options;
/* opt may be NULL (all zero).  *splits (may be NULL) receives the split-K count the host chose (1 for the kinds without one).  An option the
 * selected kind cannot take is DRE_ERR_INVALID. */
int dre_gemm_probe(dre_ctx* ctx, int kind, int transA, int transB, double alpha, const dre_gemm_view* A, const dre_gemm_view* B, double beta,
                   const dre_gemm_view* C, const dre_gemm_probe_options* opt, int* splits);

/* ---- host helpers exposed for CPU tests of the Projection shift pipeline ---------------------- */
int dre_host_eigvals(int n, const double* A, double* wr, double* wi);
int dre_host_gen_eigvals(int n, const double* A, const double* E, double* wr, double* wi);
int dre_host_svd_left(int p, int w, const double* R, double* U, double* sv);

#ifdef __cplusplus
}
#endif
#endif
