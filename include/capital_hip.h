/*
 * capital_hip.h -- C-ABI of libcapital_hip.so: the MI355X (gfx950) replacement for
 * the BLAS/LAPACK/MPI layer underneath huttered40/capital's recursive Cholesky
 * (cholinv) and CA-CholeskyQR2 (cacqr).
 *
 * This header IS the drop-in boundary.  Each entry point names the reference
 * interface it replaces (paths relative to the reference root).  All pointers
 * called A/B/C/T/data are DEVICE pointers (HBM); matrices are column-major fp64
 * exactly as the reference passes them to MKL.  Nothing here takes or returns a
 * C++ or torch type.  Every call is asynchronous on the handle's HIP stream
 * unless stated otherwise and returns a capi_status (0 = ok).
 *
 * Enum codes are the reference's own (src/blas/engine.h:23-46, src/lapack/engine.h:23-36):
 *   Transpose NoTrans=0 Trans=1 | Side Left=0 Right=1 | UpLo Lower=0 Upper=1 | Diag NonUnit=0 Unit=1
 */
#ifndef CAPITAL_HIP_H_
#define CAPITAL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct capi_handle_s* capi_handle_t;
typedef struct capi_comm_s*   capi_comm_t;

enum capi_status {
  CAPI_OK = 0,
  CAPI_EINVAL = -1,   /* bad argument (dims, enum code, null pointer, alignment) */
  CAPI_EHIP = -2,     /* a HIP runtime call failed; see capi_last_error() */
  CAPI_ENOMEM = -3,
  CAPI_ECOMM = -4,    /* RCCL failure or communicator misuse */
  CAPI_ENOTSPD = -5   /* potrf met a non-positive pivot (see capi_get_info) */
};
enum { CAPI_NOTRANS = 0, CAPI_TRANS = 1 };
enum { CAPI_LEFT = 0, CAPI_RIGHT = 1 };
enum { CAPI_LOWER = 0, CAPI_UPPER = 1 };
enum { CAPI_NONUNIT = 0, CAPI_UNIT = 1 };
/* matrix structure policies, src/matrix/structure.h:8-72 */
enum { CAPI_RECT = 0, CAPI_UPPERTRI = 1, CAPI_LOWERTRI = 2 };

/* ---- lifecycle / memory (replaces new[]/memcpy inside matrix<>, src/matrix/structure.hpp:4-26) ---- */
int  capi_version(void);
int  capi_device_count(void);
int  capi_create(capi_handle_t* h, int device);                 /* owns a new non-blocking stream */
int  capi_create_on_stream(capi_handle_t* h, int device, void* hip_stream); /* borrows the caller's stream */
int  capi_destroy(capi_handle_t h);
void* capi_get_stream(capi_handle_t h);
const char* capi_last_error(capi_handle_t h);
int  capi_malloc(capi_handle_t h, void** dptr, size_t bytes);
int  capi_free(capi_handle_t h, void* dptr);
int  capi_memset_async(capi_handle_t h, void* dptr, int value, size_t bytes);
int  capi_memcpy_h2d(capi_handle_t h, void* dst, const void* src, size_t bytes);   /* synchronous */
int  capi_memcpy_d2h(capi_handle_t h, void* dst, const void* src, size_t bytes);   /* synchronous */
int  capi_memcpy_d2d_async(capi_handle_t h, void* dst, const void* src, size_t bytes);
int  capi_sync(capi_handle_t h);
/* grow the handle's private workspace (used by in-place trmm, split-K slabs, potrf) ahead of time */
int  capi_reserve_workspace(capi_handle_t h, size_t bytes);
/* release every private workspace block of the handle (synchronises); they are re-created on demand */
int  capi_trim_workspaces(capi_handle_t h);
/* on = 1: every large launch of the handle goes out one resident round (2 x CUs workgroups: an 8 x 8 block of tiles per XCD) at a time --
 * plain and triangular outputs, TRMMs as equal-work tile pairs: same time, about half the L2-to-fabric traffic, for callers whose products
 * all run on one stream (grids, the TRSM mode); on = 0: the handle's defaults (environment: CAPI_ROUNDS, CAPI_TRMM_PAIR, CAPI_TRMM_PAIR_ROUNDS).
 * *was (may be NULL) receives the previous setting. */
int  capi_set_launch_rounds(capi_handle_t h, int on, int* was);
/* keep the handle's compute stream off `reserve` CUs (a multiple of 32: one per shader engine and XCD; 0 = all CUs again): the communication stream's kernels (RCCL's
 * send/recv on a grid) then start at once beside a tile launch instead of at its next round boundary.  Drains the handle's streams. */
int  capi_reserve_cus(capi_handle_t h, int reserve);

/* ---- BLAS layer: replaces blas::engine::_gemm/_trmm/_syrk (src/blas/interface.h:58-66,
 *      src/blas/interface.hpp:43-97 -> cblas_dgemm/dtrmm/dsyrk) ---- */
/* C <- alpha*op(A)*op(B) + beta*C  (K1-K3; call sites summa.hpp:28,139,144; cacqr.hpp:95,144) */
int capi_dgemm(capi_handle_t h, int transA, int transB, int64_t m, int64_t n, int64_t k, double alpha,
               const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
/* C(uplo) <- alpha*A^T*A + beta*C (trans=Trans, A is k x n) or alpha*A*A^T (NoTrans, A is n x k)
 * (K7; call site cacqr.hpp:15).  Only the `uplo` triangle of C is read or written. */
int capi_dsyrk(capi_handle_t h, int uplo, int trans, int64_t n, int64_t k, double alpha,
               const double* A, int64_t lda, double beta, double* C, int64_t ldc);
/* Triangular-output GEMM: C(uplo) <- alpha*op(A)*op(B) + beta*C, C is n x n.  This is what the
 * reference's summa "syrk" (summa.hpp:111-158) needs: it runs a full cblas_dgemm there because a
 * rank's two operands are different blocks; computing only the needed triangle halves the work. */
int capi_dgemmt(capi_handle_t h, int uplo, int transA, int transB, int64_t n, int64_t k, double alpha,
                const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
/* B <- alpha*op(T)*B (Left) or alpha*B*op(T) (Right); T triangular, only its `uplo` triangle is read
 * (K4-K6; call sites summa.hpp:64,71; cacqr.hpp:25,185).  In place, as cblas_dtrmm. */
int capi_dtrmm(capi_handle_t h, int side, int uplo, int trans, int diag, int64_t m, int64_t n, double alpha,
               const double* T, int64_t ldt, double* B, int64_t ldb);
/* Out-of-place form used on the hot path: C <- alpha*op(T)*B or alpha*B*op(T); C must not alias B. */
int capi_dtrmm_oop(capi_handle_t h, int side, int uplo, int trans, int diag, int64_t m, int64_t n, double alpha,
                   const double* T, int64_t ldt, const double* B, int64_t ldb, double* C, int64_t ldc);
/* accumulating form for multi-step SUMMA (d/c > 1 K-panels per layer): C <- alpha*op(T)*B + beta*C */
int capi_dtrmm_acc(capi_handle_t h, int side, int uplo, int trans, int diag, int64_t m, int64_t n, double alpha,
                   const double* T, int64_t ldt, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
/* B <- alpha*op(T)^-1*B or alpha*B*op(T)^-1.  Not in the reference (it forms trtri+trmm instead,
 * SURVEY.md quick facts); named by BASELINE.json north_star. */
int capi_dtrsm(capi_handle_t h, int side, int uplo, int trans, int diag, int64_t m, int64_t n, double alpha,
               const double* T, int64_t ldt, double* B, int64_t ldb);

/* ---- LAPACK layer: replaces lapack::engine::_potrf/_trtri (src/lapack/interface.h:49-53,
 *      src/lapack/interface.hpp:30-58 -> LAPACKE_dpotrf/dtrtri, column-major) ---- */
/* "panel32" images of a tall m x 256 panel (m % 32 == 0): m / 32 tiles of 32 rows, each tile column-major with ld 32, tile t at
 * 8192 t doubles -- element (i, j) at (i / 32) * 8192 + 32 j + i % 32.  One contiguous stream per pass instead of 256 column streams.
 * qr::cacqr (cacqr.hpp:174-193) keeps CholeskyQR2's intermediate Q1 = A R1^-1 in this form between its two sweeps (K7 / K5 of SURVEY 2.2 on
 * that image): capi_dsyrk_panel32: C(upper) = alpha A^T A + beta C, A a panel32 image of k x 256 (k >= 64 * 256);
 * capi_dtrmm_right_panel32: C = alpha B T, T 256 x 256 upper, non-unit; ldb == 0 / ldc == 0 mark B / C as panel32 images. */
int capi_dsyrk_panel32(capi_handle_t h, int64_t n, int64_t k, double alpha, const double* A32, double beta, double* C, int64_t ldc);
int capi_dtrmm_right_panel32(capi_handle_t h, int64_t m, int64_t n, double alpha, const double* T, int64_t ldt,
                             const double* B, int64_t ldb, double* C, int64_t ldc);
/* The LAPACK `info` the reference discards is kept on the device; capi_get_info() synchronises and
 * returns it (0, or 1-based index of the first non-positive pivot / zero diagonal). */
int capi_dpotrf(capi_handle_t h, int uplo, int64_t n, double* A, int64_t lda);
int capi_dtrtri(capi_handle_t h, int uplo, int diag, int64_t n, double* A, int64_t lda);
/* Fused base case of cholinv (cholinv/policy.h:190-205: potrf, memcpy, trtri): A(upper) -> R in place,
 * Rinv <- R^-1 (upper); strictly-lower parts of both outputs are zeroed (cyclic_to_local, util.hpp:131-164). */
int capi_dpotrf_trtri(capi_handle_t h, int64_t n, double* A, int64_t lda, double* Rinv, int64_t ldi);
int capi_get_info(capi_handle_t h, int* info);
/* The n x n steps of a SHIFTED CholeskyQR sweep (qr::cacqr with num_shifted > 0).  They sit beside the reference's sweep,
 * src/alg/qr/cacqr/cacqr.hpp:7-29, between its MPI_Allreduce of the Gram matrix and its cholinv call and behind that call.  Not in the
 * reference: its sweep has no shift, and its CholeskyQR2 breaks down beyond kappa(A) ~ 1e8 (shifted CholeskyQR: Fukaya et al., SIAM J.
 * Sci. Comput. 42, 2020).  rec[4] (DEVICE) is one sweep's record: s, trace(G'), ||R'||_1 ||R'||_inf, ||R'^-1||_1 ||R'^-1||_inf.
 * capi_dgram_equilibrate_shift, in place on the upper triangle of G (the lower is neither read nor written):
 *   e_j = floor(ex_j / 2), g_jj = f 2^ex_j with f in [0.5, 1) (the exponent is read from the bits, no log or sqrt), dscale[j] = 2^e_j;
 *   G' = D^-1 G D^-1, D = diag(dscale): exact, and exactly equivariant under power-of-two column scalings of A;
 *   rec[1] = trace(G') (>= ||A D^-1||_2^2), rec[0] = s = (shift_scale * (11 (m_global n + n (n + 1)) 2^-53)) * trace(G'); G' += s I.
 *   A g_jj that is zero, negative or not finite sets the info word to j + 1 as a failed pivot does (its column stays unscaled).
 *   The sums run in one workgroup in a fixed order: ranks that hold the same G compute the same s, bit for bit. */
int capi_dgram_equilibrate_shift(capi_handle_t h, int64_t n, double* G, int64_t ldg, int64_t m_global, double shift_scale,
                                 double* dscale, double* rec);
/* Behind capi_dpotrf_trtri on G' + s I: R <- R' D (columns scaled), Rinv <- D^-1 R'^-1 (rows scaled), upper triangles, by adding the
 * integer exponent (ldexp): exact.  rec[2] = ||R'||_1 ||R'||_inf >= ||R'||_2^2 and rec[3] = ||R'^-1||_1 ||R'^-1||_inf >= ||R'^-1||_2^2 of
 * the UNSCALED factors: their product bounds cond_2(G' + s I) from above, is within n^2 of it, and is 1 for G' + s I = I.
 * A diagonal entry r_jj or 1 / r_jj that leaves the normal range of fp64 when scaled (2^e_j too large or too small for it) sets the
 * info word to j + 1, as a failed pivot.  dscale == NULL stands for D = I: R and Rinv are only read (the record of a plain sweep). */
int capi_dtri_rescale(capi_handle_t h, int64_t n, double* R, int64_t ldr, double* Rinv, int64_t ldi, const double* dscale, double* rec);
/* Streaming tall-skinny products with a NARROW output, for least-squares solves on the CholeskyQR factors (qr::cacqr::least_squares: X = R^-1
 * (Q^T B) and the residual B - A X).  Not in the reference: src/alg/qr/cacqr/cacqr.hpp stops at Q and R.  1 <= r <= CAPI_TS_MAX_RHS right-hand
 * sides per call (more: CAPI_EINVAL, nothing is touched; the caller loops over column blocks); tall m >= 0, n >= 1, any leading dimensions >= the
 * row counts, pointers aligned to 8 bytes (16 bytes and even leading dimensions take the faster loads).  A is read from HBM once per call, no
 * n-wide or m-long temporary; partial sums over row slices are combined in a fixed order: bit-identical from run to run, no atomics.
 * capi_dgemtn_ts: C (n x r) <- alpha A^T B + beta C, A m x n, B m x r (beta == 0: C is not read; m == 0: C <- beta C). */
enum { CAPI_TS_MAX_RHS = 32 };
int capi_dgemtn_ts(capi_handle_t h, int64_t m, int64_t n, int64_t r, double alpha, const double* A, int64_t lda, const double* B, int64_t ldb,
                   double beta, double* C, int64_t ldc);
/* capi_dresid_ts: Rout (m x r) <- B - A X, X n x r, and colnorm2[j] <- sum_i Rout(i, j)^2 (DEVICE, r doubles).  Rout == NULL: the norms alone;
 * Rout == B: in place; colnorm2 == NULL: the residual alone; m == 0: colnorm2 <- 0. */
int capi_dresid_ts(capi_handle_t h, int64_t m, int64_t n, int64_t r, const double* A, int64_t lda, const double* X, int64_t ldx,
                   const double* B, int64_t ldb, double* Rout, int64_t ldr, double* colnorm2);
/* ---- a (packed) triangle or rectangle times a thin block: solves on the cholinv factors (cholesky::cholinv::solve).  Not in the reference:
 * src/alg/cholesky/cholinv/cholinv.hpp stops at R and R^-1.
 * C <- alpha * op(T) * B + beta * C for a thin B: 1 <= r <= CAPI_TS_MAX_RHS columns (more: CAPI_EINVAL, nothing is touched).
 * T is an m x n block of which either all (shape CAPI_RECT) or the upper triangle incl. the diagonal (CAPI_UPPERTRI, m == n;
 * nothing below the diagonal is read) takes part.
 * ldt >= m: column-major.  ldt == 0: the block lies inside a PACKED upper triangle (structure.h uppertri: column x of the
 * triangle starts at x (x + 1) / 2); T points at the block's first element and col0 is the triangle's column index of the block's
 * first column, so block column j starts at T + (col0 + j)(col0 + j + 1) / 2 - col0 (col0 + 1) / 2.
 * trans == CAPI_NOTRANS: C is m x r, B n x r.  CAPI_TRANS: C is n x r, B m x r.  C must not alias B.  beta == 0: C is not read.
 * m == 0 or n == 0: C <- beta C.  T is read from HBM once per call; partial sums are combined in a fixed order (bit-identical runs, no atomics).
 * Workspace: (slices + ceil(lines / 256)) x 256 x (16 or 32) doubles of the handle's workspace, lines = the rows of C and slices <= 256 -- 32 MiB
 * for a triangle of order 65536, but 1 GiB for 2^22 output lines at r > 16: the call is built for the factors' shapes, not for tall panels
 * (those have capi_dgemtn_ts / capi_dresid_ts).  B must be finite where T's triangle is not: inside the 32 x 32 parts that the diagonal crosses
 * the entries below the diagonal take part as zeros (0 * B(k)), so a NaN or Inf in B reaches output lines that it does not belong to. */
int capi_dtrmm_thin(capi_handle_t h, int shape, int trans, int64_t m, int64_t n, int64_t r, double alpha,
                    const double* T, int64_t ldt, int64_t col0, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
/* capi_dtrsm_thin: B (n x r, ldb >= n) <- op(T)^-1 B in place, by SUBSTITUTION, for the upper triangular T of order n with a non-unit diagonal: solves
 * on the cholinv factor R itself (cholesky::cholinv::solve with info::solve_by_substitution).  Not in the reference: cholinv.hpp stops at R and R^-1.
 * ldt >= n: column-major.  ldt == 0: a diagonal sub-triangle of a PACKED upper triangle that starts at the triangle's column col0, addressed as
 * capi_dtrmm_thin addresses it (T points at the sub-triangle's first element; offsets are 64-bit).  1 <= r <= CAPI_TS_MAX_RHS (more: CAPI_EINVAL,
 * nothing is touched); n == 0 is OK; pointers aligned to 8 bytes, any ldb.  No inverse of T or of a diagonal block is formed (reciprocals of
 * diagonal entries only): LAPACK's row-wise backward stability.  Nothing below T's diagonal is read or influences the result.  No singularity check:
 * a zero on the diagonal gives Inf or NaN as cblas_dtrsm does, and the info word is untouched.  T is read from HBM once per call: the triangle is
 * cut into leaves of order <= 512, each substituted by one workgroup, and rectangular products through capi_dtrmm_thin (csrc/trsm_thin_plan.h);
 * the steps are ordered by kernel boundaries on the handle's stream, sums have a fixed order (bit-identical runs, no atomics).
 * Workspace: capi_dtrmm_thin's for the largest product, the top level's T12 (about n / 2 output lines), of the handle's workspace; none for n <= 512. */
int capi_dtrsm_thin(capi_handle_t h, int trans, int64_t n, int64_t r, const double* T, int64_t ldt, int64_t col0, double* B, int64_t ldb);
/* ---- the rank-r update (sign = +1) or downdate (sign = -1) of an upper triangular factor and of its inverse: T'^T T' = T^T T + sign V V^T in O(n^2 r),
 * LINPACK's dchud / dchdd (cholesky::cholinv::update).  Not in the reference: cholinv.hpp stops at R and R^-1.  The conventions are those of the thin
 * calls: device pointers, column-major, 1 <= r <= CAPI_TS_MAX_RHS and sign = +1 or -1 (else CAPI_EINVAL, nothing is touched), pointers aligned to 8 bytes;
 * n == 0 is OK. ----
 * capi_dchud: T is upper triangular of order n with a positive diagonal, addressed exactly as capi_dtrsm_thin addresses it: ldt >= n is column-major,
 * ldt == 0 a diagonal sub-triangle of a PACKED upper triangle that starts at the triangle's column col0 (T points at the sub-triangle's first element;
 * offsets are 64-bit).  V is n x r (ldv >= n) and is destroyed.  Nothing below T's diagonal is read or written: it may hold NaN, and zeros there stay zeros.
 * Step k = 0 .. n - 1 has alpha = T_kk and x = the current row k of V: beta = sqrt(alpha^2 + sign ||x||^2); for every column j >= k
 * t = (alpha T_kj + sign x^T v_j) / beta, v_j <- v_j - x (T_kj + t) / (alpha + beta), T_kj <- t (the two divisions as reciprocals, taken once per step).
 * `log` is DEVICE memory of capi_dchud_log_bytes(n, r) bytes (0 for arguments out of range): per step the r + 2 doubles x_k, alpha_k, beta_k, for
 * capi_dchud_inv.  *info_host = 0 on success, or the 1-based step at which alpha^2 + sign ||x||^2 > 0 did not hold (written so that a NaN compares
 * false): a downdate that leaves the matrix not positive definite.  T is then unspecified from that row down and the status is still CAPI_OK; the stop
 * sets a device flag, later kernels of the call read it at entry and return (as in capi_dpstrf).  Reading *info_host is the call's single stream
 * synchronisation and the only host traffic; the handle's info word is not touched.
 * Method (csrc/chud_plan.h): panels of 32 rows; per panel one workgroup runs the 32 dependent steps on the diagonal block and writes the log, then a
 * wide kernel gives every trailing column a thread (v_j in registers, T through an LDS tile): 2 ceil(n / 32) - 1 launches, ordered by kernel boundaries
 * on the handle's stream: no cooperative launch, no device-side waiting, no atomics; sums have a fixed order (bit-identical runs).  T is read and
 * written once.  Workspace, of the handle's own: 8 bytes. */
size_t capi_dchud_log_bytes(int64_t n, int64_t r);
int capi_dchud(capi_handle_t h, int sign, int64_t n, int64_t r, double* T, int64_t ldt, int64_t col0, double* V, int64_t ldv, double* log,
               int* info_host);
/* capi_dchud_inv: the logged steps k0 <= k < k1 of a capi_dchud(sign, n, r, ..) applied to the rows of the upper triangular Tinv (order n, addressed as T
 * there) that belong to the diagonal sub-triangle [k0, k1): with Tinv = T^-1 before, that sub-triangle is the inverse of T' 's afterwards (k0 = 0,
 * k1 = n: Tinv <- T'^-1).  Not in the reference: cholinv.hpp stops at R and R^-1.  The step of capi_dchud on the pairs (Tinv_ck, e_c), c <= k, e_c an
 * r-vector that starts at zero and is dropped.  Nothing outside the sub-triangle is read or written: for a factor whose inverse is kept as two
 * diagonal blocks (cholinv with complete_inv == 0) the ranges [0, h1) and [h1, n) update the blocks and leave the unformed block alone.  One launch,
 * a thread per row: no chain, no synchronisation, no workspace; the same bits on every run.  0 <= k0 <= k1 <= n; k0 == k1 does nothing. */
int capi_dchud_inv(capi_handle_t h, int sign, int64_t n, int64_t r, double* Tinv, int64_t ldt, int64_t col0, const double* log, int64_t k0, int64_t k1);
/* capi_dresid_sym: Rout (n x r) <- B - S X and colnorm2[j] <- sum_i Rout(i, j)^2 (DEVICE, r doubles) for the SYMMETRIC S whose upper triangle, diagonal
 * included, is that of the column-major A (lda >= n): the residual of cholesky::cholinv::solve.  Not in the reference: cholinv.hpp stops at R and R^-1.
 * NO element below A's diagonal influences any output: it may hold NaN, Inf or garbage (inside the tiles that the diagonal crosses the unwanted
 * elements are removed by a select, not multiplied by zero).  Below 8 columns the upper triangle is read from HBM ONCE, by a kernel of its own: a
 * tile serves S X's lines of its rows and, transposed, of its columns.  From 8 columns on the call runs capi_dtrmm_thin(CAPI_UPPERTRI) twice,
 * NOTRANS and TRANS, and corrects the diagonal, which both counted: the triangle is read twice, and that measured faster there.
 * Every other convention is capi_dresid_ts's: Rout == NULL: the norms alone; Rout == B: in place; colnorm2 == NULL: the residual alone; n == 0:
 * colnorm2 <- 0; 1 <= r <= CAPI_TS_MAX_RHS (more: CAPI_EINVAL, nothing is touched); pointers aligned to 8 bytes, any leading dimensions (lda < 2^24).
 * Rout must not alias X.  Partial sums are combined in a fixed order: bit-identical from run to run, no atomics.
 * Workspace, of the handle's own.  Below 8 columns: p (p + 1) blocks of 16 x bs doubles, p (p + 1) / 2 <= the CUs and bs = n / p rounded up to 32 --
 * about 128 p n bytes, 93 MiB at n = 32768 on 256 CUs (p = 22), 2 % of the triangle.  From 8 on: capi_dtrmm_thin's, and n x r doubles. */
int capi_dresid_sym(capi_handle_t h, int64_t n, int64_t r, const double* A, int64_t lda, const double* X, int64_t ldx,
                    const double* B, int64_t ldb, double* Rout, int64_t ldr, double* colnorm2);
/* ---- how far to trust a solve: the pieces of cholesky::cholinv::condition / error_bounds (LAPACK's dpocon and dporfs around products with the
 * resident factors).  Not in the reference: cholinv.hpp stops at R and R^-1.  The conventions are those of the thin calls above: device pointers,
 * column-major, 1 <= r <= CAPI_TS_MAX_RHS (else CAPI_EINVAL, nothing is touched), pointers aligned to 8 bytes, any leading dimension >= the
 * rows, sums in a fixed order (bit-identical from run to run, no atomics), workspace of the handle's own. ---- */
/* capi_dsym_abs: W (n x r) <- |S| |X| + |B| and colmax[j] <- max_i W(i, j) (DEVICE, r doubles) for the symmetric S given by the upper triangle of the
 * column-major A, exactly as in capi_dresid_sym: dporfs's componentwise weights.  Not in the reference: cholinv.hpp stops at R and R^-1.
 * B == NULL: the product alone; W == NULL: the maxima alone; colmax == NULL: W alone; n == 0: colmax <- 0.  X = ones and B = NULL give
 * ||S||_1 in colmax[0].  NO element below A's diagonal influences any output: it may hold NaN (unwanted elements are removed by a select, never
 * multiplied by zero).  A NaN in W shows in colmax.  W must not alias X; W == B is allowed.  The kernel is capi_dresid_sym's fused kernel on absolute
 * values, at every r: 16 columns a pass, so the triangle is read from HBM ceil(r / 16) times.  Workspace: capi_dresid_sym's below 8 columns. */
int capi_dsym_abs(capi_handle_t h, int64_t n, int64_t r, const double* A, int64_t lda, const double* X, int64_t ldx,
                  const double* B, int64_t ldb, double* W, int64_t ldw, double* colmax);
/* capi_dberr: dporfs's two elementwise steps in one pass over the residual Rho = B - S X (n x r) and the weights W = |S| |X| + |B| (capi_dsym_abs).
 * Not in the reference: cholinv.hpp stops at R and R^-1.  berr[j] (DEVICE, r doubles) <- max_i |rho_ij| / w_ij where w_ij > safe2, and
 * (|rho_ij| + safe1) / (w_ij + safe1) elsewhere, safe1 = (n + 1) DBL_MIN, safe2 = safe1 / eps, eps = 2^-53: the componentwise backward error.
 * Then W(i, j) <- |rho_ij| + (n + 1) eps w_ij (+ safe1 where w_ij <= safe2): the weights of the forward bound (capi_dlacn_block's Wt).
 * One workgroup per column; n == 0: berr <- 0.  W must not alias Rho.  No workspace. */
int capi_dberr(capi_handle_t h, int64_t n, int64_t r, const double* Rho, int64_t ldr, double* W, int64_t ldw, double* berr);
/* capi_dcolamax: colmax[j] (DEVICE, r doubles) <- max_i |X(i, j)|, a NaN showing: the ||x_j||_inf that scales a forward bound.  Not in the reference:
 * cholinv.hpp stops at R and R^-1.  n == 0: zeros.  No workspace. */
int capi_dcolamax(capi_handle_t h, int64_t n, int64_t r, const double* X, int64_t ldx, double* colmax);
/* capi_dcolnorm2: out[j] (DEVICE, r doubles) <- sum_i X(i, j)^2, a NaN showing: with X = R^-T B the quadratic forms b_j^T A^-1 b_j
 * (cholesky::cholinv::quadratic_forms).  Not in the reference: cholinv.hpp stops at R and R^-1.  capi_dcolamax's sibling: one workgroup per column,
 * one fixed order of the sum.  n == 0: zeros.  No workspace. */
int capi_dcolnorm2(capi_handle_t h, int64_t n, int64_t r, const double* X, int64_t ldx, double* out);
/* ---- reductions over the cholinv factors themselves (cholesky::cholinv::inverse_diagonal, log_determinant).  Not in the reference: cholinv.hpp stops
 * at R and R^-1. ----
 * capi_dtri_rownorm2: out[i] (DEVICE, m doubles) <- beta out[i] + sum_j T(i, j)^2: with T = R^-1 the diagonal of A^-1.  Not in the reference:
 * cholinv.hpp stops at R and R^-1.  T is an m x n block addressed exactly as capi_dtrmm_thin addresses it: shape CAPI_RECT, or CAPI_UPPERTRI with
 * m == n (the upper triangle incl. the diagonal); ldt >= m is column-major, ldt == 0 a block inside a PACKED upper triangle whose first column is the
 * triangle's column col0 (T points at the block's first element; offsets are 64-bit).  Nothing below the diagonal is read into the result: it may hold
 * NaN (inside the tiles that the diagonal crosses the unwanted entries are removed by a select, never multiplied by zero).  beta == 0: out is not
 * read.  n == 0: out <- beta out.  m == 0: nothing happens.  Bad arguments: CAPI_EINVAL before any launch, nothing is touched.  T is read from HBM once
 * per call, through capi_dtrmm_thin's NOTRANS partition (csrc/tri_thin_plan.h: the same tiles, the same slices by equal bytes); per-slice partial sums
 * are combined in a fixed order (bit-identical runs, no atomics).  Workspace: (slices + ceil(m / 256)) x 256 doubles of the handle's workspace. */
int capi_dtri_rownorm2(capi_handle_t h, int shape, int64_t m, int64_t n, const double* T, int64_t ldt, int64_t col0, double beta, double* out);
/* capi_dtri_logdiag: out[0] (DEVICE) <- sum_i log T(i, i) for the upper triangular T of order n, addressed as capi_dtrsm_thin addresses it (ldt >= n, or
 * ldt == 0 and col0): with T = R half the log-determinant of A.  Not in the reference: cholinv.hpp stops at R and R^-1.  Only the diagonal is read.  No
 * sign check: a non-positive or NaN diagonal entry gives -Inf or NaN in the sum.  n == 0: 0.  One workgroup; a thread adds the entries tid, tid + 256,
 * .., and the 256 sums meet pairwise in a fixed order (bit-identical runs).  No workspace. */
int capi_dtri_logdiag(capi_handle_t h, int64_t n, const double* T, int64_t ldt, int64_t col0, double* out);
/* ---- power-of-two equilibration of a badly scaled SPD matrix (cholesky::cholinv::equilibrate; LAPACK's dpoequb + dlaqsy).  Not in the reference:
 * cholinv.hpp stops at R and R^-1.  The three calls share these conventions: DEVICE pointers, column-major; a null handle returns -1 before any device
 * call; bad arguments return CAPI_EINVAL before any launch, nothing is touched; a size of 0 is a no-op; no atomics, sums and maxima in one fixed order
 * (bit-identical runs).  The scale factors are powers of two -- the rule of capi_dgram_equilibrate_shift and capi_dtri_rescale, at any order -- so
 * every operation is exact where nothing over- or underflows, and reversible bit for bit. ----
 * capi_dpoequ2: the scale factors of A from its diagonal.  Not in the reference: cholinv.hpp stops at R and R^-1.  Only the n diagonal entries of the
 * column-major A (lda >= n) are read.  With a_jj = f 2^ex_j, f in [0.5, 1) (the exponent is taken from the bits, subnormals included; no log, no
 * sqrt): e_j = floor(ex_j / 2) and dscale[j] (n doubles) <- 2^e_j, always a normal number (-537 <= e_j <= 512); the diagonal of D^-1 A D^-1 then lies in
 * [0.5, 2).  rec (4 doubles): rec[0] = scond = min dscale / max dscale, rec[1] = amax = max a_jj, rec[2] = min a_jj, rec[3] = 0 -- or rec[3] = j + 1
 * for the FIRST j whose a_jj is zero, negative, NaN or Inf: then dscale is all ones, rec[0] = 1 and rec[1] = rec[2] = 0.  rec[3] is a word of its own,
 * not the handle's potrf info word (capi_get_info).  One workgroup.  No workspace. */
int capi_dpoequ2(capi_handle_t h, int64_t n, const double* A, int64_t lda, double* dscale, double* rec);
/* capi_dsym_scale2: a_ij <- ldexp(a_ij, -sign (e_i + e_j)) IN PLACE on the upper triangle of A, diagonal included: sign = +1 gives A_s = D^-1 A D^-1,
 * sign = -1 undoes it (anything else: CAPI_EINVAL).  Not in the reference: cholinv.hpp stops at R and R^-1.  e_i is the exponent field of dscale[i]
 * (capi_dpoequ2's output: normal powers of two).  One exponent addition per element, never two multiplications: no intermediate can overflow; zero, Inf
 * and NaN pass through unchanged, a result below the normal range is rounded once.  Nothing below the diagonal and no padding row (n .. lda - 1) is
 * read into a result or changes a bit: it may hold NaN.  Any lda >= n; 16-byte accesses where A is 16-byte aligned and lda is even, 8-byte ones
 * otherwise.  Only the 512 x 64 tiles that touch the triangle are launched; the tiles that the diagonal or the edge crosses select after loading.  The
 * triangle is read and written once: the call is bound by that stream.  No workspace. */
int capi_dsym_scale2(capi_handle_t h, int64_t n, double* A, int64_t lda, const double* dscale, int sign);
/* capi_drow_scale2: Y(i, j) <- ldexp(X(i, j), sign e_i) for an m x r block, any r >= 1: Y = D X (sign = +1) or D^-1 X (sign = -1; anything else:
 * CAPI_EINVAL), e_i as in capi_dsym_scale2.  Not in the reference: cholinv.hpp stops at R and R^-1.  ldx, ldy >= m; Y == X (with ldy == ldx) is allowed.
 * norm2: NULL, or r doubles that receive the squared column norms of Y (a NaN showing; one workgroup per column, one fixed order of the sum, as
 * capi_dcolnorm2); with NULL nothing but Y is written.  m == 0 or r == 0: nothing happens.  No workspace. */
int capi_drow_scale2(capi_handle_t h, int64_t m, int64_t r, const double* dscale, int sign, const double* X, int64_t ldx, double* Y, int64_t ldy, double* norm2);
/* capi_dlacn_block: the Hager-Higham estimator of a 1-norm (LAPACK dlacn2, Higham's refinements included) for r operators at once, by reverse
 * communication.  Not in the reference: cholinv.hpp stops at R and R^-1.  Column j estimates the 1-norm of diag(Wt(:, j)) Z -- which is
 * || Z diag(Wt(:, j)) ||_inf, dporfs's bound on || |Z| w ||_inf -- for a SYMMETRIC operator Z that the caller applies (cholinv: Z = A^-1);
 * Wt == NULL: ||Z||_1 itself.  Protocol: call with init = 1; while *active_host > 0, overwrite all r columns of X (n x r, ldx) with Z X and call
 * again with init = 0; when *active_host == 0, est[j] (DEVICE, r doubles) holds the estimates.  One launch moves every column by its own dlacn2
 * transition, so r estimates cost the products of the slowest column: at most 11.  The scaling by Wt happens inside (before the product for the
 * transposed operator, after it otherwise): the caller applies Z alone.  A finished column is frozen: its column of X is zero, its est is not
 * written again.  The call synchronises the handle's stream to return *active_host; that int is the only host traffic.  A state that is not
 * this estimator's (more than 11 products behind it, say) gives CAPI_EINVAL.  n >= 1.  `state` is DEVICE memory of capi_dlacn_state_bytes(n, r)
 * bytes (0 for arguments out of range), opaque, and belongs to one estimate from init to the end: per column the signs of the last sign vector, the
 * stage, the round, the two last positions of the maximum and the estimate.  One workgroup per column, sums in a fixed order, the FIRST maximum. */
size_t capi_dlacn_state_bytes(int64_t n, int64_t r);
int capi_dlacn_block(capi_handle_t h, int init, int64_t n, int64_t r, double* X, int64_t ldx, const double* Wt, int64_t ldw,
                     double* state, double* est, int* active_host);
/* ---- the singular value decomposition of an upper triangular R (n x n, column-major, ldr >= n), R = U diag(sigma) V^T: the job of LAPACK's dgesvj
 * for a triangle, and the last step of a tall-skinny SVD on the CholeskyQR factors (qr::cacqr::svd: A = Q R = (Q U) Sigma V^T).
 * Not in the reference: cacqr.hpp stops at Q and R.  1 <= n <= 2048 (else CAPI_EINVAL, nothing is touched; n == 1 has no pairs).  Only R's upper triangle, diagonal
 * included, is read: what lies below may be NaN and influences nothing; R is not written.  sigma (DEVICE, n doubles): non-negative, descending.
 * U and V (n x n, ldu, ldv >= n) are written in full; either or both may be NULL (both: the values alone), and they must not alias each other.
 * Method: one-sided (Hestenes) Jacobi on the columns of R^T, cyclic sweeps in round-robin order (csrc/jacobi_plan.h: N - 1 steps of up to N / 2
 * disjoint pairs, N = n rounded up to even) -- one launch per step, one workgroup per pair.  A pair is rotated when |x^T y| > sqrt(n) 2^-53 ||x|| ||y||
 * (dgesvj's criterion) and skipped when a column is zero; the first sweep that rotates nothing ends the loop, the 30th at the latest.
 * *sweeps_host receives the number of sweeps run, or -30 when the cap was hit: the call then still sorts and returns what it has, with CAPI_OK.
 * The normalised final columns are V and their norms sigma, so V costs nothing beyond the values; U is the product of the rotations, accumulated
 * only when U != NULL (two more columns per rotation), and polished by one Newton-Schulz step U (1.5 I - 0.5 U^T U) -- two n x n products on the tile
 * kernel.  Then a stable descending sort, ties by index (a NaN sorts first); a column whose norm is exactly zero stays zero.  No sign convention.
 * Steps are ordered by kernel boundaries on the handle's stream: no cooperative launch, no device-side waiting; sums have a fixed order and the only
 * atomics are the integer counts of a sweep's rotations, so every result is bit-identical from run to run and on every device that holds the same R.
 * The call synchronises the stream once per sweep to read that count (4 bytes), the only host traffic.  Non-finite input: a NaN compares false,
 * rotates nothing and comes back as NaN in sigma.  Accuracy as measured: an O(sweeps n u) normwise error, residual and sigma errors
 * of 3e-14 to 1e-13 at n = 256 where LAPACK's bidiagonal SVD gives 2e-15.  Pointers aligned to 8 bytes.
 * Workspace, of the handle's own: n x n doubles (2 n x n with U) and 2 n more. */
int capi_dgesvj(capi_handle_t h, int64_t n, const double* R, int64_t ldr, double* U, int64_t ldu, double* sigma, double* V, int64_t ldv,
                int* sweeps_host);
/* ---- Cholesky with complete pivoting of a Gram matrix (LAPACK's dpstrf, upper): the rank-revealing step of a column-pivoted CholeskyQR
 * (qr::cacqr::factor_pivoted: it takes capi_dpotrf_trtri's place in the first sweep and stops where the remaining columns are noise).
 * Not in the reference: cacqr.hpp stops at Q and R.  G is n x n, column-major, ldg >= n, 1 <= n <= 2048; anything else, a null pointer or a tol that
 * is not >= 0 returns CAPI_EINVAL with nothing touched, *rank_host included.  Only G's upper triangle, diagonal included, is read or written: what
 * lies below may be NaN and influences nothing.  On exit rows 0 .. k - 1 of the triangle hold the k x n upper trapezoid R = [R11 R12] with
 * P^T G P = R^T R + diag-block(0, S), S the (n - k) x (n - k) Schur complement; rows >= k of the triangle are unspecified.  piv (DEVICE, n ints,
 * 0-based) is always a full permutation: column j of the permuted matrix is column piv[j] of G.  *rank_host = k; reading it is the call's single
 * stream synchronisation (as sweeps_host in capi_dgesvj) and the only host traffic.  The handle's info word is not touched.
 * Stopping rule: thresh = tol * trace(G), the trace over the input diagonal, summed by one workgroup in a fixed order.  At step j, p is the FIRST
 * index of the largest remaining (Schur-updated) diagonal entry d_p; the factorization stops at rank j unless d_p > thresh -- written so that a NaN
 * compares false and stops.  tol = 0 factors until a pivot is <= 0.  Non-finite input still ends the call (every loop has a trip count fixed by n)
 * with 0 <= k <= n and piv a permutation; the values are then unspecified.
 * Method: dpstrf's blocked, lazy scheme, panels of 32 columns, one workgroup (up to 1024 threads) per panel -- updated diagonal, argmax, the
 * symmetric swap in upper storage, the swap of the rows of R already computed, the panel's row of R -- and G22 -= R_strip^T R_strip through
 * capi_dsyrk.  All ceil(n / 32) rounds are enqueued without a host round trip: a stop sets a device flag, the panel kernel zeroes its unfinished
 * strip rows, later panel kernels read the flag at entry and return.  Steps are ordered by kernel boundaries on the handle's stream: no
 * cooperative launch, no device-side waiting, no atomics; sums have a fixed order, so every result is bit-identical from run to run and on every
 * device that holds the same G -- the ranks of a 1-D grid agree on piv without communication.  Pointers aligned to 8 bytes (piv to 4).
 * Workspace, of the handle's own: 16 bytes, and capi_dsyrk's. */
int capi_dpstrf(capi_handle_t h, int64_t n, double* G, int64_t ldg, double tol, int* piv, int* rank_host);
/* The permutation as a kernel: D (n x ncols, ldd >= n) <- 0, then D(piv[i], :) <- S(i, :) for i < k (0 <= k <= n; S k x ncols, lds >= k; piv DEVICE
 * ints of which the first k are read, distinct and in 0 .. n - 1: an index outside that range writes nothing).  Not in the reference: cacqr.hpp stops
 * at Q and R.  tri = 1 takes only S's upper triangle: entries below the diagonal count as zero and are not read.  Serves M = P(:, 0:k) R11^-1 and the
 * basic least-squares solution X = P [Y; 0].  D must not alias S.  k == 0: zeros alone; n == 0 or ncols == 0: nothing.  No workspace. */
int capi_drow_scatter(capi_handle_t h, int tri, int64_t k, int64_t ncols, int64_t n, const double* S, int64_t lds, const int* piv, double* D, int64_t ldd);
/* ---- diagonally pivoted, PARTIAL Cholesky of a symmetric positive semidefinite or numerically low-rank matrix of any order, A ~= L L^T with L n x k
 * (cholesky::cholinv::factor_pivoted: what a caller has where capi_dpotrf refuses, or where k << n columns are wanted; O(n k^2), not O(n^3)).
 * Not in the reference: cholinv.hpp stops at R and R^-1.  A is n x n, column-major, lda >= n; only its UPPER triangle, diagonal included, is read --
 * what lies below may be NaN -- and A is never written.  L is n x max_rank, column-major, ldl >= n; piv and d are DEVICE arrays of n ints and n doubles.
 * 1 <= n < 2^31, 1 <= max_rank <= min(n, CAPI_PCHOL_MAX_RANK); anything else, a null pointer, lda < n, ldl < n or a NaN tol returns CAPI_EINVAL before
 * any launch, with nothing touched.  Pointers aligned to 8 bytes (piv to 4).  The handle's info word is not touched.
 * Swap-free: the factor stays in A's own ordering.  With d = diag(A) at the start, step j = 0, 1, .. takes p = the FIRST index of the largest remaining
 * d_i (ties to the smaller index, a NaN counts as -inf, chosen indices are out of the running) and stops unless d_p > thresh -- written so that a
 * NaN compares false and stops.  Otherwise, for the rows i not yet chosen, L(i, j) = (A(i, p) - sum_{l < j} L(i, l) L(p, l)) / sqrt(d_p), l ascending,
 * A(i, p) taken from the upper triangle; L(i, j) = 0 exactly for the rows chosen before; L(p, j) = sqrt(d_p); d_i <- fl(d_i - fl(L(i, j)^2)), the
 * product and the difference rounded one after the other, so that d can be recomputed from L bit for bit.
 * thresh = tol * trace(A), as in capi_dpstrf; tol < 0: LAPACK dpstrf's default n u max_i a_ii, u = 2^-53.
 * On exit *rank_host = k, 0 <= k <= max_rank; columns < k of L are written, columns >= k and the padding rows of L are NOT; piv[0 .. k) holds the chosen
 * indices in order and piv[k .. n) the others ascending, so piv is always a permutation; d[i] is the remaining Schur diagonal of a row that was not
 * chosen and 0 for a chosen one; *resid_trace_host is the sum of d over the rows not chosen -- for a PSD A the trace norm of A - L L^T.
 * Non-finite input ends the call like any other (every loop has a trip count fixed by n and max_rank): CAPI_OK, 0 <= k <= max_rank, piv a
 * permutation, the values unspecified.
 * Method (csrc/pchol_f64.hip): one launch per step over ceil(n / 256) workgroups, a thread owns a row; the pivot row L(p, 0 .. j) is staged in LDS
 * once per workgroup; a workgroup ends its step with its own (value, index) candidate for the next pivot, and every workgroup of the next launch
 * reduces those ceil(n / 256) candidates -- no workgroup reads the whole of d.  A stop sets a device flag; later launches read it at entry and return.
 * The host enqueues the steps in rounds of 64 and reads the flag once per round.  Ordered by kernel boundaries on the handle's stream alone: no
 * cooperative launch, no device-side waiting, no atomics; sums have a fixed order: two calls on the same bits give identical bytes.
 * Workspace, of the handle's own: 4 n + 64 ceil(n / 256) + 32 bytes. */
enum { CAPI_PCHOL_MAX_RANK = 4096 };
int capi_dpchol(capi_handle_t h, int64_t n, const double* A, int64_t lda, double tol, int64_t max_rank, double* L, int64_t ldl, int* piv, double* d,
                int* rank_host, double* resid_trace_host);
/* The threshold that capi_dpchol(h, n, A, lda, tol, ..) stops at, bit for bit (the same kernels sum the same diagonal in the same order).  Not in the
 * reference: cholinv.hpp stops at R and R^-1.  Reads A's diagonal alone; CAPI_EINVAL as there, with nothing touched. */
int capi_dpchol_thresh(capi_handle_t h, int64_t n, const double* A, int64_t lda, double tol, double* thresh_host);
/* ---- the diagonal pieces of M = L L^T + D on capi_dpchol's factor, D a positive diagonal (cholesky::cholinv::lowrank_prepare / lowrank_solve /
 * lowrank_quadratic_forms: Woodbury's identity with the k x k matrix C = I + L^T D^-1 L; the products, the Cholesky factorization of C and the
 * substitutions run on capi_dsyrk, capi_dpotrf, capi_dgemtn_ts, capi_dtrsm_thin and capi_dresid_ts).  Not in the reference: cholinv.hpp stops at R and R^-1.
 * The three calls share the conventions of the thin calls: DEVICE pointers, column-major, pointers aligned to 8 bytes; a null handle returns -1 before any
 * device call; bad arguments return CAPI_EINVAL before any launch, nothing is touched; a size of 0 is a no-op; no atomics, sums in one fixed order
 * (two calls on the same bits give the same bytes).  No workspace. ----
 * capi_dlr_diag: d[i] (n doubles) <- (shift + diag[i]) + schur[i], each sum rounded, in that order; diag == NULL and schur == NULL count as zeros (they are
 * not added).  Not in the reference: cholinv.hpp stops at R and R^-1.  rec (4 doubles): rec[0] = sum_i log d_i, rec[1] = min d, rec[2] = max d, rec[3] = 0 --
 * or rec[3] = j + 1 for the FIRST j whose d_j is not a finite number > 0 (zero, negative, NaN, Inf): then rec[0 .. 2] are 0, d is unspecified and a caller
 * refuses.  rec[3] is a word of its own, not the handle's potrf info word (capi_get_info).  One workgroup; a thread adds the logarithms of the entries
 * tid, tid + 1024, .., the sums meet in a butterfly inside the wave and the 16 waves in order (capi_dpoequ2's and capi_dtri_logdiag's style). */
int capi_dlr_diag(capi_handle_t h, int64_t n, double shift, const double* diag, const double* schur, double* d, double* rec);
/* capi_drow_pow: Y <- alpha diag(d)^power X + beta Y on an m x r block, any r >= 1, power = +1, -1 or -0.5 (anything else: CAPI_EINVAL).
 * Not in the reference: cholinv.hpp stops at R and R^-1.  ldx, ldy >= m; Y == X is allowed with ldy == ldx; with beta == 0 Y is not read (it may hold NaN).
 * Order of the operations, every one rounded on its own (no fused multiply-add), t the scaled element:
 *   power +1: t = x d;  power -1: t = x / d (a division per element);  power -0.5: t = x w with w = 1 / sqrt(d), taken once per row;
 *   Y = alpha t + beta y (beta == 0: Y = alpha t)
 * so that +1 and -1 give numpy's alpha * (x * d) + beta * y and alpha * (x / d) + beta * y bit for bit, and -0.5 is within 2 ulp of x / sqrt(d).
 * norm2: NULL, or r doubles that receive the squared column norms of the result Y, by a pass of its own in capi_dcolnorm2's fixed order (one workgroup
 * per column); with NULL nothing but Y is written.  16-byte accesses where X and Y are 16-byte aligned and ldx, ldy are even, 8-byte ones otherwise;
 * the padding rows m .. ld - 1 are neither read into a result nor written.  d must be positive where power < 0 (no check: a zero gives Inf or NaN).
 * A pure stream: 512 rows x 32 (or 8) columns per workgroup, a row's factor computed once. */
int capi_drow_pow(capi_handle_t h, int64_t m, int64_t r, double power, const double* d, double alpha, const double* X, int64_t ldx, double beta, double* Y,
                  int64_t ldy, double* norm2);
/* capi_ddiag_add: C(i, i) += alpha for i < n (ldc >= n): the I of C = I + L^T D^-1 L.  Not in the reference: cholinv.hpp stops at R and R^-1.  Nothing off
 * the diagonal is read or written. */
int capi_ddiag_add(capi_handle_t h, int64_t n, double alpha, double* C, int64_t ldc);
/* LAPACKE_dgeqrf / LAPACKE_dorgqr behind lapack::engine::_geqrf / _orgqr (lapack/interface.hpp:60-88; the reference has
 * the slots but no caller -- CholeskyQR2 is its QR).  Householder QR, LAPACK storage: R in the upper triangle, the
 * reflectors v_j (unit first entry implied) below it, tau[min(m,n)] on the DEVICE.  capi_dorgqr overwrites A (m x n,
 * m >= n >= k) with the first n columns of Q = H_1 ... H_k.  Blocked (compact WY, width 32) on the MFMA tile kernel.
 * Tall panels (32 <= n <= 2048, m >= 64 n) are factored by CholeskyQR2 and the LAPACK image reconstructed from it; the output is
 * dlarfg's on either side of that gate, tau = 0 for a column that is already reduced included.  k == 0: tau may be NULL. */
int capi_dgeqrf(capi_handle_t h, int64_t m, int64_t n, double* A, int64_t lda, double* tau);
int capi_dorgqr(capi_handle_t h, int64_t m, int64_t n, int64_t k, double* A, int64_t lda, const double* tau);
/* capi_dormqr: LAPACK's dormqr for side == CAPI_LEFT: C (m x r, ldc >= m) <- Q^T C (CAPI_TRANS) or Q C (CAPI_NOTRANS) with Q = H_1 ... H_k taken from
 * the first k columns of a capi_dgeqrf image A (m x k, lda >= m, m >= k >= 0) and tau (DEVICE, k doubles), without forming Q.  Not in the reference:
 * lapack/interface.h declares _geqrf and _orgqr only.  side == CAPI_RIGHT (C Q, C Q^T) is not served: CAPI_EINVAL.  A is not written.  Nothing on or
 * above A's diagonal influences the result -- that part holds R, and NaN there is harmless: the unit diagonal and the zeros above it are put in by a
 * select, never by a multiplication by zero.  tau[j] == 0 is the identity reflector and takes no special path.  Any other bad argument (a null operand
 * of a non-empty problem, lda < m, ldc < m, k > m): CAPI_EINVAL before any launch, nothing is touched.  m == 0, r == 0 or k == 0: nothing happens
 * (tau may be NULL when k == 0).  Pointers aligned to 8 bytes, any leading dimensions (16 bytes and even leading dimensions take the faster loads);
 * the padding rows m .. ld - 1 of C are neither read into a result nor written.  The handle's info word is not touched.
 * r <= CAPI_TS_MAX_RHS: panels of 32 reflectors, ascending for Q^T and descending for Q, three launches each (csrc/ormqr_plan.h): P^T [P | C] over the
 * panel's live rows in one pass on v_mfma_f64_16x16x4_f64 (row slices per workgroup, slabs added in slab order), one workgroup for T (dlarft's
 * recurrence), Z = T^T W or T W and the panel's top 32 rows, and capi_dresid_ts for C -= P Z below them.  The panel is read from HBM twice, the live
 * rows of C twice and written once; no m-long temporary.  Sums have a fixed order: no atomics, the same bits on every run.  Workspace, of the handle's
 * own: 8 KiB + at most (CUs) x 14 KiB.  r > CAPI_TS_MAX_RHS: the block-reflector loop of capi_dorgqr on the tile kernel (capi_dorgqr's workspace). */
int capi_dormqr(capi_handle_t h, int side, int trans, int64_t m, int64_t r, int64_t k, const double* A, int64_t lda, const double* tau, double* C,
                int64_t ldc);
/* capi_dgels: LAPACK's dgels(trans = 'N') for m >= n >= 1 and any r >= 1: min ||A X - B|| by Householder QR, backward stable up to kappa(A) ~ 1 / u.
 * Not in the reference: lapack/interface.h declares _geqrf and _orgqr only.  m < n (minimum-norm solutions) is not served: CAPI_EINVAL, nothing is
 * touched.  On exit A and tau (DEVICE, n doubles) hold capi_dgeqrf's image, so further right-hand sides can follow through capi_dormqr +
 * capi_dtrsm_thin; rows 0 .. n - 1 of B (m x r, ldb >= m) hold X, rows n .. m - 1 the tail of Q^T B; colnorm2 (DEVICE, r doubles, or NULL) receives the
 * squared residual norms, the column sums of squares of that tail (zeros when m == n).  *info_host is 0, or the 1-based index of the first diagonal
 * entry of R that is exactly zero or not finite: B is then left as Q^T B, no solve is done and colnorm2 is not written (rank-deficient problems:
 * capi_dgelsy below, or qr::cacqr::factor_pivoted on the Gram matrix).  The steps: capi_dgeqrf (CholeskyQR2 + reconstruction or the Householder panels, by its own choice),
 * capi_dormqr(CAPI_LEFT, CAPI_TRANS), a one-workgroup scan of R's diagonal, capi_dtrsm_thin(CAPI_NOTRANS) on R in place in A in column blocks of at most
 * CAPI_TS_MAX_RHS (substitution, no inverse), capi_dcolnorm2 on the tail.  Reading *info_host is the call's own stream synchronisation (capi_dgeqrf
 * has its own). */
int capi_dgels(capi_handle_t h, int64_t m, int64_t n, int64_t r, double* A, int64_t lda, double* tau, double* B, int64_t ldb, double* colnorm2,
               int* info_host);
/* capi_dgeqp3: QR with column pivoting of a small block, W P = Q R, LAPACK's dgeqp3 in dlaqp2's unblocked form: the rank-revealing step of capi_dgelsy,
 * run on the n x n triangle that capi_dgeqrf leaves (pivoted QR of R1 itself resolves rank down to u ||A||, where the Gram route of capi_dpstrf stops at
 * sqrt(u)).  Not in the reference: lapack/interface.h declares _geqrf and _orgqr only.  W is mr x n, column-major, DEVICE, ldw >= mr,
 * 1 <= mr, n <= CAPI_GEQP3_MAX.  On exit W holds the image of W P in LAPACK storage: with k the rank, rows < k of the upper trapezoid hold R, below the
 * diagonal of columns < k lie the reflectors (unit first entry implied); tau (DEVICE, min(mr, n) doubles) has tau[j] = 0 for j >= k; jpvt (DEVICE, n
 * ints, 0-based) is always a full permutation: column j of W P is column jpvt[j] of the input (capi_dpstrf's convention).  *rank_host = k; reading it
 * ends the call (the stream is also synchronised once per round of 64 steps, to read a 4-byte stop flag: the only host traffic).  A null handle
 * returns -1; any other bad argument (a null operand, ldw < mr, a size out of range, a NaN rtol, W or tau not aligned to 8 bytes) returns CAPI_EINVAL
 * before any launch, with nothing touched; mr == 0 or n == 0: rank 0, nothing is launched.  The handle's info word is not touched.
 * The step rule.  Running norms vn1 = vn2 = the column norms at the start.  At step j = 0, 1, ..:
 *   pivot     p is the FIRST index, under the total order on (value, original index) -- the larger value, ties to the smaller index -- of the largest
 *             running norm vn1 among the columns not yet chosen; a NaN is entered as -inf;
 *   norm      nu = ||W(j:mr, p)||_2 is recomputed from the column itself in a fixed summation order: sqrt(alpha^2 + s2), alpha = W(j, p), s2 the sum
 *             of squares below it; nu_0 is the value at step 0;
 *   stop      the factorization stops at rank j unless nu > rtol * nu_0 && nu > 0 -- written so that a NaN compares false and stops.  rtol = 0 stops
 *             only at an exactly zero remainder; rtol < 0 means max(mr, n) 2^-52.  The rank rule is this threshold on |r_jj| = nu, NOT dgelsy's
 *             incremental condition estimator;
 *   reflector dlarfg's, without its rescaling of tiny columns: beta = -sign(alpha) nu, tau = (beta - alpha) / beta, v = x / (alpha - beta); when
 *             everything below alpha is zero (s2 == 0) it is tau = 0, beta = alpha -- the form capi_dgeqrf gives such a column;
 *   update    a_c -= tau v (v^T a_c) on rows >= j of every column not chosen; then dlaqp2's two-vector downdate of its running norm:
 *             temp = max(0, 1 - (|a_jc| / vn1)^2), temp2 = temp (vn1 / vn2)^2; temp2 <= tol3z = sqrt(2^-53): vn1 = vn2 = ||a_c(j+1:mr)||_2
 *             recomputed from the column; otherwise vn1 *= sqrt(temp).  A column with vn1 == 0 keeps it.
 * After a stop rows >= k of columns >= k keep the unreduced remainder (the columns never chosen go behind the chosen ones in ascending order of their
 * original index); its columns have norm <= rtol nu_0 up to the downdate's accuracy.  Every loop's trip count is fixed by mr and n, so non-finite
 * input ends the call like any other: CAPI_OK, 0 <= k <= min(mr, n), jpvt a permutation, the values unspecified.
 * Method (csrc/qrcp_f64.hip): swap-free, one launch per step over ceil(n / 8) workgroups of 256 threads; a wave owns two columns through the whole
 * call; every workgroup reduces the per-workgroup (value, index) candidates the launch before left and forms nu, beta, tau and v itself from the
 * read-only pivot column (v staged in LDS, 16 KiB at most), so all hold the same bits; the pivot's owner writes column j of the image to a second
 * mr x n block; a last launch pair places the columns never chosen, writes jpvt and copies the image back.  A stop sets a device flag; later launches
 * read it at entry and return.  Ordered by kernel boundaries on the handle's stream alone: no cooperative launch, no device-side waiting, no atomics;
 * sums have a fixed order: two calls on the same bits give identical bytes.  Workspace, of the handle's own: 8 mr n + 20 n + 32 ceil(n / 8) + 16 bytes. */
enum { CAPI_GEQP3_MAX = 2048 };
int capi_dgeqp3(capi_handle_t h, int64_t mr, int64_t n, double* W, int64_t ldw, int* jpvt, double* tau, double rtol, int* rank_host);
/* capi_dgelsy: LAPACK's dgelsy for m >= n >= 1, n <= CAPI_GEQP3_MAX and any r >= 1: min ||A X - B|| for A of ANY rank -- the basic solution (nonzeros
 * in the k pivot columns only) or the minimum-norm one.  Not in the reference: lapack/interface.h declares _geqrf and _orgqr only.  All pointers are
 * DEVICE pointers, aligned to 8 bytes (jpvt to 4).  Everything of size m runs on capi_dgeqrf and capi_dormqr; only the n x n triangle R1 is pivoted:
 * A = Q1 R1, R1 P = Q2 R, so A P = (Q1 Q2) R, and the rank k is read off |r_jj| > rcond |r_00| (capi_dgeqp3's rule, rcond < 0: max(m, n) 2^-52; no
 * incremental condition estimator).  The steps:
 *   1. capi_dgeqrf(A, tau): on exit the image and tau are bit for bit those of a separate capi_dgeqrf call;
 *   2. capi_dormqr(CAPI_LEFT, CAPI_TRANS) on B (m x r, ldb >= m);
 *   3. F (n x n, ldf >= n) <- triu(R1), zeros below (capi_dlacpy, capi_dtrizero);
 *   4. capi_dgeqp3(n, n, F, ldf, jpvt, tauf, rcond, &k): F, tauf (n doubles) and jpvt (n ints) as that call leaves them;
 *   5. capi_dormqr(CAPI_LEFT, CAPI_TRANS, n, r, k, F, ldf, tauf, B, ldb) on the top n rows of B;
 *   6. colnorm2 (r doubles, or NULL) <- capi_dcolnorm2 over rows k .. m - 1 of B, the squared residual norms;
 *   7. basic (min_norm == 0, or k == n): Y = R11^-1 C by capi_dtrsm_thin(CAPI_NOTRANS, k, ..) on F in column blocks of at most CAPI_TS_MAX_RHS;
 *      minimum norm (min_norm != 0 and k < n): Z (n x k, ldz >= n) <- [R11 R12]^T, capi_dgeqrf(n, k, Z, ldz, tauz), T^T y = c by
 *      capi_dtrsm_thin(CAPI_TRANS, k, ..) on Z, rows k .. n - 1 of the top block <- 0, capi_dormqr(CAPI_LEFT, CAPI_NOTRANS, n, r, k, Z, ldz, tauz, B, ldb);
 *   8. X = P Y by capi_drow_scatter through the handle's workspace (n r doubles), copied into rows 0 .. n - 1 of B.
 * On exit rows n .. m - 1 of B keep the tail of Q1^T B; *rank_host = k.  k == 0 (A zero): X = 0, colnorm2 = the squared column norms of Q1^T B,
 * CAPI_OK.  Z and tauz (k doubles, so n suffice) may be NULL iff min_norm == 0.  m < n, n > CAPI_GEQP3_MAX, a null or misaligned argument, a leading
 * dimension too small, a NaN rcond: CAPI_EINVAL before any launch, nothing is touched (as capi_dgels refuses).  The handle's info word is not touched.
 * FURTHER RIGHT-HAND SIDES on the factors left in A, tau, F, tauf, jpvt, Z and tauz, by public calls alone (capital_amd.hqr.Hqr.lstsq_pivoted):
 *   capi_dormqr(CAPI_LEFT, CAPI_TRANS, m, r, n, A, lda, tau, B, ldb); capi_dormqr(CAPI_LEFT, CAPI_TRANS, n, r, k, F, ldf, tauf, B, ldb);
 *   capi_dcolnorm2(m - k, rb, B + k, ldb, ..) per block of rb <= CAPI_TS_MAX_RHS columns; then
 *   basic:        capi_dtrsm_thin(CAPI_NOTRANS, k, rb, F, ldf, 0, B, ldb) per block; capi_drow_scatter(0, k, r, n, B, ldb, jpvt, X, ldx);
 *   minimum norm: capi_dtrsm_thin(CAPI_TRANS, k, rb, Z, ldz, 0, B, ldb) per block; rows k .. n - 1 of B <- 0;
 *                 capi_dormqr(CAPI_LEFT, CAPI_NOTRANS, n, r, k, Z, ldz, tauz, B, ldb); capi_drow_scatter(0, n, r, n, B, ldb, jpvt, X, ldx). */
int capi_dgelsy(capi_handle_t h, int64_t m, int64_t n, int64_t r, double* A, int64_t lda, double* tau, double* F, int64_t ldf, double* tauf, int* jpvt,
                double* Z, int64_t ldz, double* tauz, double* B, int64_t ldb, double rcond, int min_norm, double* colnorm2, int* rank_host);
int capi_reset_info(capi_handle_t h);

/* ---- data movement: replaces serialize<> (src/matrix/serialize.hpp:12-150), the pack/unpack and
 *      axpy loops of summa (summa.hpp:33,135,147-153,216-217) and util::remove_triangle (util.hpp:266-318) ---- */
/* sub-block copy between two (possibly packed-triangular) local layouts; ranges as in serialize<>::invoke */
int capi_serialize(capi_handle_t h, int src_struct, int dst_struct,
                   const double* src, int64_t sdimX, int64_t sdimY, double* dst, int64_t ddimX, int64_t ddimY,
                   int64_t ssx, int64_t sex, int64_t ssy, int64_t sey, int64_t dsx, int64_t dex, int64_t dsy, int64_t dey);
/* same, with the copy SHAPE (rect: whole columns, uppertri: i+1 leading entries of column i, lowertri: from the
 * diagonal down) given separately from the two storage layouts -- the reference applies serialize<uppertri,uppertri>
 * to rect-stored matrices too (cholinv.hpp:13) */
int capi_serialize_shape(capi_handle_t h, int shape, int src_struct, int dst_struct,
                         const double* src, int64_t sdimX, int64_t sdimY, double* dst, int64_t ddimX, int64_t ddimY,
                         int64_t ssx, int64_t sex, int64_t ssy, int64_t sey, int64_t dsx, int64_t dex, int64_t dsy, int64_t dey);
/* B <- A for an m x n block; part: 0 all, 1 upper triangle incl. diagonal, 2 lower incl. diagonal */
int capi_dlacpy(capi_handle_t h, int part, int64_t m, int64_t n, const double* A, int64_t lda, double* B, int64_t ldb);
/* Y(part) <- alpha*X + beta*Y on an m x n block (the beta-update after summa's Allreduce, summa.hpp:33,153) */
int capi_dgeadd(capi_handle_t h, int part, int64_t m, int64_t n, double alpha, const double* X, int64_t ldx, double beta, double* Y, int64_t ldy);
/* zero the strictly lower (uplo=Upper keeps upper) or strictly upper part of an n x n block */
int capi_dtrizero(capi_handle_t h, int keep_uplo, int64_t n, double* A, int64_t lda);
/* y <- beta*y + x over count elements (M3) */
int capi_daxpby(capi_handle_t h, int64_t count, double beta, const double* x, double* y);
/* zero by GLOBAL index parity: local (i,j) is global (px+i*P, py+j*P); dir 'U' zeroes gy>gx, 'L' zeroes gy<gx */
int capi_remove_triangle(capi_handle_t h, char dir, double* A, int64_t dimX, int64_t dimY, int64_t px, int64_t py, int64_t P);
/* element-cyclic gather/scatter of the base case (util.hpp:56-230): pieces[r] (r = x*d + y... see DESIGN.md)
 * are d*d local blocks of rows_local x cols_local; cyclic is the (rows_local*d) x (cols_local*d) aggregate */
int capi_block_to_cyclic(capi_handle_t h, const double* blocked, double* cyclic, int64_t rows_local, int64_t cols_local, int64_t d);
int capi_cyclic_to_block(capi_handle_t h, double* blocked, const double* cyclic, int64_t rows_local, int64_t cols_local, int64_t d);
/* the same assembly for an OFF-diagonal aggregate (the R12 block a grid solves in TRSM mode): no part of it is zeroed */
int capi_block_to_cyclic_full(capi_handle_t h, const double* blocked, double* cyclic, int64_t rows_local, int64_t cols_local, int64_t d);
/* the same for PACKED upper-triangular pieces of rows_local (rows_local + 1) / 2 doubles each (util::block_to_cyclic_triangle /
 * cyclic_to_block_triangle, util.hpp:57-102,167-201: the Serialize policy's base-case messages, policy.h:176,322-377) */
int capi_block_to_cyclic_tri(capi_handle_t h, const double* blocked_packed, double* cyclic, int64_t rows_local, int64_t d);
int capi_cyclic_to_block_tri(capi_handle_t h, double* blocked_packed, const double* cyclic, int64_t rows_local, int64_t d);
/* util::cyclic_to_local (util.hpp:131-164): slice rank `slice_rank`'s element-cyclic piece of the aggregated factor T and of its
 * inverse TI (bc_dim x bc_dim each) into their leading local_dim x local_dim corners (ld stays bc_dim), zero below the global diagonal */
int capi_cyclic_to_local(capi_handle_t h, double* T, double* TI, int64_t local_dim, int64_t bc_dim, int64_t d, int64_t slice_rank);

/* ---- generators: replaces rect::_distribute_* (src/matrix/structure.hpp:36-129), bit-identical output ---- */
int capi_distribute_symmetric(capi_handle_t h, double* data, int64_t dimX, int64_t dimY, int64_t gdimX, int64_t gdimY,
                              int64_t px, int64_t py, int64_t PX, int64_t PY, int64_t key, int diag_dominant);
int capi_distribute_random(capi_handle_t h, double* data, int64_t dimX, int64_t dimY, int64_t gdimX, int64_t gdimY,
                           int64_t px, int64_t py, int64_t PX, int64_t PY, int64_t key);
int capi_distribute_identity(capi_handle_t h, double* data, int64_t dimX, int64_t dimY, int64_t gdimX, int64_t gdimY,
                             int64_t px, int64_t py, int64_t PX, int64_t PY, double val);

/* ---- residual reductions: replaces util::residual_local's local sums (src/util/util.hpp:25-53) ---- */
/* out[0] = sum (X[i]-Y[i])^2 over the selected part, out[1] = sum Y[i]^2; part as capi_dlacpy; out is HOST memory (synchronous) */
int capi_diff_norms(capi_handle_t h, int part, int64_t m, int64_t n, const double* X, int64_t ldx, const double* Y, int64_t ldy, double* out2);

/* ---- collectives: replaces the MPI calls of summa/util/policy (C1-C10) with RCCL on the
 *      handle's stream.  A communicator is created from a 128-byte RCCL unique id that rank 0 obtains with
 *      capi_comm_unique_id() and the launcher ships to the other ranks (torch.distributed store, MPI, a file). ---- */
int capi_comm_load_rccl(const char* librccl_path);              /* optional: choose the librccl.so to bind (default: search) */
int capi_comm_unique_id(void* id128);
int capi_comm_init_rank(capi_comm_t* comm, capi_handle_t h, int nranks, const void* id128, int rank);
int capi_comm_split(capi_comm_t parent, int color, int key, capi_comm_t* child);       /* MPI_Comm_split, topology.h:28-59,84-138; color < 0 = MPI_UNDEFINED: *child = NULL */
int capi_comm_query(capi_comm_t c, int* rank, int* size);                              /* rank and size as RCCL itself reports them */
int capi_comm_rank(capi_comm_t c, int* rank);
int capi_comm_size(capi_comm_t c, int* size);
int capi_comm_destroy(capi_comm_t c);
int capi_bcast(capi_comm_t c, double* buf, int64_t count, int root);                   /* MPI_Bcast, summa.hpp:185,193 */
int capi_allreduce_sum(capi_comm_t c, double* buf, int64_t count);                     /* MPI_Allreduce(IN_PLACE,SUM), summa.hpp:236 */
int capi_reduce_sum(capi_comm_t c, const double* send, double* recv, int64_t count, int root);  /* MPI_Reduce, cacqr.hpp:98 */
int capi_allgather(capi_comm_t c, const double* send, double* recv, int64_t count_per_rank);   /* MPI_Allgather, policy.h:176 */
int capi_sendrecv_replace(capi_comm_t c, double* buf, int64_t count, int peer, double* staging); /* MPI_Sendrecv_replace, util.hpp:240 */
/* Grid-wide set of pair transfers over ALL xGMI links of the node (csrc/pair_paths.h).  The pair collectives of the 3-D SUMMA on a
 * 2 x 2 x 2 grid -- MPI_Bcast over a row / column of two (summa.hpp:185,193), the halves of MPI_Allreduce over a depth fibre of two
 * (summa.hpp:236), MPI_Sendrecv_replace with the transpose partner (util.hpp:240) -- each move 1-2 GiB between two GPUs; as calls on
 * 2-rank communicators they use one of the sender's seven links.  Here every rank of `world` calls with the SAME dst[0..size): rank r
 * sends `count` doubles from `send` to rank dst[r] (dst[r] < 0: sends nothing); a rank is the destination of at most one transfer and
 * receives into `recv`.  Long messages are cut into `size` units: two travel directly, the others are relayed by the remaining ranks
 * (two grouped rounds of ncclSend/ncclRecv) through `scratch`, capi_pairs_scratch_count(size, count) doubles on every rank. */
int64_t capi_pairs_scratch_count(int nranks, int64_t count);
int capi_pairs_transfer(capi_comm_t world, const int* dst, const double* send, double* recv, int64_t count, double* scratch);
/* root collects / deals `count_per_rank` doubles per rank, rank r's piece at recv/send + r*count (one group of RCCL send/recv) */
int capi_gather(capi_comm_t c, const double* send, double* recv, int64_t count_per_rank, int root);   /* MPI_Gather, cholinv/policy.h:322-332 */
int capi_scatter(capi_comm_t c, const double* send, double* recv, int64_t count_per_rank, int root);  /* MPI_Scatter / MPI_Iscatter, policy.h:361-377,470-488 */

/* ---- extra streams + events: lets the host layer run collectives beside the tile kernel (the reference's
 *      MPI_Ibcast/Iallreduce chunk pipeline, summa.hpp:195-215,238-249) and copies or packing beside a factorisation.
 *      capi_stream_select(h, i) routes every following call on this handle (kernels, copies, collectives) to stream i:
 *      0 = compute stream, 1 = communication / packing stream; any other index is CAPI_EINVAL.  Each stream index has its
 *      own private workspace; events order work across streams (slot in [0, 1024)). ---- */
int capi_stream_select(capi_handle_t h, int which);
int capi_event_record(capi_handle_t h, int slot);   /* on the currently selected stream */
int capi_event_wait(capi_handle_t h, int slot);     /* the currently selected stream waits for that record */

/* ---- measurement helpers ---- */
/* register-resident v_mfma_f64_16x16x4_f64 loop on every CU: returns achieved TFLOP/s (synchronous) */
int capi_mfma_f64_peak(capi_handle_t h, int iters, double* tflops);
/* HIP-event bracket around EVERY launch of the MFMA tile kernel on the handle's stream (roofline measurement):
 * enable, run the workload, collect = number of launches, summed duration and summed algorithmic flops of one
 * kernel variant (0..3 = operand orientations at any tile size, 3 = both operands k-contiguous, the TN kernel of the
 * trailing update; 8 + v = exactly variant v, where bit 2 of v marks the 64-tile kernel: 11 = the 128-tile TN kernel
 * alone, i.e. one kernel symbol; 8 + 16 + v = dtrmm_pair_kernel (the 128-tile kernel's form for TRMMs in tile pairs) of orientation v; 100 + o = both 128-tile symbols of operand
 * orientation o; -1 = all variants). */
int capi_prof_enable(capi_handle_t h, int on);
int capi_prof_collect(capi_handle_t h, int variant, int64_t* launches, double* total_ms, double* total_flops, double* max_ms);
/* the same records timed by the kernels themselves (first workgroup's start .. last workgroup's end, wall-clock ticks): *union_ms = length
 * of the union of the selected launches' execution intervals, *sum_ms their sum.  Robust to launches of several streams interleaving. */
int capi_prof_collect_intervals(capi_handle_t h, int variant, int64_t* launches, double* union_ms, double* sum_ms, double* total_flops, double* max_ms);
/* phase markers: the reference's CRITTER_START/STOP(sym) regions (src/util/shared.h:26-35; cholinv.hpp:94-158, cacqr.hpp:82-116)
 * as roctx ranges for `rocprofv3 --marker-trace`; no-ops when no roctx library can be bound */
int capi_range_push(const char* name);
int capi_range_pop(void);
/* HIP-event timer on the handle's stream */
int capi_timer_start(capi_handle_t h);
int capi_timer_stop_ms(capi_handle_t h, float* ms);              /* synchronises */

#ifdef __cplusplus
}
#endif
#endif /* CAPITAL_HIP_H_ */
