// alg/matmult/summa/summa.h -- 3-D SUMMA on the GPUs of one node (reference src/alg/matmult/summa/summa.h:24-34,
// summa.hpp:6-254).
//
// Same four invoke() overloads keyed on the blas ArgPack.  Per multiply, rank (x,y,z) of a d x d x c grid receives the
// A panel of the row-root and the B panel of the column-root of K-class q, multiplies locally on the MFMA tile kernel
// and sums the partial products over `depth`:
//     C1 MPI_Bcast(row)  -> capi_bcast(row)      C2 MPI_Bcast(column) -> capi_bcast(column)
//     K1/K4 cblas_dgemm / cblas_dtrmm -> capi_dgemm / capi_dgemmt / capi_dtrmm_acc
//     C3 MPI_Allreduce(depth) -> capi_allreduce_sum(depth)      M3 beta-axpy -> capi_dgeadd
// Differences from the reference, all behind the same results:
//   * operands are "views" (pointer, leading dimension) into device-resident blocks, so at d == c == 1 the multiply
//     runs in place with no packing, zero-fill or axpy passes at all;
//   * the trailing update only computes the triangle that is used (capi_dgemmt) instead of a full GEMM
//     (summa.hpp:115-146 runs cblas_dgemm and repacks);
//   * any c dividing d is accepted: layer z owns K-classes q = z, z+c, ... (the reference needs c == d);
//     d == 1 with c > 1 slices the local K range instead (pure replication, used for the 2-GPU grid).
// With num_chunks > 0 the collectives of a multiply overlap its tile kernels, column chunk by column chunk.  That pipeline is built
// once (struct chunks, struct pipe, stream_chunks, depth_sum: see the table in front of them); gemm, trmm and syrk supply their whole
// operand and their local products per chunk.  The unpiped branches and colsplit_run keep schedules of their own.
#ifndef CAPITAL_MATMULT_SUMMA_H_
#define CAPITAL_MATMULT_SUMMA_H_

#include "./../../alg.h"

namespace matmult {

// contiguous device scratch handed out stack-wise; sized once per factorisation (the reference's simulate() tables)
struct arena {
  double* base = nullptr;
  int64_t cap = 0, top = 0;
  arena() = default;
  arena(const arena&) = delete;                 // owns device memory: a copy would free it twice, an assignment would leak it
  arena& operator=(const arena&) = delete;
  arena(arena&& o) noexcept : base(o.base), cap(o.cap), top(o.top) { o.base = nullptr; o.cap = o.top = 0; }
  arena& operator=(arena&& o) noexcept {
    if (this != &o) { release(); base = o.base; cap = o.cap; top = o.top; o.base = nullptr; o.cap = o.top = 0; }
    return *this;
  }
  ~arena() { release(); }
  void release() { capital::dev_free(base); base = nullptr; cap = top = 0; }
  void reserve(int64_t count) {
    if (count > cap) {
      capital::sync();
      release();                                // (an allocation that throws must not leave the freed block behind)
      base = capital::dev_alloc(count);
      cap = count;
    }
    top = 0;
  }
  double* take(int64_t count) {
    count = (count + 1) & ~(int64_t)1;  // keep 16-byte alignment
    if (top + count > cap) throw std::runtime_error("matmult::arena exhausted (sizing rule out of date)");
    double* p = base + top;
    top += count;
    return p;
  }
};

struct view {
  double* p;
  int64_t ld, rows, cols;
  bool contiguous() const { return ld == rows; }
  int64_t count() const { return rows * cols; }
};

class summa {
public:
  // ---- public overloads on matrix<> objects (summa.h:24-34) ------------------------------------------------------
  template <typename MatrixAType, typename MatrixBType, typename MatrixCType, typename CommType>
  static void invoke(MatrixAType& A, MatrixBType& B, MatrixCType& C, CommType&& CommInfo, blas::ArgPack_gemm<typename MatrixAType::ScalarType>& pack) {
    static_assert(std::is_same<typename MatrixAType::StructureType, rect>::value && std::is_same<typename MatrixBType::StructureType, rect>::value &&
                      std::is_same<typename MatrixCType::StructureType, rect>::value,
                  "summa gemm works on rect blocks (the reference's callers only pass rect: cacqr.hpp:62, validate.hpp)");
    arena& ws = scratch_arena();
    if (!(CommInfo.d == 1 && CommInfo.c == 1)) ws.reserve(2 * (A.num_elems() + B.num_elems() + C.num_elems()) + 64);
    gemm(CommInfo, (int)pack.transposeA, (int)pack.transposeB, pack.alpha, as_view(A), as_view(B), pack.beta, as_view(C), ws);
  }
  // B <- alpha * op(A) * B  or  alpha * B * op(A), A triangular (summa.hpp:46-83)
  template <typename MatrixAType, typename MatrixBType, typename CommType>
  static void invoke(MatrixAType& A, MatrixBType& B, CommType&& CommInfo, blas::ArgPack_trmm<typename MatrixAType::ScalarType>& pack) {
    static_assert(std::is_same<typename MatrixAType::StructureType, rect>::value && std::is_same<typename MatrixBType::StructureType, rect>::value,
                  "packed operands are unpacked by the algorithm layer before they reach the device summa");
    arena& ws = scratch_arena();
    ws.reserve(3 * A.num_elems() + 4 * B.num_elems() + 64);
    view out{ws.take(B.num_elems()), B.num_rows_local(), B.num_rows_local(), B.num_columns_local()};
    trmm(CommInfo, (int)pack.side, (int)pack.uplo, (int)pack.transposeA, (int)pack.diag, pack.alpha, as_view(A), as_view(B), out, ws);
    capital::dev_copy(B.data(), out.p, B.num_elems());
  }
  // C <- alpha * A^T A + beta * C (or A A^T), summa.hpp:85-96: the second operand is the partner-exchanged copy of A
  template <typename MatrixSrcType, typename MatrixDestType, typename CommType>
  static void invoke(MatrixSrcType& A, MatrixDestType& C, CommType&& CommInfo, blas::ArgPack_syrk<typename MatrixSrcType::ScalarType>& pack) {
    MatrixSrcType B = A;
    invoke(A, B, C, CommInfo, pack);
  }
  // summa.hpp:98-109: B is exchanged with the transpose partner, then the triangular-output multiply
  template <typename MatrixSrcType, typename MatrixDestType, typename CommType>
  static void invoke(MatrixSrcType& A, MatrixSrcType& B, MatrixDestType& C, CommType&& CommInfo, blas::ArgPack_syrk<typename MatrixSrcType::ScalarType>& pack) {
    static_assert(std::is_same<typename MatrixSrcType::StructureType, rect>::value && std::is_same<typename MatrixDestType::StructureType, rect>::value,
                  "packed operands are unpacked by the algorithm layer before they reach the device summa");
    util::transpose(B, CommInfo);
    arena& ws = scratch_arena();
    ws.reserve(2 * (A.num_elems() + B.num_elems() + C.num_elems()) + 64);
    syrk(CommInfo, (int)pack.uplo, (int)pack.transposeA, pack.alpha, as_view(A), as_view(B), pack.beta, as_view(C), ws);
  }

  // ---- view-level engine (used directly by cholinv / cacqr) ---------------------------------------------------------
  // C <- alpha*op(A)*op(B) + beta*C.  Operand blocks are the LOCAL blocks of this rank; roots are chosen per K-class.
  // With num_chunks > 0 (op(B) = B) the chunk pipeline below: A whole, B and the product column chunk by column chunk.
  template <typename CommType>
  static void gemm(CommType&& t, int transA, int transB, double alpha, view A, view B, double beta, view C, arena& ws) {
    capi_handle_t h = capital::handle();
    const int64_t M = C.rows, N = C.cols, K = transA ? A.rows : A.cols;
    if (t.d == 1 && t.c == 1) {
      CAPITAL_CHECK(capi_dgemm(h, transA, transB, M, N, K, alpha, A.p, A.ld, B.p, B.ld, beta, C.p, C.ld));
      return;
    }
    if (t.d == 1 && colsplit() && transB == CAPI_NOTRANS) {
      // replicated layers: layer z forms C[:, b_z : b_z+1) = alpha op(A) B[:, b_z : b_z+1) + beta C[:, ...) in place, then the blocks travel
      colsplit_run(t, N, false, C.p, C.ld,
                   [&](int64_t c0, int64_t c1) {
                     CAPITAL_CHECK(capi_dgemm(h, transA, CAPI_NOTRANS, M, c1 - c0, K, alpha, A.p, A.ld, B.p + c0 * B.ld, B.ld, beta, C.p + c0 * C.ld, C.ld));
                   },
                   [&](int64_t) { return M; }, ws);
      return;
    }
    const int64_t mark = ws.top;
    view acc = t.c > 1 ? view{ws.take(M * N), M, M, N} : C;
    const size_t steps = t.d > 1 ? t.d / t.c : 1;
    const bool piped = t.num_chunks > 0 && transB == CAPI_NOTRANS && (t.d > 1 || t.c > 1);
    const chunks plan{N, piped ? chunk_count(t.num_chunks, N) : 1};
    pipe P(piped && plan.nch > 1);
    if (!P.on) {
      if (t.d == 1) {
        // pure replication: layer z multiplies its slice of the local K range
        int64_t k0, k1;
        kslice(K, t.c, t.z, k0, k1);
        const double* a = transA ? A.p + k0 : A.p + k0 * A.ld;
        const double* b = transB ? B.p + k0 * B.ld : B.p + k0;
        CAPITAL_CHECK(capi_dgemm(h, transA, transB, M, N, k1 - k0, alpha, a, A.ld, b, B.ld, 0.0, acc.p, acc.ld));
      } else {
        for (size_t s = 0; s < steps; ++s) {
          view a = panel(t, AX_ROW, s, A, ws), b = panel(t, AX_COLUMN, s, B, ws);
          const double bt = (t.c > 1) ? (s ? 1.0 : 0.0) : (s ? 1.0 : beta);
          CAPITAL_CHECK(capi_dgemm(h, transA, transB, M, N, K, alpha, a.p, a.ld, b.p, b.ld, bt, acc.p, acc.ld));
        }
      }
      if (t.c > 1) {
        allreduce_view(t, acc, ws);
        CAPITAL_CHECK(capi_dgeadd(h, 0, M, N, 1.0, acc.p, acc.ld, beta, C.p, C.ld));
      }
      ws.top = mark;
      return;
    }
    // ---- pipelined over the output's column chunks; every K-class step s of this layer contributes to every chunk
    //      (d == 1: nothing travels before the depth sum, layer z multiplies its slice [k0,k1) of the local K range)
    const bool sliced = (t.d == 1);
    int64_t k0 = 0, k1 = K;
    if (sliced) kslice(K, t.c, t.z, k0, k1);
    std::vector<view> a(steps, A);
    P.begin();
    if (!sliced)
      for (size_t s = 0; s < steps; ++s) a[s] = panel(t, AX_ROW, s, A, ws);
    P.whole_sent();
    double* relay = relay_space(t, std::max(B.rows, acc.rows) * plan.widest(), ws);      // (one buffer for stages 3 and 5)
    const std::vector<view> b = stream_chunks(t, P, AX_COLUMN, sliced ? 0 : steps, B, plan, relay, ws);
    P.resume();
    P.products(plan, [&](int j, int64_t c0, int64_t c1) {
      P.wait(EB + j);
      for (size_t s = 0; c1 > c0 && s < steps; ++s) {
        const double bt = s ? 1.0 : (t.c > 1 ? 0.0 : beta);
        const double* ap = sliced ? (transA ? a[s].p + k0 : a[s].p + k0 * a[s].ld) : a[s].p;
        CAPITAL_CHECK(capi_dgemm(h, transA, CAPI_NOTRANS, M, c1 - c0, k1 - k0, alpha, ap, a[s].ld, b[s].p + k0 + c0 * b[s].ld, b[s].ld, bt,
                                 acc.p + c0 * acc.ld, acc.ld));
      }
    });
    depth_sum(t, P, plan, acc, [&](int64_t) { return acc.rows; }, relay, ws);
    if (t.c > 1) CAPITAL_CHECK(capi_dgeadd(h, 0, M, N, 1.0, acc.p, acc.ld, beta, C.p, C.ld));
    ws.top = mark;
  }

  // ---- the column-chunk pipeline (num_chunks > 0; the reference's MPI_Ibcast/MPI_Iallreduce chunking, summa.hpp:195-215,238-249) ----
  // The collectives of a multiply run on the handle's communication stream beside the tile kernel on the compute stream:
  // bcast of chunk j+1 || MFMA on chunk j || depth all-reduce of chunk j-1.  gemm, trmm and syrk share every stage but the fourth:
  //   1  pipe::begin      the communication stream joins the compute stream (E0)
  //   2  (the multiply), pipe::whole_sent   its "whole" operand travels first: the A panels / the packed T panels / the exchanged L
  //                       panels of every step, then EW
  //   3  stream_chunks    the other operand travels by column chunks, every K-class step of a chunk, then EB + j
  //   4  pipe::resume, pipe::products   compute stream: behind EW, per chunk the multiply's callable -- its wait for EB + j and its local
  //                       products summed over the steps --, then EC + j
  //   5  depth_sum        c > 1: communication stream, per chunk behind EC + j a depth all-reduce of the chunk, then ER, which the compute
  //                       stream awaits
  // Host calls are issued in an order that is also valid when executed sequentially.

  // how N columns are cut into nch chunks (multiples of 2 columns keep 16-byte alignment; trailing chunks can be empty)
  struct chunks {
    int64_t N;
    int nch;
    struct span {
      int64_t c0, c1;
      bool empty() const { return c1 <= c0; }
      int64_t width() const { return c1 - c0; }
    };
    span range(int j) const {
      const int64_t per = ((N + nch - 1) / nch + 1) & ~(int64_t)1;
      const int64_t c0 = std::min<int64_t>(N, per * j);
      return span{c0, std::min<int64_t>(N, c0 + per)};
    }
    int64_t widest() const { return range(0).width(); }          // (every chunk in front of the last non-empty one has the full width)
    template <typename F>
    void each(F&& f) const {                                     // f(j, c0, c1) for the non-empty chunks
      for (int j = 0; j < nch; ++j) {
        const span r = range(j);
        if (!r.empty()) f(j, r.c0, r.c1);
      }
    }
  };
  struct pipe {
    // event slots of one multiply, counted from its rolling base: EW = the whole operand, EB + j / EC + j = chunk j has arrived / is
    // computed, ER = the depth sum.  (cholinv.h's own events sit at 1000 and above.)
    enum { E0 = 0, EW = 1, EB = 2, EC = 70, ER = 140, MAX_CHUNKS = 64, SLOTS = 256, BASES = 4 };
    static_assert(EB + MAX_CHUNKS <= EC && EC + MAX_CHUNKS <= ER && ER < SLOTS && SLOTS * (BASES - 1) + ER < 1000,
                  "at most MAX_CHUNKS chunks fit between the slots, and every base + slot stays below cholinv.h's events");
    capi_handle_t h;
    bool on;
    int base;
    explicit pipe(bool enable) : h(capital::handle()), on(enable) {
      static CAPITAL_RANK_LOCAL int next = 0;
      base = next;
      next = (next + SLOTS) % (SLOTS * BASES);
    }
    void comm() { if (on) CAPITAL_CHECK(capi_stream_select(h, 1)); }
    void main() { if (on) CAPITAL_CHECK(capi_stream_select(h, 0)); }
    void rec(int s) { if (on) CAPITAL_CHECK(capi_event_record(h, base + s)); }
    void wait(int s) { if (on) CAPITAL_CHECK(capi_event_wait(h, base + s)); }
    // stage 1: what follows runs on the communication stream, behind everything enqueued so far
    void begin() { main(); rec(E0); comm(); wait(E0); }
    // stage 2 is complete: the whole operand has been enqueued
    void whole_sent() { rec(EW); }
    // stage 4: back on the compute stream, behind the whole operand ...
    void resume() { main(); wait(EW); }
    // ... and per chunk: local(j, c0, c1) waits for the chunk's arrival -- its first statement is the wait for EB + j, the consumer side of
    // stream_chunks' record, kept beside the products that read the chunk (the negative test of tests/test_gpu_multirank.py builds the
    // host layer without exactly these lines) -- and enqueues the chunk's products unless the chunk is empty; its completion is recorded here
    template <typename Local>
    void products(const chunks& plan, Local&& local) {
      for (int j = 0; j < plan.nch; ++j) {
        const chunks::span r = plan.range(j);
        local(j, r.c0, r.c1);
        rec(EC + j);
      }
    }
  };
  static constexpr int EB = pipe::EB;                            // (the name under which the multiplies wait for chunk j)
  static int chunk_count(size_t num_chunks, int64_t cols) {
    // (a chunk costs two cross-stream hand-offs -- event record on one HIP stream, wait on the other: tens of microseconds between two
    //  hardware queues, measured in round 3 --, so it has to carry work in the 100-microsecond range: 512 columns; tests shrink it)
    static const int64_t min_cols = getenv("CAPITAL_MIN_CHUNK_COLS") ? std::max(2, atoi(getenv("CAPITAL_MIN_CHUNK_COLS"))) : 512;
    int n = (int)std::min<int64_t>((int64_t)std::min<size_t>(num_chunks, pipe::MAX_CHUNKS), std::max<int64_t>(cols / min_cols, 1));
    return n < 1 ? 1 : n;
  }
  // stage 3, on the communication stream: `src` travels along `axis` column chunk by column chunk, for every one of the layer's `steps`
  // K-class steps.  Returns where step s of it lands (the root's own block if that is contiguous).  steps == 0: every layer holds src
  // already (d == 1), only the events are recorded.  The landing views and `relay` (sized for src.rows * plan.widest()) must stay
  // allocated until the multiply's last event.
  template <typename CommType>
  static std::vector<view> stream_chunks(CommType&& t, pipe& P, int axis, size_t steps, const view& src, const chunks& plan, double* relay, arena& ws) {
    std::vector<view> land(std::max<size_t>(steps, 1), src);
    for (size_t s = 0; s < steps; ++s) land[s] = landing(is_root(t, axis, s), src, ws);
    for (int j = 0; j < plan.nch; ++j) {
      const chunks::span r = plan.range(j);
      if (!r.empty())
        for (size_t s = 0; s < steps; ++s) {
          stage(is_root(t, axis, s), src, land[s], r.c0, r.c1);
          bcast_axis(t, axis, s, land[s].p + r.c0 * land[s].ld, land[s].rows * r.width(), relay);
        }
      P.rec(pipe::EB + j);
    }
    return land;
  }
  // stage 5: the sum over depth of the accumulator's column chunks, each behind its products; of chunk [c0,c1) the leading rows_of(c1)
  // rows travel (all of them, or c1 for an upper-triangular output).  `relay` sized for acc.rows * plan.widest().  Ends on the compute stream.
  template <typename CommType, typename RowsOf>
  static void depth_sum(CommType&& t, pipe& P, const chunks& plan, const view& acc, RowsOf&& rows_of, double* relay, arena& ws) {
    if (t.c == 1) { P.main(); return; }
    P.comm();
    double* half = depth_space(t, acc.rows * plan.widest(), ws);
    for (int j = 0; j < plan.nch; ++j) {
      const chunks::span r = plan.range(j);
      P.wait(pipe::EC + j);
      if (!r.empty()) allreduce_view(t, view{acc.p + r.c0 * acc.ld, acc.ld, rows_of(r.c1), r.width()}, half, relay, ws);
    }
    P.rec(pipe::ER);
    P.main(); P.wait(pipe::ER);
  }

  // Cout <- alpha*op(T)*B (Left) or alpha*B*op(T) (Right); T is this rank's block of a triangular matrix.
  // Left: T travels along `row`, B along `column`; Right: B along `row`, T along `column` (summa.hpp:59-71).
  // Cout must be contiguous (ld == rows) when the grid has more than one rank.
  template <typename CommType>
  static void trmm(CommType&& t, int side, int uplo, int trans, int diag, double alpha, view T, view B, view Cout, arena& ws) {
    capi_handle_t h = capital::handle();
    const int64_t M = B.rows, N = B.cols;
    if (t.d == 1 && t.c == 1) {
      CAPITAL_CHECK(capi_dtrmm_oop(h, side, uplo, trans, diag, M, N, alpha, T.p, T.ld, B.p, B.ld, Cout.p, Cout.ld));
      return;
    }
    const bool eff_upper = (uplo == CAPI_UPPER) != (trans == CAPI_TRANS);
    if (t.d == 1 && colsplit() && (side == CAPI_LEFT || (eff_upper && trans == CAPI_NOTRANS))) {
      // replicated layers, by output columns.  Left: Cout[:, cols] = alpha op(T) B[:, cols].  Right with an upper, untransposed T: column j
      // of the product only meets rows <= j of T: Cout[:, c0:c1) = alpha ( B[:, 0:c0) T[0:c0, c0:c1) + B[:, c0:c1) T[c0:c1, c0:c1) )
      colsplit_run(t, N, side == CAPI_RIGHT, Cout.p, Cout.ld,
                   [&](int64_t c0, int64_t c1) {
                     double* Cj = Cout.p + c0 * Cout.ld;
                     if (side == CAPI_LEFT) {
                       CAPITAL_CHECK(capi_dtrmm_oop(h, side, uplo, trans, diag, M, c1 - c0, alpha, T.p, T.ld, B.p + c0 * B.ld, B.ld, Cj, Cout.ld));
                     } else {
                       if (c0 > 0)
                         CAPITAL_CHECK(capi_dgemm(h, CAPI_NOTRANS, CAPI_NOTRANS, M, c1 - c0, c0, alpha, B.p, B.ld, T.p + c0 * T.ld, T.ld, 0.0, Cj, Cout.ld));
                       CAPITAL_CHECK(capi_dtrmm_acc(h, side, uplo, trans, diag, M, c1 - c0, alpha, T.p + c0 + c0 * T.ld, T.ld, B.p + c0 * B.ld, B.ld,
                                                    c0 > 0 ? 1.0 : 0.0, Cj, Cout.ld));
                     }
                   },
                   [&](int64_t) { return M; }, ws);
      return;
    }
    const int64_t mark = ws.top;
    const size_t steps = t.d > 1 ? t.d / t.c : 1;
    // The output-column pipeline serves every left multiply, and the right multiply with an upper, untransposed T (the inverse
    // completion, cholinv.hpp:150-154; cacqr.hpp:108-112) -- there column chunk j of the output needs B's column chunks 0..j, which
    // arrive in that order.
    const bool piped_left = side == CAPI_LEFT;
    const bool piped_right = side == CAPI_RIGHT && eff_upper && trans == CAPI_NOTRANS && t.d > 1;
    const bool piped = t.num_chunks > 0 && (piped_left || piped_right) && Cout.contiguous();
    const chunks plan{N, piped ? chunk_count(t.num_chunks, N) : 1};
    pipe P(piped && plan.nch > 1);
    double* relay = nullptr;                                     // (B and Cout are M x N: one buffer for stages 3 and 5)
    if (t.d == 1) {
      // K-slice [k0,k1) of a triangular operand: a triangle on the diagonal plus a rectangle beside it.  Nothing travels before the
      // depth sum, so of the pipeline only stage 5 runs (left multiply), behind the EC + j recorded here.
      const int64_t K = T.rows;
      int64_t k0, k1;
      kslice(K, t.c, t.z, k0, k1);
      if (P.on) relay = relay_space(t, M * plan.widest(), ws);
      plan.each([&](int j, int64_t c0, int64_t c1) {
        const int64_t nc = c1 - c0;
        if (side == CAPI_LEFT) {
          const double* Bj = B.p + c0 * B.ld;
          double* Cj = Cout.p + c0 * Cout.ld;
          CAPITAL_CHECK(capi_dgeadd(h, 0, M, nc, 0.0, Cj, Cout.ld, 0.0, Cj, Cout.ld));   // Cj = 0
          if (k1 > k0) {
            const double* Tkk = T.p + k0 + k0 * T.ld;
            // rows of op(T) that see K-columns [k0,k1): the diagonal block rows and, above (eff upper) or below them, a rectangle
            CAPITAL_CHECK(capi_dtrmm_oop(h, side, uplo, trans, diag, k1 - k0, nc, alpha, Tkk, T.ld, Bj + k0, B.ld, Cj + k0, Cout.ld));
            const int64_t r0 = eff_upper ? 0 : k1, r1 = eff_upper ? k0 : K;
            if (r1 > r0) {
              // E[r0:r1, k0:k1] = trans ? T[k0:k1, r0:r1]^T : T[r0:r1, k0:k1]
              const double* Tr = trans ? T.p + k0 + r0 * T.ld : T.p + r0 + k0 * T.ld;
              CAPITAL_CHECK(capi_dgemm(h, trans, CAPI_NOTRANS, r1 - r0, nc, k1 - k0, alpha, Tr, T.ld, Bj + k0, B.ld, 0.0, Cj + r0, Cout.ld));
            }
          }
          P.rec(pipe::EC + j);                   // (by hand: pipe::products would wait for an EB + j that nobody records here)
        } else {                                                                         // (never chunked: one pass over all of N)
          CAPITAL_CHECK(capi_dgeadd(h, 0, M, N, 0.0, Cout.p, Cout.ld, 0.0, Cout.p, Cout.ld));
          if (k1 > k0) {
            const double* Tkk = T.p + k0 + k0 * T.ld;
            CAPITAL_CHECK(capi_dtrmm_oop(h, side, uplo, trans, diag, M, k1 - k0, alpha, Tkk, T.ld, B.p + k0 * B.ld, B.ld, Cout.p + k0 * Cout.ld, Cout.ld));
            const int64_t q0 = eff_upper ? k1 : 0, q1 = eff_upper ? K : k0;
            if (q1 > q0) {
              // E[k0:k1, q0:q1] = trans ? T[q0:q1, k0:k1]^T : T[k0:k1, q0:q1]
              const double* Tr = trans ? T.p + q0 + k0 * T.ld : T.p + k0 + q0 * T.ld;
              CAPITAL_CHECK(capi_dgemm(h, CAPI_NOTRANS, trans, M, q1 - q0, k1 - k0, alpha, B.p + k0 * B.ld, B.ld, Tr, T.ld, 0.0, Cout.p + q0 * Cout.ld, Cout.ld));
            }
          }
        }
      });
    } else if (!P.on) {
      for (size_t s = 0; s < steps; ++s) {
        view tt, bb;
        if (side == CAPI_LEFT) { tt = panel_tri(t, AX_ROW, s, T, uplo, ws); bb = panel(t, AX_COLUMN, s, B, ws); }
        else { bb = panel(t, AX_ROW, s, B, ws); tt = panel_tri(t, AX_COLUMN, s, T, uplo, ws); }
        CAPITAL_CHECK(capi_dtrmm_acc(h, side, uplo, trans, diag_of_step(t, side, diag, s), M, N, alpha, tt.p, tt.ld, bb.p, bb.ld, s ? 1.0 : 0.0, Cout.p, Cout.ld));
      }
    } else {
      // the T panels of every K-class step first (whole, packed), then the B panels column chunk by column chunk
      const int axT = side == CAPI_LEFT ? AX_ROW : AX_COLUMN, axB = side == CAPI_LEFT ? AX_COLUMN : AX_ROW;
      std::vector<view> tt(steps, T);
      P.begin();
      for (size_t s = 0; s < steps; ++s) tt[s] = panel_tri(t, axT, s, T, uplo, ws);
      P.whole_sent();
      relay = relay_space(t, M * plan.widest(), ws);
      const std::vector<view> bb = stream_chunks(t, P, axB, steps, B, plan, relay, ws);
      P.resume();
      P.products(plan, [&](int j, int64_t c0, int64_t c1) {
        P.wait(EB + j);
        double* Cj = Cout.p + c0 * Cout.ld;
        for (size_t s = 0; c1 > c0 && s < steps; ++s) {
          const double b0 = s ? 1.0 : 0.0;
          const int dg = diag_of_step(t, side, diag, s);
          if (side == CAPI_LEFT) {
            CAPITAL_CHECK(capi_dtrmm_acc(h, side, uplo, trans, dg, M, c1 - c0, alpha, tt[s].p, tt[s].ld, bb[s].p + c0 * bb[s].ld, bb[s].ld, b0, Cj, Cout.ld));
          } else {
            // Cout[:, chunk] += alpha ( B[:, 0:c0] T[0:c0, chunk] + B[:, chunk] T[chunk, chunk] ): a rectangle above the chunk's triangle
            if (c0 > 0)
              CAPITAL_CHECK(capi_dgemm(h, CAPI_NOTRANS, CAPI_NOTRANS, M, c1 - c0, c0, alpha, bb[s].p, bb[s].ld, tt[s].p + c0 * tt[s].ld, tt[s].ld, b0, Cj, Cout.ld));
            CAPITAL_CHECK(capi_dtrmm_acc(h, side, uplo, trans, dg, M, c1 - c0, alpha, tt[s].p + c0 + c0 * tt[s].ld, tt[s].ld, bb[s].p + c0 * bb[s].ld, bb[s].ld,
                                         (c0 > 0 || s) ? 1.0 : 0.0, Cj, Cout.ld));
          }
        }
      });
    }
    if (P.on) depth_sum(t, P, plan, Cout, [&](int64_t) { return Cout.rows; }, relay, ws);
    else if (t.c > 1) allreduce_view(t, Cout, ws);
    ws.top = mark;
  }

  // C(uplo) <- alpha * Bx^T * A + beta*C (trans) or alpha * A * Bx^T + beta*C; Bx = partner-exchanged block (summa.hpp:111-158)
  template <typename CommType>
  static void syrk(CommType&& t, int uplo, int trans, double alpha, view A, view Bx, double beta, view C, arena& ws) {
    capi_handle_t h = capital::handle();
    const int64_t N = C.cols, K = trans ? A.rows : A.cols;
    // operand order of the local multiply (summa.hpp:137-146)
    const int tA = trans ? CAPI_TRANS : CAPI_NOTRANS, tB = trans ? CAPI_NOTRANS : CAPI_TRANS;
    if (t.d == 1 && t.c == 1) {
      const view& L = trans ? Bx : A;
      const view& Rr = trans ? A : Bx;
      CAPITAL_CHECK(capi_dgemmt(h, uplo, tA, tB, N, K, alpha, L.p, L.ld, Rr.p, Rr.ld, beta, C.p, C.ld));
      return;
    }
    if (t.d == 1 && colsplit() && trans && uplo == CAPI_UPPER) {
      // replicated layers: layer z forms its column range of the upper triangle in place (the rectangle above the range's diagonal block +
      // the block), rows 0 .. c1 of those columns travel
      colsplit_run(t, N, true, C.p, C.ld,
                   [&](int64_t c0, int64_t c1) {
                     const double* rj = A.p + c0 * A.ld;
                     if (c0 > 0)
                       CAPITAL_CHECK(capi_dgemm(h, CAPI_TRANS, CAPI_NOTRANS, c0, c1 - c0, K, alpha, Bx.p, Bx.ld, rj, A.ld, beta, C.p + c0 * C.ld, C.ld));
                     CAPITAL_CHECK(capi_dgemmt(h, CAPI_UPPER, CAPI_TRANS, CAPI_NOTRANS, c1 - c0, K, alpha, Bx.p + c0 * Bx.ld, Bx.ld, rj, A.ld, beta,
                                               C.p + c0 + c0 * C.ld, C.ld));
                   },
                   [&](int64_t c1) { return c1; }, ws);
      return;
    }
    const int64_t mark = ws.top;
    const size_t steps = t.d > 1 ? t.d / t.c : 1;
    // the pipeline is built for what cholinv issues: upper triangle, transposed form
    const bool piped = t.num_chunks > 0 && trans && uplo == CAPI_UPPER;
    const chunks plan{N, piped ? chunk_count(t.num_chunks, N) : 1};
    pipe P(piped && plan.nch > 1);
    view acc = t.c > 1 ? view{ws.take(N * N), N, N, N} : C;
    if (!P.on) {
      if (t.d == 1) {
        int64_t k0, k1;
        kslice(K, t.c, t.z, k0, k1);
        const view& L = trans ? Bx : A;
        const view& Rr = trans ? A : Bx;
        const double* l = trans ? L.p + k0 : L.p + k0 * L.ld;
        const double* r = trans ? Rr.p + k0 : Rr.p + k0 * Rr.ld;
        CAPITAL_CHECK(capi_dgemmt(h, uplo, tA, tB, N, k1 - k0, alpha, l, L.ld, r, Rr.ld, 0.0, acc.p, acc.ld));
      } else {
        for (size_t s = 0; s < steps; ++s) {
          view l, r;
          if (trans) { l = panel(t, AX_ROW, s, Bx, ws); r = panel(t, AX_COLUMN, s, A, ws); }   // distribute(B,A)
          else { l = panel(t, AX_ROW, s, A, ws); r = panel(t, AX_COLUMN, s, Bx, ws); }        // distribute(A,B)
          const double bt = (t.c > 1) ? (s ? 1.0 : 0.0) : (s ? 1.0 : beta);
          CAPITAL_CHECK(capi_dgemmt(h, uplo, tA, tB, N, K, alpha, l.p, l.ld, r.p, r.ld, bt, acc.p, acc.ld));
        }
      }
      if (t.c > 1) {
        // only the computed triangle is folded into C (and only it travels)
        allreduce_tri(t, acc, uplo, ws);
        CAPITAL_CHECK(capi_dgeadd(h, uplo == CAPI_UPPER ? 1 : 2, N, N, 1.0, acc.p, acc.ld, beta, C.p, C.ld));
      }
      ws.top = mark;
      return;
    }
    // ---- pipelined: C(upper)[:, chunk] = alpha * sum over this layer's K-class steps of L_s[:, 0:c1]^T * R_s[:, chunk]; K x N, k-contiguous
    //      (d == 1: nothing travels before the depth sum, layer z multiplies its slice [k0,k1) of the local K range)
    const bool sliced = (t.d == 1);
    int64_t k0 = 0, k1 = K;
    if (sliced) kslice(K, t.c, t.z, k0, k1);
    std::vector<view> l(steps, Bx);
    P.begin();
    if (!sliced)
      for (size_t s = 0; s < steps; ++s) l[s] = panel(t, AX_ROW, s, Bx, ws);
    P.whole_sent();
    double* relay = relay_space(t, std::max(A.rows, N) * plan.widest(), ws);             // (one buffer for stages 3 and 5)
    const std::vector<view> r = stream_chunks(t, P, AX_COLUMN, sliced ? 0 : steps, A, plan, relay, ws);
    P.resume();
    if (t.c > 1) capital::dev_zero(acc.p, acc.count());       // (the part below the computed trapezoids is folded into C as zeros)
    P.products(plan, [&](int j, int64_t c0, int64_t c1) {
      P.wait(EB + j);
      for (size_t s = 0; c1 > c0 && s < steps; ++s) {
        const double bt = s ? 1.0 : (t.c > 1 ? 0.0 : beta);
        const double* rj = r[s].p + k0 + c0 * r[s].ld;
        if (c0 > 0)   // rows above the diagonal block of this chunk: a plain rectangle
          CAPITAL_CHECK(capi_dgemm(h, CAPI_TRANS, CAPI_NOTRANS, c0, c1 - c0, k1 - k0, alpha, l[s].p + k0, l[s].ld, rj, r[s].ld, bt, acc.p + c0 * acc.ld, acc.ld));
        CAPITAL_CHECK(capi_dgemmt(h, CAPI_UPPER, CAPI_TRANS, CAPI_NOTRANS, c1 - c0, k1 - k0, alpha, l[s].p + k0 + c0 * l[s].ld, l[s].ld, rj, r[s].ld, bt,
                                  acc.p + c0 + c0 * acc.ld, acc.ld));
      }
    });
    // (rows 0 .. c1 of a chunk's columns hold the computed part; the zeros below it are not sent)
    depth_sum(t, P, plan, acc, [](int64_t c1) { return c1; }, relay, ws);
    if (t.c > 1) CAPITAL_CHECK(capi_dgeadd(h, 1, N, N, 1.0, acc.p, acc.ld, beta, C.p, C.ld));
    ws.top = mark;
  }

  static arena& scratch_arena() {
    static CAPITAL_RANK_LOCAL arena a;
    return a;
  }
  template <typename MatrixType>
  static view as_view(MatrixType& m) { return view{m.data(), m.num_rows_local(), m.num_rows_local(), m.num_columns_local()}; }

  // [k0,k1): slice z of c equal (even-sized, for 16-byte alignment) pieces of a local K range
  static void kslice(int64_t K, size_t c, size_t z, int64_t& k0, int64_t& k1) {
    int64_t per = ((K + (int64_t)c - 1) / (int64_t)c + 1) & ~(int64_t)1;
    k0 = std::min<int64_t>(K, per * (int64_t)z);
    k1 = std::min<int64_t>(K, k0 + per);
  }

  // ---- replicated layers (d == 1, c > 1: the 2-GPU grid) by OUTPUT COLUMNS ------------------------------------------------------------
  // Every layer holds the whole operands.  Round 2 sliced the K range and all-reduced the full outputs over `depth` (h^2 doubles in each
  // direction per product, plus an accumulator and an add pass).  Here layer z computes the output columns [b_z, b_z+1) -- all of K, in
  // place, with the caller's beta -- and the blocks are exchanged (c broadcasts over `depth`, both directions of the link at once with
  // c = 2): half the bytes of the all-reduce, no accumulator, and every element is computed exactly once, by the kernel and in the
  // summation order of the single-GPU run.  Triangular work (a TRMM with the triangle on the right, a triangular output) grows linearly
  // with the column index, so the boundaries sit at N sqrt(z / c).  CAPITAL_KSLICE=1 restores the K-slicing (A/B).
  static bool colsplit() { return getenv("CAPITAL_KSLICE") == nullptr; }      // (read per multiply: bench.py probes both forms in one process)
  static int64_t colsplit_bound(int64_t N, size_t c, size_t z, bool triangular) {
    if (z == 0) return 0;
    if (z >= c) return N;
    const double f = triangular ? std::sqrt((double)z / (double)c) : (double)z / (double)c;
    const int64_t b = ((int64_t)std::llround(f * (double)N) + 1) & ~(int64_t)1;
    return std::min<int64_t>(N, std::max<int64_t>(0, b));
  }
  // compute(c0, c1) enqueues the kernels that finish output columns [c0, c1) in place at `base` (leading dimension ld); rows_of(c1) = how
  // many leading rows of those columns carry the result (all of them, or c1 for an upper-triangular output).  With num_chunks > 0 the
  // exchange of chunk j (communication stream) runs beside the computation of chunk j + 1: a schedule of its own (per-layer broadcasts, no
  // accumulator) on the chunk plan and the event slots of the pipeline above.
  template <typename CommType, typename Compute, typename RowsOf>
  static void colsplit_run(CommType&& t, int64_t N, bool triangular, double* base, int64_t ld, Compute&& compute, RowsOf&& rows_of, arena& ws) {
    capi_handle_t h = capital::handle();
    const int64_t mark = ws.top;
    std::vector<int64_t> b(t.c + 1);
    int64_t widest = 0;
    for (size_t z = 0; z <= t.c; ++z) b[z] = colsplit_bound(N, t.c, z, triangular);
    for (size_t z = 0; z < t.c; ++z) widest = std::max(widest, b[z + 1] - b[z]);
    const int nch = t.num_chunks > 0 ? chunk_count(t.num_chunks, widest) : 1;
    auto plan = [&](size_t z) { return chunks{b[z + 1] - b[z], nch}; };       // every layer's column range is cut into the same number of chunks
    pipe P(nch > 1);
    double* tmp = nullptr;                                       // staging of a strided block (allocated once: it is used on the communication stream)
    int64_t tmp_need = 0;
    for (size_t z = 0; z < t.c; ++z)
      plan(z).each([&](int, int64_t c0, int64_t c1) {
        const int64_t rows = rows_of(b[z] + c1);
        if (rows != ld) tmp_need = std::max(tmp_need, rows * (c1 - c0));
      });
    if (tmp_need > 0) tmp = ws.take(tmp_need);
    P.main();
    for (int j = 0; j < nch; ++j) {
      const chunks::span r = plan(t.z).range(j);
      if (!r.empty()) compute(b[t.z] + r.c0, b[t.z] + r.c1);
      P.rec(pipe::EC + j);
    }
    P.comm();
    for (int j = 0; j < nch; ++j) {
      P.wait(pipe::EC + j);
      for (size_t z = 0; z < t.c; ++z) {
        const chunks::span r = plan(z).range(j);
        if (r.empty()) continue;
        const int64_t g0 = b[z] + r.c0, g1 = b[z] + r.c1, rows = rows_of(g1);
        double* blk = base + g0 * ld;
        if (rows == ld) {
          CAPITAL_CHECK(capi_bcast(t.depth, blk, rows * (g1 - g0), (int)z));
        } else {
          if (t.z == z) CAPITAL_CHECK(capi_dlacpy(h, 0, rows, g1 - g0, blk, ld, tmp, rows));
          CAPITAL_CHECK(capi_bcast(t.depth, tmp, rows * (g1 - g0), (int)z));
          if (t.z != z) CAPITAL_CHECK(capi_dlacpy(h, 0, rows, g1 - g0, tmp, rows, blk, ld));
        }
      }
    }
    P.rec(pipe::ER);
    P.main(); P.wait(pipe::ER);
    ws.top = mark;
  }

  enum { AX_ROW = 0, AX_COLUMN = 1 };
  // is this rank the root of the broadcast along `axis` at K-class step s?  (layer z owns K-classes z, z + c, ...)
  template <typename CommType>
  static bool is_root(CommType&& t, int axis, size_t s) { return (axis == AX_ROW ? t.x : t.y) == t.z + s * t.c; }
  // The diagonal flag of the local TRMM at K-class step s on d > 1.  The block of op(T) that meets this rank's output block at K-class q holds
  // a piece of the GLOBAL diagonal, on its own diagonal, only where q is the output block's row class (Left: op(T) is rows x K) or column class
  // (Right: K x columns); every other block's diagonal holds entries of T's triangle proper or stored zeros of the other one, which a unit flag
  // must not replace by ones.
  template <typename CommType>
  static int diag_of_step(CommType&& t, int side, int diag, size_t s) {
    return (side == CAPI_LEFT ? t.y : t.x) == t.z + s * t.c ? diag : (int)CAPI_NONUNIT;
  }

  // ---- pair collectives: over every link of the node (capi_pairs_transfer, csrc/pair_paths.h) when the grid's rows / columns /
  //      depth fibres are pairs, else as RCCL calls on the sub-communicators ---------------------------------------------------------
  // relay space for transfers of up to `count` doubles (nullptr when this grid does not relay)
  template <typename CommType>
  static double* relay_space(CommType&& t, int64_t count, arena& ws) {
    if (!t.multipath) return nullptr;
    const int64_t n = capi_pairs_scratch_count(t.size, count);
    return n > 0 ? ws.take(n) : nullptr;
  }
  // landing space for the partner's half in a pair all-reduce of up to `count` doubles
  template <typename CommType>
  static double* depth_space(CommType&& t, int64_t count, arena& ws) { return t.pairs_in_depth() ? ws.take(count / 2 + 2) : nullptr; }

  // MPI_Bcast(row | column) of `count` doubles at `buf`, root = the member whose x (y) is this layer's K-class at step s (summa.hpp:185,193)
  template <typename CommType>
  static void bcast_axis(CommType&& t, int axis, size_t s, double* buf, int64_t count, double* relay) {
    if (t.pairs_along(axis)) {
      const bool root = is_root(t, axis, s);
      const std::vector<int> dst = t.bcast_dst(axis, s);
      CAPITAL_CHECK(capi_pairs_transfer(t.world, dst.data(), root ? buf : nullptr, root ? nullptr : buf, count, relay));
    } else {
      CAPITAL_CHECK(capi_bcast(axis == AX_ROW ? t.row : t.column, buf, count, (int)(t.z + s * t.c)));
    }
  }
  // MPI_Allreduce(depth, SUM) in place (summa.hpp:236).  On a depth PAIR: each member keeps one half, the halves that are not kept
  // cross over (all links), are added, and the sums cross back -- the bytes of a two-rank ring, at the multi-path rate.  a + b is
  // commutative in IEEE arithmetic, so both members end with bit-identical sums.
  template <typename CommType>
  static void allreduce_depth(CommType&& t, double* buf, int64_t count, double* half_space, double* relay) {
    const int64_t c4 = count & ~(int64_t)3, half = c4 / 2;
    if (!t.pairs_in_depth() || half == 0) { CAPITAL_CHECK(capi_allreduce_sum(t.depth, buf, count)); return; }
    const std::vector<int> dst = t.depth_dst();
    double* keep = buf + (t.z == 0 ? 0 : half);
    double* give = buf + (t.z == 0 ? half : 0);
    CAPITAL_CHECK(capi_pairs_transfer(t.world, dst.data(), give, half_space, half, relay));
    CAPITAL_CHECK(capi_daxpby(capital::handle(), half, 1.0, half_space, keep));
    CAPITAL_CHECK(capi_pairs_transfer(t.world, dst.data(), keep, give, half, relay));
    if (count > c4) CAPITAL_CHECK(capi_allreduce_sum(t.depth, buf + c4, count - c4));     // (at most three trailing values)
  }
  // sum over depth of the block v, in place; a strided block travels as a contiguous copy.  half_space / relay sized for v.count();
  // the copy's arena space stays taken until the caller resets its mark: it lives on the communication stream of a pipelined multiply.
  template <typename CommType>
  static void allreduce_view(CommType&& t, view v, double* half_space, double* relay, arena& ws) {
    if (v.contiguous()) { allreduce_depth(t, v.p, v.count(), half_space, relay); return; }
    capi_handle_t h = capital::handle();
    double* tmp = ws.take(v.count());
    CAPITAL_CHECK(capi_dlacpy(h, 0, v.rows, v.cols, v.p, v.ld, tmp, v.rows));
    allreduce_depth(t, tmp, v.count(), half_space, relay);
    CAPITAL_CHECK(capi_dlacpy(h, 0, v.rows, v.cols, tmp, v.rows, v.p, v.ld));
  }
  // the same with the landing and relay space from the arena, outside a pipeline (all of it is given back)
  template <typename CommType>
  static void allreduce_view(CommType&& t, view v, arena& ws) {
    const int64_t mark = ws.top;
    double* half = depth_space(t, v.count(), ws);
    double* relay = t.pairs_in_depth() ? relay_space(t, v.count() / 2 + 2, ws) : nullptr;
    allreduce_view(t, v, half, relay, ws);
    ws.top = mark;
  }

  // "Own block or staged copy": a block that travels is sent from / received into `landing` -- the root's own block if that is
  // contiguous, arena space otherwise --, and the root of a strided block copies the columns [c0, c1) there before they go (`stage`).
  static view landing(bool root, const view& mine, arena& ws) {
    return view{(root && mine.contiguous()) ? mine.p : ws.take(mine.count()), mine.rows, mine.rows, mine.cols};
  }
  static void stage(bool root, const view& mine, const view& at, int64_t c0, int64_t c1) {
    if (root && !mine.contiguous())
      CAPITAL_CHECK(capi_dlacpy(capital::handle(), 0, mine.rows, c1 - c0, mine.p + c0 * mine.ld, mine.ld, at.p + c0 * at.ld, at.ld));
  }
  // The panel a rank multiplies with: the root's own block (packed to contiguous if it is a strided view) broadcast
  // over `comm`.  Non-roots receive into arena memory.  Blocks have equal shapes on all ranks of a communicator.
  static view panel(capi_comm_t comm, bool root, int root_rank, const view& mine, arena& ws) {
    int size = 1;
    CAPITAL_CHECK(capi_comm_size(comm, &size));
    if (size == 1) return mine;
    view out = landing(root, mine, ws);
    stage(root, mine, out, 0, mine.cols);
    CAPITAL_CHECK(capi_bcast(comm, out.p, out.count(), root_rank));
    return out;
  }
  // the same along an axis of the grid at K-class step s (multi-path on grids of pairs)
  template <typename CommType>
  static view panel(CommType&& t, int axis, size_t s, const view& mine, arena& ws) {
    const bool root = is_root(t, axis, s);
    if (!t.pairs_along(axis)) return panel(axis == AX_ROW ? t.row : t.column, root, (int)(t.z + s * t.c), mine, ws);
    view out = landing(root, mine, ws);
    stage(root, mine, out, 0, mine.cols);
    const int64_t mark = ws.top;
    bcast_axis(t, axis, s, out.p, out.count(), relay_space(t, out.count(), ws));
    ws.top = mark;                                              // (relay space is reused in stream order)
    return out;
  }

  // ---- triangles on the wire: n(n+1)/2 doubles instead of n^2 (the reference's Serialize policy, summa.hpp:147-148,216-217) ----------
  static bool packed_comm() { return getenv("CAPITAL_NO_PACKED_COMM") == nullptr; }      // (read per transfer)
  static int64_t tri_count(int64_t n) { return n * (n + 1) / 2; }
  // the `uplo` triangle of the square block v -> tri_count(v.rows) packed doubles, and back into a full-stride block whose other half is
  // left alone (no kernel reads it: the tile kernels truncate each tile's k-range at the diagonal and mask the diagonal panels by selection)
  static void pack_tri(const view& v, int uplo, double* packed) {
    const int64_t n = v.rows;
    const int st = uplo == CAPI_UPPER ? CAPI_UPPERTRI : CAPI_LOWERTRI;
    CAPITAL_CHECK(capi_serialize_shape(capital::handle(), st, CAPI_RECT, st, v.p, n, v.ld, packed, n, n, 0, n, 0, n, 0, n, 0, n));
  }
  static void unpack_tri(const double* packed, int uplo, const view& v) {
    const int64_t n = v.rows;
    const int st = uplo == CAPI_UPPER ? CAPI_UPPERTRI : CAPI_LOWERTRI;
    CAPITAL_CHECK(capi_serialize_shape(capital::handle(), st, st, CAPI_RECT, packed, n, n, v.p, n, v.ld, 0, n, 0, n, 0, n, 0, n));
  }
  // A TRIANGULAR operand's panel: the root packs, everyone else unpacks into arena memory
  template <typename CommType>
  static view panel_tri(CommType&& t, int axis, size_t s, const view& mine, int uplo, arena& ws) {
    capi_comm_t comm = axis == AX_ROW ? t.row : t.column;
    int size = 1;
    CAPITAL_CHECK(capi_comm_size(comm, &size));
    if (size == 1) return mine;
    if (!packed_comm() || mine.rows != mine.cols) return panel(t, axis, s, mine, ws);
    const bool root = is_root(t, axis, s);
    const int64_t n = mine.rows, np = tri_count(n);
    double* packed = ws.take(np);
    if (root) pack_tri(mine, uplo, packed);
    {
      const int64_t mark = ws.top;
      bcast_axis(t, axis, s, packed, np, relay_space(t, np, ws));
      ws.top = mark;
    }
    if (root) return mine;                                      // the root multiplies with its own block
    view out{ws.take(n * n), n, n, n};
    unpack_tri(packed, uplo, out);
    return out;
  }
  // sum over depth of the `uplo` triangle of a contiguous n x n accumulator, packed on the wire
  template <typename CommType>
  static void allreduce_tri(CommType&& t, view acc, int uplo, arena& ws) {
    if (!packed_comm() || acc.rows != acc.cols || !acc.contiguous()) { allreduce_view(t, acc, ws); return; }
    const int64_t np = tri_count(acc.rows);
    double* packed = ws.take(np);
    pack_tri(acc, uplo, packed);
    allreduce_view(t, view{packed, np, np, 1}, ws);
    unpack_tri(packed, uplo, acc);
  }
};

}  // namespace matmult

#endif  // CAPITAL_MATMULT_SUMMA_H_
