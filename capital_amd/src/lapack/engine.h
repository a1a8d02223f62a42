// lapack/engine.h -- the reference's lapack::engine operator API (src/lapack/engine.h:23-102,
// src/lapack/interface.h:49-59) on the MI355X C-ABI instead of LAPACKE (src/lapack/interface.hpp:30-88).
// n and lda stay 32-bit `int` as in the reference; A is a DEVICE pointer.  LAPACK's info, which the reference
// throws away, stays on the device and can be read with lapack::engine::info().
#ifndef CAPITAL_LAPACK_ENGINE_H_
#define CAPITAL_LAPACK_ENGINE_H_

#include "./../util/shared.h"

namespace lapack {

enum class Order : unsigned char { AlapackRowMajor = 0x0, AlapackColumnMajor = 0x1 };
enum class UpLo : unsigned char { AlapackLower = 0x0, AlapackUpper = 0x1 };
enum class Diag : unsigned char { AlapackNonUnit = 0x0, AlapackUnit = 0x1 };
enum class Side : unsigned char { AlapackLeft = 0x0, AlapackRight = 0x1 };
enum class Trans : unsigned char { AlapackNoTrans = 0x0, AlapackTrans = 0x1 };
enum class Method : unsigned char { AlapackPotrf = 0x0, AlapackTrtri = 0x1, AlapackGeqrf = 0x10, AlapackOrgqr = 0x11, AlapackOrmqr = 0x12, AlapackGels = 0x13,
                                     AlapackGeqp3 = 0x14, AlapackGelsy = 0x15 };

class ArgPack {
public:
  Method method;
};
class ArgPack_potrf : public ArgPack {
public:
  ArgPack_potrf(Order o, UpLo u) : order(o), uplo(u) { method = Method::AlapackPotrf; }
  Order order;
  UpLo uplo;
};
class ArgPack_trtri : public ArgPack {
public:
  ArgPack_trtri(Order o, UpLo u, Diag d) : order(o), uplo(u), diag(d) { method = Method::AlapackTrtri; }
  Order order;
  UpLo uplo;
  Diag diag;
};
class ArgPack_geqrf : public ArgPack {
public:
  explicit ArgPack_geqrf(Order o) : order(o) { method = Method::AlapackGeqrf; }
  Order order;
};
class ArgPack_orgqr : public ArgPack {
public:
  explicit ArgPack_orgqr(Order o) : order(o) { method = Method::AlapackOrgqr; }
  Order order;
};
// not in the reference (lapack/interface.h declares _geqrf and _orgqr only): the third member of the Householder path and the solve on it
class ArgPack_ormqr : public ArgPack {
public:
  ArgPack_ormqr(Order o, Side s, Trans t) : order(o), side(s), trans(t) { method = Method::AlapackOrmqr; }
  Order order;
  Side side;
  Trans trans;
};
class ArgPack_gels : public ArgPack {
public:
  explicit ArgPack_gels(Order o) : order(o) { method = Method::AlapackGels; }
  Order order;
};
// the rank-revealing pair: column-pivoted QR of a block of order <= CAPI_GEQP3_MAX, and least squares for A of any rank (basic or minimum-norm solution)
class ArgPack_geqp3 : public ArgPack {
public:
  explicit ArgPack_geqp3(Order o) : order(o) { method = Method::AlapackGeqp3; }
  Order order;
};
class ArgPack_gelsy : public ArgPack {
public:
  ArgPack_gelsy(Order o, bool mn) : order(o), min_norm(mn) { method = Method::AlapackGelsy; }
  Order order;
  bool min_norm;
};

class engine {
public:
  engine() = delete;
  template <typename T>
  static void _potrf(T* A, int n, int lda, const ArgPack_potrf& p);
  template <typename T>
  static void _trtri(T* A, int n, int lda, const ArgPack_trtri& p);
  // declared by the reference (lapack/interface.h:55-59, interface.hpp:60-88) with no caller anywhere;
  // served by the Householder path of csrc/qr_f64.hip.  A and tau are DEVICE pointers.
  template <typename T>
  static void _geqrf(T* A, T* tau, int m, int n, int lda, const ArgPack_geqrf& p);
  template <typename T>
  static void _orgqr(T* A, T* tau, int m, int n, int k, int lda, const ArgPack_orgqr& p);
  // C (m x r, ldc) <- Q^T C or Q C, Q = H_1 .. H_k of the _geqrf image A (m x k, lda) and tau; side Left only.  DEVICE pointers.
  template <typename T>
  static void _ormqr(const T* A, const T* tau, T* C, int m, int r, int k, int lda, int ldc, const ArgPack_ormqr& p);
  // min ||A X - B||, m >= n: A and tau leave as _geqrf's image, B (m x r, ldb) as [X; tail of Q^T B]; colnorm2 (DEVICE, r values, or null) receives
  // the squared residual norms.  Returns LAPACK's info: 0, or the 1-based index of the first zero or non-finite diagonal entry of R (no solve then).
  template <typename T>
  static int _gels(T* A, T* tau, T* B, T* colnorm2, int m, int n, int r, int lda, int ldb, const ArgPack_gels& p);
  // W (mr x n, ldw) <- the LAPACK image of W P = Q R, jpvt (DEVICE, n ints, 0-based), tau (DEVICE, min(mr, n)); stops at the first pivot column whose
  // norm is <= rtol times the first one's (rtol < 0: max(mr, n) 2^-52).  Returns the rank.
  template <typename T>
  static int _geqp3(T* W, int* jpvt, T* tau, int mr, int n, int ldw, T rtol, const ArgPack_geqp3& p);
  // min ||A X - B|| for A (m x n, m >= n) of any rank: A, tau as _geqrf leaves them; F (n x n, ldf), tauf, jpvt as _geqp3 leaves them on R1; with
  // p.min_norm Z (n x n room, ldz) and tauz hold the factorization of [R11 R12]^T (else they may be null); B (m x r, ldb) leaves as [X; tail of Q1^T B];
  // colnorm2 (DEVICE, r values, or null) receives the squared residual norms.  Returns the rank.
  template <typename T>
  static int _gelsy(T* A, T* tau, T* F, T* tauf, int* jpvt, T* Z, T* tauz, T* B, T* colnorm2, int m, int n, int r, int lda, int ldf, int ldz, int ldb,
                    T rcond, const ArgPack_gelsy& p);
  // synchronises; 0 or the 1-based index of the first non-positive pivot since the last reset
  static int info() { int v = 0; CAPITAL_CHECK(capi_get_info(capital::handle(), &v)); return v; }
  static void reset_info() { CAPITAL_CHECK(capi_reset_info(capital::handle())); }
};

template <>
inline void engine::_potrf(double* A, int n, int lda, const ArgPack_potrf& p) {
  if (p.order != Order::AlapackColumnMajor) throw std::invalid_argument("lapack::engine: only AlapackColumnMajor is served");
  CAPITAL_CHECK(capi_dpotrf(capital::handle(), (int)p.uplo, n, A, lda));
}
template <>
inline void engine::_trtri(double* A, int n, int lda, const ArgPack_trtri& p) {
  if (p.order != Order::AlapackColumnMajor) throw std::invalid_argument("lapack::engine: only AlapackColumnMajor is served");
  CAPITAL_CHECK(capi_dtrtri(capital::handle(), (int)p.uplo, (int)p.diag, n, A, lda));
}

template <>
inline void engine::_geqrf(double* A, double* tau, int m, int n, int lda, const ArgPack_geqrf& p) {
  if (p.order != Order::AlapackColumnMajor) throw std::invalid_argument("lapack::engine: only AlapackColumnMajor is served");
  CAPITAL_CHECK(capi_dgeqrf(capital::handle(), m, n, A, lda, tau));
}
template <>
inline void engine::_orgqr(double* A, double* tau, int m, int n, int k, int lda, const ArgPack_orgqr& p) {
  if (p.order != Order::AlapackColumnMajor) throw std::invalid_argument("lapack::engine: only AlapackColumnMajor is served");
  CAPITAL_CHECK(capi_dorgqr(capital::handle(), m, n, k, A, lda, tau));
}
template <>
inline void engine::_ormqr(const double* A, const double* tau, double* C, int m, int r, int k, int lda, int ldc, const ArgPack_ormqr& p) {
  if (p.order != Order::AlapackColumnMajor) throw std::invalid_argument("lapack::engine: only AlapackColumnMajor is served");
  CAPITAL_CHECK(capi_dormqr(capital::handle(), (int)p.side, (int)p.trans, m, r, k, A, lda, tau, C, ldc));
}
template <>
inline int engine::_gels(double* A, double* tau, double* B, double* colnorm2, int m, int n, int r, int lda, int ldb, const ArgPack_gels& p) {
  if (p.order != Order::AlapackColumnMajor) throw std::invalid_argument("lapack::engine: only AlapackColumnMajor is served");
  int info = 0;
  CAPITAL_CHECK(capi_dgels(capital::handle(), m, n, r, A, lda, tau, B, ldb, colnorm2, &info));
  return info;
}
template <>
inline int engine::_geqp3(double* W, int* jpvt, double* tau, int mr, int n, int ldw, double rtol, const ArgPack_geqp3& p) {
  if (p.order != Order::AlapackColumnMajor) throw std::invalid_argument("lapack::engine: only AlapackColumnMajor is served");
  int rank = 0;
  CAPITAL_CHECK(capi_dgeqp3(capital::handle(), mr, n, W, ldw, jpvt, tau, rtol, &rank));
  return rank;
}
template <>
inline int engine::_gelsy(double* A, double* tau, double* F, double* tauf, int* jpvt, double* Z, double* tauz, double* B, double* colnorm2, int m, int n,
                          int r, int lda, int ldf, int ldz, int ldb, double rcond, const ArgPack_gelsy& p) {
  if (p.order != Order::AlapackColumnMajor) throw std::invalid_argument("lapack::engine: only AlapackColumnMajor is served");
  int rank = 0;
  CAPITAL_CHECK(capi_dgelsy(capital::handle(), m, n, r, A, lda, tau, F, ldf, tauf, jpvt, Z, ldz, tauz, B, ldb, rcond, p.min_norm ? 1 : 0, colnorm2, &rank));
  return rank;
}

}  // namespace lapack

#endif  // CAPITAL_LAPACK_ENGINE_H_
