// capi_cpu_shim_lstsq.cpp -- TEST INFRASTRUCTURE ONLY.  The CPU stand-in of the C-ABI with the shifted sweep's entry points
// (tests/cpu_shim_scqr/capi_cpu_shim_scqr.cpp, taken in whole and unchanged) plus the two streaming kernels of qr::cacqr::least_squares
// (include/capital_hip.h) in plain C++, so that its host logic runs on gloo ranks (tests/test_lstsq_host.py).
#include "../cpu_shim_scqr/capi_cpu_shim_scqr.cpp"

extern "C" {

int capi_dgemtn_ts(capi_handle_t h, int64_t m, int64_t n, int64_t r, double alpha, const double* A, int64_t lda, const double* B, int64_t ldb,
                   double beta, double* C, int64_t ldc) {
  if (r < 1 || r > CAPI_TS_MAX_RHS) { snprintf(h->err, sizeof(h->err), "invalid argument: r: 1 <= r <= CAPI_TS_MAX_RHS"); return CAPI_EINVAL; }
  for (int64_t j = 0; j < r; ++j)
    for (int64_t i = 0; i < n; ++i) {
      double s = 0.0;
      for (int64_t k = 0; k < m; ++k) s += IDX(A, k, i, lda) * IDX(B, k, j, ldb);
      IDX(C, i, j, ldc) = alpha * s + (beta != 0.0 ? beta * IDX(C, i, j, ldc) : 0.0);
    }
  return 0;
}
int capi_dresid_ts(capi_handle_t h, int64_t m, int64_t n, int64_t r, const double* A, int64_t lda, const double* X, int64_t ldx, const double* B,
                   int64_t ldb, double* Rout, int64_t ldr, double* colnorm2) {
  if (r < 1 || r > CAPI_TS_MAX_RHS) { snprintf(h->err, sizeof(h->err), "invalid argument: r: 1 <= r <= CAPI_TS_MAX_RHS"); return CAPI_EINVAL; }
  for (int64_t j = 0; j < r; ++j) {
    double nrm = 0.0;
    for (int64_t i = 0; i < m; ++i) {
      double s = 0.0;
      for (int64_t k = 0; k < n; ++k) s += IDX(A, i, k, lda) * IDX(X, k, j, ldx);
      const double v = IDX(B, i, j, ldb) - s;
      if (Rout) IDX(Rout, i, j, ldr) = v;
      nrm += v * v;
    }
    if (colnorm2) colnorm2[j] = nrm;
  }
  return 0;
}

}  // extern "C"
