// capi_cpu_shim_scqr.cpp -- TEST INFRASTRUCTURE ONLY.  The oracle-backed CPU stand-in of the C-ABI (tests/cpu_shim/capi_cpu_shim.cpp, taken
// in whole and unchanged) plus the two n x n entry points of a shifted CholeskyQR sweep (include/capital_hip.h) in plain C++, so that
// qr::cacqr with num_shifted > 0 runs on gloo ranks (tests/test_shifted_cqr_host.py).
#include <cmath>

#include "../cpu_shim/capi_cpu_shim.cpp"

extern "C" {

// the n x n steps of a shifted CholeskyQR sweep (include/capital_hip.h), in plain C++
int capi_dgram_equilibrate_shift(capi_handle_t h, int64_t n, double* G, int64_t ldg, int64_t m_global, double shift_scale, double* dscale,
                                 double* rec) {
  std::vector<int> e((size_t)n, 0);
  double tr = 0.0;
  for (int64_t j = 0; j < n; ++j) {
    const double g = IDX(G, j, j, ldg);
    dscale[j] = 1.0;
    if (!(g > 0.0) || std::isinf(g)) { if (!h->info) h->info = (int)(j + 1); continue; }
    int ex;
    (void)std::frexp(g, &ex);
    e[j] = (ex - (ex & 1)) / 2;
    dscale[j] = std::ldexp(1.0, e[j]);
    tr += std::ldexp(g, -2 * e[j]);
  }
  rec[0] = (shift_scale * (11.0 * ((double)m_global * (double)n + (double)n * (double)(n + 1)) * 0x1p-53)) * tr;
  rec[1] = tr;
  for (int64_t j = 0; j < n; ++j)
    for (int64_t i = 0; i <= j; ++i) IDX(G, i, j, ldg) = std::ldexp(IDX(G, i, j, ldg), -(e[i] + e[j])) + (i == j ? rec[0] : 0.0);
  return 0;
}
int capi_dtri_rescale(capi_handle_t h, int64_t n, double* R, int64_t ldr, double* X, int64_t ldx, const double* dscale, double* rec) {
  std::vector<double> cr((size_t)n, 0.0), rr((size_t)n, 0.0), cx((size_t)n, 0.0), rx((size_t)n, 0.0);
  for (int64_t j = 0; j < n; ++j)
    for (int64_t i = 0; i <= j; ++i) {
      const double r = IDX(R, i, j, ldr), x = IDX(X, i, j, ldx);
      cr[j] += std::fabs(r); rr[i] += std::fabs(r);
      cx[j] += std::fabs(x); rx[i] += std::fabs(x);
      if (!dscale) continue;
      IDX(R, i, j, ldr) = std::ldexp(r, std::ilogb(dscale[j]));
      IDX(X, i, j, ldx) = std::ldexp(x, -std::ilogb(dscale[i]));
      if (i == j && !(std::isnormal(IDX(R, i, j, ldr)) && std::isnormal(IDX(X, i, j, ldx))) && !h->info) h->info = (int)(j + 1);
    }
  auto mx = [](const std::vector<double>& v) { double m = 0.0; for (double a : v) m = (a > m || a != a) ? a : m; return m; };
  rec[2] = mx(cr) * mx(rr);
  rec[3] = mx(cx) * mx(rx);
  return 0;
}

}  // extern "C"
