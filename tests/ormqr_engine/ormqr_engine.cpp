// tests/ormqr_engine/ormqr_engine.cpp -- lapack::engine::_geqrf, _ormqr (both trans) and _gels called with ArgPack_* objects the way a caller of
// src/lapack/engine.h builds them, at m = 700, n = 48, r = 5.  Inputs come from the product's own generator (the reference's distribute_random
// stream); every result goes to one binary file that tests/test_gpu_ormqr_engine.py compares with tests/_ormqr_ref.py and numpy's Householder solve.
// A wrong enum cast or a swapped leading dimension in the two new slots shows up here.
#include <cstdio>
#include <vector>

#include "../../capital_amd/src/lapack/engine.h"

namespace {
FILE* g_out = nullptr;
void dump(const char* name, const double* dev, int64_t count) {
  std::vector<double> h((size_t)count);
  CAPITAL_CHECK(capi_memcpy_d2h(capital::handle(), h.data(), dev, sizeof(double) * (size_t)count));
  char tag[32] = {0};
  snprintf(tag, sizeof(tag), "%s", name);
  fwrite(tag, 1, 32, g_out);
  fwrite(&count, sizeof(count), 1, g_out);
  fwrite(h.data(), sizeof(double), (size_t)count, g_out);
}
double* gen_random(int64_t rows, int64_t cols, int64_t key) {
  double* p = capital::dev_alloc(rows * cols);
  CAPITAL_CHECK(capi_distribute_random(capital::handle(), p, cols, rows, cols, rows, 0, 0, 1, 1, key));
  return p;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: ormqr_engine <out.bin>\n"); return 2; }
  try {
    capital::init(0, 0, 1, nullptr);
    g_out = fopen(argv[1], "wb");
    if (!g_out) throw std::runtime_error("cannot open output");
    using T = double;
    const int m = 700, n = 48, r = 5;
    {
      T* A = gen_random(m, n, 9); T* tau = capital::dev_alloc(n);
      lapack::ArgPack_geqrf geqrfArgs(lapack::Order::AlapackColumnMajor);
      lapack::engine::_geqrf(A, tau, m, n, m, geqrfArgs);
      dump("geqrf_A", A, (int64_t)m * n);
      dump("geqrf_tau", tau, n);
      T* C = gen_random(m, r, 11);
      lapack::ArgPack_ormqr qt(lapack::Order::AlapackColumnMajor, lapack::Side::AlapackLeft, lapack::Trans::AlapackTrans);
      lapack::engine::_ormqr((const T*)A, (const T*)tau, C, m, r, n, m, m, qt);
      dump("ormqr_qt", C, (int64_t)m * r);
      T* C2 = gen_random(m, r, 11);
      lapack::ArgPack_ormqr q(lapack::Order::AlapackColumnMajor, lapack::Side::AlapackLeft, lapack::Trans::AlapackNoTrans);
      lapack::engine::_ormqr((const T*)A, (const T*)tau, C2, m, r, n, m, m, q);
      dump("ormqr_q", C2, (int64_t)m * r);
      bool threw = false;                                    // side Right is refused by the C-ABI: CAPITAL_CHECK throws
      try {
        lapack::ArgPack_ormqr bad(lapack::Order::AlapackColumnMajor, lapack::Side::AlapackRight, lapack::Trans::AlapackTrans);
        lapack::engine::_ormqr((const T*)A, (const T*)tau, C2, m, r, n, m, m, bad);
      } catch (const std::exception&) { threw = true; }
      if (!threw) throw std::runtime_error("side Right was not refused");
      dump("ormqr_q_after_refusal", C2, (int64_t)m * r);
      capital::dev_free(A); capital::dev_free(tau); capital::dev_free(C); capital::dev_free(C2);
    }
    {
      T* A = gen_random(m, n, 9); T* tau = capital::dev_alloc(n); T* B = gen_random(m, r, 12); T* nrm = capital::dev_alloc(r);
      lapack::ArgPack_gels gelsArgs(lapack::Order::AlapackColumnMajor);
      const double info = lapack::engine::_gels(A, tau, B, nrm, m, n, r, m, m, gelsArgs);
      dump("gels_A", A, (int64_t)m * n);
      dump("gels_tau", tau, n);
      dump("gels_B", B, (int64_t)m * r);
      dump("gels_norm2", nrm, r);
      T* I = capital::dev_alloc(1);
      CAPITAL_CHECK(capi_memcpy_h2d(capital::handle(), I, &info, sizeof(double)));
      dump("gels_info", I, 1);
      bool threw = false;
      try {
        lapack::ArgPack_gels bad(lapack::Order::AlapackRowMajor);
        lapack::engine::_gels(A, tau, B, nrm, m, n, r, m, m, bad);
      } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) throw std::runtime_error("row-major request was not refused");
      capital::dev_free(A); capital::dev_free(tau); capital::dev_free(B); capital::dev_free(nrm); capital::dev_free(I);
    }
    fclose(g_out);
    capital::finalize();
    printf("ormqr_engine ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "ormqr_engine: %s\n", e.what());
    return 1;
  }
}
