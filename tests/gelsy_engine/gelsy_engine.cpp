// tests/gelsy_engine/gelsy_engine.cpp -- lapack::engine::_geqp3 and _gelsy called with ArgPack_* objects the way a caller of src/lapack/engine.h builds
// them, at m = 700, n = 48 with rank 30, r = 5.  A = G1 G2 with G1 (700 x 30) and G2 (30 x 48) from the product's own generator (the reference's
// distribute_random stream), multiplied on the device; A itself and every result go to one binary file that tests/test_gpu_gelsy_engine.py compares with
// tests/_qrcp_ref.py.  A wrong enum cast, a swapped leading dimension or a swapped pointer in the two new slots shows up here.
#include <cstdio>
#include <vector>

#include "../../capital_amd/src/lapack/engine.h"

namespace {
FILE* g_out = nullptr;
void dump_host(const char* name, const std::vector<double>& h) {
  char tag[32] = {0};
  snprintf(tag, sizeof(tag), "%s", name);
  const int64_t count = (int64_t)h.size();
  fwrite(tag, 1, 32, g_out);
  fwrite(&count, sizeof(count), 1, g_out);
  fwrite(h.data(), sizeof(double), h.size(), g_out);
}
void dump(const char* name, const double* dev, int64_t count) {
  std::vector<double> h((size_t)count);
  CAPITAL_CHECK(capi_memcpy_d2h(capital::handle(), h.data(), dev, sizeof(double) * (size_t)count));
  dump_host(name, h);
}
void dump_ints(const char* name, const int* dev, int64_t count) {
  std::vector<int> h((size_t)count);
  CAPITAL_CHECK(capi_memcpy_d2h(capital::handle(), h.data(), dev, sizeof(int) * (size_t)count));
  dump_host(name, std::vector<double>(h.begin(), h.end()));
}
double* gen_random(int64_t rows, int64_t cols, int64_t key) {
  double* p = capital::dev_alloc(rows * cols);
  CAPITAL_CHECK(capi_distribute_random(capital::handle(), p, cols, rows, cols, rows, 0, 0, 1, 1, key));
  return p;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: gelsy_engine <out.bin>\n"); return 2; }
  try {
    capital::init(0, 0, 1, nullptr);
    g_out = fopen(argv[1], "wb");
    if (!g_out) throw std::runtime_error("cannot open output");
    using T = double;
    const int m = 700, n = 48, rank = 30, r = 5;
    const double rcond = 1e-13;
    T* G1 = gen_random(m, rank, 21); T* G2 = gen_random(rank, n, 22);
    T* A0 = capital::dev_alloc((int64_t)m * n);
    CAPITAL_CHECK(capi_dgemm(capital::handle(), CAPI_NOTRANS, CAPI_NOTRANS, m, n, rank, 1.0, G1, m, G2, rank, 0.0, A0, m));
    dump("A", A0, (int64_t)m * n);
    T* B0 = gen_random(m, r, 23);
    T* A = capital::dev_alloc((int64_t)m * n); T* B = capital::dev_alloc((int64_t)m * r);
    T* tau = capital::dev_alloc(n); T* F = capital::dev_alloc(n * n); T* tauf = capital::dev_alloc(n); T* Z = capital::dev_alloc(n * n);
    T* tauz = capital::dev_alloc(n); T* nrm = capital::dev_alloc(r);
    int* jpvt = reinterpret_cast<int*>(capital::dev_alloc(n));            // n ints in the room of n doubles
    {
      CAPITAL_CHECK(capi_dlacpy(capital::handle(), 0, m, n, A0, m, A, m));
      lapack::ArgPack_geqrf geqrfArgs(lapack::Order::AlapackColumnMajor);
      lapack::engine::_geqrf(A, tau, m, n, m, geqrfArgs);
      CAPITAL_CHECK(capi_dlacpy(capital::handle(), 1, n, n, A, m, F, n));
      CAPITAL_CHECK(capi_dtrizero(capital::handle(), CAPI_UPPER, n, F, n));
      dump("geqp3_in", F, n * n);
      lapack::ArgPack_geqp3 geqp3Args(lapack::Order::AlapackColumnMajor);
      const int k = lapack::engine::_geqp3(F, jpvt, tauf, n, n, n, rcond, geqp3Args);
      dump("geqp3_F", F, n * n);
      dump("geqp3_tau", tauf, n);
      dump_ints("geqp3_jpvt", jpvt, n);
      dump_host("geqp3_rank", std::vector<double>(1, (double)k));
      bool threw = false;
      try {
        lapack::ArgPack_geqp3 bad(lapack::Order::AlapackRowMajor);
        lapack::engine::_geqp3(F, jpvt, tauf, n, n, n, rcond, bad);
      } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) throw std::runtime_error("row-major _geqp3 was not refused");
    }
    for (int mn = 1; mn >= 0; --mn) {
      CAPITAL_CHECK(capi_dlacpy(capital::handle(), 0, m, n, A0, m, A, m));
      CAPITAL_CHECK(capi_dlacpy(capital::handle(), 0, m, r, B0, m, B, m));
      lapack::ArgPack_gelsy gelsyArgs(lapack::Order::AlapackColumnMajor, mn != 0);
      const int k = lapack::engine::_gelsy(A, tau, F, tauf, jpvt, mn ? Z : (T*)nullptr, mn ? tauz : (T*)nullptr, B, nrm, m, n, r, m, n, n, m, rcond, gelsyArgs);
      dump(mn ? "gelsy_mn_B" : "gelsy_basic_B", B, (int64_t)m * r);
      dump(mn ? "gelsy_mn_norm2" : "gelsy_basic_norm2", nrm, r);
      dump_ints(mn ? "gelsy_mn_jpvt" : "gelsy_basic_jpvt", jpvt, n);
      dump_host(mn ? "gelsy_mn_rank" : "gelsy_basic_rank", std::vector<double>(1, (double)k));
    }
    dump("B", B0, (int64_t)m * r);
    bool threw = false;
    try {
      lapack::ArgPack_gelsy bad(lapack::Order::AlapackRowMajor, true);
      lapack::engine::_gelsy(A, tau, F, tauf, jpvt, Z, tauz, B, nrm, m, n, r, m, n, n, m, rcond, bad);
    } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) throw std::runtime_error("row-major _gelsy was not refused");
    for (T* p : {G1, G2, A0, B0, A, B, tau, F, tauf, Z, tauz, nrm, reinterpret_cast<T*>(jpvt)}) capital::dev_free(p);
    fclose(g_out);
    capital::finalize();
    printf("gelsy_engine ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "gelsy_engine: %s\n", e.what());
    return 1;
  }
}
