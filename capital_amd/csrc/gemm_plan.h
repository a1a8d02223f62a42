// gemm_plan.h -- how launch_gemm (gemm_f64.hip) carries out one BLAS-level product: which kernel, which tile size and split-K (a small
// makespan model in CU-cycles), and how the launches are cut (one launch, resident rounds, tile pairs, a 64-tile tail).  Plain C++17, no
// HIP: the plan is a function of the product's description, the device's CU counts, the handle's launch modes and the diagnostic
// overrides, all passed in as values.  gemm_f64.hip launches what the plan says; tests/gemm_plan checks the rules on the CPU.
#ifndef CAPITAL_GEMM_PLAN_H_
#define CAPITAL_GEMM_PLAN_H_

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "capital_hip.h"

namespace gemm_plan {

// launch geometry the kernels of gemm_f64.hip are compiled for
constexpr int BK = 16;                                       // k-panel depth of the tile kernels
constexpr int SK = BK + 2;                                   // [row][k] LDS layout: row stride in doubles (144 B)
constexpr int ST = 32, SKC = 256, SQK = 64, SLD = ST + 2;    // burst-load kernel: 32 x 32 tiles, 256-deep chunks in 64-deep quarters
constexpr int TSK_W = 256;                                   // width of the full-width tall-skinny kernels

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the product as launch_gemm's caller describes it (GemmArgs' fields, before any launch decision)
struct Product {
  int M = 0, N = 0, K = 0;
  int out_uplo = -1;                 // -1: full output; CAPI_UPPER / CAPI_LOWER: only that triangle (M == N)
  int tri_side = -1;                 // -1: none; CAPI_LEFT / CAPI_RIGHT: op(A) / op(B) is triangular
  int tri_eff_upper = 0, tri_dense = 0, tri_block = 0, tri_koff = 0;
  bool alpha_zero = false;
  double beta = 0.0;
  int batch = 0;
  bool ak = false, bkc = false;      // A transposed (k-contiguous), B k-contiguous
  bool a_is_b = false;               // A and B are the same pointer ...
  bool same_ld = false;              // ... with the same leading dimension
  bool a_vec = false, b_vec = false; // 16-byte loads legal for A / B (pointer and ld alignment)
  bool a_tiled = false, c_tiled = false;   // panel32 images (gemm_f64.hip, capi_dsyrk_panel32)
  bool ws_for_slab = true;           // split-K partials may go to the handle's primary workspace
};
struct Device { int num_cu = 256; int stream_cu = 0; };     // stream_cu: CUs of the current stream's mask, 0 = all
struct Modes { int rounds_mode = 0, pair_mode = 1, pair_rounds = 0, pair_rounds_min = 0; };   // the handle's (capi_set_launch_rounds)
struct Overrides { int force_ts = 0; int force_small = -1; };   // CAPI_FORCE_TS = 64 | 128 (0: free); CAPI_SMALL = 0 | 1 (-1: free)

enum class Path { none, scale, trmm_ts32, gram_blocks, gram_ts, small, tile, pair, refused };
enum class Reduce { none, narrow, wide };
inline const char* path_name(Path p) {
  static const char* const names[] = {"none", "scale", "trmm_ts32", "gram_blocks", "gram_ts", "small", "tile", "pair", "refused"};
  return names[(int)p];
}

struct Plan {
  Path path = Path::none;
  int ts = 0, splitk = 1, k_per_split = 0, k_rotate = 0, order = 0, share_ab = 0;
  int64_t slab_ld = 0, slab_stride = 0;   // split-K partials: splitk slabs of slab_stride doubles
  int tiles_m = 0, tiles_n = 0, ntiles = 0;   // the tiling (gram_blocks: of 256-blocks); ntiles excludes the tail's 128-tiles
  int64_t blocks = 0;                     // workgroups along x of the path's main launches together
  int64_t per_launch = 0;                 // at most this many per launch (== blocks: one launch; else resident rounds)
  int grid_y = 1;
  int tail128 = 0;                        // this many 128-tiles at the end go out re-cut into 64-tiles, in one unrecorded launch
  Reduce reduce = Reduce::none;
  size_t lds_bytes = 0;
  int variant = 0;                        // record variant of the tile / pair launches (capi_prof_collect)
  double share_den = 1.0;                 // a recorded launch of c workgroups carries c / share_den of the product's flops
  double est_us = 0.0, small_est_us = 0.0;   // the cost model's estimates
  bool recorded() const { return path == Path::tile || path == Path::pair; }
  int64_t launches() const { return per_launch ? cdiv(blocks, per_launch) : 0; }
  int64_t count(int64_t i) const { return blocks - i * per_launch < per_launch ? blocks - i * per_launch : per_launch; }
  double share(int64_t i) const { return (double)count(i) / share_den; }
};

inline int64_t count_tiles(const Product& p, int ts) {
  const int64_t tm = cdiv(p.M, ts), tn = cdiv(p.N, ts);
  return p.out_uplo < 0 ? tm * tn : tm * (tm + 1) / 2;
}

inline Plan plan(const Product& p, const Device& dev, const Modes& mode, const Overrides& ov) {
  Plan r;
  if (p.M <= 0 || p.N <= 0) return r;
  if (p.K <= 0 || p.alpha_zero) {
    if (p.beta != 1.0) r.path = Path::scale;
    return r;
  }
  const bool same_ab = p.a_is_b && p.same_ld;
  // tall-skinny right-TRMM (Q = A R^-1): persistent full-width workgroups of 32-row tiles, A read once
  if (p.tri_side == CAPI_RIGHT && p.tri_eff_upper && !p.ak && p.bkc && p.N == TSK_W && p.K == p.N && (int64_t)p.M >= 64 * (int64_t)p.N) {
    const int ntile = (int)cdiv(p.M, 32);
    r.path = Path::trmm_ts32;
    r.blocks = r.per_launch = ntile < dev.num_cu ? ntile : dev.num_cu;
    r.lds_bytes = sizeof(double) * 2 * 256 * 32;
    return r;
  }
  // Tall-skinny Gram matrix WIDER than the full-width kernel (CholeskyQR2 at n = 512..2048; config 5: n = 1024, K = 2^23): by 256-blocks.
  // The 128-tiling computes its diagonal tiles whole (36 tile-units for 32 at n = 1024: 11 % of the MFMAs produce the unwanted
  // triangle).  Here the diagonal 256-blocks go to the full-width kernel, whose 136-of-256 tile map wastes 6 % of a quarter of the
  // work, and the off-diagonal blocks are plain 256 x 256 products A_I^T A_J on the tile kernel (split-K; the four tiles of a slice
  // are consecutive arrivals on one XCD and share their panels in its L2).
  if (p.out_uplo == CAPI_UPPER && p.tri_side < 0 && p.ak && p.bkc && same_ab && p.N > TSK_W && p.N <= 2048 && p.N % TSK_W == 0 &&
      (int64_t)p.K >= 64 * (int64_t)p.N && p.ws_for_slab && p.batch <= 1) {
    r.path = Path::gram_blocks;
    r.tiles_m = r.tiles_n = p.N / TSK_W;
    r.ntiles = r.tiles_n * (r.tiles_n + 1) / 2;
    return r;
  }
  // tall-skinny Gram matrix: full-width workgroups (one resident per CU), the tall operand is read once
  if (p.out_uplo == CAPI_UPPER && p.tri_side < 0 && p.ak && p.bkc && same_ab && p.N <= TSK_W && p.N >= 64 &&
      (int64_t)p.K >= 64 * (int64_t)p.N && p.ws_for_slab) {
    const int64_t P = cdiv(p.K, BK);
    const int S = (int)(P / 32 < dev.num_cu ? (P / 32 > 0 ? P / 32 : 1) : dev.num_cu);
    r.path = Path::gram_ts;
    r.splitk = S;
    r.slab_ld = p.N;
    r.slab_stride = (int64_t)p.N * p.N;
    r.blocks = r.per_launch = S;
    r.lds_bytes = sizeof(double) * 2 * TSK_W * SK;
    r.reduce = S >= 16 && p.N <= 65535 ? Reduce::wide : (S > 1 ? Reduce::narrow : Reduce::none);
    return r;
  }
  // panel32 images are understood by the two full-width tall-skinny kernels above and by nothing below
  if (p.a_tiled || p.c_tiled) {
    r.path = Path::refused;
    return r;
  }
  // Choose tile size and split-K from a small cost model in CU-cycles.  One k-panel (16 deep) of a 128-tile keeps all
  // four MFMA pipes of a CU busy for 64 MFMAs x 64 cycles = 4096 cycles, of a 64-tile for 1024; co-resident workgroups
  // share the pipes, so a CU works through the tiles dealt to it at that rate whatever their number.  The makespan is
  // the busiest CU's queue: ceil(tiles / CUs) equal tiles, or for TRMM (k-range grows linearly along the triangular
  // dimension, longest-first dealing) the larger of the mean load and the single longest tile.
  const bool tri = p.tri_side >= 0;
  const int ncu = dev.stream_cu ? dev.stream_cu : dev.num_cu;
  const double ghz = 2.35;
  double best = 1e300;
  int best_ts = 128, best_s = 1;
  for (int ts : {128, 64}) {
    if (ov.force_ts && ov.force_ts != ts) continue;
    const double nt = (double)count_tiles(p, ts);
    const double cyc = ts == 128 ? 4096.0 : 1024.0;
    const double eff = ts == 128 ? 0.89 : 0.80;          // measured pipe utilisation of the two kernels (fast path)
    for (int sk = 1; sk <= 512; ++sk) {
      if (sk > 1 && (!p.ws_for_slab || p.K / sk < 256)) break;
      double busiest;                                     // cycles of work queued on the busiest CU
      if (!tri) {
        // a CU keeps `res` workgroups resident; the last, partially filled group of its queue runs without partners to
        // cover its barrier and load stalls (measured ~0.7x the paired rate for a lone 128-tile workgroup)
        const int64_t q = cdiv((int64_t)nt * sk, ncu);
        const int res = ts == 128 ? 2 : 4;
        const int64_t lone = q % res;
        const double per = ((double)p.K / sk / 16.0) * cyc;
        busiest = (double)(q - lone) * per + (double)lone * per / (lone == 0 ? 1.0 : (0.62 + 0.38 * (double)lone / res));
      } else {
        const double kmax = (double)p.K / sk, kavg = (0.5 * p.K + 0.5 * ts) / sk;
        const double mean = nt * sk * (kavg / 16.0) * cyc / ncu, longest = (kmax / 16.0) * cyc;
        busiest = mean * 1.08 > longest ? mean * 1.08 : longest;
      }
      double t = busiest / (ghz * 1e3 * eff) + 7.0;
      // operand panels stream from L2/MALL: ~4 TB/s effective when every tile re-reads its two panels
      // (a syrk's diagonal tiles stage one panel; a TRMM's triangular operand is small and stays cache resident)
      const double keff = tri ? 0.5 * p.K + 0.5 * ts : (double)p.K;
      const double panels = (p.out_uplo >= 0 && p.a_is_b) ? 2.0 * nt - (double)cdiv(p.N, ts) : (tri ? 1.0 * nt : 2.0 * nt);
      // (operands that fit the 256 MB Infinity Cache are re-read from there at roughly twice the HBM-side rate)
      const double footprint = ((p.a_is_b ? 0.0 : (double)p.M) + (double)p.N) * (double)p.K * 8.0;
      double t_mem = panels * ts * keff * 8.0 / (footprint <= 192.0e6 ? 8.0e6 : 4.0e6);
      // a split-K slice whose tiles all fit one XCD's resident set (<= 32 tiles: consecutive pids, started together, walking the
      // same panels in step) shares those panels in that L2: a tall product then streams each operand about once
      if (!tri && nt <= 32.0 && (double)p.K >= 64.0 * (double)(p.M > p.N ? p.M : p.N)) t_mem = footprint / 4.0e6;
      if (t_mem > t) t = t_mem;
      if (sk > 1) t = 1.12 * t + 6.0 + (double)(sk + 2) * (double)p.M * (double)p.N * (p.out_uplo >= 0 ? 0.5 : 1.0) * 8.0 / 2.5e6;
      if (t < best) { best = t; best_ts = ts; best_s = sk; }
    }
  }
  r.est_us = best;
  const int vi = (p.ak ? 2 : 0) + (p.bkc ? 1 : 0);
  // latency-bound sizes go to the burst-load 32-tile kernel: one workgroup per CU (139 KB of LDS), per 256-deep chunk
  // ~2 us of exposed load latency + 64 MFMAs per wave
  {
    const double nt32 = (double)cdiv(p.M, ST) * (double)cdiv(p.N, ST) * (p.out_uplo >= 0 ? 0.5 : 1.0);
    const double keff = tri ? 0.5 * p.K + 16.0 : (double)p.K;
    const double chunks = keff / SKC < 1.0 ? 1.0 : keff / SKC;
    r.small_est_us = (double)cdiv((int64_t)nt32, dev.num_cu) * (chunks * 2.0 + keff * (16.0 / 2200.0) * 4.0 / 4.0) + 3.0;
    bool use_small = p.M <= 512 && p.N <= 512 && p.K <= 2048;      // measured: 1.5-2x faster up to order 512, slower from 1024
    // thin products of the blocked factorization (K <= 256: a 128-row panel against up to ~2000 columns, its trailing
    // update): one staged chunk, LDS sized by K, so two workgroups share a CU at K <= 128; up to three rounds of those slots
    if (!use_small && p.K <= SKC && p.batch <= 1) {
      const double slots = (double)dev.num_cu * (p.K <= 128 ? 2.0 : 1.0);
      use_small = nt32 <= 3 * slots;
    }
    if (ov.force_small >= 0) use_small = ov.force_small != 0 && p.M <= 4096 && p.N <= 4096;
    if (use_small) {
      const int kcap = p.K >= SKC ? SKC : (int)(cdiv(p.K, SQK) * SQK);      // staged depth: LDS holds 2 x kcap x SLD doubles
      r.path = Path::small;
      r.ts = kcap;
      r.tiles_m = (int)cdiv(p.M, ST);
      r.tiles_n = (int)cdiv(p.N, ST);
      r.ntiles = r.tiles_m * r.tiles_n;
      r.blocks = r.per_launch = r.ntiles;
      r.grid_y = p.batch > 1 ? p.batch : 1;
      r.lds_bytes = sizeof(double) * 2 * (size_t)kcap * SLD;
      r.variant = vi;
      return r;
    }
  }
  r.path = Path::tile;
  r.ts = best_ts;
  r.tiles_m = (int)cdiv(p.M, r.ts);
  r.tiles_n = (int)cdiv(p.N, r.ts);
  r.ntiles = (int)count_tiles(p, r.ts);
  r.share_ab = p.out_uplo >= 0 && same_ab && p.ak == p.bkc;
  r.order = p.out_uplo >= 0 && r.tiles_n >= 16;          // a triangular output's tiles in bands of 8 tile rows
  r.k_per_split = p.K;
  if (best_s > 1) {
    const int64_t kps = cdiv(cdiv(p.K, best_s), BK) * BK;
    const int64_t sk = cdiv(p.K, kps);
    if (sk > 1) {
      r.splitk = (int)sk;
      r.k_per_split = (int)kps;
      r.k_rotate = !tri;
      r.slab_ld = p.M;
      r.slab_stride = (int64_t)p.M * p.N;
      r.reduce = Reduce::narrow;
    }
  }
  // Resident rounds (plain products).  A launch with more tiles than the chip holds (2 per CU) refills slots one by one as tiles
  // finish: within a few tile lengths the starts are smeared and tiles that share an operand panel are no longer within the ~2
  // iterations an XCD's 4 MiB L2 can bridge (its 64 resident tiles pull 2 MiB of panels through it per iteration).  One launch per
  // round restarts every XCD's 64 tiles together, as an 8 x 8 block of the tile grid (tile_of_dims' bands): 16 panels serve 64
  // tiles.  dgemm 16384^3: FETCH 139 -> 76 GB (the 8-way ideal is 69), time unchanged (118.7 vs 119.0 ms): the tiles of a plain
  // product do equal work, so the round boundary costs nothing measurable.  Triangular outputs were tried the same way (8 x 8
  // super-blocks of the triangle, 8 per round; bit 1 of rounds_mode): FETCH of the n = 32768 step 310 -> 263 GB only, dsyrk 16384
  // 62.6 -> 64.2 ms, step 237 -> 242 ms (partial rounds, diagonal super-blocks with 36 live tiles): not kept.  TRMM tiles have unequal
  // k-ranges and keep the longest-first free-running order.  OFF by default (CAPI_ROUNDS=1 turns it on; cholinv::factor
  // turns rounds on for its own call, capi_set_launch_rounds): when this was measured the only plain products inside cholinv were the
  // rectangles of a since-removed second-stream schedule -- the step's fabric traffic fell by 5 % (3625 -> 3437 GB at n = 65536), its
  // time did not change, and the per-launch durations the roofline was computed from stretched (0.876 -> 0.825 on the same box).
  // (The 256-column block launches of a tall right-TRMM were tried the same way: a round there is 512 tiles of K <= 1024, ~0.15 ms, and
  //  the launch boundaries cost 11 %: 35.1 -> 39.2 ms at m = 2^21, n = 1024.)
  const int per_round = 2 * ncu;
  const bool use_rounds = r.ts == 128 && r.splitk == 1 && !tri && per_round % 16 == 0 && p.batch <= 1 && r.ntiles >= 2 * per_round &&
                          (p.out_uplo < 0 ? (mode.rounds_mode & 1) != 0 : ((mode.rounds_mode & 2) != 0 && r.order));
  // A 128-tiling fills the chip in rounds of 2 x CUs workgroups; the last round is usually partial and its lone
  // workgroups run at ~0.6 of the paired rate (8256 tiles = 16 rounds + 64: those 64 cost almost another round).  The
  // tail is re-cut into 64-tiles (4x the workgroups, a quarter of the length) and launched right behind the full rounds.
  if (r.ts == 128 && r.splitk == 1 && !tri) {
    const int rem = r.ntiles % per_round;
    if (r.ntiles >= 2 * per_round && rem > 0 && rem <= (3 * per_round) / 4) r.tail128 = rem;
  }
  const int ntiles_all = r.ntiles;
  r.ntiles -= r.tail128;
  r.blocks = (int64_t)r.ntiles * r.splitk;
  r.per_launch = use_rounds ? per_round : r.blocks;
  r.lds_bytes = sizeof(double) * 2 * 2 * (size_t)r.ts * SK;
  r.variant = vi + (r.ts == 128 ? 0 : 4);
  r.share_den = (double)ntiles_all * r.splitk;
  // TRMM in tile pairs (dtrmm_pair_kernel): equal work per workgroup, the launch of a plain product.  Measured (tools/pair_window.py, all
  // three forms of the recursion): a launch of exactly one resident round +8..10 % (order 4096: 63 -> 68.5 TFLOP/s; 2048 x 8192: 51..55 ->
  // 55..59), two rounds +2..3 %, four +0.5..1 %, nine +-0.5 %; a launch that is NOT whole rounds loses (1152 workgroups, order 6144: 68.3
  // -> 61.5 -- the equal, long workgroups of the last 128 cost a third round).  L2-to-fabric traffic does not change (order 32768:
  // 2 x FETCH_SIZE 1.19 -> 1.22 TB).  Pairs therefore run up to four whole rounds (pair_mode 2: whenever the launch is whole rounds; 0:
  // never); larger products keep the longest-first order.  Pairs do equal work, so a launch can also go out one resident round (512
  // workgroups: an 8 x 8 block of pair-tiles per XCD) at a time at no cost in time, and every round's tiles start -- and, walking equal
  // k-ranges, stay -- together: the panels an XCD's 64 tiles share are fetched once instead of once per drifting tile (pair_rounds, from
  // K = pair_rounds_min on).
  const int ntri = p.tri_side == CAPI_LEFT ? r.tiles_m : r.tiles_n, nfree = p.tri_side == CAPI_LEFT ? r.tiles_n : r.tiles_m;
  const int64_t wgs = (int64_t)(ntri / 2) * nfree;
  if (mode.pair_mode && tri && !p.tri_dense && !p.tri_block && p.tri_koff == 0 && r.ts == 128 && r.splitk == 1 && p.beta == 0.0 &&
      p.batch <= 1 && p.M % 128 == 0 && p.N % 128 == 0 && p.K % 128 == 0 && p.a_vec && p.b_vec && (ntri & 1) == 0 && wgs % per_round == 0 &&
      (mode.pair_mode > 1 || wgs <= 4 * per_round || (mode.pair_rounds && p.K >= mode.pair_rounds_min))) {
    r.path = Path::pair;
    r.blocks = wgs;
    r.per_launch = mode.pair_rounds && wgs > per_round && p.K >= mode.pair_rounds_min ? per_round : wgs;
    r.variant = vi + 16;
    r.share_den = (double)wgs;
  }
  return r;
}

// one line: the product, the device, the modes and the plan (CAPI_DEBUG_GEMM; the product part is the planner test's input syntax)
inline int format(char* buf, size_t n, const Product& p, const Device& d, const Modes& m, const Overrides& o, const Plan& r) {
  static const char* const reduce_names[] = {"none", "narrow", "wide"};
  return snprintf(buf, n,
                  "M=%d N=%d K=%d out_uplo=%d tri_side=%d tri_eff_upper=%d tri_dense=%d tri_block=%d tri_koff=%d alpha_zero=%d beta=%.17g "
                  "batch=%d ak=%d bkc=%d a_is_b=%d same_ld=%d a_vec=%d b_vec=%d a_tiled=%d c_tiled=%d ws_for_slab=%d num_cu=%d stream_cu=%d "
                  "rounds_mode=%d pair_mode=%d pair_rounds=%d pair_rounds_min=%d force_ts=%d force_small=%d -> path=%s ts=%d splitk=%d "
                  "k_per_split=%d k_rotate=%d order=%d share_ab=%d slab_stride=%lld tiles_m=%d tiles_n=%d ntiles=%d blocks=%lld "
                  "per_launch=%lld launches=%lld grid_y=%d tail128=%d reduce=%s lds=%zu variant=%d share_den=%.17g est_us=%.1f small_est_us=%.1f",
                  p.M, p.N, p.K, p.out_uplo, p.tri_side, p.tri_eff_upper, p.tri_dense, p.tri_block, p.tri_koff, (int)p.alpha_zero, p.beta,
                  p.batch, (int)p.ak, (int)p.bkc, (int)p.a_is_b, (int)p.same_ld, (int)p.a_vec, (int)p.b_vec, (int)p.a_tiled, (int)p.c_tiled,
                  (int)p.ws_for_slab, d.num_cu, d.stream_cu, m.rounds_mode, m.pair_mode, m.pair_rounds, m.pair_rounds_min, o.force_ts,
                  o.force_small, path_name(r.path), r.ts, r.splitk, r.k_per_split, r.k_rotate, r.order, r.share_ab, (long long)r.slab_stride,
                  r.tiles_m, r.tiles_n, r.ntiles, (long long)r.blocks, (long long)r.per_launch, (long long)r.launches(), r.grid_y, r.tail128,
                  reduce_names[(int)r.reduce], r.lds_bytes, r.variant, r.share_den, r.est_us, r.small_est_us);
}

}  // namespace gemm_plan

#endif  // CAPITAL_GEMM_PLAN_H_
