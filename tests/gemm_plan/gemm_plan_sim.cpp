// gemm_plan_sim.cpp -- TEST PROGRAM (tests/test_gemm_plan.py): launch_gemm's planner (capital_amd/csrc/gemm_plan.h) on the CPU.
// Reads one product per line on stdin as key=value tokens (the names of gemm_plan::Product, Device, Modes and Overrides; anything after
// "->" is ignored, so a CAPI_DEBUG_GEMM line can be fed back as it is) and prints, per line, the planner's one-line description of the
// plan followed by " shares=s0,s1,..." (the flop share of every recorded launch).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../capital_amd/csrc/gemm_plan.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    gemm_plan::Product p;
    gemm_plan::Device d;
    gemm_plan::Modes m;
    gemm_plan::Overrides o;
    std::map<std::string, int*> ints = {
        {"M", &p.M}, {"N", &p.N}, {"K", &p.K}, {"out_uplo", &p.out_uplo}, {"tri_side", &p.tri_side}, {"tri_eff_upper", &p.tri_eff_upper},
        {"tri_dense", &p.tri_dense}, {"tri_block", &p.tri_block}, {"tri_koff", &p.tri_koff}, {"batch", &p.batch}, {"num_cu", &d.num_cu},
        {"stream_cu", &d.stream_cu}, {"rounds_mode", &m.rounds_mode}, {"pair_mode", &m.pair_mode}, {"pair_rounds", &m.pair_rounds},
        {"pair_rounds_min", &m.pair_rounds_min}, {"force_ts", &o.force_ts}, {"force_small", &o.force_small}};
    std::map<std::string, bool*> bools = {
        {"alpha_zero", &p.alpha_zero}, {"ak", &p.ak}, {"bkc", &p.bkc}, {"a_is_b", &p.a_is_b}, {"same_ld", &p.same_ld}, {"a_vec", &p.a_vec},
        {"b_vec", &p.b_vec}, {"a_tiled", &p.a_tiled}, {"c_tiled", &p.c_tiled}, {"ws_for_slab", &p.ws_for_slab}};
    std::istringstream in(line);
    std::string tok;
    while (in >> tok && tok != "->") {
      const size_t eq = tok.find('=');
      const std::string key = tok.substr(0, eq);
      const char* val = eq == std::string::npos ? "" : tok.c_str() + eq + 1;
      if (ints.count(key)) *ints[key] = atoi(val);
      else if (bools.count(key)) *bools[key] = atoi(val) != 0;
      else if (key == "beta") p.beta = strtod(val, nullptr);
      else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
    }
    const gemm_plan::Plan r = gemm_plan::plan(p, d, m, o);
    char buf[2048];
    gemm_plan::format(buf, sizeof(buf), p, d, m, o, r);
    std::string shares;
    for (int64_t i = 0; r.recorded() && i < r.launches(); ++i) {
      char v[32];
      snprintf(v, sizeof(v), "%s%.17g", i ? "," : "", r.share(i));
      shares += v;
    }
    printf("%s shares=%s\n", buf, shares.c_str());
  }
  return 0;
}
