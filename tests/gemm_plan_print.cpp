// Prints the GEMM plan (csrc/gemm_plan.cpp) of each shape read from stdin: which tile a GEMM of the path runs on,
// without a GPU.  One shape per line as key=value words; unnamed keys keep their defaults:
//   M N K groups=1 amode=0 epi=0 split=1 conc=1 ws=1 (a 4 Mi-float split-K workspace) ws_elems defer=0
//   cus=256 force=-1, and any tuning knob by its variable name (MMT_T320=0 ...); "env=1" reads the knobs from the
//   environment instead, as the library does.
// Output per line: "<tile> ks=<K slices> defer=<0|1> gm=<super-tile rows>" or "error: <why>".
//   echo "M=3904 N=768 K=3072 epi=2 conc=2" | tests/bin/gemm_plan_print
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>

#include "gemm_plan.h"

using namespace mmt;

int main() {
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    if (line[0] == '#' || line[0] == '\n') continue;
    GemmShape s{0, 0, 0, 1, A_DENSE, EPI_BF16, 1, 1, 1, 4 << 20, 0};
    GemmKnobs k;
    int cus = 256, force = -1;
    std::istringstream in(line);
    std::string w;
    bool bad = false;
    while (in >> w) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos) { bad = true; break; }
      const std::string key = w.substr(0, eq);
      const long long v = atoll(w.c_str() + eq + 1);
      struct { const char* name; int* f; } ints[] = {
          {"M", &s.M}, {"N", &s.N}, {"K", &s.K}, {"groups", &s.groups}, {"amode", &s.amode}, {"epi", &s.epi},
          {"split", &s.split}, {"conc", &s.conc}, {"ws", &s.has_ws}, {"defer", &s.defer_reduce}, {"cus", &cus},
          {"force", &force}, {"MMT_SPLIT_CFG", &k.split_cfg}, {"MMT_256S_MIN", &k.t256_min},
          {"MMT_RESID_256S", &k.resid_256s}, {"MMT_T320", &k.t320}, {"MMT_W256", &k.w256},
          {"MMT_PERSIST_MIN", &k.persist_min}, {"MMT_SPLIT_T128", &k.split_t128}, {"MMT_T192", &k.t192},
          {"MMT_SPLITK_TILES", &k.splitk_tiles}, {"MMT_SPLITK_TARGET", &k.splitk_target},
          {"MMT_SPLITK_MINKT", &k.splitk_minkt}, {"MMT_SPLITK_MAX", &k.splitk_max}, {"MMT_GM", &k.gm},
          {"MMT_GM_LONGK", &k.gm_longk}, {"MMT_GM256", &k.gm256}};
      bool found = false;
      for (auto& i : ints)
        if (key == i.name) *i.f = (int)v, found = true;
      if (key == "ws_elems") s.ws_elems = v, found = true;
      if (key == "env") k = gemm_knobs_from_env(), found = true;
      if (!found) { bad = true; break; }
    }
    if (bad || s.M <= 0 || s.N <= 0 || s.K <= 0 || cus <= 0) {
      printf("error: bad line (key=value words, M N K > 0): %s\n", w.c_str());
      continue;
    }
    if (!s.has_ws) s.ws_elems = 0;
    const GemmPlan p = gemm_plan(s, k, cus, force);
    if (p.error) printf("error: %s\n", p.error);
    else printf("%s ks=%d defer=%d gm=%d\n", gemm_tile_name(p.tile), p.ksplit, (int)p.defer, p.gm);
  }
  return 0;
}
