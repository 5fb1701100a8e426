// Prints the launch plan (csrc/conv_plan.cpp) of each f16x3 convolution read from stdin: which kernel a DiMP layer
// runs on, with its grid, LDS and K split, without a GPU.  One shape per line as key=value words; unnamed keys keep
// their defaults:
//   N H W Cin Cout kh=1 kw=kh stride=1 pad=0 Kp (the shape's own; Cin + Cin2 for a fused downsample) G=1 pool=0
//   Cin2=0 H2=0 W2=0 stride2=0 (the fused downsample) ws=-1 (bytes of split-K workspace; -1: as much as wanted)
//   nosplit=0 nopatch=0 old=0 (MMT_CONV_NOSPLIT / NOPATCH / OLD); "env=1" reads them from the environment instead,
//   as the library does.
// Output per line: "<kernel> bn= ks= grid=x,y,z lds= ws= reduce= out=HoxWo tpi= px= tiles=YxX pooled=HxW" or
// "error: <why>".
//   echo "N=32 H=18 W=18 Cin=1024 Cout=512 kh=3 pad=1" | tests/bin/conv_plan_print
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>

#include "conv_plan.h"

using namespace mmt;

int main() {
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    if (line[0] == '#' || line[0] == '\n') continue;
    ConvProblem p{0, 0, 0, 0, 0, 1, -1, 1, 0, -1, 1, false, 0, 0, 0, 0, SIZE_MAX};
    ConvKnobs k;
    int pool = 0, nosplit = 0, nopatch = 0, old = 0;
    long long ws = -1;
    std::istringstream in(line);
    std::string w;
    bool bad = false;
    while (in >> w) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos) { bad = true; break; }
      const std::string key = w.substr(0, eq);
      const long long v = atoll(w.c_str() + eq + 1);
      struct { const char* name; int* f; } ints[] = {
          {"N", &p.N}, {"H", &p.H}, {"W", &p.W}, {"Cin", &p.Cin}, {"Cout", &p.Cout}, {"kh", &p.kh}, {"kw", &p.kw},
          {"stride", &p.stride}, {"pad", &p.pad}, {"Kp", &p.Kp}, {"G", &p.G}, {"pool", &pool}, {"Cin2", &p.Cin2},
          {"H2", &p.H2}, {"W2", &p.W2}, {"stride2", &p.stride2}, {"nosplit", &nosplit}, {"nopatch", &nopatch}, {"old", &old}};
      bool found = false;
      for (auto& i : ints)
        if (key == i.name) *i.f = (int)v, found = true;
      if (key == "ws") ws = v, found = true;
      if (key == "env") k = conv_knobs_from_env(), found = true;
      if (!found) { bad = true; break; }
    }
    if (bad) {
      printf("error: bad line (key=value words): %s\n", w.c_str());
      continue;
    }
    if (p.kw < 0) p.kw = p.kh;
    if (p.Kp < 0) p.Kp = p.Cin2 ? p.Cin + p.Cin2 : (int)conv_kp(p.Cin, p.kh, p.kw);
    p.pool = pool != 0;
    p.ws_bytes = ws < 0 ? SIZE_MAX : (size_t)ws;
    k.nosplit |= nosplit != 0, k.nopatch |= nopatch != 0, k.old_generic |= old != 0;
    const ConvPlan r = conv_plan(p, k);
    if (r.error) printf("error: %s\n", r.error);
    else
      printf("%s bn=%d ks=%d grid=%u,%u,%u lds=%zu ws=%zu reduce=%d out=%dx%d tpi=%d px=%d tiles=%dx%d pooled=%dx%d\n",
             conv_kernel_name(r.kernel), r.bn, r.ks, r.grid[0], r.grid[1], r.grid[2], r.lds_bytes, r.ws_needed,
             (int)r.reduce, r.Ho, r.Wo, r.tiles_per_img, r.patch_px, r.tiles_y, r.tiles_x, r.PHo, r.PWo);
  }
  return 0;
}
