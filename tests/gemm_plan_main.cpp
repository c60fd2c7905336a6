// Reads GEMM dispatch queries from stdin (the format of tests/gemm_plan_checks.py: a label, the integers of a GemmQuery, the integers of a GemmKnobs) and
// prints gemm_plan's answer, one line per query.  Host-only: built and run by tests/test_gemm_plan_cpu.py.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "gemm_plan.h"

int main() {
  static const char* routes[] = {"refused", "skinny", "reg", "reg_sliced", "glds", "pp", "pp_sliced"};
  static const char* exts[] = {"none", "ktile", "slab", "second"};
  static const char* reduces[] = {"none", "plain", "norm", "nb", "dl"};
  std::string line, label;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream is(line);
    long v[39];
    is >> label;
    for (long& x : v)
      if (!(is >> x)) { fprintf(stderr, "bad query line: %s\n", line.c_str()); return 2; }
    GemmQuery q;
    int i = 0;
    q.M = (int)v[i++]; q.N = (int)v[i++]; q.K = (int)v[i++]; q.batch1 = v[i++]; q.batch2 = v[i++];
    q.trans_a = v[i++]; q.trans_w = v[i++]; q.out_f32 = v[i++]; q.bias = v[i++]; q.gamma = v[i++]; q.residual = v[i++];
    q.act = (int)v[i++]; q.alpha_one = v[i++]; q.ext = v[i++]; q.a_norm = v[i++]; q.a_swiglu = v[i++];
    q.ldc = v[i++]; q.ldr = v[i++]; q.ldn = v[i++]; q.stride_c = v[i++];
    q.ws = v[i++]; q.ws_aligned = v[i++]; q.ws_bytes = v[i++]; q.norm_ptrs_aligned = v[i++];
    q.tail = (int)v[i++]; q.fx = (int)v[i++]; q.ncu = v[i++];
    GemmKnobs k;
    k.variant = (int)v[i++]; k.skew = (int)v[i++]; k.split = (int)v[i++]; k.no_t160 = v[i++]; k.no_rsplit = v[i++];
    k.group_m = (int)v[i++]; k.skinny_sk = (int)v[i++]; k.norm_wg_max = v[i++];
    k.no_fx = v[i++]; k.no_nb = v[i++]; k.no_dl = v[i++]; k.no_norm_fuse = v[i++];
    const GemmPlan p = gemm_plan(q, k);
    if (p.route == ROUTE_REFUSED) { printf("%s refused\n", label.c_str()); continue; }
    const char* kernel = p.route == ROUTE_SKINNY ? "skinny" : p.kernel == K_REG ? "reg" : p.kernel == K_GLDS ? "glds" : p.kernel == K_PP256 ? "pp256" : p.kernel == K_PP128 ? "pp128" : "t160";
    printf("%s route=%s kernel=%s slices=%d rows=%d ksplit=%d tiles=%dx%d group_m=%d ext=%s reduce=%s cpt=%d fx=%d tail_done=%d launches=%d tag=%ld\n", label.c_str(),
           routes[p.route], kernel, p.slices, p.skinny_rows, (int)p.skinny_ksplit, p.tiles_m, p.tiles_n, p.group_m, exts[p.ext], reduces[p.reduce], p.cpt, (int)p.fx_fused,
           (int)p.tail_done, p.launches, p.tag);
  }
  return 0;
}
