// The decision of one llmseg_gemm_bf16 call, host-only: which kernel, how many K-slices, how the extension operands and the caller's fused tail are
// handled, how many launches -- everything gemm.hip's gemm_dispatch needs to launch without deciding anything further.  No HIP include and no device
// code: this header compiles with a plain C++17 compiler, and tests/test_gemm_plan_cpu.py pins gemm_plan's answers for the workload's shapes and the
// edges in tests/golden/gemm_plans.txt.  A change of a constant or a condition here shows as a diff of that file before it shows on a GPU.
#pragma once
#include <algorithm>
#include <cstdlib>

// The kernel of one product.  The numeric values are those of the tuning knob (llmseg_gemm_set_variant; tests and tools pass them as integers).
enum GemmKernel {
  K_REG = 0,       // R: register staging 128 x 128 (any layout, any K % 8 == 0)
  K_GLDS = 2,      // G: LDS-DMA 128 x 128
  K_AUTO = 5,      // the cost model decides (never launched)
  K_PP256 = 8,     // Q: ping-pong 256 x 256
  K_PP128 = 9,     // Q2: two-phase 128 x 256
  K_T160 = 10,     // T: two-phase 160 x 256, K-slices only
};
constexpr int T160_BM = 160, GEMM_BK = 64, GEMM_BN = 128;      // rows of the 160 x 256 tile; K-tile of every tile kernel; columns of the 128 x 128 tiles
constexpr int GEMM_ACT_NONE = 0, GEMM_FX_ROPE = 1, GEMM_FX_SWIGLU = 2;      // llmseg_hip.h's LLMSEG_ACT_NONE, LLMSEG_FX_ROPE, LLMSEG_FX_SWIGLU (gemm.hip asserts these)
inline bool is_pp(GemmKernel k) { return k == K_PP256 || k == K_PP128 || k == K_T160; }      // the 8-wave LDS-DMA tiles, 256 columns wide, one workgroup per CU
inline int pp_rows(GemmKernel k) { return k == K_PP256 ? 256 : k == K_T160 ? T160_BM : 128; }
inline GemmKernel kernel_of_knob(int v) { return v == K_REG || v == K_GLDS || is_pp((GemmKernel)v) ? (GemmKernel)v : K_AUTO; }      // unknown value -> cost model

// Cost model of the K % 64 == 0 kernels (microseconds; constants fitted to tools/gemm_bench.py on MI355X, profiles/r02*_gemm*.txt).
// One ping-pong workgroup owns a CU: a K-tile of the 256 x 256 kernel takes ~1.7 us (1.25 PF/s over 256 CUs), of the 128 x 256
// kernel ~1.0 us; prologue + epilogue ~7 / 4.5 us.  The 128 x 128 kernel shares a CU between up to 4 workgroups (2.4 us per K-tile
// each when all four are resident, latency-bound 1.3 us when alone).
// bm = the tile's rows: 256 / 128 / 160.  The 160 x 256 kernel competes for K-slice plans only.  Its K-tile measures ~1.3 x the 128-row one (slope of
// the per-call time over the 638-row shapes, profiles/r07a_gemm_t160.txt), but 4 x 16 x 4 = 256 workgroups fill every CU where 5 x 16 x 3 left 16 idle,
// and on all five N = 4096 shapes 160 x 256 x 4 slices beats 128 x 256 x 3 by 5-13 % per call: 1.13 is the price that reproduces that ordering.
constexpr double T160_KT_US = 1.13;
inline double pp_cost(long M, long N, int nt, int bm, int S, long ncu, bool f32out) {
  const long tiles = ((M + bm - 1) / bm) * ((N + 255) / 256);
  const long rounds = (tiles * S + ncu - 1) / ncu;
  const int q = (nt + S - 1) / S;
  // (round 5: re-fitting these constants to the two-phase kernel from two isolated shapes -- 0.8 + 6.4 / 1.64 + 4.5 -- moved the K-slice plans of
  // the Llama N = 4096 shapes and cost 4 % at 2 images, 6 % at 24: measured and reverted, profiles/r05g_gemm_dispatch.md)
  const double it = bm == 256 ? 1.7 : bm == 160 ? T160_KT_US : 1.0, fix = (bm == 256 ? 7.0 : 4.5) + ((S > 1 || f32out) ? 1.0 : 0.0);
  // Round 5: without K-slices a partially filled last round is priced at 0.5 + 0.5 x its fill instead of a whole round -- a CU that shares the
  // fabric with fewer neighbours fetches its operands faster (measured, tools/gemm_bench.py at the 2-image shapes: 8192 x 1280 x 1280 on 160
  // workgroups of 256 x 256 takes 35 us, not 41; the whole-round price made the 128 x 256 tile win SAM proj / lin1 / q|k|v-windows, where the
  // 256 x 256 tile measures +9 / +6 / +5 %).  K-sliced plans keep the whole-round price their slice counts were tuned with.
  double eff_rounds = (double)rounds;
  if (S == 1) {
    const long full = tiles / ncu, rem = tiles - full * ncu;
    eff_rounds = (double)full + (rem ? 0.5 + 0.5 * (double)rem / (double)ncu : 0.0);
  }
  double us = eff_rounds * (q * it + fix);
  if (S > 1) us += 2.5 + ((double)(S + 1) * M * N * 4.0) / 4.0e6;     // reduce launch: slabs read once (mostly from the Infinity Cache)
  return us;
}
inline double glds_cost(long M, long N, int nt, long ncu) {
  const long tiles = ((M + 127) / 128) * ((N + 127) / 128);
  const long full = tiles / (4 * ncu), rem = tiles - full * 4 * ncu;
  double us = (double)full * (nt * 2.4 + 4.0);
  if (rem > 0) { const double w = (double)((rem + ncu - 1) / ncu); us += nt * std::max(1.3, 0.6 * w) + 4.0; }
  return us;
}
inline bool split_ok(int nt, int S) {       // every slice needs >= 2 K-tiles (the kernel's pipeline depth)
  if (S <= 1) return S == 1;
  const int q = (nt + S - 1) / S;
  return q >= 2 && nt - (S - 1) * q >= 2;
}
// ---- the tuning and A/B switches: the environment is read once, llmseg_gemm_set_variant (tools/gemm_bench.py) sets the first three -----------------------
struct GemmKnobs {
  // the word of llmseg_gemm_set_variant: bits 0-3 a GemmKernel value (10 needs a forced slice count; anything else = 5, the default = cost model), bits 4-7 =
  // XCD skew + 1 (0 keeps the skew), bits 8-12 = forced split-K slice count for 8 / 9 / 10.  Higher bits are ignored.
  int variant = K_AUTO, skew = 13, split = 0;
  bool no_t160 = false, no_rsplit = false;      // LLMSEG_GEMM_NO_T160 / _NO_RSPLIT: no 160 x 256 K-slice plans in the cost model / no K-slices for the register-staging kernel
  int group_m = 0, skinny_sk = 1;      // LLMSEG_GEMM_GROUP_M: row tiles per group of the ping-pong tile walk (0 = by shape); LLMSEG_SKINNY_SK: 0 = the skinny kernel's waves never split K, 2 = wherever K >= 2048
  long norm_wg_max = 2048;       // LLMSEG_NORM_WG_MAX: llmseg_norm runs its workgroup-per-row kernel below this row count
  bool no_fx = false, no_nb = false, no_dl = false, no_norm_fuse = false;      // LLMSEG_GEMM_NO_FX / _NB / _DL / _NORM_FUSE: always the product + the tail's own launches
};
inline GemmKnobs& gemm_knobs() {      // the process's knobs: the environment is read at the first call
  static GemmKnobs k = [] {
    GemmKnobs e;
    auto on = [](const char* n) { return getenv(n) != nullptr; };
    auto num = [](const char* n, long dflt) { const char* v = getenv(n); return v ? atol(v) : dflt; };
    e.no_t160 = on("LLMSEG_GEMM_NO_T160"); e.no_rsplit = on("LLMSEG_GEMM_NO_RSPLIT"); e.group_m = (int)num("LLMSEG_GEMM_GROUP_M", 0);
    e.skinny_sk = (int)num("LLMSEG_SKINNY_SK", 1); e.norm_wg_max = num("LLMSEG_NORM_WG_MAX", 2048);
    e.no_fx = on("LLMSEG_GEMM_NO_FX"); e.no_nb = on("LLMSEG_GEMM_NO_NB"); e.no_dl = on("LLMSEG_GEMM_NO_DL"); e.no_norm_fuse = on("LLMSEG_GEMM_NO_NORM_FUSE");
    return e;
  }();
  return k;
}
inline void gemm_set_variant(int v) {
  GemmKnobs& k = gemm_knobs();
  k.variant = v & 15; k.split = (v >> 8) & 31; k.skew = ((v >> 4) & 15) ? ((v >> 4) & 15) - 1 : k.skew;
}
// ---- the profiling tag: slices * 10000 + class * 1000 + flags; capi.cpp groups its records by class and names the dominant one ------------------------------
inline int gemm_tag_class(GemmKernel k) { return k == K_PP128 ? 7 : k == K_T160 ? 6 : (int)k; }
inline long gemm_tag(int cls, bool ta, bool tw, bool res, int act, bool f32, bool batched, int slices) {
  return cls * 1000 + (ta ? 200 : 0) + (tw ? 100 : 0) + (res ? 20 : 0) + act * 2 + (f32 ? 1 : 0) + 40 * batched + 10000 * (slices > 1 ? slices : 0);
}
inline long gemm_tag_class_of(long tag) { return (tag % 10000) / 1000; }
inline long gemm_tag_slices(long tag) { return tag / 10000; }      // K-slices of the call (0 = none)
inline const char* gemm_class_name(long cls) {                     // '*' stands for the OUT_F32 template argument
  static const char* names[] = {"gemm_bf16_tn_kernel<*, ...> (register staging, 128x128)", "?", "gemm_bf16_tn_glds_kernel<*, 2, 1>", "gemm_skinny_kernel<M>", "?", "?", "gemm_bf16_tn_t160_kernel (K-sliced)", "gemm_bf16_tn_pp2_kernel<*, false>",
                                "gemm_bf16_tn_pp_kernel<*, false, 4>", "gemm_bf16_tn_pp_kernel<*, false, 2>"};
  return (cls >= 0 && cls < 10) ? names[cls] : "?";
}
// ---- query and plan -------------------------------------------------------------------------------------------------------------------------------------
// The fused tail of one llmseg_gemm_bf16 call: the work the caller wants behind the product (a second output, or a pointwise pass over C).  The plan says
// whether the K-sliced reduce launch (NORM / NB / DL) or the fused-epilogue kernel (FX) does it; otherwise the entry function runs the launches it stands for.
enum GemmTailKind {
  TAIL_NONE,
  TAIL_NORM,       // llmseg_gemm_args.norm_out: RMSNorm(C) * norm_w
  TAIL_NB,         // .nb_x: C = norm_bwd(product [+ LoRA term]) + nb_dres
  TAIL_DL,         // .dl_o: delta = rowsum(dO * O) per head
  TAIL_FX,         // .fx: RoPE / SwiGLU / SwiGLU backward in the epilogue
};
struct GemmQuery {      // what the decision reads of one gemm_dispatch call: integers and flags, no pointers
  int M, N, K, act;
  long batch1, batch2, ncu;                             // batch counts >= 1
  bool trans_a, trans_w, out_f32, bias, gamma, residual, alpha_one /* alpha == 1 */, ext /* A2 / W2 */, a_norm, a_swiglu /* the A-row transforms */;
  long ldc, ldr /* 0 without a residual */, ldn, stride_c;
  bool ws, ws_aligned; long ws_bytes;                   // the caller's workspace: present, 16-byte aligned, size
  bool norm_ptrs_aligned;                               // C, residual, norm_w and norm_out are all 16-byte aligned
  int tail, fx;                                         // the GemmTailKind the caller asks for; llmseg_gemm_args.fx
};
enum GemmRoute { ROUTE_REFUSED, ROUTE_SKINNY, ROUTE_REG, ROUTE_REG_SLICED, ROUTE_GLDS, ROUTE_PP, ROUTE_PP_SLICED };
// the extension operands: one more K-tile of the ping-pong kernel | K-sliced: one more fp32 slab from a K = 64 call of its own | any other kernel: the call
// runs as two calls, the second (K = 64) accumulating onto C, and the plan describes the first
enum GemmExt { EXT_NONE, EXT_KTILE, EXT_SLAB, EXT_SECOND };
enum GemmReduce { REDUCE_NONE, REDUCE_PLAIN, REDUCE_NORM, REDUCE_NB, REDUCE_DL };
struct GemmPlan {
  GemmRoute route = ROUTE_REFUSED; GemmKernel kernel = K_REG; GemmExt ext = EXT_NONE;
  int slices = 1;                                       // K-slices of the ping-pong tile or of the register-staging kernel
  int skinny_rows = 0; bool skinny_ksplit = false;      // skinny route: the kernel's row template; its waves split K
  int tiles_m = 0, tiles_n = 0, group_m = 0;
  GemmReduce reduce = REDUCE_NONE; int cpt = 0;         // sliced routes: the reduce kernel; 8-column chunks per thread of the workgroup-per-row ones (NORM / DL)
  bool fx_fused = false, tail_done = false;             // the fused epilogue applies; this call does the caller's tail
  int launches = 1; long tag = 0;                       // kernel launches of the whole call, the extension's own calls included; the profiling tag
  const char* refusal = nullptr;                        // route == ROUTE_REFUSED: why
};
inline GemmPlan gemm_plan(const GemmQuery& q, const GemmKnobs& kn) {
  GemmPlan pl;
  auto refuse = [&pl](const char* why) { pl = GemmPlan(); pl.refusal = why; return pl; };
  const bool ta = q.trans_a, tw = q.trans_w, a_xform = q.a_norm || q.a_swiglu;
  const int M = q.M, N = q.N, K = q.K, BK = GEMM_BK;
  const long batch = q.batch1 * q.batch2, ncu = q.ncu;
  const bool tail_off = (q.tail == TAIL_NORM && kn.no_norm_fuse) || (q.tail == TAIL_NB && kn.no_nb) || (q.tail == TAIL_DL && kn.no_dl) || (q.tail == TAIL_FX && kn.no_fx);
  const int tail = tail_off ? TAIL_NONE : q.tail;
  if (q.ext && !(batch == 1 && !ta && !tw && !q.out_f32)) return refuse("extension operands need batch 1, K-contiguous operands and bf16 output");
  if (a_xform && !(M <= 8 && !ta && !tw && batch == 1 && !q.ext && (K & 7) == 0 && !(q.a_norm && q.a_swiglu)))      // (with extension operands a second launch would transform A2)
    return refuse("A-row transforms (a_norm_w / a_swiglu) are decode-step fusions of the M <= 8 route and do not go with extension operands");
  const int nt = K / BK;
  GemmKernel kernel = (K % BK == 0 && !ta && !tw) ? kernel_of_knob(kn.variant) : K_REG;
  if ((kernel == K_PP256 || kernel == K_PP128) && nt < (q.ext ? 1 : 2)) kernel = K_GLDS;
  if (kernel == K_T160 && nt < 2) kernel = K_GLDS;        // (the extension product's own K = 64 launch under a forced 160 x 256 tile)
  // split-K needs a dense-enough problem for the slab layout [S][M][N], 4-column alignment and room in the caller's workspace
  const bool can_split = batch == 1 && (N & 3) == 0 && (q.ldc & 3) == 0 && q.ws && q.ws_aligned && (!q.residual || (q.ldr & 3) == 0);
  auto ws_fits = [&](int S) { return (double)(S + (q.ext ? 1 : 0)) * M * N * 4.0 <= (double)q.ws_bytes; };   // + the extension product's slab
  int split = 1;
  if (kernel == K_AUTO) {
    // auto: minimum of the cost model over {128 x 128 DMA kernel, ping-pong 256 x 256 / 128 x 256 with 1..16 K-slices}
    struct Best { GemmKernel kernel; int split; double us; } best{K_GLDS, 1, glds_cost(M, N, nt, ncu) * (double)batch};
    if (nt >= (q.ext ? 1 : 2)) {
      // tiles 256 x 256, 128 x 256 and -- K-slice plans only -- 160 x 256.  Not for the fused-epilogue calls, and not for products with a
      // residual add: the forward's residual-stream projections (o_proj, down_proj) keep the 3-slice plan, so the forward pass -- every loss and the mask
      // head's gradients, which the full-depth parity test measures against the fp32 oracle -- computes the bits it computed before; moving its fp32
      // partial sums from 3 to 4 groups re-draws that chaotic comparison (profiles/r06_spread_fulldepth_grads_seeds3-5.md).  The backward dX products and
      // lm_head's dX take the new tile.
      const bool t160 = !kn.no_t160 && !q.fx && !q.residual;
      for (const GemmKernel k : {K_PP256, K_PP128, K_T160}) {
        if (k == K_T160 && !t160) continue;
        const int bm = pp_rows(k);
        for (int S = k == K_T160 ? 2 : 1; S <= 16; ++S) {
          if (S > 1 && (!can_split || !split_ok(nt, S) || !ws_fits(S))) continue;
          if (S > 1 && ((M + bm - 1) / bm) * ((N + 255) / 256) * S > ncu) break;     // slices only to fill ONE round of the CUs
          const double us = pp_cost(M, N, nt, bm, S, ncu, q.out_f32) * (double)batch;
          if (us < best.us * 0.97 || (us < best.us && S == 1)) best = Best{k, S, us};
        }
      }
    }
    kernel = best.kernel; split = best.split;
  } else if (kernel == K_PP256 || kernel == K_PP128) {
    split = kn.split > 1 ? kn.split : 1;
    if (split > 1 && !(can_split && split_ok(nt, split) && ws_fits(split))) return refuse("the forced split-K count is not possible for this call");
  } else if (kernel == K_T160) {
    split = kn.split;
    if (!(split > 1 && can_split && split_ok(nt, split) && ws_fits(split))) return refuse("variant 10 (160 x 256, K-sliced) needs a forced split-K count >= 2 that is possible");
  }
  int ext_launches = 0;
  if (q.ext) {
    // C = epi(alpha * (A.W^T + A2.W2^T)), A2 [M][64], W2 [N][64]: fused as one more K-tile of the ping-pong kernel; any other
    // kernel runs the product as a second call that accumulates onto C (linear epilogues only)
    GemmQuery q2 = q;
    q2.K = 64; q2.ext = false; q2.bias = false; q2.tail = TAIL_NONE;
    if (is_pp(kernel) && split > 1) {
      q2.gamma = q2.residual = false; q2.ldr = 0; q2.alpha_one = true; q2.act = GEMM_ACT_NONE; q2.out_f32 = true; q2.ldc = N; q2.ws = false; q2.ws_bytes = 0;
      const GemmPlan slab = gemm_plan(q2, kn);
      if (slab.route == ROUTE_REFUSED) return slab;
      pl.ext = EXT_SLAB; ext_launches = slab.launches;
    } else if (!is_pp(kernel)) {
      if (q.act != GEMM_ACT_NONE || q.gamma) return refuse("extension operands on this shape need a linear epilogue");
      GemmQuery q1 = q;
      q1.ext = false; q1.tail = TAIL_NONE; q2.residual = true; q2.ldr = q.ldc;          // no tail: the caller's work comes after BOTH calls (the entry function runs it)
      GemmPlan first = gemm_plan(q1, kn);
      const GemmPlan second = gemm_plan(q2, kn);
      if (first.route == ROUTE_REFUSED || second.route == ROUTE_REFUSED) return first.route == ROUTE_REFUSED ? first : second;
      first.ext = EXT_SECOND; first.launches += second.launches;
      return first;
    } else pl.ext = EXT_KTILE;
  }
  if (M <= 8 && !ta && !tw && batch == 1 && !q.ext && (K & 7) == 0 && (kn.variant == K_AUTO || a_xform)) {
    // skinny GEMM (decode steps, single-row head GEMMs): a weight stream, HBM-bound
    pl.route = ROUTE_SKINNY;
    pl.tag = gemm_tag(3 /* the skinny kernel's class */, false, false, q.residual, q.act, q.out_f32, false, 1);
    pl.skinny_ksplit = kn.skinny_sk == 2 ? K >= 2048 : (kn.skinny_sk && N <= 8192 && K >= 2048);      // fewer than 2 waves per SIMD otherwise: the workgroup's waves split K instead
    pl.skinny_rows = M == 1 ? 1 : M == 2 ? 2 : M <= 4 ? 4 : 8;
    return pl;
  }
  const bool pp = is_pp(kernel);
  const int bm = pp ? pp_rows(kernel) : 128, bn = pp ? 256 : GEMM_BN;
  pl.kernel = kernel; pl.tiles_m = (M + bm - 1) / bm; pl.tiles_n = (N + bn - 1) / bn;
  // ping-pong tile walk (tools/gemm_bench.py sweeps): short matrices (Llama, <= 32 row tiles) with few column tiles (N = 4096: o, down,
  // the dX products) keep all of M in one group so a W column tile is fetched once per XCD; with many column tiles (qkv, gate|up, lm_head at
  // 16-24 images: 20-30 row tiles x 48-126 column tiles) an XCD's 32 concurrent tiles would be ONE column tile deep and re-stream all of A
  // (63 MB at 24 images) per column tile -- 8 row tiles per group make the concurrent set 8 x 4 (+5..8 %: qkv 1017 -> 1100, gate|up
  // 1215 -> 1300, lm_head 1234 -> 1310 TF/s at 16 images); tall ones (SAM, 384+ row tiles) walk 4 row tiles per group (+3..6 % at K = 5120)
  pl.group_m = kn.group_m > 0 ? kn.group_m : (pl.tiles_m <= 32 ? ((pl.tiles_n > 16 && pl.tiles_m > 8) ? 8 : pl.tiles_m) : 4);
  pl.tag = gemm_tag(gemm_tag_class(kernel), ta, tw, q.residual, q.act, q.out_f32, batch > 1, split);
  // Register-staging kernel (transposed operands / K % 64 != 0) on a grid that leaves most CUs idle with a long serial K loop (a lone
  // workgroup takes 1.2-3 us per K-tile, all of it exposed latency: 512 x 256 x 2048 with W stored [K][N] was 75 us on 8 workgroups):
  // K-slices as the (inner) batch index, fp32 slabs in the caller's workspace, epilogue in the reduce launch.
  if (kernel == K_REG && q.batch2 == 1 && (N & 3) == 0 && (q.ldc & 3) == 0 && q.ws && q.ws_aligned && (!q.residual || ((q.ldr & 3) == 0 && batch == 1)) &&
      ((q.stride_c & 3) == 0 || batch == 1) && !kn.no_rsplit) {
    const long tiles = (long)pl.tiles_m * pl.tiles_n * batch;
    const int ntr = (K + BK - 1) / BK;
    int S = (tiles * 4 <= ncu && ntr >= 8) ? (int)std::min<long>({(long)ncu / std::max<long>(tiles, 1), (long)ntr / 2, 32L}) : 1;
    while (S > 1 && (double)S * batch * M * N * 4.0 > (double)q.ws_bytes) --S;
    if (S > 1) { const int qt = (ntr + S - 1) / S; S = (ntr + qt - 1) / qt; }
    if (S > 1) { pl.route = ROUTE_REG_SLICED; pl.slices = S; pl.reduce = REDUCE_PLAIN; pl.launches = 2; return pl; }
  }
  if (pp && split > 1) {
    // the reduce launch sums the slabs (+ the extension product's) and applies the epilogue; the caller's tail rides in it where a row kernel can do both:
    // only where llmseg_norm / llmseg_norm_bwd_add would run their workgroup-per-row kernels on this shape (same arithmetic, same bits) and the epilogue
    // is the plain residual add
    const bool plain = !q.out_f32 && !q.bias && !q.gamma && q.act == GEMM_ACT_NONE;
    const bool fuse_norm = tail == TAIL_NORM && plain && q.alpha_one && M >= 64 && M < kn.norm_wg_max && N >= 2048 && N <= 8192 && (N & 7) == 0 && (q.ldc & 7) == 0 &&
                           (!q.residual || (q.ldr & 7) == 0) && (q.ldn & 7) == 0 && q.norm_ptrs_aligned;
    const bool fuse_nb = tail == TAIL_NB && plain && q.alpha_one && !q.residual && M >= 64 && N >= 2048 && N <= 8192 && (N & 7) == 0;
    const bool fuse_dl = tail == TAIL_DL && plain && !q.residual && N <= 8192 && (N & 127) == 0 && (q.ldc & 7) == 0;
    const int cpt = ((N >> 3) + 255) / 256;
    pl.route = ROUTE_PP_SLICED; pl.slices = split; pl.launches = 2 + ext_launches;
    pl.reduce = fuse_dl ? REDUCE_DL : fuse_nb ? REDUCE_NB : fuse_norm ? REDUCE_NORM : REDUCE_PLAIN;
    if (pl.reduce == REDUCE_DL || pl.reduce == REDUCE_NORM) pl.cpt = cpt <= 1 ? 1 : cpt <= 2 ? 2 : 4;
    pl.tail_done = pl.reduce != REDUCE_PLAIN;
  } else if (pp) {
    // one K-slice of a ping-pong tile (K_T160 never gets here: every plan of it has slices).  Fused Llama-layer epilogues (llmseg_gemm_args.fx) on shapes whose
    // tiles hold whole pairs; gemm_fx runs the pointwise launch otherwise.  The 128-row tile serves the layer at 2 images per micro-step, the 256-row tile the fused
    // accumulation window and 24-image micro-batches.
    pl.route = ROUTE_PP;
    pl.fx_fused = pl.tail_done = tail == TAIL_FX && !q.out_f32 && batch == 1 && (q.fx == GEMM_FX_ROPE ? (N % 256) == 0 && q.ext : q.fx == GEMM_FX_SWIGLU ? ((N / 2) % 128) == 0 : (N % 64) == 0);
  } else pl.route = kernel == K_GLDS ? ROUTE_GLDS : ROUTE_REG;
  return pl;
}
