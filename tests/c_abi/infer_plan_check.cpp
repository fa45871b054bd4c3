// Stand-alone host check of csrc/infer_plan.h (built with -fsanitize=address,undefined by tests/test_host_abi.py).
//   infer_plan_check CONFIGS.txt
// CONFIGS.txt: one configuration per line, the switches of a recorded case of tests/golden/infer_routes.json
//   id wino_min_batch wino_tile trunk_min_batch trunk_min_fill small keep f16 rot_normalizer fuse tail_parts tail_parts_ch ovr_ab2 ovr_heads
// For every configuration and n = 1 .. 72 (the first one, the default, also up to SE3TN_MAX_BATCH_LIMIT) the plan must hold the
// invariants below; for n <= 72 the launch names and the written stages are printed, one tab-separated line per cell
//   R <id> <n> <name;name;...> <stage,stage,...>
// which the pytest holds against the recorded launches and against the Python route model.  Exits non-zero at the first violation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "infer_plan.h"

using namespace se3tn;

static const char* g_where = "";
static int g_n = 0;
#define CHECK(cond)                                                                                              \
  do {                                                                                                           \
    if (!(cond)) { std::fprintf(stderr, "line %d (%s, n = %d): %s\n", __LINE__, g_where, g_n, #cond); return 1; } \
  } while (0)

static const size_t PART_BYTES = (size_t)16 * 1024 * 121 * 16 * sizeof(float);   // se3tn_create's split-K workspace

struct Switches {
  char id[64];
  int wmin, tile, tmin, tfill, small, keep, f16, fuse, tail_parts, tail_parts_ch, ovr[2];
  double rn;
};

// the configuration of a context created with the library's defaults, weights loaded, then switched as the case says: what
// wino_prepare / split_prepare of api.cpp leave derived
static InferConfig config_for(const Switches& s, int n) {
  InferConfig c;
  std::memset(&c, 0, sizeof(c));
  c.n = n; c.prec = s.f16 ? SE3TN_PREC_F16X3 : SE3TN_PREC_F32; c.keep_intermediates = s.keep; c.small_kernels = s.small;
  c.tail_parts = s.tail_parts; c.tail_parts_ch = s.tail_parts_ch;
  c.wino_min_batch = s.wmin; c.wino_tile = s.tile; c.auto_tile_override[0] = s.ovr[0]; c.auto_tile_override[1] = s.ovr[1];
  c.wino_fuse = s.fuse; c.gemmp = -1; c.wino64_min_batch = s.tmin; c.wino64_min_fill = s.tfill; c.num_cus = 256;
  c.part_bytes = PART_BYTES; c.tn = 0.03; c.rn = s.rn;
  const bool six = s.tile == 6 || s.tile == SE3TN_WINOGRAD_TILE_AUTO || s.tile == SE3TN_WINOGRAD_TILE_6_4;
  c.ready = READY_WINO_VM | READY_TRUNK | (s.tile == 2 ? READY_U2 : READY_U4) | (six ? READY_U6 : 0u) |
            (s.f16 ? READY_SPLIT_W : 0u) | (s.f16 && s.tile != 2 ? READY_SPLIT_U4 : 0u);
  return c;
}

static bool same_step(const ConvStep& a, const ConvStep& b) {
  return a.algo == b.algo && a.reduce == b.reduce && a.tile == b.tile && a.slices == b.slices && a.gemm.kind == b.gemm.kind &&
         a.gemm.tiles == b.gemm.tiles && a.gemm.grid == b.gemm.grid;
}
static bool same_plan(const InferPlan& a, const InferPlan& b) {
  for (int i = 0; i < NUM_CONV3; ++i)
    if (!same_step(a.conv[i], b.conv[i])) return false;
  return a.stem == b.stem && a.tail == b.tail && a.block[0] == b.block[0] && a.block[1] == b.block[1] &&
         a.tail_stores_word == b.tail_stores_word && a.tail_ch == b.tail_ch && a.written == b.written;
}

static int check_invariants(const InferConfig& c, const InferPlan& p) {
  const bool fast = c.prec == SE3TN_PREC_F16X3, keep = c.keep_intermediates != 0;
  const ConvRow* rows = conv_table();
  for (int i = 0; i < NUM_CONV3; ++i) {
    const ConvRow& r = rows[i];
    const ConvStep& s = p.conv[i];
    const Conv3& sp = conv_specs()[r.id];
    CHECK(r.id == (ConvId)i);
    CHECK(s.algo != ConvStep::NONE);
    const int ho = (r.hin - 1) / r.stride + 1, M = c.n * ho * ho;
    // a conv leaves its slices unreduced only as the last head conv on the slices algorithm under the "parts" tail
    if (!s.reduce) CHECK(r.id == LH2_2 && s.algo == ConvStep::SLICES && p.tail == InferPlan::TAIL_PARTS);
    if (s.algo == ConvStep::SLICES || s.algo == ConvStep::SPLITK) {
      CHECK(s.slices > 0);
      CHECK((size_t)s.slices * sp.groups * M * sp.cout * sizeof(float) <= c.part_bytes);
    } else {
      CHECK(s.slices == 0);
    }
    if (s.algo == ConvStep::SPLITK) {
      const int ks = sp.cin / 32 * 9;
      CHECK(ks % s.slices == 0 && ks / s.slices >= SE3TN_SPLITK_MIN_STEPS);
    }
    if (s.algo == ConvStep::SLICES || s.algo == ConvStep::SMALL64) CHECK(!fast && c.n <= SMALL_MAX_IMG);
    if (s.algo == ConvStep::SLICES) CHECK(s.slices == conv_slices_small_count(sp.cin, r.stride, r.hin));
    if (s.algo == ConvStep::SLAB) CHECK(r.stride == 1);
    if (s.algo == ConvStep::GATHER) CHECK(r.stride == 2);
    const int blk = wino_block_of(r.id);
    if (s.algo == ConvStep::WINO) {
      CHECK(blk >= 0 && (s.tile == 2 || s.tile == 4 || s.tile == 6));
      CHECK(!(fast && s.tile == 6));                         // F(6x6) never under f16x3
      CHECK(!fast || p.block[blk]);                          // f16x3 has no conv-by-conv Winograd
      CHECK((c.ready & READY_WINO_VM) && wino_planes_ready(c, s.tile));
      const int nf = (s.tile + 2) * (s.tile + 2), th = (r.hin + s.tile - 1) / s.tile, T = c.n * th * th;
      CHECK(s.gemm.kind != GemmPlan::NONE);
      if (s.gemm.kind == GemmPlan::PERSISTENT) {
        CHECK(!fast && sp.cout % 256 == 0 && (sp.groups * nf) % 8 == 0);
        CHECK(s.gemm.tiles == (sp.cout / 256) * ((T + 127) / 128) * sp.groups * nf);
        CHECK(s.gemm.grid >= 1 && s.gemm.grid <= s.gemm.tiles && s.gemm.grid <= c.num_cus);
      }
    } else {
      CHECK(s.gemm.kind == GemmPlan::NONE && s.tile == 0);
      CHECK(blk < 0 || !p.block[blk]);
    }
    if (s.algo == ConvStep::WINO64) CHECK(r.id <= L64_4 && !fast && (c.ready & READY_TRUNK));
  }
  for (int b = 0; b < 2; ++b)
    if (p.block[b]) {   // a fused block only with its planes ready, both convs on one tile
      const ConvStep &s1 = p.conv[b == 0 ? LAB2_1 : LH2_1], &s2 = p.conv[b == 0 ? LAB2_2 : LH2_2];
      CHECK(s1.algo == ConvStep::WINO && s2.algo == ConvStep::WINO && s1.tile == s2.tile && (s1.tile == 4 || s1.tile == 6));
      CHECK(same_step(s1, s2));
      CHECK(c.wino_fuse && (c.ready & READY_WINO_VM) && wino_planes_ready(c, s1.tile) && (!fast || (c.ready & READY_SPLIT_U4)));
      CHECK(!(fast && b == 0));
    }
  CHECK((p.tail == InferPlan::TAIL_FUSED) == p.block[1]);
  CHECK((p.tail == InferPlan::TAIL_PARTS) == !p.conv[LH2_2].reduce);
  CHECK(p.tail_stores_word == (p.tail != InferPlan::TAIL_FUSED));
  if (p.tail == InferPlan::TAIL_PARTS) CHECK(!keep && (p.tail_ch == 16 || p.tail_ch == 32) && p.conv[LH2_2].slices == 8);
  // the written mask, from the steps
  unsigned w = STAGE_POOL | STAGE_T64 | STAGE_Q64 | STAGE_AB;
  if (p.stem == InferPlan::STEM_BIG) w |= STAGE_STEM;
  if (!p.block[0] || keep) w |= STAGE_AB_T;
  if (!p.block[1] || keep) w |= STAGE_HEAD_T;
  if ((p.block[1] && keep) || p.tail == InferPlan::TAIL_PLAIN) w |= STAGE_HEAD;
  CHECK(p.written == w);
  if (p.stem == InferPlan::STEM_SMALL) CHECK(!fast && !keep && c.n <= SE3TN_STEM_SMALL_MAX_N);
  return 0;
}

// With a readiness bit cleared the plan falls back as the code always has: it does not refuse (the f16x3 panels excepted: without
// them the mode has no kernel).  Each fallback is stated as "the plan of the same configuration with the matching switch off"
static int check_fallbacks(const InferConfig& c, const InferPlan& full) {
  const bool fast = c.prec == SE3TN_PREC_F16X3;
  InferPlan p, q;
  InferConfig d = c, e = c;
  d.ready &= ~READY_WINO_VM; e.wino_min_batch = 0;   // no workspaces = Winograd off
  CHECK(plan_infer(d, p) == INFER_PLAN_OK && plan_infer(e, q) == INFER_PLAN_OK && same_plan(p, q));
  d = c; e = c; d.ready &= ~READY_TRUNK; e.wino64_min_batch = 0;   // no trunk planes = the fused trunk kernel off
  CHECK(plan_infer(d, p) == INFER_PLAN_OK && plan_infer(e, q) == INFER_PLAN_OK && same_plan(p, q));
  e = c; e.wino_min_batch = 0;
  CHECK(plan_infer(e, q) == INFER_PLAN_OK);        // q: Winograd off
  for (unsigned bit : {(unsigned)READY_U2, (unsigned)READY_U4, (unsigned)READY_U6}) {   // a missing plane set: the blocks of that tile, and only they
    const int tile = bit == READY_U2 ? 2 : bit == READY_U4 ? 4 : 6;
    d = c; d.ready &= ~bit;
    CHECK(plan_infer(d, p) == INFER_PLAN_OK);
    for (int b = 0; b < 2; ++b) {
      const InferPlan& want = tile_for(c, b) == tile ? q : full;
      for (ConvId id : {b == 0 ? LAB2_1 : LH2_1, b == 0 ? LAB2_2 : LH2_2}) {
        // (the last head conv may keep or lose its reduce with the tail: compared through the tail below)
        CHECK(p.conv[id].algo == want.conv[id].algo && p.conv[id].tile == want.conv[id].tile && p.conv[id].slices == want.conv[id].slices);
      }
      CHECK(p.block[b] == want.block[b]);
    }
    CHECK(p.tail == (tile_for(c, 1) == tile ? q.tail : full.tail));
    for (int i = 0; i <= LAB1; ++i) CHECK(same_step(p.conv[i], full.conv[i]));
    CHECK(same_step(p.conv[LH1], full.conv[LH1]) && p.stem == full.stem);
    if (int rc = check_invariants(d, p)) return rc;
  }
  d = c; e = c; d.ready &= ~READY_SPLIT_U4;   // no split F(4x4) planes: f16x3 runs its heads conv by conv; float32 does not care
  if (fast) e.wino_fuse = 0;
  CHECK(plan_infer(d, p) == INFER_PLAN_OK && plan_infer(e, q) == INFER_PLAN_OK && same_plan(p, q));
  d = c; d.ready &= ~READY_SPLIT_W;
  CHECK(plan_infer(d, p) == (fast ? INFER_PLAN_NO_SPLIT_PANELS : INFER_PLAN_OK));
  if (!fast) CHECK(same_plan(p, full));
  return 0;
}

static void print_cell(const Switches& s, const InferConfig& c, const InferPlan& p) {
  const bool fast = c.prec == SE3TN_PREC_F16X3;
  std::string names = "to_padded_input;";   // (the recorded calls hand in external tensors)
  names += stem_label(p, 0);
  if (p.stem == InferPlan::STEM_BIG) names += std::string(";") + stem_label(p, 1);
  const ConvRow* rows = conv_table();
  for (int i = 0; i < NUM_CONV3; ++i) {
    const int blk = wino_block_of(rows[i].id);
    names += ";" + step_label(rows[i], p.conv[i], fast, blk >= 0 && p.block[blk], blk == 1);
  }
  if (const char* t = tail_label(p)) names += std::string(";") + t;
  static const struct { unsigned bit; const char* name; } stages[] = {{STAGE_STEM, "stem"}, {STAGE_POOL, "pool"}, {STAGE_T64, "t64"}, {STAGE_Q64, "q64"},
                                                                       {STAGE_AB, "ab"}, {STAGE_AB_T, "ab_t"}, {STAGE_HEAD, "head"}, {STAGE_HEAD_T, "head_t"}};
  std::string st;
  for (const auto& g : stages)
    if (p.written & g.bit) st += (st.empty() ? "" : ",") + std::string(g.name);
  std::printf("R\t%s\t%d\t%s\t%s\n", s.id, c.n, names.c_str(), st.c_str());
}

// the mixed-model call: for k = 1 .. 5 the explicitly chosen family IS the default configuration's plan of k pairs; beyond, an error
static int check_small_family(const Switches& dflt) {
  g_where = "small family";
  for (int k = 0; k <= 8; ++k) {
    g_n = k;
    InferConfig c = config_for(dflt, k);
    c.small_family = 1;
    InferPlan p, q;
    const InferPlanStatus st = plan_infer(c, p);
    if (k < 1 || k > 5) { CHECK(st == INFER_PLAN_FAMILY_MISS); continue; }
    CHECK(st == INFER_PLAN_OK);
    CHECK(plan_infer(config_for(dflt, k), q) == INFER_PLAN_OK && same_plan(p, q));
    if (int rc = check_invariants(c, p)) return rc;
    // chosen explicitly: the context's own switches do not move it ...
    c.small_kernels = 0; c.tail_parts = 0; c.wino_min_batch = 1; c.tail_parts_ch = 32;
    CHECK(plan_infer(c, q) == INFER_PLAN_OK && same_plan(p, q));
    // ... and what it cannot run is an error, not another algorithm
    c.part_bytes = 0;
    CHECK(plan_infer(c, q) == INFER_PLAN_FAMILY_MISS);
    c = config_for(dflt, k); c.small_family = 1; c.prec = SE3TN_PREC_F16X3; c.ready |= READY_SPLIT_W;
    CHECK(plan_infer(c, q) == INFER_PLAN_FAMILY_MISS);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: infer_plan_check CONFIGS.txt\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<Switches> all;
  Switches s;
  while (std::fscanf(f, "%63s %d %d %d %d %d %d %d %lf %d %d %d %d %d", s.id, &s.wmin, &s.tile, &s.tmin, &s.tfill, &s.small, &s.keep, &s.f16, &s.rn,
                     &s.fuse, &s.tail_parts, &s.tail_parts_ch, &s.ovr[0], &s.ovr[1]) == 14)
    all.push_back(s);
  std::fclose(f);
  if (all.empty() || std::strcmp(all[0].id, "default") != 0) { std::fprintf(stderr, "the first configuration must be `default`\n"); return 2; }
  long cells = 0;
  for (size_t k = 0; k < all.size(); ++k) {
    g_where = all[k].id;
    const int n_max = k == 0 ? SE3TN_MAX_BATCH_LIMIT : 72;
    for (int n = 1; n <= n_max; ++n) {
      g_n = n;
      const InferConfig c = config_for(all[k], n);
      InferPlan p;
      CHECK(plan_infer(c, p) == INFER_PLAN_OK);
      if (int rc = check_invariants(c, p)) return rc;
      if (int rc = check_fallbacks(c, p)) return rc;
      if (n <= 72) print_cell(all[k], c, p);
      ++cells;
    }
  }
  if (int rc = check_small_family(all[0])) return rc;
  // the persistent GEMM where it is forced (SE3TN_WINO_GEMMP=1) and where it is off: still only on the shapes it can tile
  for (int gp = 0; gp <= 1; ++gp)
    for (int n = 1; n <= 72; ++n) {
      g_where = gp ? "gemmp 1" : "gemmp 0"; g_n = n;
      InferConfig c = config_for(all[0], n);
      c.gemmp = gp;
      InferPlan p;
      CHECK(plan_infer(c, p) == INFER_PLAN_OK);
      if (int rc = check_invariants(c, p)) return rc;
      for (int i = 0; i < NUM_CONV3; ++i) CHECK(gp == 1 || p.conv[i].gemm.kind != GemmPlan::PERSISTENT);
    }
  std::printf("infer_plan_check: ok (%ld cells)\n", cells);
  return 0;
}
