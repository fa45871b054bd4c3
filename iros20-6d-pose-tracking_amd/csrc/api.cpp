// C ABI of the hot path (include/se3tracknet.h).  Host orchestration only: every kernel lives in
// the .hip files.  One context per (process, device).
#include <cmath>
#include <thread>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "hip_buffers.h"
#include "pose_align_plan.h"
#include "pose_errors_plan.h"
#include "pose_grid_plan.h"
#include "pose_search_plan.h"
#include "scene_fit_plan.h"
#include "se3tn_internal.h"
#include "tex_pyramid.h"
#include "track_plan.h"
#include "verify_plan.h"
#include "weights.h"

using namespace se3tn;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
static int hipfail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return (int)e;
}
#define HIPCHK(x)                                  \
  do {                                             \
    hipError_t _e = (x);                           \
    if (_e != hipSuccess) return hipfail(_e, #x);  \
  } while (0)

enum { MAX_LAUNCHES = 24, MAX_SLOTS = 64 };

// one captured se3tn_infer: every argument that is baked into the kernel launches -- the pointers, the layout, and the InferConfig the
// route was planned from (infer_plan.h: a switch that influences the route is in the key because the plan could not have read it otherwise)
struct GraphKey {
  const void *A, *B, *trans, *rot, *poseA, *poseB, *blob;
  int layout;
  InferConfig cfg;
  bool operator==(const GraphKey& o) const { return std::memcmp(this, &o, sizeof(GraphKey)) == 0; }
};
struct GraphEntry {
  GraphKey key;
  hipGraphExec_t exec = nullptr;  // null: seen once (run eagerly, which also sets the kernels' LDS attributes)
  InferPlan plan;                 // what the captured sequence runs (its STAGE_* mask, its tail)
};
static_assert(std::is_trivially_copyable<GraphEntry>::value, "the graph cache moves its entries as bytes (GraphKey is compared as bytes)");

struct se3tn_ctx {
  int device = -1, max_batch = 0;
  TensorMap tensors;
  std::vector<float> packed;
  DeviceBuf<float> blob_owned;
  const float* blob = nullptr;
  BlobLayout L;
  // activations (NHWC float32)
  DeviceBuf<float> inA, inB;                    // [mb,182,182,4] (3-pixel zero border)
  DeviceBuf<float> stem;                        // [mb,88,88,128]
  // zero-bordered conv activations (se3tn_internal.h: ConvArgs)
  DeviceBuf<float> pool, t64, q64;              // [mb,46,46,128]
  DeviceBuf<float> ab, ab_t;                    // [mb,24,24,256]
  DeviceBuf<float> head, head_t;                // [mb,13,13,1024]
  DeviceBuf<float> head_f;                      // f16x3 mode: float32 output of the last head conv (the
                                                // in-place residual update cannot change format)
  unsigned written = 0;                         // STAGE_* the last infer wrote (the others hold older data: se3tn_debug_buffer refuses them)
  InferPlan plan;                               // the route of the last forward pass that was planned (infer_plan.h)
  DeviceBuf<float> logits;                      // [mb,6]
  DeviceBuf<float> fcpart;                      // [mb,2,<=32,3] partial FC dot products (fused Winograd tail: 8 slices per head; tail_kernel 8; tail_parts_kernel 32)
  bool keep_intermediates = false;              // se3tn_keep_intermediates: fused blocks also store ab_t / head_t / head
  int auto_tile_override[2] = {0, 0};           // SE3TN_WINOGRAD_AUTO_TILE_AB2 / _HEADS = 4 | 6: what AUTO picks per block (rounding studies)
  int gemmp = -1;                               // SE3TN_WINO_GEMMP = 0 | 1: never | always the persistent 128 x 256 Winograd GEMM (default: by tile count)
  bool wino_fuse = true;                        // whole residual blocks as one fused launch sequence (SE3TN_WINOGRAD_FUSE=0: conv by conv)
  DeviceBuf<float> part;                        // split-K partial sums (small-batch latency path)
  int tail_parts_ch = 16;                       // SE3TN_TAIL_PARTS=2: 32 workgroups x 32 channels per pair instead of 64 x 16 (developer A/B)
  bool tail_parts = true;                       // SE3TN_TAIL_PARTS=0 (developer switch): batch 1-5 keeps conv_reduce + tail_kernel after the last head conv
  bool small_kernels = true;                    // SE3TN_SMALL_KERNELS=0 (developer switch): batch 1-5 through the split-K kernels only
  // Winograd F(m x m,3x3) path (wino_mfma.hip) of convAB2.* and trans|rot conv2.* at n >= wino_min_batch
  int wino_min_batch = SE3TN_WINOGRAD_DEFAULT_MIN_BATCH;  // 0 = never
  int wino_tile = SE3TN_WINOGRAD_DEFAULT_TILE;            // m = 2 | 4 | 6 | SE3TN_WINOGRAD_TILE_AUTO
  int wino_tile_derived = 0;                              // the m wino_u was derived for
  DeviceBuf<float> wino_u[4];                   // U = G g G^T of LAB2_1, LAB2_2, LH2_1, LH2_2 (tile 2 | 4: wino_tile_derived)
  DeviceBuf<float> wino_u6[4];                  // the F(6x6) planes of the same four convs (tile 6 | AUTO only)
  const float* wino6_blob = nullptr;                        // the blob wino_u6 was derived from
  DeviceBuf<float> wino_v, wino_m;              // [g][16][T][C] input tiles / per-frequency products
  const float* wino_blob = nullptr;             // the blob wino_u was derived from
  // fused F(2x2) path of the 64-channel trunk (wino64_fused.hip) at n >= wino64_min_batch (0 = never)
  int wino64_min_batch = SE3TN_TRUNK_WINOGRAD_DEFAULT_MIN_BATCH;
  int wino64_min_fill = SE3TN_TRUNK_WINOGRAD_DEFAULT_MIN_FILL;
  int num_cus = 256;   // compute units of the device (the fused trunk kernel runs one workgroup per CU: it pays in full rounds only)
  DeviceBuf<float> wino64_u[4];   // F(2x2) planes of L64_1..L64_4 ([group][chunk 2][16][64][32])
  const float* wino64_blob = nullptr;
  SplitLayout SL;                               // f16x3 mode: split panels in split_w (derived from the blob, not part of it)
  DeviceBuf<float> split_w;
  const float* split_blob = nullptr;            // the blob split_w was derived from
  DeviceBuf<float> wino_us[4];                  // f16x3 Winograd blocks: U as split rows ...
  DeviceBuf<float> wino_usc[4];                 // ... and their per-(group, frequency, cout) 2^-k
  const float* wino_us_blob = nullptr;          // the blob / tile the split planes were derived for
  int wino_us_tile = 0;
  int prec = SE3TN_PREC_F32;                    // se3tn_set_precision
  int offset_rule = SE3TN_OFFSET_RULE_NUMPY1;   // se3tn_set_offset_rule
  int raster_sub_bits = 4;                      // se3tn_set_raster_rule: sub-pixel bits of the rasteriser's window coordinates
  // se3tn_on_track: pinned host staging [pose 128 B | frame window rgb | depth], its device mirror, device outputs and their pinned copy
  PinnedBuf<uint8_t> trk_host; DeviceBuf<uint8_t> trk_dev; size_t trk_bytes = 0;
  PinnedBuf<uint8_t> trk_out;   // ONE mapped pinned block: host address get() | device address dev()
  // se3tn_on_track_batch / _objects: instance table (pinned host + device, fill_instance), z-buffers, image A stack, staging (the
  // TrackWindows of track_plan.h, upload_staged), outputs (read_back_tracks) -- grown at first use / larger n (reserve_track_batch)
  int tb_cap = 0;
  size_t tb_stage_bytes = 0;
  PinnedBuf<uint8_t> tb_inst_host; DeviceBuf<uint8_t> tb_inst_dev;   // [cap RasterInstance | cap RasterMaterial]
  DeviceBuf<unsigned long long> tb_zbuf;
  DeviceBuf<uint8_t> tb_rgbA, tb_stage_dev, tb_out_dev;
  PinnedBuf<uint8_t> tb_stage_host, tb_out_host;
  DeviceBuf<uint16_t> tb_depthA;
  // SE3TN_ROUTE_FRAME meshes (se3tn_on_track, se3tn_on_track_batch, _objects): the rendered rectangles [64 zero bytes | rgb of every pair |
  // depth of every pair] and, for n pairs, their z-buffers -- fr_px pixels in all (pairs x the largest rectangle of the call), grown at need
  // (reserve_frame_rects).
  // The 64 bytes in front are zeroed at allocation and never written: the 1 x 1 image A of a window that misses the frame
  DeviceBuf<uint8_t> fr_sub;
  DeviceBuf<unsigned long long> fr_zbuf;
  size_t fr_px = 0;
  // se3tn_on_track_objects: rasteriser scratch of up to mo_cap instances of up to mo_V vertices / mo_F triangles (several meshes per launch)
  int mo_cap = 0, mo_V = 0, mo_F = 0;
  RasterScratch mo;
  // se3tn_fit_stats: per-pair counters [max_batch][FitArgs::WORDS] (se3tn_create; zero between launches).  se3tn_set_fit_check: the
  // tolerance (0 = off), the estimate renders [fit_cap,176,176,3] / [fit_cap,176,176] and the records in MAPPED pinned memory (host
  // address | device address) -- allocated by the first tracking call with the check on; fit_last_n: pairs of the last tracking call
  // this context executed whose records are valid (0: none)
  DeviceBuf<unsigned> fit_counters;
  int fit_tol = 0, fit_last_n = 0, fit_cap = 0;
  DeviceBuf<uint8_t> fit_rgb; DeviceBuf<uint16_t> fit_depth;
  PinnedBuf<se3tn_fit> fit_host;
  // se3tn_color_stats(_scene) / se3tn_verify_poses(_scene)_host: per-pair counters [max_batch][FitArgs::COLOUR_WORDS] (se3tn_create; zero between launches)
  DeviceBuf<unsigned> color_counters;
  // the scene stage.  se3tn_scene_stats: the counters [SCENE_COUNTER_WORDS] (se3tn_create; zero between launches).  se3tn_scene_fit:
  // buffers of the stage's OWN, so that no tracking call reads what a scene call wrote and the other way round -- the pinned instance
  // table and its device mirror ([cap RasterInstance | cap RasterMaterial]), rasteriser scratch for sc_cap instances of up to sc_V
  // vertices / sc_F triangles, the rendered rectangles ([64 bytes | rgb | depth], fr_sub's layout) and their z-buffers for sc_px
  // pixels in all; grown at need (scene_reserve).  sc_table_event: recorded behind the table's upload, waited for before the next
  // call rewrites the pinned table (the call itself is stream-ordered)
  DeviceBuf<unsigned> sc_counters;
  int sc_cap = 0, sc_V = 0, sc_F = 0;
  RasterScratch sc_mo;
  PinnedBuf<uint8_t> sc_inst_host; DeviceBuf<uint8_t> sc_inst_dev;
  size_t sc_px = 0;
  DeviceBuf<uint8_t> sc_sub;
  DeviceBuf<unsigned long long> sc_zbuf;
  hipEvent_t sc_table_event = nullptr; bool sc_table_busy = false;
  // the synchronous _host entry points of the pose family (StagedCall): pinned staging of ps_cap bytes and its device mirror, laid out
  // per call (pose_errors_plan.h: pe_stage_*, pose_search_plan.h: PsStage, pose_grid_plan.h: PgStage, pose_align_plan.h: PaStage)
  PinnedBuf<unsigned char> ps_host; DeviceBuf<unsigned char> ps_dev; size_t ps_cap = 0;
  // where the last se3tn_search_pose_grid_scene_host left its scene frame in ps_dev (se3tn_last_search_scene); H = 0: nowhere -- the
  // next staged call lays the buffer out anew
  size_t ps_scene_off = 0; int ps_scene_H = 0, ps_scene_W = 0;
  bool rearm_counters = false;                  // a failed launch sequence: clear tail_arrive before the next one
  DeviceBuf<int> tail_arrive;                   // [max_batch] arrival counters of tail_kernel's 16 workgroups per pair (zero between launches)
  int* tail_flag = nullptr; int tail_seq = 0;   // set around se3tn_on_track's infer: the tail kernel stores tail_seq to this (mapped) word
  hipStream_t trk_copy_stream = nullptr; hipEvent_t trk_copy_event = nullptr;
  DeviceBuf<uint8_t> trk_rgbA; DeviceBuf<uint16_t> trk_depthA;
  int in_split[2] = {0, 0};                     // pixel format currently held by inA / inB
  bool last_fast = false;                       // the last infer ran the f16x3 kernels (ab is split rows)
  DeviceBuf<int> overflow;                      // device flag: a split-row store left the f16 range
  DeviceBuf<unsigned long long> zbuf;           // rasteriser z-buffer keys, one per pixel (176*176, grown by se3tn_render_frame)
  DeviceBuf<float> fd_buf;                      // se3tn_fill_depth scratch for frames of up to fd_pixels: 3 images + minmax[2] + lut[4098]
  size_t fd_pixels = 0;
  bool use_graphs = false;                      // se3tn_enable_graphs
  std::vector<GraphEntry> graphs;
  double mean[8], stdv[8];
  bool have_norm = false;
  double tn = 0.03, rn = 5.0 * 3.14159265358979323846 / 180.0;
  // profiling
  bool prof = false;
  int slots = 0;          // number of event sets (one per profiled se3tn_infer, used round-robin)
  long long infer_count = 0;
  hipEvent_t* ev = nullptr;  // points at evs[slot]
  hipEvent_t evs[MAX_SLOTS][MAX_LAUNCHES + 1];
  int n_launch = 0;
  int slot_launches[MAX_SLOTS];
  const char* names[MAX_LAUNCHES];
  bool is_conv[MAX_LAUNCHES];
  // (the buffers free themselves; frees go to the owning device whatever device is current)
  ~se3tn_ctx() {
    for (auto& g : graphs)
      if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (trk_copy_event) (void)hipEventDestroy(trk_copy_event);
    if (sc_table_event) (void)hipEventDestroy(sc_table_event);
    if (trk_copy_stream) (void)hipStreamDestroy(trk_copy_stream);
    for (int s = 0; s < slots; ++s)
      for (auto& e : evs[s]) (void)hipEventDestroy(e);
  }
};

struct se3tn_mesh {
  DeviceBuf<float> verts, normals, colors;
  DeviceBuf<int> faces;
  int V = 0, F = 0;
  RasterScratch scratch;   // of one instance (se3tn_render*, se3tn_on_track)
  // batched rasteriser scratch (se3tn_on_track_batch): batch_cap instances
  int batch_cap = 0;
  RasterScratch batch;
  // pyrender-style material (se3tn_mesh_set_texture): uv per vertex, RGB mip pyramid, Kd
  DeviceBuf<float> uv;
  DeviceBuf<uint8_t> tex;
  int tw = 0, th = 0, tlevels = 0;
  unsigned tex_off[16] = {};
  float kd[3] = {1.f, 1.f, 1.f};
  bool has_material = false;        // se3tn_mesh_set_texture has been called (a texture, or a Kd over the vertex colours)
  int route = SE3TN_ROUTE_WINDOW;   // se3tn_mesh_set_route: the renderer se3tn_on_track / _batch use for image A
};

// se3tn_points_create: the model points of se3tn_pose_errors and the partial sums of one chunk of pairs
struct se3tn_points {
  int device = -1, P = 0;
  DeviceBuf<double> xyz;    // [P,3]
  DeviceBuf<double> part;   // [PE_CHUNK][tiles][2] (pose_errors_plan.h)
  DeviceBuf<double> nrm;    // [P,3] normals (se3tn_points_set_normals), or empty: read by se3tn_score_pose_grid with facing only
};

// Init-time entry points that allocate or launch (plane derivation, workspace growth) run on the CONTEXT's device whatever device the
// calling thread has current (two contexts on two GPUs in one process: ADVICE r3), and leave the caller's current device as it was.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    if (device < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) err = hipSetDevice(device);
    else prev = -1;   // nothing to restore
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// The gate EVERY growth of a lazily sized buffer passes once its capacity test has failed.  Order: guard (the growth runs on the
// context's device; `g` is the caller's so that it outlives the allocations), drain (alloc() frees the old block, and another stream
// of this context may still be reading it: the whole DEVICE is waited for), then alloc() buffer by buffer, the capacity published
// LAST -- a capacity kept in a field of its own is zeroed before the first alloc(), so a half-failed growth reads as empty and the
// next call grows again
static int begin_growth(DeviceGuard& g) {
  if (g.err != hipSuccess) return hipfail(g.err, "hipSetDevice");
  HIPCHK(hipDeviceSynchronize());
  return SE3TN_OK;
}
static void raster_scratch(RasterArgs& a, const RasterScratch& s) {
  a.vpost = s.vpost.get(); a.vsnap = s.vsnap.get(); a.big = s.big.get(); a.clipq = s.clipq.get();
}

// ---- Winograd workspaces ----------------------------------------------------------------------------
static const ConvId kWinoConvs[4] = {LAB2_1, LAB2_2, LH2_1, LH2_2};
static int wino_slot(ConvId id) {
  for (int i = 0; i < 4; ++i)
    if (kWinoConvs[i] == id) return i;
  return -1;
}
// V / M: the largest layer shape over m = 2 | 4 | 6, floats per image: (m=2) 16 x 36 tiles x 1024 ch | 16 x 121 x 256
// (m = 6: 64 frequencies x 4 | 16 tiles: smaller)
static size_t wino_ws_floats(int max_batch) {
  const size_t head = (size_t)16 * 36 * 1024, ab = (size_t)16 * 121 * 256;
  return (size_t)max_batch * (head > ab ? head : ab);
}
static const ConvId kWino64Convs[4] = {L64_1, L64_2, L64_3, L64_4};
static int wino64_prepare(se3tn_ctx* c, hipStream_t st) {
  if (c->wino64_min_batch <= 0 || c->max_batch < c->wino64_min_batch || !c->blob || c->wino64_blob == c->blob) return SE3TN_OK;
  for (int i = 0; i < 4; ++i) {
    const Conv3& s = conv_specs()[kWino64Convs[i]];
    const size_t per_g = (size_t)16 * s.cin * s.cout;
    if (!c->wino64_u[i]) HIPCHK(c->wino64_u[i].alloc(s.groups * per_g));
    for (int g = 0; g < s.groups; ++g)
      HIPCHK(launch_wino_weights(c->blob + c->L.conv_w[kWino64Convs[i]] + (size_t)g * conv3_words(s.cin, s.cout),
                                 c->wino64_u[i].get() + g * per_g, s.cin, s.cout, 2, st));
  }
  HIPCHK(hipStreamSynchronize(st));  // init-time
  c->wino64_blob = c->blob;
  return SE3TN_OK;
}

static int wino_prepare(se3tn_ctx* c, hipStream_t st) {
  DeviceGuard dg(c->device);
  HIPCHK(dg.err);
  if (int rc = wino64_prepare(c, st)) return rc;
  if (c->wino_min_batch <= 0 || c->max_batch < c->wino_min_batch) return SE3TN_OK;
  if (!c->wino_v) {
    HIPCHK(c->wino_v.alloc(wino_ws_floats(c->max_batch)));
    HIPCHK(c->wino_m.alloc(wino_ws_floats(c->max_batch)));
    for (int i = 0; i < 4; ++i) {
      const Conv3& s = conv_specs()[kWinoConvs[i]];
      HIPCHK(c->wino_u[i].alloc((size_t)s.groups * 36 * s.cin * s.cout));
    }
  }
  const int tile = c->wino_tile == 2 ? 2 : 4;   // the planes in wino_u (tile 6 | AUTO keep the F(4x4) set there as well)
  if (c->blob && (c->wino_tile == 6 || c->wino_tile == SE3TN_WINOGRAD_TILE_AUTO || c->wino_tile == SE3TN_WINOGRAD_TILE_6_4) &&
      c->wino6_blob != c->blob) {
    for (int i = 0; i < 4; ++i) {
      const Conv3& s = conv_specs()[kWinoConvs[i]];
      if (!c->wino_u6[i]) HIPCHK(c->wino_u6[i].alloc((size_t)s.groups * 64 * s.cin * s.cout));
      for (int g = 0; g < s.groups; ++g)
        HIPCHK(launch_wino_weights(c->blob + c->L.conv_w[kWinoConvs[i]] + (size_t)g * conv3_words(s.cin, s.cout),
                                   c->wino_u6[i].get() + (size_t)g * 64 * s.cin * s.cout, s.cin, s.cout, 6, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // init-time
    c->wino6_blob = c->blob;
  }
  if (c->blob && (c->wino_blob != c->blob || c->wino_tile_derived != tile)) {
    const bool new_blob = c->wino_blob != c->blob;
    const int nf = (tile + 2) * (tile + 2);
    for (int i = 0; i < 4; ++i) {
      const Conv3& s = conv_specs()[kWinoConvs[i]];
      for (int g = 0; g < s.groups; ++g)
        HIPCHK(launch_wino_weights(c->blob + c->L.conv_w[kWinoConvs[i]] + (size_t)g * conv3_words(s.cin, s.cout),
                                   c->wino_u[i].get() + (size_t)g * nf * s.cin * s.cout, s.cin, s.cout, tile, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // init-time
    c->wino_blob = c->blob;
    c->wino_tile_derived = tile;
    if (new_blob) c->wino_us_blob = nullptr;   // the f16x3 split planes (always of the F(4x4) U) follow the weights
  }
  return SE3TN_OK;
}

// f16x3 mode: the split-f16 panels + per-cout scales, derived on the device from the bound float32 blob (init time: called
// from se3tn_set_precision / se3tn_upload_weights / se3tn_bind_weights, never from a stream-ordered compute call)
static int split_prepare(se3tn_ctx* c, hipStream_t st) {
  if (c->device < 0 || c->prec != SE3TN_PREC_F16X3 || !c->blob) return SE3TN_OK;
  DeviceGuard dg(c->device);
  HIPCHK(dg.err);
  if (c->split_blob != c->blob) {
    if (!c->split_w) HIPCHK(c->split_w.alloc(c->SL.total));
    HIPCHK(launch_split_weights(c->blob, c->L, c->split_w.get(), c->SL, st));
    HIPCHK(hipStreamSynchronize(st));  // init-time
    c->split_blob = c->blob;
  }
  // the fused F(4x4) blocks in f16x3 mode: split rows of U = G g G^T (derived by wino_prepare, which runs first)
  if (c->wino_u[0].get() && c->wino_blob == c->blob && c->wino_tile_derived == 4 &&
      (c->wino_us_blob != c->blob || c->wino_us_tile != 4)) {
    for (int i = 0; i < 4; ++i) {
      const Conv3& s = conv_specs()[kWinoConvs[i]];
      const size_t per_g = (size_t)36 * s.cin * s.cout;
      if (!c->wino_us[i]) {
        HIPCHK(c->wino_us[i].alloc(s.groups * per_g));
        HIPCHK(c->wino_usc[i].alloc((size_t)s.groups * 36 * s.cout));
      }
      for (int g = 0; g < s.groups; ++g)
        HIPCHK(launch_split_wino_u(c->wino_u[i].get() + g * per_g, c->wino_us[i].get() + g * per_g, c->wino_usc[i].get() + (size_t)g * 36 * s.cout, s.cin,
                                   s.cout, 36, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    c->wino_us_blob = c->blob;
    c->wino_us_tile = 4;
  }
  return SE3TN_OK;
}

// scratch of se3tn_fill_depth (3 float images + min/max + table) and the rasteriser's z-buffer: grown here, at start-up
// (se3tn_reserve) or on the first call with a larger frame (begin_growth)
static int reserve_fill_depth(se3tn_ctx* c, size_t px) {
  if (px <= c->fd_pixels) return SE3TN_OK;
  DeviceGuard dg(c->device);
  if (int rc = begin_growth(dg)) return rc;
  c->fd_pixels = 0;
  HIPCHK(c->fd_buf.alloc(3 * px + 2 + 4098 + 2));
  c->fd_pixels = px;
  return SE3TN_OK;
}
static int reserve_zbuf(se3tn_ctx* c, size_t px) {
  if (px <= c->zbuf.count()) return SE3TN_OK;
  DeviceGuard dg(c->device);
  if (int rc = begin_growth(dg)) return rc;
  HIPCHK(c->zbuf.alloc(px));
  return SE3TN_OK;
}
static bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
// A stream-ordered entry point whose scratch is too small (not reserved: se3tn_reserve) grows it now -- impossible inside a stream
// capture.  fill: the depth fill's scratch for a frame of px pixels, else the rasteriser's z-buffer for px pixels of a `what`
static int grow_now_or_refuse(se3tn_ctx* c, const char* fn, bool fill, const char* what, size_t px, void* stream) {
  if (px <= (fill ? c->fd_pixels : c->zbuf.count())) return SE3TN_OK;
  if (stream_is_capturing((hipStream_t)stream))
    return fail(SE3TN_E_STATE, std::string(fn) + (fill ? ": scratch" : ": z-buffer") + " too small for this " + what +
                                   " inside a stream capture: call se3tn_reserve(ctx, H, W) first");
  return fill ? reserve_fill_depth(c, px) : reserve_zbuf(c, px);
}

// ---- what the entry points of the pose family share ------------------------------------------------------------------------------------
// The refusals, piece by piece; each entry point composes them in its own order
static int refuse_if(bool bad, int code, const char* who, const std::string& msg) { return bad ? fail(code, std::string(who) + ": " + msg) : SE3TN_OK; }
static int null_argument(const char* who) { return refuse_if(true, SE3TN_E_ARG, who, "NULL argument"); }
static int device_check(const char* who, const se3tn_ctx* c, const char* verb) {
  return refuse_if(c->device < 0, SE3TN_E_ARG, who, std::string("host-only context (device = -1) has no device to ") + verb + " on");
}
static int same_device_check(const char* who, const se3tn_ctx* c, const se3tn_points* p) {
  return refuse_if(p->device != c->device, SE3TN_E_ARG, who, "the points live on another device than the context");
}
static int normals_check(const char* who, const se3tn_points* p, const char* lead) {
  return refuse_if(!p->nrm, SE3TN_E_STATE, who, std::string(lead) + "the points handle has no normals (se3tn_points_set_normals)");
}
static int frame_check(const char* who, int H, int W) { return refuse_if(H < 1 || W < 1, SE3TN_E_ARG, who, "empty frame (H or W < 1)"); }
static int mm_check(const char* who, const char* name, int mm) {   // tol_mm, gate_mm
  return refuse_if(mm < 1 || mm > 65535, SE3TN_E_ARG, who, std::string(name) + " = " + std::to_string(mm) + " outside [1, 65535]");
}
static int count_check(const char* who, int n, int most, const char* most_name) {
  return refuse_if(n < 1 || n > most, SE3TN_E_ARG, who,
                   "n = " + std::to_string(n) + " outside [1, " + most_name + " = " + std::to_string(most) + "]");
}
// what a _host entry point asks of its arrays: the first `used` of every `stride` elements of a (and of b, if given) are finite.
// (A row is tested without a branch per element: a branch each, or a modulus to find the row, costs 20-170 us per 9,317 poses.)
static int finite_check(const char* who, const char* noun, const double* a, const double* b, size_t n, int stride, int used) {
  for (size_t r = 0; r < n; ++r) {
    bool bad = false;
    for (int k = 0; k < used; ++k) bad |= !std::isfinite(a[r * stride + k]) || (b && !std::isfinite(b[r * stride + k]));
    if (bad) return refuse_if(true, SE3TN_E_ARG, who, std::string(noun) + " " + std::to_string(r) + " has an entry that is not finite");
  }
  return SE3TN_OK;
}
static int finite_K_check(const char* who, const double K[9]) {
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(K[i])) return refuse_if(true, SE3TN_E_ARG, who, "K entry " + std::to_string(i) + " is not finite");
  return SE3TN_OK;
}
// One synchronous _host call on the context's staging pair (ps_host / ps_dev), which is laid out for THIS call: the upload is one
// contiguous run from 0, and so is the read-back.  The caller copies its inputs to h between grow() and upload(), enqueues its
// launches on d between upload() and finish(), and copies its results from h after finish().  Nothing outlives the call, so no
// call sees another's bytes.
struct StagedCall {
  se3tn_ctx* c;
  const char* who;
  hipStream_t st;
  unsigned char* h = nullptr;   // pinned host
  unsigned char* d = nullptr;   // its device mirror
  int refuse_capture() const { return refuse_if(stream_is_capturing(st), SE3TN_E_STATE, who, "the call is synchronous, it cannot be captured"); }
  int grow(size_t bytes) {
    c->ps_scene_H = c->ps_scene_W = 0;   // (this call's layout replaces whatever a scene search left)
    if (bytes > c->ps_cap) {   // first / larger call: the staging belongs to the context's device
      DeviceGuard dg(c->device);
      if (int rc = begin_growth(dg)) return rc;
      c->ps_cap = 0;
      HIPCHK(c->ps_host.alloc(bytes));
      HIPCHK(c->ps_dev.alloc(bytes));
      c->ps_cap = bytes;
    }
    h = c->ps_host.get();
    d = c->ps_dev.get();
    return SE3TN_OK;
  }
  int upload(size_t bytes) const {
    HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
    return SE3TN_OK;
  }
  int finish(size_t at, size_t bytes) const {   // the read-back of [at, at + bytes), and the wait
    HIPCHK(hipMemcpyAsync(h + at, d + at, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SE3TN_OK;
  }
  template <class T> T* dev(size_t at) const { return reinterpret_cast<T*>(d + at); }
};

// ---- the crop records: what se3tn_fit_stats, the fit check, se3tn_color_stats and se3tn_verify_poses_host share ----------------------------
// what se3tn_fit_stats and se3tn_color_stats refuse alike (rgb_read: the colour record reads rgb too)
static int crops_check(const std::string& who, const se3tn_ctx* c, const se3tn_crop* model, const se3tn_crop* observed, int n, int tol_mm,
                       const void* out_dev, bool rgb_read) {
  if (!c || c->device < 0 || !model || !observed || !out_dev) return fail(SE3TN_E_ARG, who + ": bad argument");
  if (n < 1 || n > c->max_batch) return fail(SE3TN_E_ARG, who + ": n outside [1, max_batch]");
  if (tol_mm < 1 || tol_mm > 65535) return fail(SE3TN_E_ARG, who + ": tol_mm outside [1, 65535]");
  for (int i = 0; i < n; ++i)
    for (const se3tn_crop* k : {model + i, observed + i})
      if ((rgb_read && !k->rgb) || !k->depth || k->H < 1 || k->W < 1 || k->right <= k->left || k->bottom <= k->top)
        return fail(SE3TN_E_ARG, who + ": descriptor " + std::to_string(i) + (rgb_read ? ": NULL rgb or depth" : ": NULL depth") + ", empty image or empty window");
  return SE3TN_OK;
}

// The crop records of n pairs, Args::MAX pairs per launch (the descriptors travel as kernel arguments): pair(j, m, o) fills
// pair j's descriptors -- Args = FitSceneArgs, the scene-aware rule: pair(j, m, o, s).  `colour` asks for the colour records too and picks the context's counters
// (fit launches and colour launches on two streams of one context do not touch each other's words); raw_depth: the raw crop stacks (FitArgs)
template <class Args = FitArgs, class Pair>
static int fit_launches(se3tn_ctx* c, int n, Pair pair, se3tn_fit* fit, se3tn_color_fit* colour, int tol, uint8_t* raw_rgb, uint16_t* raw_depth,
                        hipStream_t st) {
  unsigned* const counters = colour ? c->color_counters.get() : c->fit_counters.get();
  const size_t words = colour ? FitArgs::COLOUR_WORDS : FitArgs::WORDS;
  for (int g0 = 0; g0 < n; g0 += Args::MAX) {
    const int k = n - g0 < Args::MAX ? n - g0 : Args::MAX;
    Args a;
    for (int j = 0; j < k; ++j) { if constexpr (Args::SCENE) pair(g0 + j, a.m[j], a.o[j], a.s[j]); else pair(g0 + j, a.m[j], a.o[j]); }
    a.counters = counters + words * g0;
    a.fit = fit ? fit + g0 : nullptr;
    a.colour = colour ? colour + g0 : nullptr;
    a.tol = tol;
    if constexpr (!Args::SCENE) if (raw_depth) {
      a.raw_rgb = raw_rgb + (size_t)g0 * RES * RES * 3;
      a.raw_depth = raw_depth + (size_t)g0 * RES * RES;
    }
    HIPCHK(launch_fit_stats(a, k, st));
  }
  return SE3TN_OK;
}

extern "C" {

const char* se3tn_version(void) { return "se3tracknet-gfx950 0.6.0 (blob v7)"; }
const char* se3tn_last_error(void) { return g_err.c_str(); }

int se3tn_create(int device, int max_batch, se3tn_ctx** out) {
  if (!out || max_batch < 1) return fail(SE3TN_E_ARG, "se3tn_create: bad argument");
  if (max_batch > SE3TN_MAX_BATCH_LIMIT)   // (the kernels' 32-bit byte offsets from a tensor's base: include/se3tracknet.h)
    return fail(SE3TN_E_ARG, "se3tn_create: max_batch " + std::to_string(max_batch) + " exceeds SE3TN_MAX_BATCH_LIMIT (" +
                                 std::to_string(SE3TN_MAX_BATCH_LIMIT) + "): run larger sets as several calls");
  se3tn_ctx* c = new se3tn_ctx();
  c->device = device;
  c->max_batch = max_batch;
  c->L = blob_layout();
  c->SL = split_layout();
  if (const char* e = std::getenv("SE3TN_WINOGRAD_AUTO_TILE_AB2")) c->auto_tile_override[0] = (std::atoi(e) == 4 || std::atoi(e) == 6) ? std::atoi(e) : 0;
  if (const char* e = std::getenv("SE3TN_WINOGRAD_AUTO_TILE_HEADS")) c->auto_tile_override[1] = (std::atoi(e) == 4 || std::atoi(e) == 6) ? std::atoi(e) : 0;
  if (const char* e = std::getenv("SE3TN_WINO_GEMMP")) c->gemmp = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("SE3TN_WINOGRAD_FUSE")) c->wino_fuse = std::atoi(e) != 0;      // developer A/B switch (and the tests'
                                                                                                  // bit-equality check of the two forms)
  if (const char* e = std::getenv("SE3TN_TRUNK_WINOGRAD")) c->wino64_min_batch = std::atoi(e);   // developer A/B switch
  if (const char* e = std::getenv("SE3TN_TRUNK_WINOGRAD_FILL")) c->wino64_min_fill = std::atoi(e);   // (scripts/trunk_sweep.sh)
  for (int i = 0; i < 8; ++i) { c->mean[i] = 0.0; c->stdv[i] = 1.0; }
  if (device >= 0) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) { delete c; return hipfail(e, "hipGetDeviceProperties"); }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      std::string a = prop.gcnArchName;
      delete c;
      return fail(SE3TN_E_DEVICE, "device is " + a + ", this library is built for gfx950 only");
    }
    if (prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
    e = hipSetDevice(device);
    if (e != hipSuccess) { delete c; return hipfail(e, "hipSetDevice"); }
    const size_t mb = (size_t)max_batch;
    auto padded = [&](int s, int ch) { return (mb * (s + 2) * (s + 2) + PAD_SLACK_PX) * ch; };
    struct { DeviceBuf<float>* p; size_t words; bool zero; } bufs[] = {
        {&c->inA, (mb * IN_P + IN_SLACK_ROWS) * IN_P * 4, true},
        {&c->inB, (mb * IN_P + IN_SLACK_ROWS) * IN_P * 4, true},
        {&c->stem, mb * S1 * S1 * 128, false}, {&c->pool, padded(S2, 128), true},
        {&c->t64, padded(S2, 128), true},      {&c->q64, padded(S2, 128), true},
        {&c->ab, padded(S3, 256), true},       {&c->ab_t, padded(S3, 256), true},
        {&c->head, padded(S4, 1024), true},    {&c->head_t, padded(S4, 1024), true},
        {&c->head_f, padded(S4, 1024), true},
        {&c->logits, mb * 6, true},           {&c->fcpart, mb * 192, true}};
    for (auto& b : bufs) {
      // the one-pixel borders are written here once and never again (kernels store interiors only)
      e = b.p->alloc(b.words, b.zero);
      if (e != hipSuccess) { delete c; return hipfail(e, "hipMalloc(workspace)"); }
    }
    // split-K workspace: 16 slices of the widest layer (1024 couts x 121 px) up to batch 16
    e = c->part.alloc((size_t)16 * 1024 * 121 * 16);
    if (e == hipSuccess) e = c->tail_arrive.alloc(c->max_batch, true);
    if (e == hipSuccess) e = c->fit_counters.alloc((size_t)FitArgs::WORDS * c->max_batch, true);
    if (e == hipSuccess) e = c->color_counters.alloc((size_t)FitArgs::COLOUR_WORDS * c->max_batch, true);
    if (e == hipSuccess) e = c->sc_counters.alloc((size_t)SCENE_COUNTER_WORDS, true);
    if (const char* sk = std::getenv("SE3TN_SMALL_KERNELS")) c->small_kernels = std::atoi(sk) != 0;
    if (const char* tp = std::getenv("SE3TN_TAIL_PARTS")) { c->tail_parts = std::atoi(tp) != 0; c->tail_parts_ch = std::atoi(tp) == 2 ? 32 : 16; }
    if (e != hipSuccess) { delete c; return hipfail(e, "hipMalloc(split-K workspace)"); }
    e = c->zbuf.alloc((size_t)RES * RES);
    if (e != hipSuccess) { delete c; return hipfail(e, "hipMalloc(zbuf)"); }
    e = c->overflow.alloc(1, true);
    if (e != hipSuccess) { delete c; return hipfail(e, "hipMalloc(overflow flag)"); }
    e = hipDeviceSynchronize();
    if (e != hipSuccess) { delete c; return hipfail(e, "hipDeviceSynchronize"); }
  }
  *out = c;
  return SE3TN_OK;
}

void se3tn_destroy(se3tn_ctx* c) { delete c; }

int se3tn_max_batch(const se3tn_ctx* c) { return c ? c->max_batch : 0; }

int se3tn_set_tensor(se3tn_ctx* c, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!c || !key || !data || !shape || ndim < 1 || ndim > 4) return fail(SE3TN_E_ARG, "se3tn_set_tensor: bad argument");
  for (const ExpectedTensor& e : expected_tensors()) {
    if (e.key != key) continue;
    if ((int)e.shape.size() != ndim) return fail(SE3TN_E_SHAPE, std::string("rank mismatch for ") + key);
    size_t count = 1;
    for (int i = 0; i < ndim; ++i) {
      if (shape[i] != e.shape[i]) return fail(SE3TN_E_SHAPE, std::string("shape mismatch for ") + key);
      count *= (size_t)shape[i];
    }
    StoredTensor& t = c->tensors[key];
    t.shape.assign(shape, shape + ndim);
    t.data.assign(data, data + count);
    return SE3TN_OK;
  }
  return fail(SE3TN_E_KEY, std::string("unexpected state_dict key: ") + key);
}

int se3tn_pack_weights(se3tn_ctx* c) {
  if (!c) return fail(SE3TN_E_ARG, "null ctx");
  std::string err = pack_blob(c->tensors, c->packed);
  if (!err.empty()) return fail(SE3TN_E_KEY, err);
  c->tensors.clear();
  return SE3TN_OK;
}

size_t se3tn_packed_bytes(const se3tn_ctx* c) { return c ? c->L.total * sizeof(float) : 0; }
const void* se3tn_packed_host(const se3tn_ctx* c) { return (c && !c->packed.empty()) ? c->packed.data() : nullptr; }

int se3tn_upload_weights(se3tn_ctx* c, void* stream) {
  if (!c || c->device < 0) return fail(SE3TN_E_ARG, "se3tn_upload_weights: no device context");
  if (c->packed.empty()) return fail(SE3TN_E_STATE, "se3tn_upload_weights: call se3tn_pack_weights first");
  DeviceGuard dg(c->device);   // init-time entry point: runs on the context's device, leaves the caller's current device alone
  HIPCHK(dg.err);
  if (!c->blob_owned) HIPCHK(c->blob_owned.alloc(c->L.total));
  HIPCHK(hipMemcpyAsync(c->blob_owned.get(), c->packed.data(), c->L.total * sizeof(float), hipMemcpyHostToDevice,
                        (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));  // init-time only: the host vector may go away
  c->blob = c->blob_owned.get();
  c->wino_blob = nullptr;  // same address, new contents: every derived plane set follows the weights
  c->wino6_blob = nullptr;
  c->wino64_blob = nullptr;
  c->split_blob = nullptr;
  c->wino_us_blob = nullptr;
  if (int rc = wino_prepare(c, (hipStream_t)stream)) return rc;
  return split_prepare(c, (hipStream_t)stream);
}

int se3tn_bind_weights(se3tn_ctx* c, const void* device_blob, size_t bytes) {
  if (!c || c->device < 0 || !device_blob) return fail(SE3TN_E_ARG, "se3tn_bind_weights: bad argument");
  if (bytes != c->L.total * sizeof(float)) return fail(SE3TN_E_SHAPE, "se3tn_bind_weights: blob size mismatch");
  DeviceGuard dg(c->device);
  HIPCHK(dg.err);
  uint32_t hdr[4];
  HIPCHK(hipMemcpy(hdr, device_blob, sizeof(hdr), hipMemcpyDeviceToHost));  // init-time validation
  if (hdr[0] != BLOB_MAGIC || hdr[1] != BLOB_VERSION || hdr[2] != (uint32_t)c->L.total)
    return fail(SE3TN_E_SHAPE, "se3tn_bind_weights: bad blob header");
  c->blob = (const float*)device_blob;
  c->wino_blob = nullptr;
  c->wino6_blob = nullptr;
  c->wino64_blob = nullptr;
  c->split_blob = nullptr;
  c->wino_us_blob = nullptr;
  if (int rc = wino_prepare(c, nullptr)) return rc;
  return split_prepare(c, nullptr);
}

int se3tn_set_winograd(se3tn_ctx* c, int min_batch, int tile) {
  if (!c || min_batch < 0 || (tile != 0 && tile != 2 && tile != 4 && tile != 6 && tile != SE3TN_WINOGRAD_TILE_AUTO && tile != SE3TN_WINOGRAD_TILE_6_4))
    return fail(SE3TN_E_ARG, "se3tn_set_winograd: min_batch >= 0 and tile in {0, 2, 4, 6, SE3TN_WINOGRAD_TILE_6_4, SE3TN_WINOGRAD_TILE_AUTO}");
  c->wino_min_batch = min_batch;
  if (tile) c->wino_tile = tile;
  if (c->device < 0) return SE3TN_OK;
  if (int rc = wino_prepare(c, nullptr)) return rc;
  return split_prepare(c, nullptr);
}

int se3tn_set_trunk_winograd(se3tn_ctx* c, int min_batch, int min_fill_percent) {
  if (!c || min_batch < 0 || min_fill_percent < 0 || min_fill_percent > 100)
    return fail(SE3TN_E_ARG, "se3tn_set_trunk_winograd: min_batch >= 0, 0 <= min_fill_percent <= 100");
  c->wino64_min_batch = min_batch;
  c->wino64_min_fill = min_fill_percent;
  if (c->device < 0) return SE3TN_OK;
  return wino_prepare(c, nullptr);
}

int se3tn_get_trunk_winograd(const se3tn_ctx* c, int* min_batch, int* min_fill_percent) {
  if (!c || !min_batch || !min_fill_percent) return fail(SE3TN_E_ARG, "se3tn_get_trunk_winograd: bad argument");
  *min_batch = c->wino64_min_batch;
  *min_fill_percent = c->wino64_min_fill;
  return SE3TN_OK;
}

int se3tn_get_winograd(const se3tn_ctx* c, int* min_batch, int* tile) {
  if (!c || !min_batch || !tile) return fail(SE3TN_E_ARG, "se3tn_get_winograd: bad argument");
  *min_batch = c->wino_min_batch;
  *tile = c->wino_tile;
  return SE3TN_OK;
}

int se3tn_set_normalization(se3tn_ctx* c, const double mean[8], const double stdv[8]) {
  if (!c || !mean || !stdv) return fail(SE3TN_E_ARG, "se3tn_set_normalization: bad argument");
  std::memcpy(c->mean, mean, sizeof(c->mean));
  std::memcpy(c->stdv, stdv, sizeof(c->stdv));
  c->have_norm = true;
  return SE3TN_OK;
}

int se3tn_set_precision(se3tn_ctx* c, int mode) {
  if (!c || (mode != SE3TN_PREC_F32 && mode != SE3TN_PREC_F16X3)) return fail(SE3TN_E_ARG, "se3tn_set_precision: bad mode");
  c->prec = mode;
  // first selection of f16x3 (or new weights since): derive the split panels from the bound blob -- here, not in se3tn_infer
  // (after U: the split rows of the F(4x4) planes come from wino_u)
  if (c->device >= 0) {
    if (int rc = wino_prepare(c, nullptr)) return rc;
  }
  return split_prepare(c, nullptr);
}

int se3tn_reserve(se3tn_ctx* c, int H, int W) {
  if (!c || c->device < 0 || H < 1 || W < 1) return fail(SE3TN_E_ARG, "se3tn_reserve: bad argument");
  DeviceGuard dg(c->device);
  HIPCHK(dg.err);
  if (int rc = reserve_fill_depth(c, (size_t)H * W)) return rc;
  if (int rc = reserve_zbuf(c, (size_t)H * W)) return rc;
  if (int rc = wino_prepare(c, nullptr)) return rc;
  return split_prepare(c, nullptr);
}

size_t se3tn_split_weights_bytes(const se3tn_ctx* c) { return c ? c->SL.total * sizeof(float) : 0; }
const void* se3tn_split_weights_device(const se3tn_ctx* c) { return (c && c->split_blob) ? c->split_w.get() : nullptr; }
int se3tn_split_weights_host(const void* packed_blob_host, size_t blob_bytes, void* out_split, size_t out_bytes) {
  const BlobLayout L = blob_layout();
  const SplitLayout S = split_layout();
  if (!packed_blob_host || !out_split || blob_bytes != L.total * sizeof(float) || out_bytes != S.total * sizeof(float))
    return fail(SE3TN_E_ARG, "se3tn_split_weights_host: bad argument");
  split_blob_host((const float*)packed_blob_host, (float*)out_split);
  return SE3TN_OK;
}

int se3tn_keep_intermediates(se3tn_ctx* c, int on) {
  if (!c) return fail(SE3TN_E_ARG, "null ctx");
  c->keep_intermediates = on != 0;
  return SE3TN_OK;
}

int se3tn_overflow(se3tn_ctx* c, int* flag) {
  if (!c || c->device < 0 || !flag) return fail(SE3TN_E_ARG, "se3tn_overflow: bad argument");
  HIPCHK(hipMemcpy(flag, c->overflow.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (*flag) HIPCHK(hipMemset(c->overflow.get(), 0, sizeof(int)));
  return SE3TN_OK;
}

int se3tn_set_offset_rule(se3tn_ctx* c, int rule) {
  if (!c || (rule != SE3TN_OFFSET_RULE_NUMPY1 && rule != SE3TN_OFFSET_RULE_NUMPY2)) return fail(SE3TN_E_ARG, "se3tn_set_offset_rule: bad rule");
  c->offset_rule = rule;
  return SE3TN_OK;
}
int se3tn_get_offset_rule(const se3tn_ctx* c) { return c ? c->offset_rule : -1; }

int se3tn_set_normalizers(se3tn_ctx* c, double tn, double rn) {
  if (!c) return fail(SE3TN_E_ARG, "null ctx");
  c->tn = tn;
  c->rn = rn;
  return SE3TN_OK;
}

float* se3tn_input_buffer(se3tn_ctx* c, int which) { return !c ? nullptr : (which == 0 ? c->inA.get() : c->inB.get()); }

// se3tn_preprocess; raw_rgb / raw_depth non-null: crop i also leaves its raw pixels (crop_bbox alone) as image i of [n,176,176,3] /
// [n,176,176] (image A of the full-frame route: se3tn_on_track_batch)
static int preprocess_impl(se3tn_ctx* c, const se3tn_crop* crops, int n, float* out, uint8_t* raw_rgb, uint16_t* raw_depth, void* stream) {
  if (!c || c->device < 0 || !crops || !out || n < 0) return fail(SE3TN_E_ARG, "se3tn_preprocess: bad argument");
  if (!c->have_norm) return fail(SE3TN_E_STATE, "se3tn_preprocess: call se3tn_set_normalization first");
  // the context's own input buffers hold max_batch images: more crops would run past them
  if ((out == c->inA.get() || out == c->inB.get()) && n > c->max_batch)
    return fail(SE3TN_E_ARG, "se3tn_preprocess: n > max_batch for the context's input buffer");
  for (int i = 0; i < n; ++i) {
    const se3tn_crop& k = crops[i];
    if (!k.rgb || !k.depth || k.H < 1 || k.W < 1 || k.right <= k.left || k.bottom <= k.top || (k.stats & ~1))
      return fail(SE3TN_E_ARG, "se3tn_preprocess: bad crop descriptor " + std::to_string(i));
  }
  CropArgs a;
  std::memcpy(a.mean, c->mean, sizeof(a.mean));
  std::memcpy(a.stdv, c->stdv, sizeof(a.stdv));
  for (int i0 = 0; i0 < n; i0 += CropArgs::MAX) {
    a.n = (n - i0 < CropArgs::MAX) ? n - i0 : CropArgs::MAX;
    std::memcpy(a.c, crops + i0, sizeof(se3tn_crop) * a.n);
    // the context's own input buffers are zero-bordered [n,182,182,4]; anything else is plain NHWC
    a.padded = (out == c->inA.get() || out == c->inB.get()) ? 1 : 0;
    // the context's input buffers hold split pixels in f16x3 mode (consumed by the f16 stem)
    a.split = (a.padded && c->prec == SE3TN_PREC_F16X3) ? 1 : 0;
    a.overflow = c->overflow.get();
    a.offset_rule = c->offset_rule;
    if (a.padded) c->in_split[out == c->inA.get() ? 0 : 1] = a.split;
    a.out = out + (size_t)i0 * (a.padded ? IN_P * IN_P : RES * RES) * 4;
    a.out2 = nullptr; a.n_first = a.n;
    a.raw_rgb = raw_rgb ? raw_rgb + (size_t)i0 * RES * RES * 3 : nullptr;
    a.raw_depth = raw_rgb ? raw_depth + (size_t)i0 * RES * RES : nullptr;
    HIPCHK(launch_preprocess(a, (hipStream_t)stream));
  }
  return SE3TN_OK;
}

int se3tn_preprocess(se3tn_ctx* c, const se3tn_crop* crops, int n, float* out, void* stream) {
  return preprocess_impl(c, crops, n, out, nullptr, nullptr, stream);
}

int se3tn_crop_raw(se3tn_ctx* c, const se3tn_crop* k, uint8_t* rgb_out, uint16_t* depth_out, void* stream) {
  if (!c || c->device < 0 || !k || !rgb_out || !depth_out) return fail(SE3TN_E_ARG, "se3tn_crop_raw: bad argument");
  if (!k->rgb || !k->depth || k->H < 1 || k->W < 1 || k->right <= k->left || k->bottom <= k->top)
    return fail(SE3TN_E_ARG, "se3tn_crop_raw: bad crop descriptor");
  HIPCHK(launch_crop_raw(*k, rgb_out, depth_out, (hipStream_t)stream));
  return SE3TN_OK;
}

static int prof_mark(se3tn_ctx* c, hipStream_t st, const char* name, bool is_conv) {
  if (!c->prof) return 0;
  if (c->n_launch >= MAX_LAUNCHES) return 0;
  c->names[c->n_launch] = name;
  c->is_conv[c->n_launch] = is_conv;
  ++c->n_launch;
  return (int)hipEventRecord(c->ev[c->n_launch], st);
}

// the labels of infer_plan.h's step_label, interned: the strings live as long as the library (only ever reached by a profiled call)
static const char* intern_label(const std::string& label) {
  static std::mutex mu;
  static std::set<std::string> names;
  std::lock_guard<std::mutex> lk(mu);
  return names.insert(label).first->c_str();
}

// Everything the route of a forward pass of n pairs depends on (infer_plan.h), read from the context in ONE place.  `f` is zeroed by the
// caller: it is compared as bytes (GraphKey)
static void fill_config(const se3tn_ctx* c, int n, bool small_family, InferConfig& f) {
  f.n = n; f.prec = c->prec; f.keep_intermediates = c->keep_intermediates ? 1 : 0;
  f.small_kernels = c->small_kernels ? 1 : 0; f.small_family = small_family ? 1 : 0;
  f.tail_parts = c->tail_parts ? 1 : 0; f.tail_parts_ch = c->tail_parts_ch;
  f.wino_min_batch = c->wino_min_batch; f.wino_tile = c->wino_tile;
  f.auto_tile_override[0] = c->auto_tile_override[0]; f.auto_tile_override[1] = c->auto_tile_override[1];
  f.wino_fuse = c->wino_fuse ? 1 : 0; f.gemmp = c->gemmp;
  f.wino64_min_batch = c->wino64_min_batch; f.wino64_min_fill = c->wino64_min_fill; f.num_cus = c->num_cus;
  f.part_bytes = c->part.count() * sizeof(float);
  f.tn = c->tn; f.rn = c->rn;
  f.ready = (c->wino_v.get() ? READY_WINO_VM : 0u) | (c->wino_tile_derived == 2 ? READY_U2 : c->wino_tile_derived == 4 ? READY_U4 : 0u) |
            (c->wino_u6[0].get() && c->wino6_blob == c->blob ? READY_U6 : 0u) | (c->wino64_blob == c->blob ? READY_TRUNK : 0u) |
            (c->split_blob == c->blob ? READY_SPLIT_W : 0u) | (c->wino_us_blob == c->blob && c->wino_us_tile == 4 ? READY_SPLIT_U4 : 0u);
}

// ---- executing a planned forward pass: conv_table() rows -> kernel argument blocks ----------------------------------------------------
static float* tensor_ptr(se3tn_ctx* c, const TensorRef& t, bool fast) {
  float* p = nullptr;
  switch (t.buf) {
    case BUF_POOL: p = c->pool.get(); break;
    case BUF_T64: p = c->t64.get(); break;
    case BUF_Q64: p = c->q64.get(); break;
    case BUF_AB: p = c->ab.get(); break;
    case BUF_AB_T: p = c->ab_t.get(); break;
    case BUF_HEAD: p = c->head.get(); break;
    case BUF_HEAD_T: p = c->head_t.get(); break;
    case BUF_HEAD_OUT: p = fast ? c->head_f.get() : c->head.get(); break;
    case BUF_NONE: return nullptr;
  }
  return p + t.ch;
}
// ip != nullptr: the mixed-model call (image i reads w / bias ip->off[i] floats from W)
static void fill_conv_args(se3tn_ctx* c, const ConvRow& r, int n, const float* W, const ImgParams* ip, bool fast, ConvArgs& a) {
  const Conv3& s = conv_specs()[r.id];
  a = ConvArgs{};
  a.in = tensor_ptr(c, r.in, fast); a.w = W + c->L.conv_w[r.id]; a.bias = W + c->L.conv_b[r.id];
  if (fast) {
    a.fast = 1;
    a.overflow = c->overflow.get();
    a.w = c->split_w.get() + c->SL.conv_ws[r.id];
    a.wscale = c->split_w.get() + c->SL.conv_sc[r.id];
  }
  a.res = tensor_ptr(c, r.res, fast); a.out = tensor_ptr(c, r.out, fast);
  a.part = c->part.get(); a.part_bytes = c->part.count() * sizeof(float);
  a.in_ld = r.in.ld; a.res_ld = r.res.ld; a.out_ld = r.out.ld;
  a.H = r.hin; a.W = r.hin; a.Ho = (r.hin - 1) / r.stride + 1; a.Wo = a.Ho;
  a.M = n * a.Ho * a.Wo;
  a.groups = s.groups;
  a.in_gs = r.in.gs; a.res_gs = r.res.gs; a.out_gs = r.out.gs; a.bias_gs = s.cout;
  a.w_gs = (long long)conv3_words(s.cin, s.cout);
  if (ip) {
    a.per_img = 1;
    std::memcpy(a.img_off, ip->off, sizeof(a.img_off));
  }
}
// split: the f16x3 form of a fused F(4x4) block (split-row activations / V / U, float32 M)
static void fill_wino_args(se3tn_ctx* c, const ConvRow& r, int tile, int n, const float* W, bool split, WinoArgs& w) {
  const Conv3& s = conv_specs()[r.id];
  const int ws = wino_slot(r.id);
  w = WinoArgs{};
  w.in = tensor_ptr(c, r.in, split); w.bias = W + c->L.conv_b[r.id]; w.res = tensor_ptr(c, r.res, split); w.out = tensor_ptr(c, r.out, split);
  w.U = tile == 6 ? c->wino_u6[ws].get() : c->wino_u[ws].get();
  w.V = c->wino_v.get(); w.Mw = c->wino_m.get();
  w.in_ld = r.in.ld; w.res_ld = r.res.ld; w.out_ld = r.out.ld;
  w.m = tile; w.nf = (tile + 2) * (tile + 2);
  w.H = r.hin; w.W = r.hin; w.th = (r.hin + tile - 1) / tile; w.tw = w.th;
  w.n = n; w.T = n * w.th * w.tw;
  w.C = s.cin; w.Cout = s.cout; w.groups = s.groups;
  w.in_gs = r.in.gs; w.res_gs = r.res.gs; w.out_gs = r.out.gs; w.bias_gs = s.cout;
  w.u_gs = (long long)w.nf * s.cin * s.cout;
  if (split) {
    w.split = 1;
    w.U = c->wino_us[ws].get(); w.uscale = c->wino_usc[ws].get();
    w.overflow = c->overflow.get();
  }
}

static int infer_launch(se3tn_ctx* c, const float* A, const float* B, int n, int layout, float* trans, float* rot,
                        const double* poseA, double* poseB, void* stream);

int se3tn_enable_graphs(se3tn_ctx* c, int on) {
  if (!c || c->device < 0) return fail(SE3TN_E_ARG, "se3tn_enable_graphs: no device context");
  c->use_graphs = on != 0;
  return SE3TN_OK;
}

// With graphs enabled, the ~25 dependent launches of one se3tn_infer are captured once per argument
// set (second call with identical arguments; the first runs eagerly) and replayed with one
// hipGraphLaunch afterwards: the batch-1 tracking step is launch-bound (kernels of 10-30 us).
static int infer_graph_or_launch(se3tn_ctx* c, const float* A, const float* B, int n, int layout, float* trans, float* rot,
                                 const double* poseA, double* poseB, void* stream);

int se3tn_infer(se3tn_ctx* c, const float* A, const float* B, int n, int layout, float* trans, float* rot,
                const double* poseA, double* poseB, void* stream) {
  if (c && c->rearm_counters && c->device >= 0 && !stream_is_capturing((hipStream_t)stream)) {
    // a launch sequence that failed half-way can leave the tail's arrival counters non-zero, and every
    // later frame would then find no "last" workgroup: clear them, stream-ordered, before the next frame
    if (c->tail_arrive) HIPCHK(hipMemsetAsync(c->tail_arrive.get(), 0, sizeof(int) * c->max_batch, (hipStream_t)stream));
    c->rearm_counters = false;
  }
  const int rc = infer_graph_or_launch(c, A, B, n, layout, trans, rot, poseA, poseB, stream);
  if (rc != SE3TN_OK && rc != SE3TN_E_ARG && rc != SE3TN_E_STATE && c) c->rearm_counters = true;
  return rc;
}

static int infer_graph_or_launch(se3tn_ctx* c, const float* A, const float* B, int n, int layout, float* trans, float* rot,
                                 const double* poseA, double* poseB, void* stream) {
  if (!c || !c->use_graphs || c->prof || stream == nullptr)  // the null stream cannot be captured
    return infer_launch(c, A, B, n, layout, trans, rot, poseA, poseB, stream);
  if (n < 1 || n > c->max_batch) return infer_launch(c, A, B, n, layout, trans, rot, poseA, poseB, stream);   // (refused there)
  GraphKey key;
  std::memset(&key, 0, sizeof(key));
  key.A = A; key.B = B; key.trans = trans; key.rot = rot; key.poseA = poseA; key.poseB = poseB; key.blob = c->blob;
  key.layout = layout;
  fill_config(c, n, false, key.cfg);
  hipStream_t st = (hipStream_t)stream;
  for (auto& g : c->graphs) {
    if (!(g.key == key)) continue;
    if (g.exec) {
      const int want_split = c->prec == SE3TN_PREC_F16X3 ? 1 : 0;
      if ((A == c->inA.get() && c->in_split[0] != want_split) || (B == c->inB.get() && c->in_split[1] != want_split))
        return fail(SE3TN_E_STATE, "se3tn_infer: the input buffers were filled under a different precision mode");
      HIPCHK(hipGraphLaunch(g.exec, st));
      c->last_fast = key.cfg.prec == SE3TN_PREC_F16X3;
      c->plan = g.plan;
      c->written = g.plan.written;
      return SE3TN_OK;
    }
    // second sighting: capture
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = infer_launch(c, A, B, n, layout, trans, rot, poseA, poseB, stream);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc != SE3TN_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return hipfail(e, "hipStreamEndCapture");
    const hipError_t e2 = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e2 != hipSuccess) { g.exec = nullptr; return hipfail(e2, "hipGraphInstantiate"); }
    g.plan = c->plan;
    HIPCHK(hipGraphLaunch(g.exec, st));
    return SE3TN_OK;
  }
  if (c->graphs.size() >= 16) {  // bounded cache: drop the oldest entry
    if (c->graphs.front().exec) (void)hipGraphExecDestroy(c->graphs.front().exec);
    c->graphs.erase(c->graphs.begin());
  }
  c->graphs.emplace_back();
  std::memcpy(&c->graphs.back().key, &key, sizeof(key));   // (as bytes, the zeroed padding included: that is how it is compared)
  return infer_launch(c, A, B, n, layout, trans, rot, poseA, poseB, stream);
}

// One forward pass as planned: the stem, the ten convs of conv_table() in order (a fused block takes its two rows in one launch
// sequence), the tail.  ip != nullptr: the mixed-model call -- image i reads its parameters ip->off[i] floats from W and composes its
// pose with ip->tn[i] / rn[i]; it is never profiled
static int run_plan(se3tn_ctx* c, const InferConfig& cfg, const InferPlan& p, const float* W, const ImgParams* ip, const float* A,
                    const float* B, float* trans, float* rot, const double* poseA, double* poseB, hipStream_t st) {
  const BlobLayout& L = c->L;
  const int n = cfg.n;
  const bool fast = cfg.prec == SE3TN_PREC_F16X3, keep = cfg.keep_intermediates != 0;  // fast: both the big-tile and the split-K kernels
  const bool named = c->prof && !ip;
  auto mark = [&](const char* name, bool is_conv) -> int { return ip ? 0 : prof_mark(c, st, name, is_conv); };
  c->last_fast = fast;
  c->written = 0;          // (until this sequence has been enqueued in full)
  if (p.stem == InferPlan::STEM_SMALL) {
    HIPCHK(launch_stem_pool_small_multi(A, B, W + L.stem_w, W + L.stem_b, c->pool.get(), n, ip ? ip->off : nullptr, st));
    HIPCHK((hipError_t)mark(stem_label(p, 0), false));
  } else {
    if (fast)
      HIPCHK(launch_stem(A, B, c->split_w.get() + c->SL.stem_ws, W + L.stem_b, c->split_w.get() + c->SL.stem_sc, c->stem.get(), n, st));
    else
      HIPCHK(launch_stem(A, B, W + L.stem_w, W + L.stem_b, nullptr, c->stem.get(), n, st));
    HIPCHK((hipError_t)mark(stem_label(p, 0), false));
    HIPCHK(launch_maxpool(c->stem.get(), c->pool.get(), n, fast ? 1 : 0, c->overflow.get(), st));
    HIPCHK((hipError_t)mark(stem_label(p, 1), false));
  }
  struct MarkCtx { se3tn_ctx* c; hipStream_t st; const char* name; };
  auto mark_fn = [](void* m_) -> int { MarkCtx* m = (MarkCtx*)m_; return prof_mark(m->c, m->st, m->name, true); };
  const ConvRow* rows = conv_table();
  for (int i = 0; i < NUM_CONV3; ++i) {
    const ConvRow& r = rows[i];
    const ConvStep& s = p.conv[i];
    const Conv3& sp = conv_specs()[r.id];
    const int blk = wino_block_of(r.id);
    const bool in_block = blk >= 0 && p.block[blk];
    const char* name = named ? intern_label(step_label(r, s, fast, in_block, blk == 1)) : r.name;
    hipError_t e;
    if (in_block) {   // rows i, i + 1: conv1's out-transform fused with conv2's in-transform, the heads' last one with the tail
      const ConvRow& r2 = rows[++i];
      WinoArgs w, w2;   // (w2: conv2's planes, scales and bias; its tensors follow from conv1's inside launch_wino_block)
      fill_wino_args(c, r, s.tile, n, W, fast, w);
      fill_wino_args(c, r2, s.tile, n, W, fast, w2);
      w.res_ld = w.in_ld; w.res_gs = w.in_gs;   // (conv2's residual is conv1's input)
      const TailArgs tl{W + L.fc_w, W + L.fc_b, c->logits.get(), c->fcpart.get(), trans, rot, poseA, poseB, cfg.tn, cfg.rn};
      // the kept head activation is float32 (in f16x3 mode head itself holds split rows)
      float* keep2 = (blk == 1 && keep) ? tensor_ptr(c, r2.out, fast) : nullptr;
      MarkCtx mc{c, st, name};
      e = launch_wino_block(w, s.gemm, w2.U, w2.uscale, w2.bias, const_cast<float*>(w.in), keep ? 1 : 0, keep2, blk == 1 ? &tl : nullptr, st, mark_fn, &mc);
      if (e != hipSuccess) return hipfail(e, r2.name);
      name = named ? intern_label(step_label(r2, p.conv[i], fast, true, blk == 1)) : r2.name;
    } else if (s.algo == ConvStep::WINO) {
      WinoArgs w;
      fill_wino_args(c, r, s.tile, n, W, false, w);
      e = launch_wino_conv(w, s.gemm, r.epi, st);
    } else if (s.algo == ConvStep::WINO64) {
      e = launch_wino64(tensor_ptr(c, r.in, fast), r.in.ld, r.in.gs, c->wino64_u[(int)r.id - (int)L64_1].get(), (long long)16 * sp.cin * sp.cout,
                        W + L.conv_b[r.id], sp.cout, tensor_ptr(c, r.res, fast), r.res.ld, r.res.gs, tensor_ptr(c, r.out, fast), r.out.ld,
                        r.out.gs, n, sp.groups, r.epi, st);
    } else {
      ConvArgs a;
      fill_conv_args(c, r, n, W, ip, fast, a);
      e = launch_conv3x3(a, s, sp.cin, sp.cout, r.stride, r.epi, st);
    }
    if (e != hipSuccess) return hipfail(e, r.name);
    if (int rc = mark(name, true)) return rc;
  }
  if (p.tail == InferPlan::TAIL_PARTS) {   // the slices of the last head conv go to the tail unreduced
    const int M = n * S4 * S4;
    HIPCHK(launch_tail_parts(c->part.get(), p.conv[LH2_2].slices, (size_t)2 * M * 512, M, W + L.conv_b[LH2_2], c->head.get(), 1024, W + L.fc_w, W + L.fc_b,
                             c->logits.get(), trans, rot, poseA, poseB, ip ? 0.0 : cfg.tn, ip ? 0.0 : cfg.rn, n, st, c->fcpart.get(), c->tail_arrive.get(),
                             ip ? nullptr : c->tail_flag, ip ? 0 : c->tail_seq, p.tail_ch, ip));
  } else if (p.tail == InferPlan::TAIL_PLAIN) {
    HIPCHK(launch_tail(tensor_ptr(c, rows[LH2_2].out, fast), W + L.fc_w, W + L.fc_b, c->logits.get(), trans, rot, poseA, poseB, cfg.tn, cfg.rn, n, st,
                       c->fcpart.get(), c->tail_arrive.get(), c->tail_flag, c->tail_seq));
  }
  if (const char* name = tail_label(p)) HIPCHK((hipError_t)mark(name, false));
  c->written = p.written;
  return SE3TN_OK;
}

static int infer_launch(se3tn_ctx* c, const float* A, const float* B, int n, int layout, float* trans, float* rot,
                        const double* poseA, double* poseB, void* stream) {
  if (!c || c->device < 0 || !A || !B) return fail(SE3TN_E_ARG, "se3tn_infer: bad argument");
  if (n < 1 || n > c->max_batch) return fail(SE3TN_E_ARG, "se3tn_infer: n outside [1, max_batch]");
  if (!c->blob) return fail(SE3TN_E_STATE, "se3tn_infer: weights not uploaded/bound");
  if ((poseA == nullptr) != (poseB == nullptr)) return fail(SE3TN_E_ARG, "se3tn_infer: poseA and poseB go together");
  if (layout != SE3TN_NCHW && layout != SE3TN_NHWC) return fail(SE3TN_E_ARG, "se3tn_infer: bad layout");
  hipStream_t st = (hipStream_t)stream;
  c->n_launch = 0;
  int slot = 0;
  if (c->prof) {
    slot = (int)(c->infer_count++ % c->slots);
    c->ev = c->evs[slot];
    HIPCHK(hipEventRecord(c->ev[0], st));
  }

  const int want_split = c->prec == SE3TN_PREC_F16X3 ? 1 : 0;
  if (A != c->inA.get() || B != c->inB.get()) {  // external tensors: copy into the zero-bordered input buffers
    if (A != c->inA.get()) {
      HIPCHK(launch_to_padded_input(A, c->inA.get(), n, layout == SE3TN_NCHW, want_split, c->overflow.get(), st));
      c->in_split[0] = want_split;
    }
    if (B != c->inB.get()) {
      HIPCHK(launch_to_padded_input(B, c->inB.get(), n, layout == SE3TN_NCHW, want_split, c->overflow.get(), st));
      c->in_split[1] = want_split;
    }
    HIPCHK((hipError_t)prof_mark(c, st, "to_padded_input", false));
    A = c->inA.get();
    B = c->inB.get();
  }
  if (c->in_split[0] != want_split || c->in_split[1] != want_split)
    return fail(SE3TN_E_STATE, "se3tn_infer: the input buffers were filled under a different precision mode "
                               "(call se3tn_set_precision before se3tn_preprocess)");
  InferConfig cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  fill_config(c, n, false, cfg);
  if (plan_infer(cfg, c->plan) != INFER_PLAN_OK)
    return fail(SE3TN_E_STATE, "se3tn_infer: f16x3 split panels not derived (se3tn_set_precision after the weights are bound)");
  if (int rc = run_plan(c, cfg, c->plan, c->blob, nullptr, A, B, trans, rot, poseA, poseB, st)) return rc;
  if (c->prof) c->slot_launches[slot] = c->n_launch;
  return SE3TN_OK;
}

int se3tn_get_feature(se3tn_ctx* c, int n, float* feature_nchw, void* stream) {
  if (!c || c->device < 0 || !feature_nchw || n < 1 || n > c->max_batch) return fail(SE3TN_E_ARG, "se3tn_get_feature: bad argument");
  HIPCHK(launch_padded_nhwc_to_nchw(c->ab.get(), feature_nchw, n, S3, S3, 256, c->last_fast ? 1 : 0, (hipStream_t)stream));
  return SE3TN_OK;
}

const float* se3tn_logits(se3tn_ctx* c) { return c ? c->logits.get() : nullptr; }

int se3tn_debug_buffer(se3tn_ctx* c, const char* name, const float** ptr, int32_t dims[3]) {
  if (!c || !name || !ptr || !dims) return fail(SE3TN_E_ARG, "se3tn_debug_buffer: bad argument");
  struct { const char* n; const float* p; int h, w, ch; unsigned stage; } t[] = {   // (stage 0: the inputs, whoever filled them)
      {"inA", c->inA.get(), IN_P, IN_P, 4, 0},    {"inB", c->inB.get(), IN_P, IN_P, 4, 0},     {"stem", c->stem.get(), S1, S1, 128, STAGE_STEM},
      {"pool", c->pool.get(), S2 + 2, S2 + 2, 128, STAGE_POOL},    {"t64", c->t64.get(), S2 + 2, S2 + 2, 128, STAGE_T64},
      {"q64", c->q64.get(), S2 + 2, S2 + 2, 128, STAGE_Q64},       {"ab", c->ab.get(), S3 + 2, S3 + 2, 256, STAGE_AB},
      {"ab_t", c->ab_t.get(), S3 + 2, S3 + 2, 256, STAGE_AB_T},    {"head", c->last_fast ? c->head_f.get() : c->head.get(), S4 + 2, S4 + 2, 1024, STAGE_HEAD},
      {"head_t", c->head_t.get(), S4 + 2, S4 + 2, 1024, STAGE_HEAD_T}};
  for (auto& e : t)
    if (std::strcmp(e.n, name) == 0) {
      if (e.stage && !(c->written & e.stage))
        return fail(SE3TN_E_STATE, std::string("se3tn_debug_buffer: \"") + name + "\" was not written by the last se3tn_infer (its route keeps "
                                   "that stage on chip or never forms it; se3tn_keep_intermediates makes it written)");
      *ptr = e.p; dims[0] = e.h; dims[1] = e.w; dims[2] = e.ch;
      return SE3TN_OK;
    }
  return fail(SE3TN_E_KEY, std::string("unknown buffer ") + name);
}

// ---- rasteriser: replaces VispyRenderer (vispy_renderer.py:47-178) on the per-frame path ---------
int se3tn_mesh_create(se3tn_ctx* c, const float* verts, const float* normals, const float* colors01, int V,
                      const int32_t* faces, int F, se3tn_mesh** out) {
  if (!c || c->device < 0 || !verts || !normals || !colors01 || !faces || V < 3 || F < 1 || !out)
    return fail(SE3TN_E_ARG, "se3tn_mesh_create: bad argument");
  for (int i = 0; i < 3 * F; ++i)
    if (faces[i] < 0 || faces[i] >= V) return fail(SE3TN_E_ARG, "se3tn_mesh_create: face index out of range");
  se3tn_mesh* m = new se3tn_mesh();
  m->V = V; m->F = F;
  struct { DeviceBuf<float>* p; const float* src; } up[] = {{&m->verts, verts}, {&m->normals, normals}, {&m->colors, colors01}};
  hipError_t e = hipSuccess;
  for (auto& u : up) {
    if (e == hipSuccess) e = u.p->alloc((size_t)3 * V);
    if (e == hipSuccess) e = hipMemcpy(u.p->get(), u.src, sizeof(float) * 3 * V, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = m->faces.alloc((size_t)3 * F);
  if (e == hipSuccess) e = hipMemcpy(m->faces.get(), faces, sizeof(int) * 3 * F, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = m->scratch.alloc(V, F, 1);
  if (e != hipSuccess) { delete m; return hipfail(e, "se3tn_mesh_create"); }
  *out = m;
  return SE3TN_OK;
}

int se3tn_mesh_set_texture(se3tn_mesh* m, const float* uv, const uint8_t* rgb, int tw, int th, const float kd[3]) {
  if (!m || (rgb && (!uv || tw < 1 || th < 1))) return fail(SE3TN_E_ARG, "se3tn_mesh_set_texture: bad argument");
  if (kd) { m->kd[0] = kd[0]; m->kd[1] = kd[1]; m->kd[2] = kd[2]; }
  if (m->uv || m->tex) (void)hipDeviceSynchronize();   // a render may still be reading the old material
  m->uv.reset();
  m->tex.reset();
  m->tlevels = 0;
  m->has_material = true;
  if (!rgb) return SE3TN_OK;
  // mip pyramid: 2x2 box filter per level, levels back to back (tex_pyramid.h)
  std::vector<uint8_t> pyr;
  const int levels = se3tn_build_mip_pyramid(rgb, tw, th, pyr, m->tex_off);
  // both buffers exist and are filled before either is published: the resolve kernel reads uv whenever tex is set
  DeviceBuf<uint8_t> d_tex;
  DeviceBuf<float> d_uv;
  hipError_t e = d_tex.alloc(pyr.size());
  if (e == hipSuccess) e = hipMemcpy(d_tex.get(), pyr.data(), pyr.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = d_uv.alloc((size_t)2 * m->V);
  if (e == hipSuccess) e = hipMemcpy(d_uv.get(), uv, sizeof(float) * 2 * m->V, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hipfail(e, "se3tn_mesh_set_texture");
  m->tex = std::move(d_tex); m->uv = std::move(d_uv);
  m->tw = tw; m->th = th; m->tlevels = levels;
  return SE3TN_OK;
}

void se3tn_mesh_destroy(se3tn_mesh* m) { delete m; }

// what both renderers share
static void raster_common(RasterArgs& a, se3tn_ctx* c, se3tn_mesh* m, uint8_t* rgb, uint16_t* depth) {
  a.verts = m->verts.get(); a.normals = m->normals.get(); a.colors = m->colors.get(); a.faces = m->faces.get();
  raster_scratch(a, m->scratch);
  a.zbuf = c->zbuf.get(); a.rgb = rgb; a.depth = depth; a.V = m->V; a.F = m->F;
  a.numpy_rule = c->offset_rule; a.sub_bits = c->raster_sub_bits;
}
// proj * view as the vertex shader evaluates it (vispy_renderer.py:92): per column of the result, products accumulated left to
// right in float32, never fused (volatile keeps the host compiler from contracting or re-associating)
static void raster_pv(RasterArgs& a, const float P[4][4], const float V[4][4]) {
  for (int j = 0; j < 4; ++j)
    for (int r = 0; r < 4; ++r) {
      volatile float acc = P[r][0] * V[0][j];
      for (int k = 1; k < 4; ++k) {
        volatile float prod = P[r][k] * V[k][j];
        acc = acc + prod;
      }
      a.PV[4 * r + j] = acc;
    }
}

int se3tn_set_raster_rule(se3tn_ctx* c, int sub_bits) {
  if (!c || (sub_bits != 4 && sub_bits != 8)) return fail(SE3TN_E_ARG, "se3tn_set_raster_rule: sub-pixel bits must be 4 or 8");
  c->raster_sub_bits = sub_bits;
  return SE3TN_OK;
}
int se3tn_get_raster_rule(const se3tn_ctx* c) { return c ? c->raster_sub_bits : -1; }

int se3tn_set_small_kernels(se3tn_ctx* c, int on) {
  if (!c) return fail(SE3TN_E_ARG, "null ctx");
  c->small_kernels = on != 0;
  return SE3TN_OK;
}
int se3tn_get_small_kernels(const se3tn_ctx* c) { return c ? (c->small_kernels ? 1 : 0) : -1; }

// The float32 uniforms of the reference's VispyRenderer for one pose / window: a.PV, a.light, a.dA, a.dB
// (false: singular pose)
static bool vispy_uniforms(RasterArgs& a, const double ob_in_cam[16], const double K[9], const int32_t window[4]) {
  // The float32 uniforms the reference uploads, formed as it forms them (float64 numpy, then the cast of the upload):
  // update_cam_mat (vispy_renderer.py:135-150): ortho (rounded to float32 FIRST, :146) . proj in float64 ...
  const double n = R_NEAR_D, f = R_FAR_D;
  const double left = window[0], top = window[1], right = window[2], bottom = window[3];
  const double o00 = (double)(float)(2.0 / (right - left)), o03 = (double)(float)(-(right + left) / (right - left));
  const double o11 = (double)(float)(2.0 / (top - bottom)), o13 = (double)(float)(-(top + bottom) / (top - bottom));
  const double o22 = (double)(float)(-2.0 / (f - n)), o23 = (double)(float)(-(f + n) / (f - n));
  double OP[4][4] = {{o00 * K[0], 0.0, o00 * -K[2] + o03 * -1.0, 0.0},
                     {0.0, o11 * K[4], o11 * -K[5] + o13 * -1.0, 0.0},
                     {0.0, 0.0, o22 * (n + f) + o23 * -1.0, o22 * (n * f)},
                     {0.0, 0.0, -1.0, 0.0}};
  a.dA = OP[2][2]; a.dB = OP[2][3];   // projection_matrix[2,2], [3,2] of the stored TRANSPOSE (:149, :163-164)
  // ... view = ob2cam_gl = inv(glcam_in_cvcam) . ob_in_cam = diag(1,-1,-1,1) . ob_in_cam (predict.py:202-207), exact in float64
  float P32[4][4], V32[4][4];
  const double sgn[4] = {1.0, -1.0, -1.0, 1.0};
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      P32[r][q] = (float)OP[r][q];
      V32[r][q] = (float)(sgn[r] * ob_in_cam[4 * r + q]);
    }
  raster_pv(a, P32, V32);
  // light_direction = (inv(ob2cam_gl^T) . [0, 0.1, -0.9, 1])[:3] (vispy_renderer.py:172) in float64.  With G = [R' t'; 0 1]:
  // inv(G^T) = [inv(R'^T) 0; * 1], so the first three components are inv(R')^T . (0, 0.1, -0.9) -- a true inverse (adjugate /
  // determinant), not R' itself: poses composed over many frames are orthonormal only to float32 rounding.
  double R[3][3], adjT[3][3];
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) R[r][q] = sgn[r] * ob_in_cam[4 * r + q];
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) {   // cofactor (r, q) = entry (r, q) of adj(R)^T = det(R) inv(R)^T
      const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, q1 = (q + 1) % 3, q2 = (q + 2) % 3;
      adjT[r][q] = R[r1][q1] * R[r2][q2] - R[r1][q2] * R[r2][q1];
    }
  const double det = R[0][0] * adjT[0][0] + R[0][1] * adjT[0][1] + R[0][2] * adjT[0][2];
  if (det == 0.0) return false;
  const double l[3] = {0.0, 0.1, -0.9};
  for (int r = 0; r < 3; ++r) a.light[r] = (float)((adjT[r][0] * l[0] + adjT[r][1] * l[1] + adjT[r][2] * l[2]) / det);
  return true;
}

int se3tn_render(se3tn_ctx* c, se3tn_mesh* m, const double ob_in_cam[16], const double K[9], const int32_t window[4],
                 uint8_t* rgb, uint16_t* depth, void* stream) {
  if (!c || c->device < 0 || !m || !ob_in_cam || !K || !window || !rgb || !depth)
    return fail(SE3TN_E_ARG, "se3tn_render: bad argument");
  if (window[2] <= window[0] || window[3] <= window[1]) return fail(SE3TN_E_ARG, "se3tn_render: empty window");
  RasterArgs a{};
  raster_common(a, c, m, rgb, depth);
  a.rw = RES; a.rh = RES; a.mode = 0;
  if (!vispy_uniforms(a, ob_in_cam, K, window)) return fail(SE3TN_E_ARG, "se3tn_render: singular pose");
  HIPCHK(launch_raster(a, (hipStream_t)stream));
  return SE3TN_OK;
}

// ---- the pyrender-style renderer (offscreen_renderer.py:48-83): full frame, or a rectangle of it -------------------------------
// material and the projection of mode 1: pyrender's IntrinsicsCamera at W x H (GL clip space, y up) times cvcam_in_glcam . ob_in_cam,
// formed in float64 and uploaded as ONE float32 matrix; the vertex shader multiplies it with the position
static void frame_uniforms(RasterArgs& a, const se3tn_mesh* m, const double ob_in_cam[16], const double K[9], int W, int H) {
  a.rw = W; a.rh = H; a.mode = 1;
  a.uv = m->uv.get(); a.tex = m->tex.get(); a.tw = m->tw; a.th = m->th; a.tlevels = m->tlevels;
  for (int i = 0; i < 16; ++i) a.tex_off[i] = m->tex_off[i];
  a.kd[0] = m->kd[0]; a.kd[1] = m->kd[1]; a.kd[2] = m->kd[2];
  const double n = R_NEAR_D, f = R_FAR_D;
  double P[4][4] = {{2.0 * K[0] / W, 0.0, 1.0 - 2.0 * K[2] / W, 0.0},
                    {0.0, 2.0 * K[4] / H, 2.0 * K[5] / H - 1.0, 0.0},
                    {0.0, 0.0, (f + n) / (n - f), 2.0 * f * n / (n - f)},
                    {0.0, 0.0, -1.0, 0.0}};
  const double sgn[4] = {1.0, -1.0, -1.0, 1.0};
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      double acc = 0.0;
      for (int k = 0; k < 4; ++k) acc += P[r][k] * (sgn[k] * ob_in_cam[4 * k + q]);
      a.PV[4 * r + q] = (float)acc;
    }
}
// rect = {x0, y0, x1, y1} in OpenCV image coordinates -> the scissor in GL window coordinates (row 0 at the bottom)
static void rect_to_scissor(const int32_t rect[4], int H, int s[4]) {
  s[0] = rect[0]; s[1] = H - rect[3]; s[2] = rect[2]; s[3] = H - rect[1];
}
// sub-images and z-buffers of the SE3TN_ROUTE_FRAME calls for `px` pixels in all (never inside a capture: the callers are synchronous)
static int reserve_frame_route(se3tn_ctx* c, size_t px) {
  if (px <= c->fr_px) return SE3TN_OK;
  DeviceGuard dg(c->device);
  if (int rc = begin_growth(dg)) return rc;
  c->fr_px = 0;
  HIPCHK(c->fr_sub.alloc(64 + ((px * 3 + 63) & ~(size_t)63) + px * 2 + 64));
  HIPCHK(c->fr_zbuf.alloc(px));
  HIPCHK(hipMemset(c->fr_sub.get(), 0, 64));
  c->fr_px = px;
  return SE3TN_OK;
}

int se3tn_mesh_set_route(se3tn_mesh* m, int route) {
  if (!m || (route != SE3TN_ROUTE_WINDOW && route != SE3TN_ROUTE_FRAME)) return fail(SE3TN_E_ARG, "se3tn_mesh_set_route: bad argument");
  m->route = route;
  return SE3TN_OK;
}
int se3tn_mesh_get_route(const se3tn_mesh* m) { return m ? m->route : -1; }

int se3tn_render_frame_rect(se3tn_ctx* c, se3tn_mesh* m, const double ob_in_cam[16], const double K[9], int W, int H, const int32_t rect[4],
                            uint8_t* rgb_sub, uint16_t* depth_sub, void* stream) {
  if (!c || c->device < 0 || !m || !ob_in_cam || !K || !rect || !rgb_sub || !depth_sub || W < 1 || H < 1)
    return fail(SE3TN_E_ARG, "se3tn_render_frame_rect: bad argument");
  if (H > 2048) return fail(SE3TN_E_ARG, "se3tn_render_frame_rect: frames of more than 2048 rows are not supported");
  if (rect[2] <= rect[0] || rect[3] <= rect[1]) return fail(SE3TN_E_ARG, "se3tn_render_frame_rect: empty rectangle");
  if (rect[0] < 0 || rect[1] < 0 || rect[2] > W || rect[3] > H) return fail(SE3TN_E_ARG, "se3tn_render_frame_rect: rectangle outside the frame");
  const size_t px = (size_t)(rect[2] - rect[0]) * (size_t)(rect[3] - rect[1]);
  if (int rc = grow_now_or_refuse(c, "se3tn_render_frame_rect", false, "rectangle", px, stream)) return rc;
  RasterArgs a{};
  raster_common(a, c, m, rgb_sub, depth_sub);
  frame_uniforms(a, m, ob_in_cam, K, W, H);
  int s[4];
  rect_to_scissor(rect, H, s);
  a.scissor = 1; a.sx0 = s[0]; a.sy0 = s[1]; a.sx1 = s[2]; a.sy1 = s[3]; a.spx = (int)px;
  HIPCHK(launch_raster(a, (hipStream_t)stream));
  return SE3TN_OK;
}

static int fill_depth_rect_enqueue(se3tn_ctx* c, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate, int blur,
                                   const int32_t comp[4], uint16_t* out_full, const int32_t sub[4], uint16_t* out_sub, hipStream_t st);
static int fill_depth_rects_enqueue(se3tn_ctx* c, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate, int blur,
                                    int n, const int32_t* rects, const size_t* offs, uint16_t* out_base, uint16_t* out_full, hipStream_t st);

// the live camera's part of se3tn_on_track_live and se3tn_on_track_objects_live: `rgb` / `depth` of on_track_frame / on_track_objects_frame
// are then the camera's colour frame in color_order and its RAW depth frame, filled on the device (predict_ros.py:38-46)
struct LiveFrame {
  int color_order;
  double max_depth_m;
  int extrapolate, blur;
  uint16_t* depth_filled;   // device [H,W] or nullptr
};

// From the upload of a staged (pinned) buffer on, that buffer is travelling: the next call would overwrite it under the copy, so every
// error return synchronises the copy stream first.  One of these per body, armed at the upload; done() once the launch stream (which
// waits for the copy) has been waited for
struct StagedUpload {
  hipStream_t copy;
  ~StagedUpload() { if (copy) (void)hipStreamSynchronize(copy); }
  void done() { copy = nullptr; }
};
static int upload_staged(se3tn_ctx* c, uint8_t* dev, const uint8_t* host, size_t bytes, hipStream_t st);
// the copy stream of upload_staged and its event, made by the first tracking call (under that call's DeviceGuard)
static int copy_stream(se3tn_ctx* c) {
  if (!c->trk_copy_stream) HIPCHK(hipStreamCreateWithFlags(&c->trk_copy_stream, hipStreamNonBlocking));
  if (!c->trk_copy_event) HIPCHK(hipEventCreateWithFlags(&c->trk_copy_event, hipEventDisableTiming));
  return SE3TN_OK;
}
static int fit_check_stage(se3tn_ctx* c, int n, const se3tn_mesh* const* meshes, const double* est, const double K[9], int H, int W,
                           const se3tn::TrackWindow* windows, bool frame_route, const uint8_t* b_base, hipStream_t st, const std::string& who);

// se3tn_on_track (live == nullptr) and se3tn_on_track_live: one body, two staging steps
static int on_track_frame(se3tn_ctx* c, se3tn_mesh* m, const double prev_pose[16], const double K[9], double object_width_mm,
                          const uint8_t* rgb, const uint16_t* depth, int H, int W, const LiveFrame* live, uint8_t* rgbA_dev,
                          uint16_t* depthA_dev, double pose_out[16], float trans_out[3], float rot_out[3], int32_t bbox_vu[8], void* stream) {
  const char* who = live ? "se3tn_on_track_live" : "se3tn_on_track";
  if (!c || c->device < 0 || !m || !prev_pose || !K || !rgb || !depth || H < 1 || W < 1 || !pose_out || !(object_width_mm > 0))
    return fail(SE3TN_E_ARG, std::string(who) + ": bad argument");
  if (live && ((unsigned)live->color_order > 1u || (unsigned)live->blur > 2u))
    return fail(SE3TN_E_ARG, "se3tn_on_track_live: bad color_order or blur");
  if (!c->have_norm) return fail(SE3TN_E_STATE, std::string(who) + ": call se3tn_set_normalization first");
  hipStream_t st = (hipStream_t)stream;
  if (live && stream_is_capturing(st)) return fail(SE3TN_E_STATE, "se3tn_on_track_live: the call is synchronous, it cannot be captured");
  c->fit_last_n = 0;
  if (c->fit_tol && stream_is_capturing(st)) return fail(SE3TN_E_STATE, std::string(who) + ": the fit check waits for the stream, it cannot be captured");
  static const bool trace = std::getenv("SE3TN_TRACK_TRACE") != nullptr;   // developer switch: host-side timeline of the call
  static double acc_both[2][7] = {{0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}};
  static int ncall_both[2] = {0, 0};
  double* acc = acc_both[live ? 1 : 0];
  int& ncall = ncall_both[live ? 1 : 0];
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = trace ? now() : 0.0;
  auto a64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
  const size_t fpx = (size_t)H * W;
  // start-up allocations (first call / larger frame): pinned staging for a whole frame, its device mirror, outputs
  // (live: pose | window rgb | one zero pixel | RAW depth frame | the window's filled depth, written on the device)
  const size_t need = live ? 256 + a64(fpx * 3) + 64 + a64(fpx * 2) + fpx * 2 + 64 : 256 + fpx * 5 + 64;
  if (live)
    if (int rc = reserve_fill_depth(c, fpx)) return rc;
  if (need > c->trk_bytes) {   //  staging buffers belong to the context's device, whatever the caller's current one
    DeviceGuard dg(c->device);
    if (int rc = begin_growth(dg)) return rc;
    c->trk_bytes = 0;
    HIPCHK(c->trk_host.alloc(need));
    HIPCHK(c->trk_dev.alloc(need));
    c->trk_bytes = need;
  }
  if (!c->trk_depthA) {   // (the first call; trk_depthA is made last, so a first call that failed half-way is made up for by the next)
    DeviceGuard dg(c->device);
    if (int rc = begin_growth(dg)) return rc;
    if (int rc = copy_stream(c)) return rc;
    // pose | trans | rot | completion word in MAPPED pinned host memory: the tail kernel writes them across the bus itself and the
    // host polls the word -- no device-to-host copy, no stream wake-up on the per-frame critical path
    HIPCHK(c->trk_out.alloc(256, true, true));
    HIPCHK(c->trk_rgbA.alloc((size_t)RES * RES * 3));
    HIPCHK(c->trk_depthA.alloc((size_t)RES * RES));
  }
  // the windows of the pair and the part of the frame that travels (track_plan.h; host float64, round half to even), behind the pose
  TrackWindow w;
  size_t planned = 256;
  const PlanStatus ps = plan_window(prev_pose, K, object_width_mm, H, W, planned, w);
  if (ps == PlanStatus::NOT_IN_FRONT) return fail(SE3TN_E_ARG, std::string(who) + ": pose is not in front of the camera (z <= 0 or not finite)");
  if (ps == PlanStatus::EMPTY_WINDOW) return fail(SE3TN_E_ARG, std::string(who) + ": empty crop window (pose behind the camera?)");
  // image A first: its four launches run on the device while the host stages the frame
  uint8_t* rA = rgbA_dev ? rgbA_dev : c->trk_rgbA.get();
  uint16_t* dA = depthA_dev ? depthA_dev : c->trk_depthA.get();
  const bool frame_route = m->route == SE3TN_ROUTE_FRAME;
  size_t subA_d_off = 0;   // frame route: offset of the sub-image's depth in c->fr_sub
  if (frame_route) {
    // predict.py:209-213: the full-frame render cropped with the SAME window as the camera frame -- only the rectangle of the frame
    // the window covers is rendered (every byte of it as se3tn_render_frame gives it)
    if (H > 2048) return fail(SE3TN_E_ARG, std::string(who) + ": frames of more than 2048 rows are not supported on SE3TN_ROUTE_FRAME");
    if (int rc = reserve_frame_route(c, (size_t)H * W)) return rc;
    if (!w.miss) {
      const size_t px = (size_t)w.sw * w.sh;
      subA_d_off = 64 + a64(px * 3);
      RasterArgs ra{};
      raster_common(ra, c, m, c->fr_sub.get() + 64, (uint16_t*)(c->fr_sub.get() + subA_d_off));
      ra.zbuf = c->fr_zbuf.get();
      frame_uniforms(ra, m, prev_pose, K, W, H);
      const int32_t rectA[4] = {w.x0, w.y0, w.x0 + w.sw, w.y0 + w.sh};
      int s[4];
      rect_to_scissor(rectA, H, s);
      ra.scissor = 1; ra.sx0 = s[0]; ra.sy0 = s[1]; ra.sx1 = s[2]; ra.sy1 = s[3]; ra.spx = (int)px;
      HIPCHK(launch_raster(ra, st));
    }
  } else if (int rc = se3tn_render(c, m, prev_pose, K, w.winA, rA, dA, stream)) {
    return rc;
  }
  const double t1 = trace ? now() : 0.0;
  // only the part of the frame the window covers travels: rows / columns [y0, y1) x [x0, x1) into pinned memory, ONE copy
  // with the pose in front, on a copy stream of its own (beside the rasteriser, not behind it)
  uint8_t* hp = c->trk_host.get();
  std::memcpy(hp, prev_pose, 128);
  size_t bytes, raw_off = 0;
  const bool fill = live && (!w.miss || live->depth_filled);
  if (live) {
    // window rgb with the channel order made RGB on the way | one zero pixel (a window that misses the frame) | the WHOLE raw depth frame;
    // the window's filled depth is written behind it by the rectangle pass below
    const size_t z_off = w.off_d;
    raw_off = z_off + 64;
    stage_window(w, rgb, nullptr, W, hp, live->color_order == SE3TN_COLOR_BGR);
    std::memset(hp + z_off, 0, 2);
    if (fill) std::memcpy(hp + raw_off, depth, fpx * 2);
    bytes = fill ? raw_off + fpx * 2 : raw_off;
    w.off_d = w.miss ? z_off : a64(raw_off + fpx * 2);   // image B's depth on the device
  } else {
    stage_window(w, rgb, depth, W, hp);
    bytes = w.off_d + (size_t)w.sw * w.sh * 2;
  }
  StagedUpload up{c->trk_copy_stream};
  if (int rc = upload_staged(c, c->trk_dev.get(), hp, bytes, st)) return rc;
  const double t2 = trace ? now() : 0.0;
  if (fill) {   // predict_ros.py:38-41 for the pixels the crop reads (the whole frame when the caller wants it)
    const int32_t whole[4] = {0, 0, W, H}, sub[4] = {w.x0, w.y0, w.x0 + w.sw, w.y0 + w.sh};
    const int rc = fill_depth_rect_enqueue(c, (const uint16_t*)(c->trk_dev.get() + raw_off), H, W, live->max_depth_m,
                                           live->extrapolate, live->blur, live->depth_filled ? whole : sub, live->depth_filled, sub,
                                           w.miss ? nullptr : (uint16_t*)(c->trk_dev.get() + w.off_d), st);
    if (rc) return rc;
  }
  const double t2f = trace ? now() : 0.0;
  // image A and image B in ONE preprocess launch (data_augmentation.py:124-189 for both, with poseA's z)
  CropArgs a;
  std::memcpy(a.mean, c->mean, sizeof(a.mean));
  std::memcpy(a.stdv, c->stdv, sizeof(a.stdv));
  // frame route: image A = the rendered rectangle (a window that misses the frame: the 1 x 1 zero image in front of the buffer); the same
  // launch writes its raw crop = Tracker.render_window (the one not given goes to the internal buffer)
  const ImageA imgA = frame_route ? ImageA{c->fr_sub.get() + 64, (const uint16_t*)(c->fr_sub.get() + subA_d_off), c->fr_sub.get()} : ImageA{rA, dA, nullptr};
  crop_pair(w, prev_pose[11] * 1000, imgA, c->trk_dev.get(), a.c[0], a.c[1]);
  if (frame_route && (rgbA_dev || depthA_dev)) { a.raw_rgb = rA; a.raw_depth = dA; }
  a.n = 2; a.n_first = 1; a.out = c->inA.get(); a.out2 = c->inB.get(); a.padded = 1;
  a.split = c->prec == SE3TN_PREC_F16X3 ? 1 : 0;
  a.overflow = c->overflow.get(); a.offset_rule = c->offset_rule;
  c->in_split[0] = c->in_split[1] = a.split;
  if (const hipError_t e = launch_preprocess(a, st)) return hipfail(e, "launch_preprocess");
  const double t3 = trace ? now() : 0.0;
  float* trans_d = (float*)(c->trk_out.dev() + 128);
  float* rot_d = (float*)(c->trk_out.dev() + 144);
  int* flag_d = (int*)(c->trk_out.dev() + 192);
  volatile int* flag_h = (volatile int*)(c->trk_out.get() + 192);
  const bool poll = !c->use_graphs && !c->prof;   // (a captured graph would replay a stale sequence number)
  const int seq = ++c->tail_seq == 0 ? ++c->tail_seq : c->tail_seq;
  c->tail_flag = poll ? flag_d : nullptr;
  const int rc_inf = se3tn_infer(c, c->inA.get(), c->inB.get(), 1, SE3TN_NHWC, trans_d, rot_d, (const double*)c->trk_dev.get(), (double*)c->trk_out.dev(), stream);
  // only launch_tail / launch_tail_parts take the word: the fused heads' tail (TailArgs) never stores it, and polling for it would spin
  // for the whole 5 ms before the stream wait
  const bool stored = poll && rc_inf == SE3TN_OK && c->plan.tail_stores_word;
  c->tail_flag = nullptr;
  if (rc_inf) return rc_inf;
  const double t4 = trace ? now() : 0.0;
  bool seen = false;
  if (stored) {   // 5 ms of polling covers every healthy frame; anything slower (or a fault) falls through to the stream wait
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(5);
    for (;;) {
      for (int it = 0; it < 256 && !seen; ++it) seen = __atomic_load_n((const int*)flag_h, __ATOMIC_ACQUIRE) == seq;
      if (seen || std::chrono::steady_clock::now() > t_end) break;
    }
  }
  if (!seen) HIPCHK(hipStreamSynchronize(st));
  up.done();
  if (trace) {
    const double t5 = now();
    const double d[7] = {t1 - t0, t2 - t1, t3 - t2f, t4 - t3, t5 - t4, t5 - t0, t2f - t2};
    for (int i = 0; i < 7; ++i) acc[i] += d[i];
    if (++ncall % 200 == 0) {
      if (live)
        std::fprintf(stderr, "se3tn_on_track_live host timeline (mean of 200, us): bbox+render enqueue %.1f | stage+H2D enqueue %.1f | fill enqueue %.1f | "
                     "preprocess enqueue %.1f | infer enqueue %.1f | wait for the tail's word %.1f | total %.1f\n", acc[0] / 200, acc[1] / 200,
                     acc[6] / 200, acc[2] / 200, acc[3] / 200, acc[4] / 200, acc[5] / 200);
      else
        std::fprintf(stderr, "se3tn_on_track host timeline (mean of 200, us): bbox+render enqueue %.1f | stage+H2D enqueue %.1f | preprocess enqueue %.1f | "
                     "infer enqueue %.1f | wait for the tail's word %.1f | total %.1f\n", acc[0] / 200, acc[1] / 200, acc[2] / 200, acc[3] / 200, acc[4] / 200, acc[5] / 200);
      for (int i = 0; i < 7; ++i) acc[i] = 0;
    }
  }
  std::memcpy(pose_out, c->trk_out.get(), 128);
  if (trans_out) std::memcpy(trans_out, c->trk_out.get() + 128, 12);
  if (rot_out) std::memcpy(rot_out, c->trk_out.get() + 144, 12);
  if (bbox_vu) std::memcpy(bbox_vu, w.vu, sizeof(w.vu));
  if (c->fit_tol) {
    const se3tn_mesh* mm = m;
    return fit_check_stage(c, 1, &mm, pose_out, K, H, W, &w, frame_route, c->trk_dev.get(), st, who);
  }
  return SE3TN_OK;
}

int se3tn_on_track(se3tn_ctx* c, se3tn_mesh* m, const double prev_pose[16], const double K[9], double object_width_mm,
                   const uint8_t* rgb, const uint16_t* depth, int H, int W, uint8_t* rgbA_dev, uint16_t* depthA_dev,
                   double pose_out[16], float trans_out[3], float rot_out[3], int32_t bbox_vu[8], void* stream) {
  return on_track_frame(c, m, prev_pose, K, object_width_mm, rgb, depth, H, W, nullptr, rgbA_dev, depthA_dev, pose_out, trans_out, rot_out,
                        bbox_vu, stream);
}

int se3tn_on_track_live(se3tn_ctx* c, se3tn_mesh* m, const double prev_pose[16], const double K[9], double object_width_mm,
                        const uint8_t* color, int color_order, const uint16_t* depth_raw, int H, int W, double max_depth_m, int extrapolate,
                        int blur, uint16_t* depth_filled_dev, uint8_t* rgbA_dev, uint16_t* depthA_dev, double pose_out[16],
                        float trans_out[3], float rot_out[3], int32_t bbox_vu[8], void* stream) {
  const LiveFrame live{color_order, max_depth_m, extrapolate, blur, depth_filled_dev};
  return on_track_frame(c, m, prev_pose, K, object_width_mm, color, depth_raw, H, W, &live, rgbA_dev, depthA_dev, pose_out, trans_out,
                        rot_out, bbox_vu, stream);
}

// ---- n tracks per call -------------------------------------------------------------------------------------------------------
// start-up allocations of se3tn_on_track_batch (first call, a larger n, a larger mesh or frame)
// (m == nullptr: the context's part only -- se3tn_on_track_objects keeps the rasteriser scratch itself)
static int reserve_track_batch(se3tn_ctx* c, se3tn_mesh* m, int n, size_t stage_bytes) {
  if (n <= c->tb_cap && (!m || n <= m->batch_cap) && stage_bytes <= c->tb_stage_bytes) return SE3TN_OK;
  DeviceGuard dg(c->device);
  if (int rc = begin_growth(dg)) return rc;
  const int cap = n > c->max_batch ? n : c->max_batch;
  if (n > c->tb_cap) {
    c->tb_cap = 0;
    HIPCHK(c->tb_inst_host.alloc((sizeof(RasterInstance) + sizeof(RasterMaterial)) * cap));
    HIPCHK(c->tb_out_host.alloc((size_t)cap * 160));
    HIPCHK(c->tb_inst_dev.alloc((sizeof(RasterInstance) + sizeof(RasterMaterial)) * cap));
    HIPCHK(c->tb_zbuf.alloc((size_t)RES * RES * cap));
    HIPCHK(c->tb_rgbA.alloc((size_t)RES * RES * 3 * cap));
    HIPCHK(c->tb_depthA.alloc((size_t)RES * RES * cap));
    HIPCHK(c->tb_out_dev.alloc((size_t)cap * 160));
    c->tb_cap = cap;
  }
  if (m && n > m->batch_cap) {
    m->batch_cap = 0;
    HIPCHK(m->batch.alloc(m->V, m->F, cap));
    m->batch_cap = cap;
  }
  if (stage_bytes > c->tb_stage_bytes) {
    c->tb_stage_bytes = 0;
    HIPCHK(c->tb_stage_host.alloc(stage_bytes));
    HIPCHK(c->tb_stage_dev.alloc(stage_bytes));
    c->tb_stage_bytes = stage_bytes;
  }
  return copy_stream(c);
}

// SE3TN_ROUTE_FRAME (predict.py:209-213): per pair the rectangle of the full-frame render its crop window covers -- the same rectangle as
// the staged part of the camera frame.  Z-buffers and sub-images are sized by the largest rectangle of the call (maxpx; 0: every window
// misses the frame); fr_d_off: where the depth sub-images start in c->fr_sub
static int reserve_frame_rects(se3tn_ctx* c, int n, const TrackWindow* windows, int H, int W, size_t* maxpx, size_t* fr_d_off) {
  size_t mx = 0;
  for (int i = 0; i < n; ++i)
    if (!windows[i].miss) mx = std::max(mx, (size_t)windows[i].sw * (size_t)windows[i].sh);
  const size_t need = mx ? (size_t)n * mx : 1, cap = (size_t)n * H * W;
  // windows change from frame to frame: grow with half as much again in hand (never past n whole frames)
  if (need > c->fr_px)
    if (int rc = reserve_frame_route(c, std::max(need, std::min(need + need / 2, cap)))) return rc;
  *maxpx = mx;
  *fr_d_off = 64 + (((size_t)n * mx * 3 + 63) & ~(size_t)63);
  return SE3TN_OK;
}

// image A of pair i of n: its 176 x 176 render in the stack rA / dA, or (frame route) its rectangle in c->fr_sub
static ImageA image_a(const se3tn_ctx* c, bool frame_route, int i, const uint8_t* rA, const uint16_t* dA, size_t maxpx, size_t fr_d_off) {
  if (frame_route) return ImageA{c->fr_sub.get() + 64 + (size_t)i * maxpx * 3, (const uint16_t*)(c->fr_sub.get() + fr_d_off) + (size_t)i * maxpx, c->fr_sub.get()};
  return ImageA{rA + (size_t)i * RES * RES * 3, dA + (size_t)i * RES * RES, nullptr};
}

// One record of the rasteriser's instance table: the uniforms of `pose` and, on the frame route, the pair's rectangle as a scissor
// (mesh pointers and material: se3tn_on_track_objects adds them).  false: singular pose (window route)
static bool fill_instance(RasterInstance& I, bool frame_route, const se3tn_mesh* m, const double pose[16], const double K[9], int W, int H,
                          const TrackWindow& t) {
  RasterArgs one{};
  if (frame_route) {
    frame_uniforms(one, m, pose, K, W, H);
    const int32_t r[4] = {t.x0, t.y0, t.x0 + t.sw, t.y0 + t.sh};
    if (!t.miss) rect_to_scissor(r, H, I.rect);
    // the window misses the frame: an empty rectangle.  The instance still runs its vertex / triangle / queue workgroups (one grid
    // for all instances) and writes nothing: a few microseconds wasted on a case a tracker does not stay in
    else I.rect[0] = I.rect[1] = I.rect[2] = I.rect[3] = 0;
  } else if (!vispy_uniforms(one, pose, K, t.winA)) {
    return false;
  }
  std::memcpy(I.PV, one.PV, sizeof(I.PV));
  std::memcpy(I.light, one.light, sizeof(I.light));
  I._pad = 0.f; I.dA = one.dA; I.dB = one.dB;
  return true;
}

// the staged (pinned) buffer goes up in ONE copy on the copy stream (beside the rasteriser, not behind it); `st` waits for it
static int upload_staged(se3tn_ctx* c, uint8_t* dev, const uint8_t* host, size_t bytes, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->trk_copy_stream));
  HIPCHK(hipEventRecord(c->trk_copy_event, c->trk_copy_stream));
  HIPCHK(hipStreamWaitEvent(st, c->trk_copy_event, 0));
  return SE3TN_OK;
}

// [n poses | n trans | n rot] of c->tb_out_dev back to the caller (waits for `st`), and the bboxes of the windows
static int read_back_tracks(se3tn_ctx* c, int n, hipStream_t st, double* pose_out, float* trans_out, float* rot_out, int32_t* bbox_vu,
                            const TrackWindow* windows) {
  HIPCHK(hipMemcpyAsync(c->tb_out_host.get(), c->tb_out_dev.get(), (size_t)n * 152, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::memcpy(pose_out, c->tb_out_host.get(), (size_t)n * 128);
  if (trans_out) std::memcpy(trans_out, c->tb_out_host.get() + (size_t)n * 128, (size_t)n * 12);
  if (rot_out) std::memcpy(rot_out, c->tb_out_host.get() + (size_t)n * 140, (size_t)n * 12);
  if (bbox_vu)
    for (int i = 0; i < n; ++i) std::memcpy(bbox_vu + 8 * (size_t)i, windows[i].vu, sizeof(windows[i].vu));
  return SE3TN_OK;
}

// ---- the fit record ---------------------------------------------------------------------------------------------------------------
int se3tn_fit_stats(se3tn_ctx* c, const se3tn_crop* model, const se3tn_crop* observed, int n, int tol_mm, se3tn_fit* out_dev, void* stream) {
  if (int rc = crops_check("se3tn_fit_stats", c, model, observed, n, tol_mm, out_dev, false)) return rc;
  return fit_launches(c, n, [&](int j, se3tn_crop& m, se3tn_crop& o) { m = model[j]; o = observed[j]; }, out_dev, nullptr, tol_mm, nullptr, nullptr,
                      (hipStream_t)stream);
}

int se3tn_set_fit_check(se3tn_ctx* c, int tol_mm) {
  if (!c || tol_mm < 0 || tol_mm > 65535) return fail(SE3TN_E_ARG, "se3tn_set_fit_check: tol_mm must be 0 (off) or 1 .. 65535");
  c->fit_tol = tol_mm;
  return SE3TN_OK;
}
int se3tn_get_fit_check(const se3tn_ctx* c) { return c ? c->fit_tol : -1; }

int se3tn_last_fit(se3tn_ctx* c, int n, se3tn_fit* out_host) {
  if (!c || !out_host || n < 1) return fail(SE3TN_E_ARG, "se3tn_last_fit: bad argument");
  if (c->fit_last_n == 0) return fail(SE3TN_E_STATE, "se3tn_last_fit: the last tracking call of this context left no records (se3tn_set_fit_check off, or the call failed)");
  if (c->fit_last_n != n) return fail(SE3TN_E_STATE, "se3tn_last_fit: the last tracking call held " + std::to_string(c->fit_last_n) + " pairs, not " + std::to_string(n));
  std::memcpy(out_host, c->fit_host.get(), sizeof(se3tn_fit) * (size_t)n);
  return SE3TN_OK;
}

int se3tn_last_fit_images(se3tn_ctx* c, const uint8_t** rgb_dev, const uint16_t** depth_dev) {
  if (!c) return fail(SE3TN_E_ARG, "se3tn_last_fit_images: null ctx");
  if (c->fit_last_n == 0) return fail(SE3TN_E_STATE, "se3tn_last_fit_images: the last tracking call of this context left no estimate renders (se3tn_set_fit_check off, or the call failed)");
  if (rgb_dev) *rgb_dev = c->fit_rgb.get();
  if (depth_dev) *depth_dev = c->fit_depth.get();
  return SE3TN_OK;
}

// ---- the colour record --------------------------------------------------------------------------------------------------------------
int se3tn_color_stats(se3tn_ctx* c, const se3tn_crop* model, const se3tn_crop* observed, int n, int tol_mm, se3tn_fit* fit_out_dev,
                      se3tn_color_fit* out_dev, void* stream) {
  if (int rc = crops_check("se3tn_color_stats", c, model, observed, n, tol_mm, out_dev, true)) return rc;
  return fit_launches(c, n, [&](int j, se3tn_crop& m, se3tn_crop& o) { m = model[j]; o = observed[j]; }, fit_out_dev, out_dev, tol_mm, nullptr, nullptr,
                      (hipStream_t)stream);
}

// the operation order is the header's; utils.color_score states it again in NumPy
double se3tn_color_score(const se3tn_color_fit* r, int min_px, double per_channel[3]) {
  double z[3] = {0.0, 0.0, 0.0};
  if (r && (long long)r->px >= (long long)min_px) {
    const int64_t n = (int64_t)r->px;
    for (int ch = 0; ch < 3; ++ch) {
      const int64_t sm = r->sum_m[ch], so = r->sum_o[ch];
      const int64_t cov = n * (int64_t)r->sum_mo[ch] - sm * so;
      const int64_t vm = n * (int64_t)r->sum_mm[ch] - sm * sm;
      const int64_t vo = n * (int64_t)r->sum_oo[ch] - so * so;
      if (vm > 0 && vo > 0) z[ch] = (double)cov / (std::sqrt((double)vm) * std::sqrt((double)vo));
    }
  }
  if (per_channel) { per_channel[0] = z[0]; per_channel[1] = z[1]; per_channel[2] = z[2]; }
  return ((z[0] + z[1]) + z[2]) / 3.0;
}

// ---- ADD / ADD-S of n pose pairs ---------------------------------------------------------------------------------------------------
int se3tn_points_create(se3tn_ctx* c, const double* xyz, int P, se3tn_points** out) {
  if (!c || !xyz || !out) return fail(SE3TN_E_ARG, "se3tn_points_create: NULL argument");
  if (c->device < 0) return fail(SE3TN_E_ARG, "se3tn_points_create: host-only context (device = -1) has no device to hold the points");
  if (P < 1 || P > PE_MAX_POINTS)
    return fail(SE3TN_E_ARG, "se3tn_points_create: P = " + std::to_string(P) + " outside [1, SE3TN_POSE_ERRORS_MAX_POINTS = " +
                                 std::to_string(PE_MAX_POINTS) + "]");
  for (size_t i = 0; i < (size_t)3 * P; ++i)
    if (!std::isfinite(xyz[i])) return fail(SE3TN_E_ARG, "se3tn_points_create: coordinate " + std::to_string(i) + " is not finite");
  DeviceGuard dg(c->device);
  if (dg.err != hipSuccess) return hipfail(dg.err, "hipSetDevice");
  se3tn_points* p = new se3tn_points();
  p->device = c->device; p->P = P;
  hipError_t e = p->xyz.alloc((size_t)3 * P);
  if (e == hipSuccess) e = hipMemcpy(p->xyz.get(), xyz, sizeof(double) * 3 * (size_t)P, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = p->part.alloc(pe_scratch_doubles(P), true);
  if (e != hipSuccess) { delete p; return hipfail(e, "se3tn_points_create"); }
  *out = p;
  return SE3TN_OK;
}

void se3tn_points_destroy(se3tn_points* p) { delete p; }
int se3tn_points_count(const se3tn_points* p) { return p ? p->P : -1; }

int se3tn_points_set_normals(se3tn_points* p, const double* nxyz) {
  if (!p) return fail(SE3TN_E_ARG, "se3tn_points_set_normals: NULL points");
  if (!nxyz) { p->nrm.reset(); return SE3TN_OK; }
  for (size_t i = 0; i < (size_t)3 * p->P; ++i)
    if (!std::isfinite(nxyz[i])) return fail(SE3TN_E_ARG, "se3tn_points_set_normals: component " + std::to_string(i) + " is not finite");
  DeviceGuard dg(p->device);
  if (dg.err != hipSuccess) return hipfail(dg.err, "hipSetDevice");
  DeviceBuf<double> fresh;   // the handle keeps what it had unless the upload succeeds
  hipError_t e = fresh.alloc((size_t)3 * p->P);
  if (e == hipSuccess) e = hipMemcpy(fresh.get(), nxyz, sizeof(double) * 3 * (size_t)p->P, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hipfail(e, "se3tn_points_set_normals");
  p->nrm = std::move(fresh);
  return SE3TN_OK;
}
int se3tn_points_has_normals(const se3tn_points* p) { return p ? (p->nrm ? 1 : 0) : -1; }

// the chunks of one call, enqueued on st (both entry points)
static int pose_errors_enqueue(const se3tn_points* p, int n, const double* pred, const double* gt, double* add, double* adds, hipStream_t st) {
  for (int ch = 0, nch = pe_chunks(n); ch < nch; ++ch) {
    const PeChunk k = pe_chunk(n, ch);
    PoseErrArgs a;
    a.pts = p->xyz.get(); a.P = p->P;
    a.pred = pred + k.first * 16; a.gt = gt + k.first * 16;
    a.part = p->part.get();
    a.add = add ? add + k.first : nullptr;
    a.adds = adds ? adds + k.first : nullptr;
    HIPCHK(launch_pose_errors(a, k.count, st));
  }
  return SE3TN_OK;
}

static int pose_errors_check(const char* who, const se3tn_ctx* c, const se3tn_points* p, int n, const void* pred, const void* gt,
                             const void* add, const void* adds) {
  if (!c || c->device < 0 || !p) return fail(SE3TN_E_ARG, std::string(who) + ": NULL or host-only context, or NULL points");
  if (int rc = same_device_check(who, c, p)) return rc;
  if (n < 1) return fail(SE3TN_E_ARG, std::string(who) + ": n < 1");
  if (!pred || !gt) return fail(SE3TN_E_ARG, std::string(who) + ": NULL poses");
  if (!add && !adds) return fail(SE3TN_E_ARG, std::string(who) + ": both outputs NULL");
  return SE3TN_OK;
}

int se3tn_pose_errors(se3tn_ctx* c, const se3tn_points* p, int n, const double* pred_dev, const double* gt_dev, double* add_dev,
                      double* adds_dev, void* stream) {
  if (int rc = pose_errors_check("se3tn_pose_errors", c, p, n, pred_dev, gt_dev, add_dev, adds_dev)) return rc;
  return pose_errors_enqueue(p, n, pred_dev, gt_dev, add_dev, adds_dev, (hipStream_t)stream);
}

int se3tn_pose_errors_host(se3tn_ctx* c, const se3tn_points* p, int n, const double* pred, const double* gt, double* add_out,
                           double* adds_out, void* stream) {
  const char* who = "se3tn_pose_errors_host";
  if (int rc = pose_errors_check(who, c, p, n, pred, gt, add_out, adds_out)) return rc;
  StagedCall sc{c, who, (hipStream_t)stream};
  if (int rc = sc.refuse_capture()) return rc;
  if (int rc = finite_check(who, "pose", pred, gt, (size_t)n, 16, 16)) return rc;
  if (int rc = sc.grow(sizeof(double) * pe_stage_doubles(n))) return rc;
  // pe_stage_*, in doubles: poses and results are each one contiguous run
  double* h = reinterpret_cast<double*>(sc.h);
  double* d = sc.dev<double>(0);
  std::memcpy(h, pred, sizeof(double) * 16 * (size_t)n);
  std::memcpy(h + pe_stage_gt(n), gt, sizeof(double) * 16 * (size_t)n);
  if (int rc = sc.upload(sizeof(double) * pe_stage_add(n))) return rc;
  if (int rc = pose_errors_enqueue(p, n, d, d + pe_stage_gt(n), add_out ? d + pe_stage_add(n) : nullptr,
                                   adds_out ? d + pe_stage_adds(n) : nullptr, sc.st))
    return rc;
  // one read-back: [add | adds], or the one that was asked for
  const size_t r0 = add_out ? pe_stage_add(n) : pe_stage_adds(n);
  const size_t rn = (size_t)n * ((add_out ? 1 : 0) + (adds_out ? 1 : 0));
  if (int rc = sc.finish(sizeof(double) * r0, sizeof(double) * rn)) return rc;
  if (add_out) std::memcpy(add_out, h + pe_stage_add(n), sizeof(double) * (size_t)n);
  if (adds_out) std::memcpy(adds_out, h + pe_stage_adds(n), sizeof(double) * (size_t)n);
  return SE3TN_OK;
}

// ---- n candidate poses against one depth frame, the best k ----------------------------------------------------------------------------
// NULL pointers and a host-only context first (ok_ptrs: every pointer of the call), then the numbers
static int pose_search_check(const char* who, const se3tn_ctx* c, bool ok_ptrs, const se3tn_points* p, bool with_points, int n) {
  if (!c || !ok_ptrs || (with_points && !p)) return null_argument(who);
  if (int rc = device_check(who, c, "search")) return rc;
  if (with_points)
    if (int rc = same_device_check(who, c, p)) return rc;
  return count_check(who, n, PS_MAX_POSES, "SE3TN_POSE_SEARCH_MAX_POSES");
}
static int pose_score_check(const char* who, int H, int W, int tol_mm) {
  if (int rc = mm_check(who, "tol_mm", tol_mm)) return rc;
  return frame_check(who, H, W);
}
static int pose_rank_check(const char* who, int n, int k) {
  const int kmax = n < PS_RANK_MAX ? n : PS_RANK_MAX;
  if (k < 1 || k > kmax)
    return fail(SE3TN_E_ARG, std::string(who) + ": k = " + std::to_string(k) + " outside [1, min(n, SE3TN_POSE_RANK_MAX = " +
                                 std::to_string(PS_RANK_MAX) + ") = " + std::to_string(kmax) + "]");
  return SE3TN_OK;
}
static PoseScoreArgs pose_score_args(const se3tn_points* p, const double* poses, const uint16_t* depth, int H, int W, const double K[9],
                                     int tol_mm, se3tn_point_fit* out) {
  PoseScoreArgs a;
  a.pts = p->xyz.get(); a.P = p->P; a.poses = poses; a.depth = depth; a.H = H; a.W = W; a.tol = tol_mm; a.out = out;
  for (int i = 0; i < 9; ++i) a.K[i] = K[i];
  return a;
}
// the tail of both searches: the k best of the n records at s.fit, read back and copied out
static int rank_and_finish(const StagedCall& sc, const PsRankTail& s, int n, int k, int32_t* idx_out, se3tn_point_fit* fit_out) {
  HIPCHK(launch_pose_rank(sc.dev<se3tn_point_fit>(s.fit), n, k, sc.dev<int32_t>(s.idx), sc.dev<se3tn_point_fit>(s.top_fit), sc.st));
  if (int rc = sc.finish(s.top_fit, s.readback_bytes)) return rc;
  std::memcpy(fit_out, sc.h + s.top_fit, sizeof(se3tn_point_fit) * (size_t)k);
  std::memcpy(idx_out, sc.h + s.idx, sizeof(int32_t) * (size_t)k);
  return SE3TN_OK;
}

int se3tn_score_poses(se3tn_ctx* c, const se3tn_points* p, int n, const double* poses_dev, const uint16_t* depth_dev, int H, int W,
                      const double K[9], int tol_mm, se3tn_point_fit* fit_dev, void* stream) {
  const char* who = "se3tn_score_poses";
  if (int rc = pose_search_check(who, c, poses_dev && depth_dev && K && fit_dev, p, true, n)) return rc;
  if (int rc = pose_score_check(who, H, W, tol_mm)) return rc;
  HIPCHK(launch_pose_score(pose_score_args(p, poses_dev, depth_dev, H, W, K, tol_mm, fit_dev), n, (hipStream_t)stream));
  return SE3TN_OK;
}

int se3tn_rank_poses(se3tn_ctx* c, int n, const se3tn_point_fit* fit_dev, int k, int32_t* idx_dev, void* stream) {
  const char* who = "se3tn_rank_poses";
  if (int rc = pose_search_check(who, c, fit_dev && idx_dev, nullptr, false, n)) return rc;
  if (int rc = pose_rank_check(who, n, k)) return rc;
  HIPCHK(launch_pose_rank(fit_dev, n, k, idx_dev, nullptr, (hipStream_t)stream));
  return SE3TN_OK;
}

int se3tn_search_poses_host(se3tn_ctx* c, const se3tn_points* p, int n, const double* poses, const uint16_t* depth, int H, int W,
                            const double K[9], int tol_mm, int k, int32_t* idx_out, se3tn_point_fit* fit_out, void* stream) {
  const char* who = "se3tn_search_poses_host";
  if (int rc = pose_search_check(who, c, poses && depth && K && idx_out && fit_out, p, true, n)) return rc;
  if (int rc = pose_score_check(who, H, W, tol_mm)) return rc;
  if (int rc = pose_rank_check(who, n, k)) return rc;
  StagedCall sc{c, who, (hipStream_t)stream};
  if (int rc = sc.refuse_capture()) return rc;
  if (int rc = finite_K_check(who, K)) return rc;
  if (int rc = finite_check(who, "pose", poses, nullptr, (size_t)n, 16, 16)) return rc;
  const PsStage s = ps_stage(n, H, W, k);
  if (int rc = sc.grow(s.bytes)) return rc;
  std::memcpy(sc.h + s.poses, poses, sizeof(double) * 16 * (size_t)n);
  std::memcpy(sc.h + s.depth, depth, sizeof(uint16_t) * (size_t)H * (size_t)W);
  if (int rc = sc.upload(s.upload_bytes)) return rc;
  HIPCHK(launch_pose_score(pose_score_args(p, sc.dev<double>(s.poses), sc.dev<uint16_t>(s.depth), H, W, K, tol_mm,
                                           sc.dev<se3tn_point_fit>(s.fit)), n, sc.st));
  return rank_and_finish(sc, s, n, k, idx_out, fit_out);
}

// ---- n_rot x n_trans candidate poses [R_r | t_t] against one depth frame, the best k ----------------------------------------------
// NULL pointers first, then the numbers, then the context and the handle (which is not read before the context is known to have a
// device): every refusal has its own message, on a host-only context too
static int pose_grid_numbers_check(const char* who, int n_rot, int n_trans, int H, int W, int tol_mm, int facing) {
  if (n_rot < 1 || n_trans < 1 || (long long)n_rot * (long long)n_trans > (long long)PS_MAX_POSES)
    return fail(SE3TN_E_ARG, std::string(who) + ": n_rot = " + std::to_string(n_rot) + ", n_trans = " + std::to_string(n_trans) +
                                 ": both must be >= 1 and their product <= SE3TN_POSE_SEARCH_MAX_POSES = " + std::to_string(PS_MAX_POSES));
  if (int rc = pose_score_check(who, H, W, tol_mm)) return rc;
  return refuse_if(facing != 0 && facing != 1, SE3TN_E_ARG, who, "facing = " + std::to_string(facing) + " is neither 0 nor 1");
}
static int pose_grid_context_check(const char* who, const se3tn_ctx* c, const se3tn_points* p, int facing) {
  if (int rc = device_check(who, c, "search")) return rc;
  if (int rc = same_device_check(who, c, p)) return rc;
  return facing ? normals_check(who, p, "facing = 1 but ") : SE3TN_OK;
}
static int pose_grid_check(const char* who, const se3tn_ctx* c, bool ok_ptrs, const se3tn_points* p, int n_rot, int n_trans, int H, int W,
                           int tol_mm, int facing) {
  if (!c || !ok_ptrs || !p) return null_argument(who);
  if (int rc = pose_grid_numbers_check(who, n_rot, n_trans, H, W, tol_mm, facing)) return rc;
  return pose_grid_context_check(who, c, p, facing);
}
static PoseGridArgs pose_grid_args(const se3tn_points* p, const double* rots, int n_trans, const double* trans, const uint16_t* depth, int H,
                                   int W, const double K[9], int tol_mm, int facing, se3tn_point_fit* out, const uint16_t* scene = nullptr) {
  PoseGridArgs a;
  a.pts = p->xyz.get(); a.nrm = p->nrm.get(); a.P = p->P; a.rots = rots; a.trans = trans; a.n_trans = n_trans;
  a.depth = depth; a.H = H; a.W = W; a.tol = tol_mm; a.facing = facing; a.out = out; a.scene = scene;
  for (int i = 0; i < 9; ++i) a.K[i] = K[i];
  return a;
}

int se3tn_score_pose_grid(se3tn_ctx* c, const se3tn_points* p, int n_rot, const double* rots_dev, int n_trans, const double* trans_dev,
                          const uint16_t* depth_dev, int H, int W, const double K[9], int tol_mm, int facing, se3tn_point_fit* fit_dev,
                          void* stream) {
  const char* who = "se3tn_score_pose_grid";
  if (int rc = pose_grid_check(who, c, rots_dev && trans_dev && depth_dev && K && fit_dev, p, n_rot, n_trans, H, W, tol_mm, facing)) return rc;
  HIPCHK(launch_pose_grid(pose_grid_args(p, rots_dev, n_trans, trans_dev, depth_dev, H, W, K, tol_mm, facing, fit_dev), n_rot,
                          (hipStream_t)stream));
  return SE3TN_OK;
}

int se3tn_search_pose_grid_host(se3tn_ctx* c, const se3tn_points* p, int n_rot, const double* rots, int n_trans, const double* trans,
                                const uint16_t* depth, int H, int W, const double K[9], int tol_mm, int facing, int k, int32_t* idx_out,
                                se3tn_point_fit* fit_out, void* stream) {
  const char* who = "se3tn_search_pose_grid_host";
  if (int rc = pose_grid_check(who, c, rots && trans && depth && K && idx_out && fit_out, p, n_rot, n_trans, H, W, tol_mm, facing)) return rc;
  const int n = n_rot * n_trans;
  if (int rc = pose_rank_check(who, n, k)) return rc;
  StagedCall sc{c, who, (hipStream_t)stream};
  if (int rc = sc.refuse_capture()) return rc;
  if (int rc = finite_K_check(who, K)) return rc;
  if (int rc = finite_check(who, "rotation", rots, nullptr, (size_t)n_rot, 9, 9)) return rc;
  if (int rc = finite_check(who, "translation", trans, nullptr, (size_t)n_trans, 3, 3)) return rc;
  const PgStage s = pg_stage(n_rot, n_trans, H, W, k);
  if (int rc = sc.grow(s.bytes)) return rc;
  std::memcpy(sc.h + s.rots, rots, sizeof(double) * 9 * (size_t)n_rot);
  std::memcpy(sc.h + s.trans, trans, sizeof(double) * 3 * (size_t)n_trans);
  std::memcpy(sc.h + s.depth, depth, sizeof(uint16_t) * (size_t)H * (size_t)W);
  if (int rc = sc.upload(s.upload_bytes)) return rc;
  HIPCHK(launch_pose_grid(pose_grid_args(p, sc.dev<double>(s.rots), n_trans, sc.dev<double>(s.trans), sc.dev<uint16_t>(s.depth), H, W, K,
                                         tol_mm, facing, sc.dev<se3tn_point_fit>(s.fit)), n_rot, sc.st));
  return rank_and_finish(sc, s, n, k, idx_out, fit_out);
}

// ---- n pose hypotheses aligned to one depth frame: point-to-plane steps, all iterations in one launch ----------------------------------
// NULL pointers first, then the numbers, then the context and the handle (which is not read before the context is known to have a
// device): every refusal has its own message, on a host-only context too
// scene_tol_mm: NULL for the plain entry points, the hidden verdict's tolerance for the scene-aware ones
static int pose_align_check(const char* who, const se3tn_ctx* c, bool ok_ptrs, const se3tn_points* p, int n, int H, int W,
                            const se3tn_align_params* q, const int* scene_tol_mm = nullptr) {
  const std::string w(who);
  if (!c || !ok_ptrs || !p || !q) return null_argument(who);
  if (int rc = count_check(who, n, PA_MAX_POSES, "SE3TN_POSE_ALIGN_MAX_POSES")) return rc;
  if (int rc = mm_check(who, "gate_mm", q->gate_mm)) return rc;
  if (q->iters < 1 || q->iters > PA_MAX_ITERS)
    return fail(SE3TN_E_ARG, w + ": iters = " + std::to_string(q->iters) + " outside [1, SE3TN_POSE_ALIGN_MAX_ITERS = " +
                                 std::to_string(PA_MAX_ITERS) + "]");
  if (q->min_pairs < 6 || q->min_pairs > (1 << 20))
    return fail(SE3TN_E_ARG, w + ": min_pairs = " + std::to_string(q->min_pairs) + " outside [6, 2^20] (six unknowns)");
  if (q->_reserved != 0) return fail(SE3TN_E_ARG, w + ": params._reserved = " + std::to_string(q->_reserved) + " is not 0");
  if (!(q->damping >= 0.0) || !std::isfinite(q->damping)) return fail(SE3TN_E_ARG, w + ": damping is negative or not finite");
  if (!(q->stop >= 0.0) || !std::isfinite(q->stop)) return fail(SE3TN_E_ARG, w + ": stop is negative or not finite");
  if (scene_tol_mm)
    if (int rc = mm_check(who, "scene_tol_mm", *scene_tol_mm)) return rc;
  if (int rc = frame_check(who, H, W)) return rc;
  if (int rc = device_check(who, c, "align")) return rc;
  if (int rc = same_device_check(who, c, p)) return rc;
  return normals_check(who, p, "");
}
static PoseAlignArgs pose_align_args(const se3tn_points* p, const double* poses, const uint16_t* depth, int H, int W, const double K[9],
                                     const se3tn_align_params* q, double* poses_out, se3tn_align_rec* rec, int64_t* sums,
                                     const uint16_t* scene = nullptr, int scene_tol_mm = 0) {
  PoseAlignArgs a;
  a.pts = p->xyz.get(); a.nrm = p->nrm.get(); a.P = p->P; a.poses = poses; a.depth = depth; a.H = H; a.W = W; a.p = *q;
  a.poses_out = poses_out; a.rec = rec; a.sums = sums; a.scene = scene; a.scene_tol = scene_tol_mm;
  for (int i = 0; i < 9; ++i) a.K[i] = K[i];
  return a;
}

int se3tn_align_poses(se3tn_ctx* c, const se3tn_points* p, int n, const double* poses_dev, const uint16_t* depth_dev, int H, int W,
                      const double K[9], const se3tn_align_params* params, double* poses_out_dev, se3tn_align_rec* rec_dev,
                      int64_t* sums_dev, void* stream) {
  const char* who = "se3tn_align_poses";
  if (int rc = pose_align_check(who, c, poses_dev && depth_dev && K && poses_out_dev && rec_dev, p, n, H, W, params)) return rc;
  HIPCHK(launch_pose_align(pose_align_args(p, poses_dev, depth_dev, H, W, K, params, poses_out_dev, rec_dev, sums_dev), n,
                           (hipStream_t)stream));
  return SE3TN_OK;
}

int se3tn_align_poses_host(se3tn_ctx* c, const se3tn_points* p, int n, const double* poses, const uint16_t* depth, int H, int W,
                           const double K[9], const se3tn_align_params* params, double* poses_out, se3tn_align_rec* rec_out,
                           int64_t* sums_out, void* stream) {
  const char* who = "se3tn_align_poses_host";
  if (int rc = pose_align_check(who, c, poses && depth && K && poses_out && rec_out, p, n, H, W, params)) return rc;
  StagedCall sc{c, who, (hipStream_t)stream};
  if (int rc = sc.refuse_capture()) return rc;
  if (int rc = finite_K_check(who, K)) return rc;
  if (int rc = finite_check(who, "pose", poses, nullptr, (size_t)n, 16, 12)) return rc;   // row 3 is not read
  const PaStage s = pa_stage(n, H, W, sums_out ? 1 : 0);
  if (int rc = sc.grow(s.bytes)) return rc;
  std::memcpy(sc.h + s.poses, poses, sizeof(double) * 16 * (size_t)n);
  std::memcpy(sc.h + s.depth, depth, sizeof(uint16_t) * (size_t)H * (size_t)W);
  if (int rc = sc.upload(s.upload_bytes)) return rc;
  HIPCHK(launch_pose_align(pose_align_args(p, sc.dev<double>(s.poses), sc.dev<uint16_t>(s.depth), H, W, K, params, sc.dev<double>(s.poses_out),
                                           sc.dev<se3tn_align_rec>(s.rec), sums_out ? sc.dev<int64_t>(s.sums) : nullptr), n, sc.st));
  if (int rc = sc.finish(s.poses_out, s.readback_bytes)) return rc;
  std::memcpy(poses_out, sc.h + s.poses_out, sizeof(double) * 16 * (size_t)n);
  std::memcpy(rec_out, sc.h + s.rec, sizeof(se3tn_align_rec) * (size_t)n);
  if (sums_out) std::memcpy(sums_out, sc.h + s.sums, sizeof(int64_t) * SE3TN_POSE_ALIGN_SUMS * (size_t)n);
  return SE3TN_OK;
}

// ---- the alignment among tracked objects: points hidden by the composed scene are not paired --------------------------------------------
// (the kernel writes se3tn_scene_align_rec records through PoseAlignArgs::rec: pose_align_math.h holds the two layouts equal)
int se3tn_align_poses_scene(se3tn_ctx* c, const se3tn_points* p, int n, const double* poses_dev, const uint16_t* depth_dev,
                            const uint16_t* scene_dev, int H, int W, const double K[9], const se3tn_align_params* params, int scene_tol_mm,
                            double* poses_out_dev, se3tn_scene_align_rec* rec_dev, int64_t* sums_dev, void* stream) {
  const char* who = "se3tn_align_poses_scene";
  if (int rc = pose_align_check(who, c, poses_dev && depth_dev && scene_dev && K && poses_out_dev && rec_dev, p, n, H, W, params, &scene_tol_mm))
    return rc;
  HIPCHK(launch_pose_align(pose_align_args(p, poses_dev, depth_dev, H, W, K, params, poses_out_dev, reinterpret_cast<se3tn_align_rec*>(rec_dev),
                                           sums_dev, scene_dev, scene_tol_mm), n, (hipStream_t)stream));
  return SE3TN_OK;
}

int se3tn_align_poses_scene_host(se3tn_ctx* c, const se3tn_points* p, int n, const double* poses, const uint16_t* depth, const uint16_t* scene,
                                 int H, int W, const double K[9], const se3tn_align_params* params, int scene_tol_mm, double* poses_out,
                                 se3tn_scene_align_rec* rec_out, int64_t* sums_out, void* stream) {
  const char* who = "se3tn_align_poses_scene_host";
  if (int rc = pose_align_check(who, c, poses && depth && scene && K && poses_out && rec_out, p, n, H, W, params, &scene_tol_mm)) return rc;
  StagedCall sc{c, who, (hipStream_t)stream};
  if (int rc = sc.refuse_capture()) return rc;
  if (int rc = finite_K_check(who, K)) return rc;
  if (int rc = finite_check(who, "pose", poses, nullptr, (size_t)n, 16, 12)) return rc;   // row 3 is not read
  const PaSceneStage s = pa_stage_scene(n, H, W, sums_out ? 1 : 0);
  if (int rc = sc.grow(s.bytes)) return rc;
  const size_t frame_bytes = sizeof(uint16_t) * (size_t)H * (size_t)W;
  std::memcpy(sc.h + s.poses, poses, sizeof(double) * 16 * (size_t)n);
  std::memcpy(sc.h + s.depth, depth, frame_bytes);
  std::memcpy(sc.h + s.scene, scene, frame_bytes);
  if (int rc = sc.upload(s.upload_bytes)) return rc;
  HIPCHK(launch_pose_align(pose_align_args(p, sc.dev<double>(s.poses), sc.dev<uint16_t>(s.depth), H, W, K, params, sc.dev<double>(s.poses_out),
                                           sc.dev<se3tn_align_rec>(s.rec), sums_out ? sc.dev<int64_t>(s.sums) : nullptr,
                                           sc.dev<uint16_t>(s.scene), scene_tol_mm), n, sc.st));
  if (int rc = sc.finish(s.poses_out, s.readback_bytes)) return rc;
  std::memcpy(poses_out, sc.h + s.poses_out, sizeof(double) * 16 * (size_t)n);
  std::memcpy(rec_out, sc.h + s.rec, sizeof(se3tn_scene_align_rec) * (size_t)n);
  if (sums_out) std::memcpy(sums_out, sc.h + s.sums, sizeof(int64_t) * SE3TN_POSE_ALIGN_SUMS * (size_t)n);
  return SE3TN_OK;
}

static int reserve_objects_raster(se3tn_ctx* c, int n, const se3tn_mesh* const* meshes);
// where raster_instances keeps its scratch, its instance table and (frame route) its sub-images and z-buffers: the context's
// (nullptr), or the scene stage's own
struct RasterHome {
  const RasterScratch* mo;
  uint8_t *inst_host, *inst_dev, *sub;
  unsigned long long* zbuf;
};
static int raster_instances(se3tn_ctx* c, int n, const se3tn_mesh* const* meshes, const double* poses, const double K[9], int H, int W,
                            const TrackWindow* windows, bool frame_route, uint8_t* rgb, uint16_t* depth, size_t maxpx, size_t fr_d_off,
                            hipStream_t st, int* singular, const RasterHome* home = nullptr);

// se3tn_set_fit_check's stage of the three bodies, after their pose read-back (so `st` is idle and the instance table, the rasteriser
// scratch and, on the frame route, the rectangles' sub-images and z-buffers of image A are free again): every pair's mesh rendered at
// its ESTIMATE est[i] in the window of its PREVIOUS pose -- the window route at windows[i].winA into the context's render stack, the
// frame route into the rectangle image A was rendered into -- n instances in the rasteriser's four launches, each with its own mesh
// (and material); then the fit kernel: the model descriptor is what crop_pair builds for image A, now showing that render, the observed
// one is image B's (the staged window at b_base; live: the filled depth the rectangle pass wrote; a miss: its zero pixel).  On the frame
// route the fit launch also leaves the raw 176 x 176 crop of every render in the stack.  The records land in mapped pinned memory;
// the call waits for `st` once more
static int fit_check_stage(se3tn_ctx* c, int n, const se3tn_mesh* const* meshes, const double* est, const double K[9], int H, int W,
                           const TrackWindow* windows, bool frame_route, const uint8_t* b_base, hipStream_t st, const std::string& who) {
  if (n > c->fit_cap) {   // first call with the check on (or a larger n than max_batch: never)
    DeviceGuard dg(c->device);
    if (int rc = begin_growth(dg)) return rc;
    c->fit_cap = 0;
    const int cap = n > c->max_batch ? n : c->max_batch;
    HIPCHK(c->fit_rgb.alloc((size_t)RES * RES * 3 * cap));
    HIPCHK(c->fit_depth.alloc((size_t)RES * RES * cap));
    HIPCHK(c->fit_host.alloc(cap, true, true));
    c->fit_cap = cap;
  }
  if (int rc = reserve_track_batch(c, nullptr, n, 0)) return rc;
  if (int rc = reserve_objects_raster(c, n, meshes)) return rc;
  size_t maxpx = 0, fr_d_off = 0;
  if (frame_route)
    if (int rc = reserve_frame_rects(c, n, windows, H, W, &maxpx, &fr_d_off)) return rc;
  int singular = -1;
  if (int rc = raster_instances(c, n, meshes, est, K, H, W, windows, frame_route, c->fit_rgb.get(), c->fit_depth.get(), maxpx, fr_d_off, st,
                                &singular))
    return singular >= 0 ? fail(SE3TN_E_ARG, who + ": fit check: singular pose estimate") : rc;
  auto pair = [&](int j, se3tn_crop& m, se3tn_crop& o) {
    crop_pair(windows[j], 0.0, image_a(c, frame_route, j, c->fit_rgb.get(), c->fit_depth.get(), maxpx, fr_d_off), b_base, m, o);
  };
  if (int rc = fit_launches(c, n, pair, c->fit_host.dev(), nullptr, c->fit_tol, frame_route ? c->fit_rgb.get() : nullptr,
                            frame_route ? c->fit_depth.get() : nullptr, st))
    return rc;
  HIPCHK(hipStreamSynchronize(st));
  c->fit_last_n = n;
  return SE3TN_OK;
}

int se3tn_on_track_batch(se3tn_ctx* c, se3tn_mesh* m, int n, const double* prev_poses, const double K[9], double object_width_mm,
                         const uint8_t* const* rgb, const uint16_t* const* depth, int H, int W, uint8_t* rgbA_dev, uint16_t* depthA_dev,
                         double* pose_out, float* trans_out, float* rot_out, int32_t* bbox_vu, void* stream) {
  if (!c || c->device < 0 || !m || !prev_poses || !K || !rgb || !depth || H < 1 || W < 1 || !pose_out || !(object_width_mm > 0))
    return fail(SE3TN_E_ARG, "se3tn_on_track_batch: bad argument");
  if (n < 1 || n > c->max_batch) return fail(SE3TN_E_ARG, "se3tn_on_track_batch: n outside [1, max_batch]");
  if (!c->have_norm) return fail(SE3TN_E_STATE, "se3tn_on_track_batch: call se3tn_set_normalization first");
  if (stream_is_capturing((hipStream_t)stream)) return fail(SE3TN_E_STATE, "se3tn_on_track_batch: synchronous call, not capturable");
  c->fit_last_n = 0;
  hipStream_t st = (hipStream_t)stream;
  static const bool trace = std::getenv("SE3TN_TRACK_TRACE") != nullptr;   // developer switch: host-side timeline of the call
  static double tb_acc[6] = {0, 0, 0, 0, 0, 0};
  static int tb_calls = 0;
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = trace ? now() : 0.0;
  // pass 1 (host float64): the windows of every pair (predict.py:231-235 / :201-206) and the size of the staged sub-images
  std::vector<TrackWindow> windows(n);
  size_t bytes = (((size_t)n * 128) + 255) & ~(size_t)255;   // the poses in front
  for (int i = 0; i < n; ++i) {
    if (!rgb[i] || !depth[i]) return fail(SE3TN_E_ARG, "se3tn_on_track_batch: null frame pointer");
    const PlanStatus ps = plan_window(prev_poses + 16 * (size_t)i, K, object_width_mm, H, W, bytes, windows[i]);
    if (ps == PlanStatus::NOT_IN_FRONT) return fail(SE3TN_E_ARG, "se3tn_on_track_batch: a pose is not in front of the camera (z <= 0 or not finite)");
    if (ps == PlanStatus::EMPTY_WINDOW) return fail(SE3TN_E_ARG, "se3tn_on_track_batch: empty crop window");
  }
  if (int rc = reserve_track_batch(c, m, n, bytes)) return rc;
  // image A of all n poses: the instance table goes up on the launch stream, then FOUR launches (grid.y = pose)
  uint8_t* rA = rgbA_dev ? rgbA_dev : c->tb_rgbA.get();
  uint16_t* dA = depthA_dev ? depthA_dev : c->tb_depthA.get();
  const bool frame_route = m->route == SE3TN_ROUTE_FRAME;
  size_t maxpx = 0, fr_d_off = 0;
  if (frame_route) {
    if (H > 2048) return fail(SE3TN_E_ARG, "se3tn_on_track_batch: frames of more than 2048 rows are not supported on SE3TN_ROUTE_FRAME");
    if (int rc = reserve_frame_rects(c, n, windows.data(), H, W, &maxpx, &fr_d_off)) return rc;
  }
  RasterArgs ra{};
  raster_common(ra, c, m, rA, dA);
  ra.rw = RES; ra.rh = RES; ra.mode = 0;
  if (frame_route) {
    frame_uniforms(ra, m, prev_poses, K, W, H);   // material, frame size (the matrix comes from the instance table)
    ra.rgb = c->fr_sub.get() + 64; ra.depth = (uint16_t*)(c->fr_sub.get() + fr_d_off);
    ra.scissor = 1; ra.spx = (int)maxpx;
  }
  raster_scratch(ra, m->batch);
  ra.zbuf = frame_route ? c->fr_zbuf.get() : c->tb_zbuf.get();
  RasterInstance* inst_host = (RasterInstance*)c->tb_inst_host.get();
  for (int i = 0; i < n; ++i)
    if (!fill_instance(inst_host[i], frame_route, m, prev_poses + 16 * (size_t)i, K, W, H, windows[i]))
      return fail(SE3TN_E_ARG, "se3tn_on_track_batch: singular pose");
  if (!frame_route || maxpx > 0) {
    HIPCHK(hipMemcpyAsync(c->tb_inst_dev.get(), inst_host, sizeof(RasterInstance) * n, hipMemcpyHostToDevice, st));
    ra.inst = (const RasterInstance*)c->tb_inst_dev.get();
    HIPCHK(launch_raster(ra, st, n));
  }
  const double t1 = trace ? now() : 0.0;
  // the frames' windows: staged through pinned memory while the rasteriser runs, ONE copy with the poses in front
  uint8_t* hp = c->tb_stage_host.get();
  std::memcpy(hp, prev_poses, (size_t)n * 128);
  auto stage_pairs = [&](int i0, int i1) {
    for (int i = i0; i < i1; ++i) stage_window(windows[i], rgb[i], depth[i], W, hp);
  };
  // above ~8 MB the row-wise gather is worth helper threads (measured, profiles/r06_tracker_batch_staging.txt: 13.5 MB at 64 tracks 0.34-0.43 ms
  // on one core, 0.25 ms on four; 4.5 MB at 21 tracks 0.10 ms on one core, 0.15 ms on four -- the thread start costs more than it
  // saves); SE3TN_STAGE_THREADS = 1 .. 8 (default 4) sets the number of threads incl. the caller's
  static const int stage_threads = [] {
    const char* e = std::getenv("SE3TN_STAGE_THREADS");
    const int v = e ? std::atoi(e) : 4;
    return v < 1 ? 1 : (v > 8 ? 8 : v);
  }();
  const int nth = bytes > ((size_t)8 << 20) ? (stage_threads < n ? stage_threads : n) : 1;
  if (nth > 1) {
    std::vector<std::thread> helpers;
    for (int k = 1; k < nth; ++k) helpers.emplace_back(stage_pairs, (int)((long long)n * k / nth), (int)((long long)n * (k + 1) / nth));
    stage_pairs(0, n / nth);
    for (auto& h : helpers) h.join();
  } else {
    stage_pairs(0, n);
  }
  const double t2 = trace ? now() : 0.0;
  StagedUpload up{c->trk_copy_stream};
  if (int rc = upload_staged(c, c->tb_stage_dev.get(), hp, bytes, st)) return rc;
  // both crops of every pair (data_augmentation.py:124-189 with poseA's z), 64 descriptors per launch
  std::vector<se3tn_crop> crops(2 * (size_t)n);
  for (int i = 0; i < n; ++i)
    crop_pair(windows[i], prev_poses[16 * (size_t)i + 11] * 1000, image_a(c, frame_route, i, rA, dA, maxpx, fr_d_off), c->tb_stage_dev.get(), crops[i],
              crops[(size_t)n + i]);
  // frame route: the crops of image A also leave their raw pixels (crop_bbox of the render = Tracker.render_window) in rgbA_dev / depthA_dev
  const bool rawA = frame_route && (rgbA_dev || depthA_dev);
  int rc = preprocess_impl(c, crops.data(), n, c->inA.get(), rawA ? rA : nullptr, rawA ? dA : nullptr, stream);
  if (rc == SE3TN_OK) rc = se3tn_preprocess(c, crops.data() + n, n, c->inB.get(), stream);
  float* trans_d = (float*)(c->tb_out_dev.get() + (size_t)n * 128);
  float* rot_d = trans_d + 3 * (size_t)n;
  if (rc == SE3TN_OK)
    rc = se3tn_infer(c, c->inA.get(), c->inB.get(), n, SE3TN_NHWC, trans_d, rot_d, (const double*)c->tb_stage_dev.get(), (double*)c->tb_out_dev.get(), stream);
  if (rc != SE3TN_OK) return rc;
  const double t3 = trace ? now() : 0.0;
  if ((rc = read_back_tracks(c, n, st, pose_out, trans_out, rot_out, bbox_vu, windows.data()))) return rc;
  up.done();
  if (trace) {
    const double t4 = now();
    const double d[5] = {t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0};
    for (int i = 0; i < 5; ++i) tb_acc[i] += d[i];
    if (++tb_calls % 50 == 0) {
      std::fprintf(stderr, "se3tn_on_track_batch host timeline (n = %d, mean of 50, us): bboxes + uniforms + render enqueue %.1f | staging %.1f MB %.1f | "
                   "upload + crops + infer enqueue %.1f | wait for the device %.1f | total %.1f\n", n, tb_acc[0] / 50, bytes / 1e6, tb_acc[1] / 50,
                   tb_acc[2] / 50, tb_acc[3] / 50, tb_acc[4] / 50);
      for (double& v : tb_acc) v = 0;
    }
  }
  if (c->fit_tol) {
    const std::vector<const se3tn_mesh*> meshes(n, m);
    return fit_check_stage(c, n, meshes.data(), pose_out, K, H, W, windows.data(), frame_route, c->tb_stage_dev.get(), st, "se3tn_on_track_batch");
  }
  return SE3TN_OK;
}

// ---- n objects (n models) in one camera frame per call ------------------------------------------------------------------------------
// rasteriser scratch for n instances of meshes of up to V vertices / F triangles (se3tn_on_track_objects; grown at first use)
static void largest_mesh(const se3tn_mesh* const* meshes, int n, int* V, int* F) {
  *V = *F = 0;
  for (int i = 0; i < n; ++i) {
    *V = meshes[i]->V > *V ? meshes[i]->V : *V;
    *F = meshes[i]->F > *F ? meshes[i]->F : *F;
  }
}
static int reserve_objects_raster(se3tn_ctx* c, int n, const se3tn_mesh* const* meshes) {
  int V, F;
  largest_mesh(meshes, n, &V, &F);
  if (n <= c->mo_cap && V <= c->mo_V && F <= c->mo_F) return SE3TN_OK;
  DeviceGuard dg(c->device);
  if (int rc = begin_growth(dg)) return rc;
  const int cap = n > c->max_batch ? n : c->max_batch;
  V = V > c->mo_V ? V : c->mo_V;
  F = F > c->mo_F ? F : c->mo_F;
  c->mo_cap = 0; c->mo_V = 0; c->mo_F = 0;
  HIPCHK(c->mo.alloc(V, F, cap));
  c->mo_cap = cap; c->mo_V = V; c->mo_F = F;
  return SE3TN_OK;
}

// n instances in the rasteriser's FOUR launches (grid.y = instance), every one with its own mesh, pose and window and, on the frame
// route, its own material: the instance table (the materials behind the n instance records) goes up in one copy on `st`.  Window
// route: the 176 x 176 renders land in the stacks rgb / depth; frame route: every rectangle in c->fr_sub (maxpx, fr_d_off:
// reserve_frame_rects) -- or all of these where `home` says.  The scratch, the table and the z-buffers are reserved.  A singular pose: SE3TN_E_ARG with *singular = its
// index and no text (the refusal is the caller's)
static int raster_instances(se3tn_ctx* c, int n, const se3tn_mesh* const* meshes, const double* poses, const double K[9], int H, int W,
                            const TrackWindow* windows, bool frame_route, uint8_t* rgb, uint16_t* depth, size_t maxpx, size_t fr_d_off,
                            hipStream_t st, int* singular, const RasterHome* home) {
  const RasterHome ctx_home{&c->mo, c->tb_inst_host.get(), c->tb_inst_dev.get(), c->fr_sub.get(), c->fr_zbuf.get()};
  if (!home) home = &ctx_home;
  RasterArgs ra{};
  raster_common(ra, c, const_cast<se3tn_mesh*>(meshes[0]), rgb, depth);
  ra.rw = RES; ra.rh = RES; ra.mode = 0;
  raster_scratch(ra, *home->mo);
  ra.zbuf = c->tb_zbuf.get();
  largest_mesh(meshes, n, &ra.V, &ra.F);
  ra.inst_mesh = 1;
  RasterInstance* inst_host = (RasterInstance*)home->inst_host;
  RasterMaterial* mat_host = (RasterMaterial*)(inst_host + n);
  if (frame_route) {
    ra.rw = W; ra.rh = H; ra.mode = 1;   // (matrix, mesh, material and rectangle come from the tables)
    ra.rgb = home->sub + 64; ra.depth = (uint16_t*)(home->sub + fr_d_off);
    ra.zbuf = home->zbuf;
    ra.scissor = 1; ra.spx = (int)maxpx;
    ra.inst_mesh = 2;   // every instance with its own material: the table behind the n instance records
  }
  for (int i = 0; i < n; ++i) {
    const se3tn_mesh* m = meshes[i];
    RasterInstance& I = inst_host[i];
    if (!fill_instance(I, frame_route, m, poses + 16 * (size_t)i, K, W, H, windows[i])) {
      *singular = i;
      return SE3TN_E_ARG;
    }
    I.verts = m->verts.get(); I.normals = m->normals.get(); I.colors = m->colors.get(); I.faces = m->faces.get(); I.V = m->V; I.F = m->F;
    if (frame_route) {
      RasterMaterial& M = mat_host[i];
      M.uv = m->uv.get(); M.tex = m->tex.get(); M.tw = m->tw; M.th = m->th; M.tlevels = m->tlevels;
      std::memcpy(M.kd, m->kd, sizeof(M.kd));
      std::memcpy(M.tex_off, m->tex_off, sizeof(M.tex_off));
    }
  }
  if (frame_route && maxpx == 0) return SE3TN_OK;   // (every window off the frame: nothing to render)
  const size_t tab_bytes = sizeof(RasterInstance) * n + (frame_route ? sizeof(RasterMaterial) * n : 0);
  HIPCHK(hipMemcpyAsync(home->inst_dev, inst_host, tab_bytes, hipMemcpyHostToDevice, st));
  ra.inst = (const RasterInstance*)home->inst_dev;
  HIPCHK(launch_raster(ra, st, n));
  return SE3TN_OK;
}

// ---- which of n hypotheses does the frame confirm ----------------------------------------------------------------------------------
// The front half of se3tn_on_track_batch with the hypothesis in the place of prev_pose: windows, image A of every pose, the frame's
// windows staged in one copy -- then the depth and colour records instead of the network.  The staging buffer carries the records in
// front (verify_plan.h: where se3tn_on_track_batch carries its poses), written by the kernel and read back in one copy; the upload
// starts behind them.  The stages are se3tn_on_track_batch's, the rasteriser path is se3tn_on_track_objects': raster_instances() with
// n copies of the one mesh (inst_mesh = 1, or 2 on the frame route: mesh and material per instance from the table), on the CONTEXT's
// scratch c->mo (reserve_objects_raster) -- not m->batch and not se3tn_on_track_batch's own launch, so the mesh is not touched.  The
// bytes are those of that launch (tests/test_gpu_color_fit.py holds them equal).  What the call writes: c->mo, the instance table
// (tb_inst_host / tb_inst_dev), tb_rgbA / tb_depthA / tb_zbuf or fr_sub / fr_zbuf, tb_stage_host / tb_stage_dev and the colour
// counters (re-armed by the kernel) -- every one rewritten by a tracking call before it reads it
// the body of se3tn_verify_poses_host and (scene_dev != NULL) se3tn_verify_poses_scene_host, the entry points at the end of this file
static int verify_poses(const char* who, se3tn_ctx* c, se3tn_mesh* m, const double* poses, int n, const double K[9], double object_width_mm,
                        const uint8_t* rgb, const uint16_t* depth, const uint16_t* scene_dev, int H, int W, int tol_mm, se3tn_fit* fit_out,
                        se3tn_color_fit* color_out, int32_t* bbox_out) {
  if (!c || !m || !poses || !K || !rgb || !depth || !fit_out || !color_out) return null_argument(who);
  if (int rc = frame_check(who, H, W)) return rc;
  if (int rc = refuse_if(!(object_width_mm > 0), SE3TN_E_ARG, who, "object_width_mm must be > 0")) return rc;
  if (int rc = mm_check(who, "tol_mm", tol_mm)) return rc;
  if (int rc = device_check(who, c, "verify")) return rc;
  if (int rc = count_check(who, n, c->max_batch, "se3tn_max_batch")) return rc;
  hipStream_t st = nullptr;
  {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(st, &cs);   // (the default stream under another stream's capture: an error, refused too)
    if (e != hipSuccess) (void)hipGetLastError();
    if (int rc = refuse_if(e != hipSuccess || cs != hipStreamCaptureStatusNone, SE3TN_E_STATE, who, "the call is synchronous, it cannot be captured"))
      return rc;
  }
  if (int rc = finite_K_check(who, K)) return rc;
  const std::string w(who);
  std::vector<TrackWindow> windows(n);
  const VerifyLayout L = plan_verify(n);
  size_t bytes = L.begin;
  for (int i = 0; i < n; ++i) {
    const PlanStatus ps = plan_window(poses + 16 * (size_t)i, K, object_width_mm, H, W, bytes, windows[i]);
    if (ps == PlanStatus::NOT_IN_FRONT) return fail(SE3TN_E_ARG, w + ": pose " + std::to_string(i) + " is not in front of the camera (z <= 0 or not finite)");
    if (ps == PlanStatus::EMPTY_WINDOW) return fail(SE3TN_E_ARG, w + ": pose " + std::to_string(i) + ": empty crop window");
  }
  const bool frame_route = m->route == SE3TN_ROUTE_FRAME;
  if (frame_route && H > 2048) return fail(SE3TN_E_ARG, w + ": frames of more than 2048 rows are not supported on SE3TN_ROUTE_FRAME");
  if (int rc = reserve_track_batch(c, nullptr, n, bytes)) return rc;
  const std::vector<const se3tn_mesh*> meshes(n, m);
  if (int rc = reserve_objects_raster(c, n, meshes.data())) return rc;
  size_t maxpx = 0, fr_d_off = 0;
  if (frame_route)
    if (int rc = reserve_frame_rects(c, n, windows.data(), H, W, &maxpx, &fr_d_off)) return rc;
  // image A of all n poses: the instance table goes up on the launch stream, then FOUR launches (grid.y = pose)
  uint8_t* rA = c->tb_rgbA.get();
  uint16_t* dA = c->tb_depthA.get();
  int singular = -1;
  if (int rc = raster_instances(c, n, meshes.data(), poses, K, H, W, windows.data(), frame_route, rA, dA, maxpx, fr_d_off, st, &singular))
    return singular >= 0 ? fail(SE3TN_E_ARG, w + ": pose " + std::to_string(singular) + " is singular") : rc;
  // the frame's n windows: staged through pinned memory while the rasteriser runs, ONE copy
  uint8_t* hp = c->tb_stage_host.get();
  for (int i = 0; i < n; ++i) stage_window(windows[i], rgb, depth, W, hp);
  StagedUpload up{c->trk_copy_stream};
  if (int rc = upload_staged(c, c->tb_stage_dev.get() + L.begin, hp + L.begin, bytes - L.begin, st)) return rc;   // (every window stages >= 64 bytes)
  se3tn_fit* fit_dev = (se3tn_fit*)(c->tb_stage_dev.get() + L.fit_off);
  se3tn_color_fit* col_dev = (se3tn_color_fit*)(c->tb_stage_dev.get() + L.color_off);
  auto pair = [&](int j, se3tn_crop& m, se3tn_crop& o) { crop_pair(windows[j], 0.0, image_a(c, frame_route, j, rA, dA, maxpx, fr_d_off), c->tb_stage_dev.get(), m, o); };
  auto triple = [&](int j, se3tn_crop& m, se3tn_crop& o, se3tn_crop& s) { pair(j, m, o); crop_scene(windows[j], scene_dev, H, W, s); };
  if (int rc = scene_dev ? fit_launches<FitSceneArgs>(c, n, triple, fit_dev, col_dev, tol_mm, nullptr, nullptr, st)
                         : fit_launches(c, n, pair, fit_dev, col_dev, tol_mm, nullptr, nullptr, st)) return rc;
  HIPCHK(hipMemcpyAsync(hp, c->tb_stage_dev.get(), L.rec_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  up.done();
  std::memcpy(fit_out, hp + L.fit_off, sizeof(se3tn_fit) * (size_t)n);
  std::memcpy(color_out, hp + L.color_off, sizeof(se3tn_color_fit) * (size_t)n);
  if (bbox_out)
    for (int i = 0; i < n; ++i) std::memcpy(bbox_out + 8 * (size_t)i, windows[i].vu, sizeof(windows[i].vu));
  return SE3TN_OK;
}

// ---- the objects of one frame as one scene -------------------------------------------------------------------------------------------
// what the three entry points refuse alike, before anything is allocated or written
static int scene_numbers_check(const char* who, const se3tn_ctx* c, int n, int H, int W, bool rendering) {
  if (int rc = refuse_if(rendering && H > 2048, SE3TN_E_ARG, who, "frames of more than 2048 rows are not supported (as se3tn_render_frame)")) return rc;
  if (int rc = refuse_if(!scene_frame_ok(H, W), SE3TN_E_ARG, who, "H * W > 2^21 pixels: sum_abs_mm could overflow its word")) return rc;
  const int most = c->max_batch < SE3TN_SCENE_MAX_OBJECTS ? c->max_batch : SE3TN_SCENE_MAX_OBJECTS;
  return count_check(who, n, most, "min(SE3TN_SCENE_MAX_OBJECTS, se3tn_max_batch)");
}
static int scene_args_check(const char* who, const se3tn_ctx* c, int n, int tol_mm, int H, int W, bool rendering) {
  if (int rc = frame_check(who, H, W)) return rc;
  if (int rc = mm_check(who, "tol_mm", tol_mm)) return rc;
  if (int rc = scene_numbers_check(who, c, n, H, W, rendering)) return rc;
  return device_check(who, c, "compose the scene");
}

// the kernel on n checked layers
static int scene_enqueue(se3tn_ctx* c, int n, const se3tn_scene_layer* layers, const uint16_t* observed, int H, int W, int tol_mm,
                         struct se3tn_scene_fit* out, uint8_t* ids, uint16_t* scene, hipStream_t st) {
  SceneArgs a{};
  int32_t rects[4 * SceneArgs::MAX];
  for (int i = 0; i < n; ++i) {
    std::memcpy(rects + 4 * i, layers[i].rect, sizeof(layers[i].rect));
    const bool empty = scene_rect_empty(layers[i].rect);
    a.l[i].depth = empty ? nullptr : layers[i].depth;
    a.l[i].x0 = empty ? 0 : layers[i].rect[0]; a.l[i].y0 = empty ? 0 : layers[i].rect[1];
    a.l[i].x1 = empty ? 0 : layers[i].rect[2]; a.l[i].y1 = empty ? 0 : layers[i].rect[3];
  }
  a.observed = observed; a.H = H; a.W = W; a.n = n; a.tol = tol_mm;
  a.plan = plan_scene(n, rects, H, W, ids != nullptr || scene != nullptr);
  a.counters = c->sc_counters.get();
  a.out = out; a.ids = ids; a.scene = scene;
  HIPCHK(launch_scene_fit(a, st));
  return SE3TN_OK;
}

int se3tn_scene_stats(se3tn_ctx* c, int n, const se3tn_scene_layer* layers, const uint16_t* observed_dev, int H, int W, int tol_mm,
                      struct se3tn_scene_fit* out_dev, uint8_t* ids_dev, uint16_t* scene_dev, void* stream) {
  const char* who = "se3tn_scene_stats";
  if (!c || !layers || !observed_dev || !out_dev) return null_argument(who);
  if (int rc = scene_args_check(who, c, n, tol_mm, H, W, false)) return rc;
  for (int i = 0; i < n; ++i) {
    if (int rc = refuse_if(!scene_rect_ok(layers[i].rect, H, W), SE3TN_E_ARG, who,
                           "layer " + std::to_string(i) + ": its rectangle is not empty and not inside the frame")) return rc;
    if (int rc = refuse_if(!scene_rect_empty(layers[i].rect) && !layers[i].depth, SE3TN_E_ARG, who,
                           "layer " + std::to_string(i) + ": NULL depth")) return rc;
  }
  return scene_enqueue(c, n, layers, observed_dev, H, W, tol_mm, out_dev, ids_dev, scene_dev, (hipStream_t)stream);
}

// the refusals of se3tn_scene_fit / _host that concern the objects, and per object the window of its pose (plan_window: x0, y0, sw,
// sh = se3tn_frame_rect's rectangle, miss = a window off the frame)
static int scene_windows(const char* who, int n, const se3tn_object* objs, const double* poses, const double K[9], int H, int W,
                         std::vector<TrackWindow>& windows, std::vector<const se3tn_mesh*>& meshes) {
  const std::string w(who);
  if (int rc = finite_K_check(who, K)) return rc;
  if (int rc = finite_check(who, "pose", poses, nullptr, (size_t)n, 16, 12)) return rc;
  windows.resize(n);
  meshes.resize(n);
  size_t bytes = 0;   // (nothing is staged: the offsets plan_window hands out are not used)
  for (int i = 0; i < n; ++i) {
    if (int rc = refuse_if(!objs[i].mesh, SE3TN_E_ARG, who, "object " + std::to_string(i) + " has no mesh")) return rc;
    if (int rc = refuse_if(!(objs[i].object_width_mm > 0), SE3TN_E_ARG, who, "object " + std::to_string(i) + ": object_width_mm must be > 0")) return rc;
    const PlanStatus ps = plan_window(poses + 16 * (size_t)i, K, objs[i].object_width_mm, H, W, bytes, windows[i]);
    if (ps == PlanStatus::NOT_IN_FRONT) return fail(SE3TN_E_ARG, w + ": pose " + std::to_string(i) + " is not in front of the camera (z <= 0 or not finite)");
    if (ps == PlanStatus::EMPTY_WINDOW) return fail(SE3TN_E_ARG, w + ": pose " + std::to_string(i) + ": empty crop window");
    meshes[i] = objs[i].mesh;
  }
  return SE3TN_OK;
}

// the scene stage's own buffers for n instances of these meshes and these rectangles (sized as reserve_frame_rects sizes fr_sub:
// n x the largest rectangle of the call, half as much again in hand, never past n whole frames)
static int scene_reserve(se3tn_ctx* c, int n, const se3tn_mesh* const* meshes, const TrackWindow* windows, int H, int W, size_t* maxpx,
                         size_t* d_off) {
  int V, F;
  largest_mesh(meshes, n, &V, &F);
  size_t mx = 0;
  for (int i = 0; i < n; ++i)
    if (!windows[i].miss) mx = std::max(mx, (size_t)windows[i].sw * (size_t)windows[i].sh);
  const size_t need = mx ? (size_t)n * mx : 1, most = (size_t)n * H * W;
  *maxpx = mx;
  *d_off = 64 + (((size_t)n * mx * 3 + 63) & ~(size_t)63);
  if (n <= c->sc_cap && V <= c->sc_V && F <= c->sc_F && need <= c->sc_px) return SE3TN_OK;
  DeviceGuard dg(c->device);
  if (int rc = begin_growth(dg)) return rc;
  c->sc_table_busy = false;   // (the device has been drained)
  if (!c->sc_table_event) HIPCHK(hipEventCreateWithFlags(&c->sc_table_event, hipEventDisableTiming));
  if (n > c->sc_cap || V > c->sc_V || F > c->sc_F) {
    const int cap = n > c->max_batch ? n : c->max_batch;
    V = V > c->sc_V ? V : c->sc_V;
    F = F > c->sc_F ? F : c->sc_F;
    c->sc_cap = 0; c->sc_V = 0; c->sc_F = 0;
    HIPCHK(c->sc_inst_host.alloc((sizeof(RasterInstance) + sizeof(RasterMaterial)) * cap));
    HIPCHK(c->sc_inst_dev.alloc((sizeof(RasterInstance) + sizeof(RasterMaterial)) * cap));
    HIPCHK(c->sc_mo.alloc(V, F, cap));
    c->sc_cap = cap; c->sc_V = V; c->sc_F = F;
  }
  if (need > c->sc_px) {
    const size_t px = std::max(need, std::min(need + need / 2, most));
    c->sc_px = 0;
    HIPCHK(c->sc_sub.alloc(64 + ((px * 3 + 63) & ~(size_t)63) + px * 2 + 64));
    HIPCHK(c->sc_zbuf.alloc(px));
    c->sc_px = px;
  }
  return SE3TN_OK;
}

// render + kernel on `st`; everything has been checked
static int scene_fit_enqueue(se3tn_ctx* c, int n, const std::vector<const se3tn_mesh*>& meshes, const std::vector<TrackWindow>& windows,
                             const double* poses, const double K[9], const uint16_t* depth_dev, int H, int W, int tol_mm,
                             struct se3tn_scene_fit* out, uint8_t* ids, uint16_t* scene, hipStream_t st) {
  size_t maxpx = 0, d_off = 0;
  if (int rc = scene_reserve(c, n, meshes.data(), windows.data(), H, W, &maxpx, &d_off)) return rc;
  if (c->sc_table_busy) {   // the previous call's table may still be on its way up: wait for that copy (not for its launches)
    HIPCHK(hipEventSynchronize(c->sc_table_event));
    c->sc_table_busy = false;
  }
  const RasterHome home{&c->sc_mo, c->sc_inst_host.get(), c->sc_inst_dev.get(), c->sc_sub.get(), c->sc_zbuf.get()};
  int singular = -1;   // (never set in frame mode)
  const int rr = raster_instances(c, n, meshes.data(), poses, K, H, W, windows.data(), true, nullptr, nullptr, maxpx, d_off, st, &singular, &home);
  if (maxpx != 0) {
    HIPCHK(hipEventRecord(c->sc_table_event, st));
    c->sc_table_busy = true;
  }
  if (rr) return rr;
  se3tn_scene_layer layers[SE3TN_SCENE_MAX_OBJECTS];
  for (int i = 0; i < n; ++i) {
    const TrackWindow& t = windows[i];
    layers[i].depth = t.miss ? nullptr : (const uint16_t*)(c->sc_sub.get() + d_off) + (size_t)i * maxpx;
    const int32_t r[4] = {t.x0, t.y0, t.x0 + t.sw, t.y0 + t.sh};
    for (int k = 0; k < 4; ++k) layers[i].rect[k] = t.miss ? 0 : r[k];
  }
  return scene_enqueue(c, n, layers, depth_dev, H, W, tol_mm, out, ids, scene, st);
}

int se3tn_scene_fit(se3tn_ctx* c, int n, const se3tn_object* objs, const double* poses, const double K[9], const uint16_t* depth_dev, int H,
                    int W, int tol_mm, struct se3tn_scene_fit* out_dev, uint8_t* ids_dev, uint16_t* scene_dev, void* stream) {
  const char* who = "se3tn_scene_fit";
  if (!c || !objs || !poses || !K || !depth_dev || !out_dev) return null_argument(who);
  if (int rc = scene_args_check(who, c, n, tol_mm, H, W, true)) return rc;
  std::vector<TrackWindow> windows;
  std::vector<const se3tn_mesh*> meshes;
  if (int rc = scene_windows(who, n, objs, poses, K, H, W, windows, meshes)) return rc;
  if (int rc = refuse_if(stream_is_capturing((hipStream_t)stream), SE3TN_E_STATE, who,
                         "the poses are host arguments, a captured call could not carry new ones: capture se3tn_scene_stats instead")) return rc;
  return scene_fit_enqueue(c, n, meshes, windows, poses, K, depth_dev, H, W, tol_mm, out_dev, ids_dev, scene_dev, (hipStream_t)stream);
}

int se3tn_scene_fit_host(se3tn_ctx* c, int n, const se3tn_object* objs, const double* poses, const double K[9], const uint16_t* depth, int H,
                         int W, int tol_mm, struct se3tn_scene_fit* out, uint8_t* ids, uint16_t* scene, void* stream) {
  const char* who = "se3tn_scene_fit_host";
  if (!c || !objs || !poses || !K || !depth || !out) return null_argument(who);
  if (int rc = scene_args_check(who, c, n, tol_mm, H, W, true)) return rc;
  std::vector<TrackWindow> windows;
  std::vector<const se3tn_mesh*> meshes;
  if (int rc = scene_windows(who, n, objs, poses, K, H, W, windows, meshes)) return rc;
  StagedCall sc{c, who, (hipStream_t)stream};
  if (int rc = sc.refuse_capture()) return rc;
  const SceneStage L = plan_scene_stage(n, H, W, ids != nullptr, scene != nullptr);
  if (int rc = sc.grow(L.total)) return rc;
  std::memcpy(sc.h, depth, L.up_bytes);
  if (int rc = sc.upload(L.up_bytes)) return rc;
  if (int rc = scene_fit_enqueue(c, n, meshes, windows, poses, K, sc.dev<uint16_t>(0), H, W, tol_mm, sc.dev<struct se3tn_scene_fit>(L.rec_off),
                                 ids ? sc.dev<uint8_t>(L.ids_off) : nullptr, scene ? sc.dev<uint16_t>(L.scene_off) : nullptr, sc.st)) {
    (void)hipStreamSynchronize(sc.st);   // (the upload reads the pinned staging: let it end before the next call writes there)
    return rc;
  }
  if (int rc = sc.finish(L.rec_off, L.total - L.rec_off)) return rc;
  std::memcpy(out, sc.h + L.rec_off, sizeof(struct se3tn_scene_fit) * (size_t)n);
  if (ids) std::memcpy(ids, sc.h + L.ids_off, (size_t)H * W);
  if (scene) std::memcpy(scene, sc.h + L.scene_off, (size_t)H * W * 2);
  return SE3TN_OK;
}

// ---- the lattice search among tracked objects: the scene-aware rule -----------------------------------------------------------------------
static_assert(sizeof(se3tn_scene_point_fit) == sizeof(se3tn_point_fit) && offsetof(se3tn_scene_point_fit, inlier_pts) == offsetof(se3tn_point_fit, inlier_pts) &&
                  offsetof(se3tn_scene_point_fit, behind_pts) == offsetof(se3tn_point_fit, behind_pts) &&
                  offsetof(se3tn_scene_point_fit, hidden_pts) == offsetof(se3tn_point_fit, _reserved),
              "the ranking reads scene-aware records through a cast");
static_assert(sizeof(struct se3tn_scene_fit) == PG_OCC_FIT_BYTES, "pose_grid_plan.h lays the occluders' records out");

int se3tn_score_pose_grid_scene(se3tn_ctx* c, const se3tn_points* p, int n_rot, const double* rots_dev, int n_trans, const double* trans_dev,
                                const uint16_t* depth_dev, const uint16_t* scene_dev, int H, int W, const double K[9], int tol_mm, int facing,
                                se3tn_scene_point_fit* fit_dev, void* stream) {
  const char* who = "se3tn_score_pose_grid_scene";
  if (int rc = pose_grid_check(who, c, rots_dev && trans_dev && depth_dev && scene_dev && K && fit_dev, p, n_rot, n_trans, H, W, tol_mm, facing))
    return rc;
  HIPCHK(launch_pose_grid(pose_grid_args(p, rots_dev, n_trans, trans_dev, depth_dev, H, W, K, tol_mm, facing,
                                         reinterpret_cast<se3tn_point_fit*>(fit_dev), scene_dev), n_rot, (hipStream_t)stream));
  return SE3TN_OK;
}

int se3tn_search_pose_grid_scene_host(se3tn_ctx* c, const se3tn_points* p, int n_rot, const double* rots, int n_trans, const double* trans,
                                      const uint16_t* depth, int H, int W, const double K[9], int tol_mm, int facing, int k, int n_occ,
                                      const se3tn_object* occluders, const double* occ_poses, int32_t* idx_out, se3tn_scene_point_fit* fit_out,
                                      struct se3tn_scene_fit* occ_fit_out, void* stream) {
  const char* who = "se3tn_search_pose_grid_scene_host";
  // the numbers and the occluders first, then the context and the handle, then what is read from the caller's arrays
  if (!c || !p || !rots || !trans || !depth || !K || !idx_out || !fit_out || !occluders || !occ_poses) return null_argument(who);
  if (int rc = pose_grid_numbers_check(who, n_rot, n_trans, H, W, tol_mm, facing)) return rc;
  const int n = n_rot * n_trans;
  if (int rc = pose_rank_check(who, n, k)) return rc;
  if (int rc = scene_numbers_check(who, c, n_occ, H, W, true)) return rc;
  std::vector<TrackWindow> windows;
  std::vector<const se3tn_mesh*> meshes;
  if (int rc = scene_windows(who, n_occ, occluders, occ_poses, K, H, W, windows, meshes)) return rc;
  if (int rc = pose_grid_context_check(who, c, p, facing)) return rc;
  StagedCall sc{c, who, (hipStream_t)stream};
  if (int rc = sc.refuse_capture()) return rc;
  if (int rc = finite_check(who, "rotation", rots, nullptr, (size_t)n_rot, 9, 9)) return rc;
  if (int rc = finite_check(who, "translation", trans, nullptr, (size_t)n_trans, 3, 3)) return rc;
  const PgSceneStage s = pg_scene_stage(n_rot, n_trans, H, W, k, n_occ);
  if (int rc = sc.grow(s.bytes)) return rc;
  std::memcpy(sc.h + s.rots, rots, sizeof(double) * 9 * (size_t)n_rot);
  std::memcpy(sc.h + s.trans, trans, sizeof(double) * 3 * (size_t)n_trans);
  std::memcpy(sc.h + s.depth, depth, sizeof(uint16_t) * (size_t)H * (size_t)W);
  if (int rc = sc.upload(s.upload_bytes)) return rc;
  // the occluders rendered and composed against the staged frame: their records, and the scene frame the search reads
  if (int rc = scene_fit_enqueue(c, n_occ, meshes, windows, occ_poses, K, sc.dev<uint16_t>(s.depth), H, W, tol_mm,
                                 sc.dev<struct se3tn_scene_fit>(s.occ_fit), nullptr, sc.dev<uint16_t>(s.scene), sc.st)) {
    (void)hipStreamSynchronize(sc.st);   // (the upload reads the pinned staging: let it end before the next call writes there)
    return rc;
  }
  HIPCHK(launch_pose_grid(pose_grid_args(p, sc.dev<double>(s.rots), n_trans, sc.dev<double>(s.trans), sc.dev<uint16_t>(s.depth), H, W, K,
                                         tol_mm, facing, sc.dev<se3tn_point_fit>(s.fit), sc.dev<uint16_t>(s.scene)), n_rot, sc.st));
  HIPCHK(launch_pose_rank(sc.dev<se3tn_point_fit>(s.fit), n, k, sc.dev<int32_t>(s.idx), sc.dev<se3tn_point_fit>(s.top_fit), sc.st));
  if (int rc = sc.finish(s.readback_at, s.readback_bytes)) return rc;
  std::memcpy(fit_out, sc.h + s.top_fit, sizeof(se3tn_scene_point_fit) * (size_t)k);
  std::memcpy(idx_out, sc.h + s.idx, sizeof(int32_t) * (size_t)k);
  if (occ_fit_out) std::memcpy(occ_fit_out, sc.h + s.occ_fit, sizeof(struct se3tn_scene_fit) * (size_t)n_occ);
  c->ps_scene_off = s.scene; c->ps_scene_H = H; c->ps_scene_W = W;
  return SE3TN_OK;
}

int se3tn_last_search_scene(se3tn_ctx* c, const uint16_t** scene_dev, int* H, int* W) {
  const char* who = "se3tn_last_search_scene";
  if (!c || !scene_dev || !H || !W) return null_argument(who);
  if (int rc = refuse_if(c->ps_scene_H < 1, SE3TN_E_STATE, who,
                         "no scene frame: se3tn_search_pose_grid_scene_host has not succeeded, or another _host call has used the staging since")) return rc;
  *scene_dev = reinterpret_cast<const uint16_t*>(c->ps_dev.get() + c->ps_scene_off);
  *H = c->ps_scene_H; *W = c->ps_scene_W;
  return SE3TN_OK;
}

// The network on k <= 5 pairs of (possibly) k models, through the batch 1-5 family chosen EXPLICITLY (InferConfig::small_family) -- not
// through the predicates of a default context: stem + pool in one launch, the four trunk convs (conv64_small), the five 128 ..
// 512-channel convs as channel slices (+ conv_reduce), the tail on the last conv's partial sums.  That is the plan of one pair of a
// default context (tests/c_abi/infer_plan_check.cpp holds the two equal); every kernel of it works image by image in a layer-fixed
// order, and here image i reads its parameters ip.off[i] floats from W.
static int infer_small_objects(se3tn_ctx* c, const float* W, const ImgParams& ip, const float* A, const float* B, int k, float* trans,
                               float* rot, const double* poseA, double* poseB, hipStream_t st) {
  InferConfig cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  fill_config(c, k, true, cfg);
  if (plan_infer(cfg, c->plan) != INFER_PLAN_OK)
    return fail(SE3TN_E_ARG, "se3tn_on_track_objects: the batch 1-5 kernel family has no kernel for a launch of " + std::to_string(k) + " pairs");
  return run_plan(c, cfg, c->plan, W, &ip, A, B, trans, rot, poseA, poseB, st);
}

// se3tn_on_track_objects (live == nullptr) and se3tn_on_track_objects_live: one body, two staging steps
static int on_track_objects_frame(se3tn_ctx* c, int n, const se3tn_object* objs, const double* prev_poses, const double K[9], const uint8_t* rgb,
                                  const uint16_t* depth, int H, int W, const LiveFrame* live, uint8_t* rgbA_dev, uint16_t* depthA_dev,
                                  double* pose_out, float* trans_out, float* rot_out, int32_t* bbox_vu, void* stream) {
  const std::string fn = live ? "se3tn_on_track_objects_live" : "se3tn_on_track_objects";
  if (!c || c->device < 0 || !objs || !prev_poses || !K || !rgb || !depth || H < 1 || W < 1 || !pose_out)
    return fail(SE3TN_E_ARG, fn + ": bad argument");
  if (n < 1 || n > c->max_batch) return fail(SE3TN_E_ARG, fn + ": n outside [1, max_batch]");
  if (live && ((unsigned)live->color_order > 1u || (unsigned)live->blur > 2u)) return fail(SE3TN_E_ARG, fn + ": bad color_order or blur");
  if (c->prec != SE3TN_PREC_F32)
    return fail(SE3TN_E_STATE, fn + ": ctx is in SE3TN_PREC_F16X3 (the batch 1-5 kernel family is float32)");
  if (!c->small_kernels) return fail(SE3TN_E_STATE, fn + ": ctx has the batch 1-5 kernels switched off (se3tn_set_small_kernels)");
  if (c->keep_intermediates) return fail(SE3TN_E_STATE, fn + ": ctx keeps intermediates (se3tn_keep_intermediates)");
  if (stream_is_capturing((hipStream_t)stream)) return fail(SE3TN_E_STATE, fn + ": synchronous call, not capturable");
  c->fit_last_n = 0;
  const std::string who = fn + ": object ";
  std::vector<const se3tn_mesh*> meshes(n > 0 ? n : 0);
  // one rasteriser mode per launch, so one route per call: all objects on SE3TN_ROUTE_WINDOW (vertex-colour meshes) or all on
  // SE3TN_ROUTE_FRAME (meshes with a material: a texture, or a Kd over the vertex colours)
  bool frame_route = false;
  for (int i = 0; i < n; ++i) {
    const se3tn_object& o = objs[i];
    const std::string id = who + std::to_string(i);
    if (!o.mesh) return fail(SE3TN_E_ARG, id + ": null mesh");
    const bool fr = o.mesh->route == SE3TN_ROUTE_FRAME;
    if (!fr && (o.mesh->tex.get() || o.mesh->uv.get()))
      return fail(SE3TN_E_ARG, id + ": textured mesh on SE3TN_ROUTE_WINDOW (the full-frame renderer's route: se3tn_mesh_set_route)");
    if (fr && !o.mesh->has_material)
      return fail(SE3TN_E_ARG, id + ": mesh on SE3TN_ROUTE_FRAME without a material (se3tn_mesh_set_texture: a texture, or a Kd over the vertex colours)");
    if (i == 0) frame_route = fr;
    else if (fr != frame_route)
      return fail(SE3TN_E_ARG, id + ": the call mixes SE3TN_ROUTE_WINDOW and SE3TN_ROUTE_FRAME objects (one rasteriser mode per launch: one route per call)");
    if (!(o.object_width_mm > 0)) return fail(SE3TN_E_ARG, id + ": object width must be > 0");
    const se3tn_ctx* m = o.model;
    if (!m) return fail(SE3TN_E_ARG, id + ": null model");
    if (!m->blob) return fail(SE3TN_E_STATE, id + ": model has no weights (se3tn_upload_weights / se3tn_bind_weights)");
    if (!m->have_norm) return fail(SE3TN_E_STATE, id + ": model has no normalisation (se3tn_set_normalization)");
    if (m->device != c->device) return fail(SE3TN_E_STATE, id + ": model lives on another device than ctx");
    if (m->L.total != c->L.total) return fail(SE3TN_E_STATE, id + ": model's packed size differs from ctx's");
    if (m->offset_rule != c->offset_rule) return fail(SE3TN_E_STATE, id + ": model's offset rule differs from ctx's (se3tn_set_offset_rule)");
    if (m->raster_sub_bits != c->raster_sub_bits) return fail(SE3TN_E_STATE, id + ": model's raster rule differs from ctx's (se3tn_set_raster_rule)");
    if (((uintptr_t)m->blob - (uintptr_t)objs[0].model->blob) % sizeof(float) != 0)
      return fail(SE3TN_E_STATE, id + ": model's weight blob is not float-aligned to the others'");
    meshes[i] = o.mesh;
  }
  if (frame_route && H > 2048)
    return fail(SE3TN_E_ARG, fn + ": frames of more than 2048 rows are not supported on SE3TN_ROUTE_FRAME");
  hipStream_t st = (hipStream_t)stream;
  // pass 1 (host float64): the windows of every object (predict.py:231-235 / :201-206) and its staged sub-image of the frame
  std::vector<TrackWindow> windows(n);
  const size_t norm_off = (((size_t)n * 128) + 255) & ~(size_t)255;              // the poses in front, then mean | std per object
  const size_t win_off = norm_off + ((((size_t)n * 128) + 255) & ~(size_t)255);
  size_t bytes = win_off;
  for (int i = 0; i < n; ++i) {
    const PlanStatus ps = plan_window(prev_poses + 16 * (size_t)i, K, objs[i].object_width_mm, H, W, bytes, windows[i]);
    if (ps == PlanStatus::NOT_IN_FRONT) return fail(SE3TN_E_ARG, who + std::to_string(i) + ": pose is not in front of the camera (z <= 0 or not finite)");
    if (ps == PlanStatus::EMPTY_WINDOW) return fail(SE3TN_E_ARG, who + std::to_string(i) + ": empty crop window");
  }
  // live: colour windows | zero pixel | the whole RAW depth frame, once | (device only) every object's filled depth window (track_plan.h)
  LiveLayout lay{};
  bool fill = false;
  if (live) {
    lay = plan_live(n, windows.data(), H, W, win_off);
    fill = lay.fills > 0 || live->depth_filled;
    bytes = lay.total;
    if (int rc = reserve_fill_depth(c, (size_t)H * W)) return rc;
  }
  if (int rc = reserve_track_batch(c, nullptr, n, bytes)) return rc;
  if (int rc = reserve_objects_raster(c, n, meshes.data())) return rc;
  size_t maxpx = 0, fr_d_off = 0;
  if (frame_route)
    if (int rc = reserve_frame_rects(c, n, windows.data(), H, W, &maxpx, &fr_d_off)) return rc;
  if (c->rearm_counters) {   // (as se3tn_infer: a launch sequence that failed half-way may have left the tail's counters non-zero)
    HIPCHK(hipMemsetAsync(c->tail_arrive.get(), 0, sizeof(int) * c->max_batch, st));
    c->rearm_counters = false;
  }
  // image A of all n objects: FOUR launches (grid.y = object), every instance with its own mesh
  uint8_t* rA = rgbA_dev ? rgbA_dev : c->tb_rgbA.get();
  uint16_t* dA = depthA_dev ? depthA_dev : c->tb_depthA.get();
  int singular = -1;
  if (int rc = raster_instances(c, n, meshes.data(), prev_poses, K, H, W, windows.data(), frame_route, rA, dA, maxpx, fr_d_off, st, &singular))
    return singular >= 0 ? fail(SE3TN_E_ARG, who + std::to_string(singular) + ": singular pose") : rc;
  // the poses, every object's mean | std and the frame's n windows: staged through pinned memory while the rasteriser runs, ONE copy
  uint8_t* hp = c->tb_stage_host.get();
  std::memcpy(hp, prev_poses, (size_t)n * 128);
  double* norm_h = (double*)(hp + norm_off);
  for (int i = 0; i < n; ++i) {
    std::memcpy(norm_h + 16 * (size_t)i, objs[i].model->mean, 8 * sizeof(double));
    std::memcpy(norm_h + 16 * (size_t)i + 8, objs[i].model->stdv, 8 * sizeof(double));
  }
  if (live) {
    for (int i = 0; i < n; ++i) stage_window(windows[i], rgb, nullptr, W, hp, live->color_order == SE3TN_COLOR_BGR);
    std::memset(hp + lay.zero_off, 0, 2);
    if (fill) std::memcpy(hp + lay.raw_off, depth, (size_t)H * W * 2);
  } else {
    for (int i = 0; i < n; ++i) stage_window(windows[i], rgb, depth, W, hp);
  }
  StagedUpload up{c->trk_copy_stream};
  if (int rc = upload_staged(c, c->tb_stage_dev.get(), hp, !live ? bytes : fill ? lay.upload_bytes : lay.raw_off, st)) return rc;
  if (fill) {   // predict_ros.py:38-41 ONCE for the frame, then the pixels each object's crop reads (and the whole frame when the caller wants it)
    std::vector<int32_t> rects(4 * (size_t)n, 0);   // (a miss keeps the empty rectangle: skipped)
    std::vector<size_t> offs(n, 0);
    for (int i = 0; i < n; ++i) {
      const TrackWindow& t = windows[i];
      if (t.miss) continue;
      rects[4 * (size_t)i] = t.x0; rects[4 * (size_t)i + 1] = t.y0; rects[4 * (size_t)i + 2] = t.x0 + t.sw; rects[4 * (size_t)i + 3] = t.y0 + t.sh;
      offs[i] = t.off_d / 2;
    }
    if (int rc = fill_depth_rects_enqueue(c, (const uint16_t*)(c->tb_stage_dev.get() + lay.raw_off), H, W, live->max_depth_m, live->extrapolate,
                                          live->blur, n, rects.data(), offs.data(), (uint16_t*)c->tb_stage_dev.get(), live->depth_filled, st))
      return rc;
  }
  // both crops of every object, each normalised with its own model's mean / std (the device table staged above); up to 32 objects
  // (64 descriptors) per launch: images A into inA, images B into inB
  const size_t img_floats = (size_t)IN_P * IN_P * 4;
  int rc = SE3TN_OK;
  for (int g0 = 0; g0 < n && rc == SE3TN_OK; g0 += CropArgs::MAX / 2) {
    const int kg = n - g0 < CropArgs::MAX / 2 ? n - g0 : CropArgs::MAX / 2;
    CropArgs a;
    std::memcpy(a.mean, c->mean, sizeof(a.mean));
    std::memcpy(a.stdv, c->stdv, sizeof(a.stdv));
    for (int j = 0; j < kg; ++j) {
      const int i = g0 + j;
      crop_pair(windows[i], prev_poses[16 * (size_t)i + 11] * 1000, image_a(c, frame_route, i, rA, dA, maxpx, fr_d_off), c->tb_stage_dev.get(),
                a.c[j], a.c[kg + j]);
    }
    // frame route: the crops of image A also leave their raw pixels (crop_bbox of the render = Tracker.render_window) in rgbA_dev /
    // depthA_dev (the one not given goes to the internal buffer)
    if (frame_route && (rgbA_dev || depthA_dev)) {
      a.raw_rgb = rA + (size_t)g0 * RES * RES * 3;
      a.raw_depth = dA + (size_t)g0 * RES * RES;
    }
    a.n = 2 * kg; a.n_first = kg;
    a.out = c->inA.get() + (size_t)g0 * img_floats; a.out2 = c->inB.get() + (size_t)g0 * img_floats; a.padded = 1; a.split = 0;
    a.overflow = c->overflow.get(); a.offset_rule = c->offset_rule;
    a.norm = (const double*)(c->tb_stage_dev.get() + norm_off) + 16 * (size_t)g0;
    if (const hipError_t e = launch_preprocess(a, st)) rc = hipfail(e, "launch_preprocess");
  }
  c->in_split[0] = c->in_split[1] = 0;
  // the network, chunks of at most 5 objects; image j of a chunk reads its model's blob at off[j] floats from the chunk's first blob
  float* trans_d = (float*)(c->tb_out_dev.get() + (size_t)n * 128);
  float* rot_d = trans_d + 3 * (size_t)n;
  for (int i0 = 0; i0 < n && rc == SE3TN_OK; i0 += SE3TN_SLICES_SMALL_MAX_N) {
    const int k = n - i0 < SE3TN_SLICES_SMALL_MAX_N ? n - i0 : SE3TN_SLICES_SMALL_MAX_N;
    const float* W0 = objs[i0].model->blob;
    ImgParams ip{};
    for (int j = 0; j < k; ++j) {
      const se3tn_ctx* m = objs[i0 + j].model;
      ip.off[j] = (long long)(((intptr_t)m->blob - (intptr_t)W0) / (intptr_t)sizeof(float));
      ip.tn[j] = m->tn;
      ip.rn[j] = m->rn;
    }
    rc = infer_small_objects(c, W0, ip, c->inA.get() + (size_t)i0 * img_floats, c->inB.get() + (size_t)i0 * img_floats, k, trans_d + 3 * (size_t)i0,
                             rot_d + 3 * (size_t)i0, (const double*)c->tb_stage_dev.get() + 16 * (size_t)i0, (double*)c->tb_out_dev.get() + 16 * (size_t)i0, st);
  }
  if (rc != SE3TN_OK) { c->rearm_counters = true; return rc; }
  if ((rc = read_back_tracks(c, n, st, pose_out, trans_out, rot_out, bbox_vu, windows.data()))) return rc;
  up.done();
  if (c->fit_tol) {
    return fit_check_stage(c, n, meshes.data(), pose_out, K, H, W, windows.data(), frame_route, c->tb_stage_dev.get(), st, fn);
  }
  return SE3TN_OK;
}

int se3tn_on_track_objects(se3tn_ctx* c, int n, const se3tn_object* objs, const double* prev_poses, const double K[9], const uint8_t* rgb,
                           const uint16_t* depth, int H, int W, uint8_t* rgbA_dev, uint16_t* depthA_dev, double* pose_out, float* trans_out,
                           float* rot_out, int32_t* bbox_vu, void* stream) {
  return on_track_objects_frame(c, n, objs, prev_poses, K, rgb, depth, H, W, nullptr, rgbA_dev, depthA_dev, pose_out, trans_out, rot_out,
                                bbox_vu, stream);
}

int se3tn_on_track_objects_live(se3tn_ctx* c, int n, const se3tn_object* objs, const double* prev_poses, const double K[9],
                                const uint8_t* color, int color_order, const uint16_t* depth_raw, int H, int W, double max_depth_m,
                                int extrapolate, int blur, uint16_t* depth_filled_dev, uint8_t* rgbA_dev, uint16_t* depthA_dev,
                                double* pose_out, float* trans_out, float* rot_out, int32_t* bbox_vu, void* stream) {
  const LiveFrame live{color_order, max_depth_m, extrapolate, blur, depth_filled_dev};
  return on_track_objects_frame(c, n, objs, prev_poses, K, color, depth_raw, H, W, &live, rgbA_dev, depthA_dev, pose_out, trans_out, rot_out,
                                bbox_vu, stream);
}

// the scratch of the depth fill as its launches take it (Utils.py:505 cv2.bilateralFilter(depth, 5, 1.5, 2.0))
static FillDepthArgs fill_depth_args(se3tn_ctx* c, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate, int blur) {
  const size_t px = (size_t)H * W;
  FillDepthArgs f{};
  f.depth_mm = depth_mm; f.H = H; f.W = W; f.max_depth = max_depth_m; f.extrapolate = extrapolate; f.blur = blur;
  f.sigma_color = 1.5; f.sigma_space = 2.0;
  f.buf0 = c->fd_buf.get(); f.buf1 = c->fd_buf.get() + px; f.buf2 = c->fd_buf.get() + 2 * px;
  f.minmax = reinterpret_cast<unsigned*>(c->fd_buf.get() + 3 * px);
  f.lut = c->fd_buf.get() + 3 * px + 2;
  return f;
}

int se3tn_fill_depth(se3tn_ctx* c, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate, int blur,
                     uint16_t* out_mm, float* out_m, void* stream) {
  if (!c || c->device < 0 || !depth_mm || H < 1 || W < 1 || (!out_mm && !out_m) || blur < 0 || blur > 2)
    return fail(SE3TN_E_ARG, "se3tn_fill_depth: bad argument");
  const size_t px = (size_t)H * W;
  if (int rc = grow_now_or_refuse(c, "se3tn_fill_depth", true, "frame", px, stream)) return rc;
  FillDepthArgs a = fill_depth_args(c, depth_mm, H, W, max_depth_m, extrapolate, blur);
  a.out_mm = out_mm; a.out_m = out_m;
  HIPCHK(launch_fill_depth(a, (hipStream_t)stream));
  return SE3TN_OK;
}

// comp: the pixels the last pass computes (written to out_full at their place in the frame); sub: the rectangle out_sub holds.
// Both inside the frame and not empty; the scratch is reserved.
static int fill_depth_rect_enqueue(se3tn_ctx* c, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate, int blur,
                                   const int32_t comp[4], uint16_t* out_full, const int32_t sub[4], uint16_t* out_sub, hipStream_t st) {
  FillDepthRectArgs a{};
  a.f = fill_depth_args(c, depth_mm, H, W, max_depth_m, extrapolate, blur);
  a.cx0 = comp[0]; a.cy0 = comp[1]; a.cx1 = comp[2]; a.cy1 = comp[3];
  a.out_full = out_full; a.out_sub = out_sub;
  a.sx0 = sub[0]; a.sy0 = sub[1]; a.sx1 = sub[2]; a.sy1 = sub[3];
  HIPCHK(launch_fill_depth_rect(a, st));
  return SE3TN_OK;
}

int se3tn_fill_depth_rect(se3tn_ctx* c, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate, int blur,
                          const int32_t rect[4], uint16_t* out_mm_sub, void* stream) {
  if (!c || c->device < 0 || !depth_mm || H < 1 || W < 1 || !rect || !out_mm_sub || blur < 0 || blur > 2)
    return fail(SE3TN_E_ARG, "se3tn_fill_depth_rect: bad argument");
  if (rect[2] <= rect[0] || rect[3] <= rect[1]) return fail(SE3TN_E_ARG, "se3tn_fill_depth_rect: empty rectangle");
  if (rect[0] < 0 || rect[1] < 0 || rect[2] > W || rect[3] > H) return fail(SE3TN_E_ARG, "se3tn_fill_depth_rect: rectangle outside the frame");
  const size_t px = (size_t)H * W;
  if (int rc = grow_now_or_refuse(c, "se3tn_fill_depth_rect", true, "frame", px, stream)) return rc;
  return fill_depth_rect_enqueue(c, depth_mm, H, W, max_depth_m, extrapolate, blur, rect, nullptr, rect, out_mm_sub, (hipStream_t)stream);
}

// rects: every one inside the frame or empty; the scratch is reserved
static int fill_depth_rects_enqueue(se3tn_ctx* c, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate, int blur,
                                    int n, const int32_t* rects, const size_t* offs, uint16_t* out_base, uint16_t* out_full, hipStream_t st) {
  FillDepthRectsArgs a{};
  a.f = fill_depth_args(c, depth_mm, H, W, max_depth_m, extrapolate, blur);
  a.n = n; a.rects = rects; a.offs = offs; a.out_base = out_base; a.out_full = out_full;
  HIPCHK(launch_fill_depth_rects(a, st));
  return SE3TN_OK;
}

int se3tn_fill_depth_rects(se3tn_ctx* c, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate, int blur, int n,
                           const int32_t* rects, const size_t* out_offsets, uint16_t* out_mm_base, void* stream) {
  if (!c || c->device < 0 || !depth_mm || H < 1 || W < 1 || n < 1 || !rects || !out_offsets || !out_mm_base || blur < 0 || blur > 2)
    return fail(SE3TN_E_ARG, "se3tn_fill_depth_rects: bad argument");
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const int32_t* r = rects + 4 * (size_t)i;
    if (r[2] <= r[0] || r[3] <= r[1]) continue;   // what se3tn_frame_rect reports for a window that misses the frame: skipped
    if (r[0] < 0 || r[1] < 0 || r[2] > W || r[3] > H)
      return fail(SE3TN_E_ARG, "se3tn_fill_depth_rects: rectangle " + std::to_string(i) + " is not inside the frame");
    any = true;
  }
  if (!any) return SE3TN_OK;
  const size_t px = (size_t)H * W;
  if (int rc = grow_now_or_refuse(c, "se3tn_fill_depth_rects", true, "frame", px, stream)) return rc;
  return fill_depth_rects_enqueue(c, depth_mm, H, W, max_depth_m, extrapolate, blur, n, rects, out_offsets, out_mm_base, nullptr,
                                  (hipStream_t)stream);
}

int se3tn_render_frame(se3tn_ctx* c, se3tn_mesh* m, const double ob_in_cam[16], const double K[9], int W, int H, uint8_t* rgb,
                       uint16_t* depth, void* stream) {
  if (!c || c->device < 0 || !m || !ob_in_cam || !K || !rgb || !depth || W < 1 || H < 1)
    return fail(SE3TN_E_ARG, "se3tn_render_frame: bad argument");
  const size_t px = (size_t)W * H;
  if (int rc = grow_now_or_refuse(c, "se3tn_render_frame", false, "frame", px, stream)) return rc;
  if (H > 2048) return fail(SE3TN_E_ARG, "se3tn_render_frame: frames of more than 2048 rows are not supported");
  RasterArgs a{};
  raster_common(a, c, m, rgb, depth);
  frame_uniforms(a, m, ob_in_cam, K, W, H);
  HIPCHK(launch_raster(a, (hipStream_t)stream));
  return SE3TN_OK;
}

int se3tn_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  if (!dst || !src) return fail(SE3TN_E_ARG, "se3tn_memcpy_d2d: null pointer");
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SE3TN_OK;
}

int se3tn_profile_enable(se3tn_ctx* c, int slots) {
  if (!c || c->device < 0 || slots < 0 || slots > MAX_SLOTS) return fail(SE3TN_E_ARG, "se3tn_profile_enable: bad argument");
  for (int s = c->slots; s < slots; ++s) {
    for (auto& e : c->evs[s]) HIPCHK(hipEventCreate(&e));
    c->slot_launches[s] = 0;
    c->slots = s + 1;
  }
  c->prof = slots > 0;
  c->infer_count = 0;
  for (int s = 0; s < c->slots; ++s) c->slot_launches[s] = 0;
  return SE3TN_OK;
}

int se3tn_profile_read(se3tn_ctx* c, int slot, float* conv_ms, int* conv_launches, float* total_ms) {
  if (!c || slot < 0 || slot >= c->slots || c->slot_launches[slot] == 0)
    return fail(SE3TN_E_STATE, "se3tn_profile_read: nothing recorded in this slot");
  const int nl = c->slot_launches[slot];
  hipEvent_t* ev = c->evs[slot];
  HIPCHK(hipEventSynchronize(ev[nl]));
  float conv = 0.f, tot = 0.f;
  int nconv = 0;
  for (int i = 0; i < nl; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
    tot += ms;
    if (c->is_conv[i]) { conv += ms; ++nconv; }
  }
  if (conv_ms) *conv_ms = conv;
  if (conv_launches) *conv_launches = nconv;
  if (total_ms) *total_ms = tot;
  return SE3TN_OK;
}

int se3tn_profile_launches(se3tn_ctx* c, int slot, int cap, const char** names, float* ms) {
  if (!c || slot < 0 || slot >= c->slots || c->slot_launches[slot] == 0) {
    fail(SE3TN_E_STATE, "se3tn_profile_launches: nothing recorded in this slot");
    return 0;
  }
  const int nl = c->slot_launches[slot];
  hipEvent_t* ev = c->evs[slot];
  if (hipEventSynchronize(ev[nl]) != hipSuccess) return 0;
  int k = nl < cap ? nl : cap;
  for (int i = 0; i < k; ++i) {
    if (names) names[i] = c->names[i];
    if (ms && hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess) return 0;
  }
  return k;
}

// ---- host-side float64 pieces -----------------------------------------------------------------

int se3tn_compute_bbox(const double pose[16], const double K[9], double width, int32_t out_vu[8]) {
  if (!pose || !K || !out_vu) return fail(SE3TN_E_ARG, "se3tn_compute_bbox: bad argument");
  // Utils.py:302-316 with scale=(1000,1000,1000)
  const double x = pose[3] * 1000, y = pose[7] * 1000, z = pose[11] * 1000, off = width / 2;
  const double px[4] = {x - off, x - off, x + off, x + off};
  const double py[4] = {y - off, y + off, y - off, y + off};
  for (int i = 0; i < 4; ++i) {
    const double u = px[i] * K[0] / z + K[2];
    const double v = py[i] * K[4] / z + K[5];
    out_vu[2 * i + 0] = (int32_t)round_half_even(v);
    out_vu[2 * i + 1] = (int32_t)round_half_even(u);
  }
  return SE3TN_OK;
}

int se3tn_frame_rect(const double pose[16], const double K[9], double width, int H, int W, int32_t rect[4]) {
  if (!pose || !K || !rect || H < 1 || W < 1 || !(width > 0)) return fail(SE3TN_E_ARG, "se3tn_frame_rect: bad argument");
  int32_t win[4];
  if (!(pose[11] > 0) || !std::isfinite(pose[3]) || !std::isfinite(pose[7]) || !std::isfinite(pose[11]) ||
      !bbox_window(pose, K, width, 1000.0, win, nullptr))
    return fail(SE3TN_E_ARG, "se3tn_frame_rect: pose is not in front of the camera (z <= 0 or not finite)");
  if (win[2] <= win[0] || win[3] <= win[1]) return fail(SE3TN_E_ARG, "se3tn_frame_rect: empty crop window");
  (void)window_rect(win, H, W, rect);
  return SE3TN_OK;
}

int se3tn_pose_update_host(const double A[16], const float trans[3], const float rot[3], double tn, double rn,
                           double B[16]) {
  if (!A || !trans || !rot || !B) return fail(SE3TN_E_ARG, "se3tn_pose_update_host: bad argument");
  const float tf = (float)tn, rf = (float)rn;
  const volatile float t0 = trans[0] * tf, t1 = trans[1] * tf, t2 = trans[2] * tf;
  const volatile float r0 = rot[0] * rf, r1 = rot[1] * rf, r2 = rot[2] * rf;
  const double rx = r0, ry = r1, rz = r2;
  double R[9];
  const double theta = std::sqrt(rx * rx + ry * ry + rz * rz);
  if (theta < 2.220446049250313e-16) {
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  } else {
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
    const double x = rx * it, y = ry * it, z = rz * it;
    const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    const double rxm[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    for (int i = 0; i < 9; ++i) R[i] = c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i] + s * rxm[i];
  }
  for (int i = 0; i < 9; ++i) R[i] = (double)(float)R[i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc += R[i * 3 + k] * A[k * 4 + j];
      B[i * 4 + j] = acc;
    }
  B[3] = (double)t0 + A[3];
  B[7] = (double)t1 + A[7];
  B[11] = (double)t2 + A[11];
  B[12] = B[13] = B[14] = 0.0;
  B[15] = 1.0;
  return SE3TN_OK;
}

// ---- the colour record among tracked objects (the scene-aware rule of fit_rule.h) ---------------------------------------------------
// (down here so that no line of the code above moves: tests/pose_family_limits.py names lines of it)
int se3tn_color_stats_scene(se3tn_ctx* c, const se3tn_crop* model, const se3tn_crop* observed, const se3tn_crop* scene, int n, int tol_mm,
                            se3tn_fit* fit_out_dev, se3tn_color_fit* out_dev, void* stream) {
  const std::string who = "se3tn_color_stats_scene";
  if (!scene) return fail(SE3TN_E_ARG, who + ": bad argument");
  if (int rc = crops_check(who, c, model, observed, n, tol_mm, out_dev, true)) return rc;
  for (int i = 0; i < n; ++i) {
    const se3tn_crop& k = scene[i];
    if (!k.depth) return fail(SE3TN_E_ARG, who + ": scene descriptor " + std::to_string(i) + ": NULL depth");
    if (k.H < 1 || k.W < 1 || k.right <= k.left || k.bottom <= k.top)
      return fail(SE3TN_E_ARG, who + ": scene descriptor " + std::to_string(i) + ": empty image or empty window");
  }
  auto triple = [&](int j, se3tn_crop& m, se3tn_crop& o, se3tn_crop& s) { m = model[j]; o = observed[j]; s = scene[j]; };
  return fit_launches<FitSceneArgs>(c, n, triple, fit_out_dev, out_dev, tol_mm, nullptr, nullptr, (hipStream_t)stream);
}

// the two entry points of verify_poses(): without a scene the plain rule (fit_launches on FitArgs), with one the scene-aware rule -- pose
// j's scene descriptor is the frame-sized scene_dev under the un-shifted window winB of the pose (crop_scene, track_plan.h)
int se3tn_verify_poses_host(se3tn_ctx* c, se3tn_mesh* m, const double* poses, int n, const double K[9], double object_width_mm,
                            const uint8_t* rgb, const uint16_t* depth, int H, int W, int tol_mm, se3tn_fit* fit_out,
                            se3tn_color_fit* color_out, int32_t* bbox_out) {
  return verify_poses("se3tn_verify_poses_host", c, m, poses, n, K, object_width_mm, rgb, depth, nullptr, H, W, tol_mm, fit_out, color_out, bbox_out);
}

int se3tn_verify_poses_scene_host(se3tn_ctx* c, se3tn_mesh* m, const double* poses, int n, const double K[9], double object_width_mm,
                                  const uint8_t* rgb, const uint16_t* depth, const uint16_t* scene_dev, int H, int W, int tol_mm,
                                  se3tn_fit* fit_out, se3tn_color_fit* color_out, int32_t* bbox_out) {
  const char* who = "se3tn_verify_poses_scene_host";
  if (!scene_dev) return null_argument(who);
  return verify_poses(who, c, m, poses, n, K, object_width_mm, rgb, depth, scene_dev, H, W, tol_mm, fit_out, color_out, bbox_out);
}

}  // extern "C"
