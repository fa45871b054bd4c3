// Tiling, index arithmetic, LDS layout and staging layout of the product-lattice pose search (pose_grid.hip, api.cpp:
// se3tn_score_pose_grid, se3tn_search_pose_grid_host, and their scene-aware counterparts se3tn_score_pose_grid_scene,
// se3tn_search_pose_grid_scene_host).  Host and device; no HIP header is needed to read it (tests/c_abi/pose_grid_plan_check.cpp and
// tests/c_abi/scene_search_check.cpp run it on the host under sanitizers).
//
// Candidate i = r * n_trans + t is the pose [R_r | t_t].  One workgroup of PG_THREADS threads scores one rotation against one tile
// of PG_TT translations: workgroup b of the one-dimensional grid has rotation b / tiles and translation tile b % tiles, tiles =
// ceil(n_trans / PG_TT).  (One dimension, not (tiles, n_rot): n_rot may reach 2^20 and a grid's y extent ends at 65,535; the product
// n_rot * tiles <= n_rot * n_trans <= 2^20 always fits x.)  The workgroup walks the model in tiles of PG_PT points: all threads
// rotate a tile into LDS, then wave w takes the translations w, w + PG_WAVES, ... of its tile and its lanes the points lane,
// lane + 64, ... of the point tile.  A translation belongs to ONE wave, so its row of counters in LDS has one writer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pose_search_plan.h"

namespace se3tn {

constexpr int PG_THREADS = 256;
constexpr int PG_WAVES = PG_THREADS / 64;
constexpr int PG_PT = 1024;        // model points rotated into LDS at a time
constexpr int PG_TT = 16;          // translations per workgroup: PG_TT / PG_WAVES per wave
constexpr int PG_ROW_WORDS = 6;    // counters of one translation: points (facing) | in frame, seen, inlier, front, behind
static_assert(PG_TT % PG_WAVES == 0, "every wave walks the same number of translations of a full tile");
static_assert(PG_TT * PG_ROW_WORDS <= PG_THREADS && PG_TT * PS_FIT_WORDS <= PG_THREADS, "one thread per counter / record word");

SE3TN_PS_HD inline int pg_tiles(int n_trans) { return (n_trans + PG_TT - 1) / PG_TT; }           // translation tiles per rotation
SE3TN_PS_HD inline int pg_point_tiles(int P) { return (P + PG_PT - 1) / PG_PT; }
SE3TN_PS_HD inline long long pg_grid(int n_rot, int n_trans) { return (long long)n_rot * pg_tiles(n_trans); }
// workgroup b: its rotation, the first translation of its tile and how many translations the tile holds
SE3TN_PS_HD inline int pg_rot_of(int b, int n_trans) { return b / pg_tiles(n_trans); }
SE3TN_PS_HD inline int pg_trans0_of(int b, int n_trans) { return (b % pg_tiles(n_trans)) * PG_TT; }
SE3TN_PS_HD inline int pg_trans_count(int t0, int n_trans) { return n_trans - t0 < PG_TT ? n_trans - t0 : PG_TT; }
SE3TN_PS_HD inline int pg_point_count(int p0, int P) { return P - p0 < PG_PT ? P - p0 : PG_PT; }
// the wave that owns translation k of a tile (k < PG_TT)
SE3TN_PS_HD inline int pg_wave_of(int k) { return k % PG_WAVES; }
SE3TN_PS_HD inline size_t pg_candidate(int r, int t, int n_trans) { return (size_t)r * (size_t)n_trans + (size_t)t; }

// LDS of a workgroup, in BYTES: [planes x PG_PT doubles | PG_TT rows of PG_ROW_WORDS uint32].  planes = 3 (qx | qy | qz of the
// rotated points, each plane contiguous: lane l reads double l of a run of 64, no bank conflict) or 6 with `facing` (the rotated
// normals n'x | n'y | n'z behind them).  24,960 / 49,536 bytes: six / three workgroups share a CU's 160 KiB.
SE3TN_PS_HD inline int pg_planes(int facing) { return facing ? 6 : 3; }
SE3TN_PS_HD inline size_t pg_lds_rows(int facing) { return (size_t)pg_planes(facing) * PG_PT * sizeof(double); }   // byte offset of the rows
SE3TN_PS_HD inline size_t pg_lds_bytes(int facing) { return pg_lds_rows(facing) + (size_t)PG_TT * PG_ROW_WORDS * sizeof(uint32_t); }
SE3TN_PS_HD inline size_t pg_lds_plane(int plane) { return (size_t)plane * PG_PT * sizeof(double); }               // byte offset of a plane
SE3TN_PS_HD inline size_t pg_lds_row(int facing, int k) { return pg_lds_rows(facing) + (size_t)k * PG_ROW_WORDS * sizeof(uint32_t); }

// The scene-aware instantiation (se3tn_score_pose_grid_scene) keeps a seventh counter, hidden, behind the six: its rows are
// PG_SCENE_ROW_WORDS wide and start where the plain rows start.  25,024 / 49,600 bytes, 64 more than the plain layouts: still six /
// three workgroups per 160 KiB CU, so LDS does not change how many share one.
constexpr int PG_SCENE_ROW_WORDS = 7;   // points (facing) | in frame, seen, inlier, front, behind | hidden
constexpr int PG_SCENE_HIDDEN = 6;      // the row word of hidden; record word 7
static_assert(PG_TT * PG_SCENE_ROW_WORDS <= PG_THREADS, "one thread per counter");
SE3TN_PS_HD inline int pg_row_words(int scene) { return scene ? PG_SCENE_ROW_WORDS : PG_ROW_WORDS; }
SE3TN_PS_HD inline size_t pg_scene_lds_bytes(int facing) { return pg_lds_rows(facing) + (size_t)PG_TT * PG_SCENE_ROW_WORDS * sizeof(uint32_t); }
SE3TN_PS_HD inline size_t pg_scene_lds_row(int facing, int k) { return pg_lds_rows(facing) + (size_t)k * PG_SCENE_ROW_WORDS * sizeof(uint32_t); }

// Staging of se3tn_search_pose_grid_host (pose_search_plan.h has the head and the rank tail):
//   [rots n_rot x 9 doubles | trans n_trans x 3 doubles | frame | rank tail of n = n_rot * n_trans records]
struct PgStage : PsHead, PsRankTail {
  size_t rots, trans;   // byte offsets
};
SE3TN_PS_HD inline PgStage pg_stage(int n_rot, int n_trans, int H, int W, int k) {
  PgStage s;
  s.rots = 0;
  s.trans = (size_t)n_rot * 9 * sizeof(double);
  ps_rank_tail(s, ps_head(s, s.trans + (size_t)n_trans * 3 * sizeof(double), H, W), (size_t)n_rot * (size_t)n_trans, k);
  return s;
}

// Staging of se3tn_search_pose_grid_scene_host:
//   [rots | trans | frame | pad to 8 | scene H x W uint16 | pad to 8 | fit n records | occ_fit n_occ x PG_OCC_FIT_BYTES | top_fit k | idx k | pad to 8]
// The upload is the head, [0, upload_bytes), as above; the scene frame is composed on the device and stays there; the occluders'
// records lie between the n records and the winners' so that ONE read-back, [readback_at, readback_at + readback_bytes), brings
// them, the k records and the k indices.
constexpr size_t PG_OCC_FIT_BYTES = 48;   // a struct se3tn_scene_fit (api.cpp holds the two equal)
struct PgSceneStage : PsHead, PsRankTail {
  size_t rots, trans, scene, occ_fit;   // byte offsets
  size_t readback_at;                   // == occ_fit; readback_bytes counts from here
};
SE3TN_PS_HD inline PgSceneStage pg_scene_stage(int n_rot, int n_trans, int H, int W, int k, int n_occ) {
  PgSceneStage s;
  const size_t n = (size_t)n_rot * (size_t)n_trans;
  s.rots = 0;
  s.trans = (size_t)n_rot * 9 * sizeof(double);
  s.scene = ps_head(s, s.trans + (size_t)n_trans * 3 * sizeof(double), H, W);
  s.fit = ps_align8(s.scene + (size_t)H * (size_t)W * sizeof(uint16_t));
  s.occ_fit = s.fit + n * sizeof(se3tn_point_fit);
  s.top_fit = s.occ_fit + (size_t)n_occ * PG_OCC_FIT_BYTES;
  s.idx = s.top_fit + (size_t)k * sizeof(se3tn_point_fit);
  s.readback_at = s.occ_fit;
  s.readback_bytes = (size_t)n_occ * PG_OCC_FIT_BYTES + (size_t)k * (sizeof(se3tn_point_fit) + sizeof(int32_t));
  s.bytes = ps_align8(s.idx + (size_t)k * sizeof(int32_t));
  return s;
}

}  // namespace se3tn
