// Launch geometry, LDS layout and staging layout of the pose alignment (pose_align.hip, api.cpp: se3tn_align_poses,
// se3tn_align_poses_host, and their scene-aware counterparts se3tn_align_poses_scene, se3tn_align_poses_scene_host).  Host and
// device; no HIP header is needed to read it (tests/c_abi/pose_align_check.cpp and pose_align_scene_check.cpp run it on the host
// under sanitizers).
//
// One workgroup of PA_THREADS threads serves one pose through ALL its iterations (grid.x = n <= PA_MAX_POSES): thread t takes the
// model points t, t + PA_THREADS, ... and keeps the 28 int64 sums and the two counts in registers; wave64 xor shuffles, then lane 0
// of each wave stores its PA_ROW_WORDS words into the wave's row of LDS; after a barrier thread w < PA_ROW_WORDS adds word w of the
// PA_WAVES rows; after another barrier thread 0 solves, updates the pose in LDS and sets the `done` word; a third barrier, and every
// thread reads the new pose.  No other workgroup is involved at any point.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pose_search_plan.h"

namespace se3tn {

// 256 threads: 8 poses x 2,620 points x 20 iterations take 423 us, with 1,024 (-DSE3TN_PA_THREADS=1024 builds that variant) 681 us --
// its register ceiling of 128 spills the solve to scratch and its barriers and cross-wave sum span 16 waves (profiles/EXPERIMENTS.md
// item 83)
#ifndef SE3TN_PA_THREADS
#define SE3TN_PA_THREADS 256
#endif
constexpr int PA_THREADS = SE3TN_PA_THREADS;
constexpr int PA_WAVES = PA_THREADS / 64;
constexpr int PA_MAX_POSES = SE3TN_POSE_ALIGN_MAX_POSES;
constexpr int PA_MAX_ITERS = SE3TN_POSE_ALIGN_MAX_ITERS;
constexpr int PA_ROW_WORDS = SE3TN_POSE_ALIGN_SUMS + 2;   // int64 words a wave hands over: the 28 sums | pairs | facing points
constexpr int PA_W_PAIRS = SE3TN_POSE_ALIGN_SUMS, PA_W_FACING = SE3TN_POSE_ALIGN_SUMS + 1;
static_assert(PA_THREADS == 256 || PA_THREADS == 1024, "a multiple of the wave, at most a workgroup");
static_assert(PA_ROW_WORDS <= PA_THREADS, "one thread per word of the cross-wave sum");
static_assert(sizeof(se3tn_align_rec) == 40 && sizeof(se3tn_align_params) == 32, "the records of include/se3tracknet.h");

// the points of thread t: pa_first(t), + PA_THREADS, ... < P
SE3TN_PS_HD inline int pa_first(int t) { return t; }
SE3TN_PS_HD inline int pa_stride() { return PA_THREADS; }
SE3TN_PS_HD inline int pa_count(int t, int P) { return t < P ? (P - t + PA_THREADS - 1) / PA_THREADS : 0; }

// LDS of a workgroup, in int64 WORDS: [PA_WAVES rows of PA_ROW_WORDS | PA_ROW_WORDS totals]; the pose (12 doubles) and the done
// word are separate statics of the kernel
SE3TN_PS_HD inline int pa_lds_row(int wave) { return wave * PA_ROW_WORDS; }
SE3TN_PS_HD inline int pa_lds_total() { return PA_WAVES * PA_ROW_WORDS; }
SE3TN_PS_HD inline int pa_lds_words() { return (PA_WAVES + 1) * PA_ROW_WORDS; }

// The scene-aware instantiation (se3tn_align_poses_scene) keeps a third count, hidden, behind the two: a wave hands over
// PA_SCENE_ROW_WORDS words, and the rows and the totals are laid out as above with that width (1,240 bytes instead of 1,200).
constexpr int PA_SCENE_ROW_WORDS = SE3TN_POSE_ALIGN_SUMS + 3;   // the 28 sums | pairs | facing points | hidden points
constexpr int PA_W_HIDDEN = SE3TN_POSE_ALIGN_SUMS + 2;
static_assert(PA_SCENE_ROW_WORDS <= PA_THREADS, "one thread per word of the cross-wave sum");
static_assert(sizeof(se3tn_scene_align_rec) == 40, "the record of include/se3tracknet.h");
SE3TN_PS_HD inline int pa_row_words(int scene) { return scene ? PA_SCENE_ROW_WORDS : PA_ROW_WORDS; }
SE3TN_PS_HD inline int pa_scene_lds_row(int wave) { return wave * PA_SCENE_ROW_WORDS; }
SE3TN_PS_HD inline int pa_scene_lds_total() { return PA_WAVES * PA_SCENE_ROW_WORDS; }
SE3TN_PS_HD inline int pa_scene_lds_words() { return (PA_WAVES + 1) * PA_SCENE_ROW_WORDS; }

// Staging of se3tn_align_poses_host (pose_search_plan.h has the head):
//   [poses n x 16 doubles | frame | poses_out n x 16 doubles | rec n x 40 | sums n x 28 int64]
// One read-back covers [poses_out, poses_out + readback_bytes): the poses and the records, and the sums when they were asked for.
struct PaStage : PsHead {
  size_t poses, poses_out, rec, sums;   // byte offsets
  size_t readback_bytes;                // from poses_out
  size_t bytes;                         // the whole buffer
};
SE3TN_PS_HD inline PaStage pa_stage(int n, int H, int W, int with_sums) {
  PaStage s;
  s.poses = 0;
  s.poses_out = ps_head(s, (size_t)n * 16 * sizeof(double), H, W);
  s.rec = s.poses_out + (size_t)n * 16 * sizeof(double);
  s.sums = s.rec + (size_t)n * sizeof(se3tn_align_rec);
  s.readback_bytes = (s.sums - s.poses_out) + (with_sums ? (size_t)n * SE3TN_POSE_ALIGN_SUMS * sizeof(int64_t) : 0);
  s.bytes = s.sums + (size_t)n * SE3TN_POSE_ALIGN_SUMS * sizeof(int64_t);
  return s;
}

// Staging of se3tn_align_poses_scene_host:
//   [poses n x 16 doubles | frame | pad to 8 | scene H x W uint16 | pad to 8 | poses_out n x 16 doubles | rec n x 40 | sums n x 28 int64]
// The scene frame is an input here: ONE upload covers [0, upload_bytes), the poses, the frame and the scene; the read-back is as above.
struct PaSceneStage : PaStage {
  size_t scene;   // byte offset
};
SE3TN_PS_HD inline PaSceneStage pa_stage_scene(int n, int H, int W, int with_sums) {
  PaSceneStage s;
  s.poses = 0;
  s.scene = ps_head(s, (size_t)n * 16 * sizeof(double), H, W);
  s.upload_bytes = s.scene + (size_t)H * (size_t)W * sizeof(uint16_t);
  s.poses_out = ps_align8(s.upload_bytes);
  s.rec = s.poses_out + (size_t)n * 16 * sizeof(double);
  s.sums = s.rec + (size_t)n * sizeof(se3tn_scene_align_rec);
  s.readback_bytes = (s.sums - s.poses_out) + (with_sums ? (size_t)n * SE3TN_POSE_ALIGN_SUMS * sizeof(int64_t) : 0);
  s.bytes = s.sums + (size_t)n * SE3TN_POSE_ALIGN_SUMS * sizeof(int64_t);
  return s;
}

}  // namespace se3tn
