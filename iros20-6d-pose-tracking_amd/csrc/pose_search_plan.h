// Rank key, launch geometry and staging layout of the pose search (pose_search.hip, api.cpp: se3tn_score_poses, se3tn_rank_poses,
// se3tn_search_poses_host).  Host and device; no HIP header is needed to read it (tests/c_abi/pose_search_plan_check.cpp runs it on
// the host under sanitizers).
//
// Scoring: one workgroup of PS_THREADS threads per candidate pose (grid.x = n <= PS_MAX_POSES); thread t takes the model points
// t, t + PS_THREADS, ...  Ranking: ONE workgroup of PS_THREADS threads, k rounds over the n keys.
//
// The key of record i of a call orders the candidates: more inliers first, then fewer points the sensor sees through, then the
// lower index.  The three fields do not overlap (20 + 20 bits below the inlier count), so the order of the keys IS the order of
// the tuples (inlier descending, behind ascending, index ascending), and keys are unique within a call because indices are.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/se3tracknet.h"
#include "pose_transform.h"   // SE3TN_PS_HD

namespace se3tn {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_MAX_POSES = SE3TN_POSE_SEARCH_MAX_POSES;
constexpr int PS_RANK_MAX = SE3TN_POSE_RANK_MAX;
constexpr int PS_FIT_WORDS = 8;                          // uint32 words of a se3tn_point_fit
constexpr uint32_t PS_FIELD_MAX = (1u << 20) - 1;        // the largest value of the two 20-bit fields of a key
static_assert(PS_MAX_POSES == (1 << 20), "an index fills the low 20 bits of a key");
static_assert(SE3TN_POSE_ERRORS_MAX_POINTS <= (1 << 20), "an inlier count stays below 2^21: inlier * 2^40 fits 64 bits with room");
static_assert(sizeof(se3tn_point_fit) == 4 * PS_FIT_WORDS, "a record is eight words");

// inlier_pts * 2^40 + (2^20 - 1 - min(behind_pts, 2^20 - 1)) * 2^20 + (2^20 - 1 - index), index < 2^20.  Every record of
// se3tn_score_poses has inlier_pts <= P <= 2^20; a record from elsewhere with more is taken as 2^20 (the sum cannot overflow).
SE3TN_PS_HD inline uint64_t ps_key(uint32_t inlier_pts, uint32_t behind_pts, uint32_t index) {
  const uint64_t in = inlier_pts > PS_FIELD_MAX + 1 ? (uint64_t)PS_FIELD_MAX + 1 : inlier_pts;
  const uint64_t be = behind_pts > PS_FIELD_MAX ? PS_FIELD_MAX : behind_pts;
  return (in << 40) + (((uint64_t)PS_FIELD_MAX - be) << 20) + ((uint64_t)PS_FIELD_MAX - (uint64_t)index);
}
// the inverse: what a key says about its record
SE3TN_PS_HD inline uint32_t ps_key_inliers(uint64_t key) { return (uint32_t)(key >> 40); }
SE3TN_PS_HD inline uint32_t ps_key_behind(uint64_t key) { return PS_FIELD_MAX - (uint32_t)((key >> 20) & PS_FIELD_MAX); }   // clamped count
SE3TN_PS_HD inline uint32_t ps_key_index(uint64_t key) { return PS_FIELD_MAX - (uint32_t)(key & PS_FIELD_MAX); }

// Staging of the synchronous _host entry points of the pose family (api.cpp: StagedCall), in BYTES, pinned host and device mirror
// alike.  Every layout starts with the HEAD [inputs | depth H x W uint16 | pad to 8]: one upload covers [0, upload_bytes), the inputs
// and the frame.  The searches end with the RANK TAIL [fit n records | top_fit k records | idx k int32 | pad to 8]: one read-back
// covers [top_fit, top_fit + k x 36), the records of the k winners, then their indices; the n records before them stay on the device.
SE3TN_PS_HD inline size_t ps_align8(size_t b) { return (b + 7) & ~(size_t)7; }
struct PsHead {
  size_t depth;          // byte offset of the frame: the inputs end here
  size_t upload_bytes;   // from 0
};
// fills the head for `input_bytes` of inputs and returns where the outputs begin
SE3TN_PS_HD inline size_t ps_head(PsHead& s, size_t input_bytes, int H, int W) {
  s.depth = input_bytes;
  s.upload_bytes = s.depth + (size_t)H * (size_t)W * sizeof(uint16_t);
  return ps_align8(s.upload_bytes);
}
struct PsRankTail {
  size_t fit, top_fit, idx;   // byte offsets
  size_t readback_bytes;      // from top_fit
  size_t bytes;               // the whole buffer
};
SE3TN_PS_HD inline void ps_rank_tail(PsRankTail& s, size_t at, size_t n, int k) {
  s.fit = at;
  s.top_fit = s.fit + n * sizeof(se3tn_point_fit);
  s.idx = s.top_fit + (size_t)k * sizeof(se3tn_point_fit);
  s.readback_bytes = (size_t)k * (sizeof(se3tn_point_fit) + sizeof(int32_t));
  s.bytes = ps_align8(s.idx + (size_t)k * sizeof(int32_t));
}

// se3tn_search_poses_host: [poses n x 16 doubles | frame | rank tail]
struct PsStage : PsHead, PsRankTail {
  size_t poses;   // byte offset
};
SE3TN_PS_HD inline PsStage ps_stage(int n, int H, int W, int k) {
  PsStage s;
  s.poses = 0;
  ps_rank_tail(s, ps_head(s, (size_t)n * 16 * sizeof(double), H, W), (size_t)n, k);
  return s;
}

}  // namespace se3tn
