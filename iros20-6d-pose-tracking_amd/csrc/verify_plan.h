// Host-only: the staging buffer of se3tn_verify_poses_host (api.cpp), on top of track_plan.h.  The buffer carries the call's RESULTS in
// front -- where se3tn_on_track_batch carries its poses -- and the frame's windows behind them:
//   n se3tn_fit | n se3tn_color_fit | padding to 256 bytes | the windows plan_window places, from `begin` on
// The records are written on the device and read back in one copy of rec_bytes from 0; the upload is one copy from `begin` on.
// No HIP in here, so a plain host program can include it (tests/c_abi/verify_plan_check.cpp).
#pragma once
#include "track_plan.h"

namespace se3tn {

struct VerifyLayout {
  size_t fit_off;     // n se3tn_fit (always 0)
  size_t color_off;   // n se3tn_color_fit, directly behind them
  size_t rec_bytes;   // end of the records = size of the read-back
  size_t begin;       // where the first window may lie: rec_bytes rounded up to 256 bytes (plan_window keeps 64-byte alignment from there)
};

inline VerifyLayout plan_verify(int n) {
  VerifyLayout L{};
  L.fit_off = 0;
  L.color_off = (size_t)n * sizeof(se3tn_fit);
  L.rec_bytes = L.color_off + (size_t)n * sizeof(se3tn_color_fit);
  L.begin = (L.rec_bytes + 255) & ~(size_t)255;
  return L;
}

}  // namespace se3tn
