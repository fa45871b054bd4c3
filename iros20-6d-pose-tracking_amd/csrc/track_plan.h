// Host-only: the float64 / byte arithmetic the one-call tracking bodies of api.cpp share (on_track_frame, se3tn_on_track_batch,
// se3tn_on_track_objects) -- per pair the crop windows, the part of the camera frame that is staged, where it lies in the staging
// buffer and the two crop descriptors.  No HIP in here, so a plain host program can include it (tests/c_abi/track_plan_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/se3tracknet.h"

namespace se3tn {

// np.round: round half to even
inline double round_half_even(double x) { return std::nearbyint(x); }

// Utils.py:302-316 compute_bbox with scale (1000, sy, 1000) -> (left, top, right, bottom) = min / max of the (u, v) corners
// Returns false when a corner is not a finite value inside the int32 range (z == 0, NaN, a pose at the camera centre): the
// float -> int cast would be undefined behaviour.
inline bool bbox_window(const double pose[16], const double K[9], double width, double sy, int32_t win[4], int32_t vu[8]) {
  const double x = pose[3] * 1000, y = pose[7] * sy, z = pose[11] * 1000, off = width / 2;
  const double px[4] = {x - off, x - off, x + off, x + off};
  const double py[4] = {y - off, y + off, y - off, y + off};
  int32_t umin = INT32_MAX, umax = INT32_MIN, vmin = INT32_MAX, vmax = INT32_MIN;
  for (int i = 0; i < 4; ++i) {
    const double uf = round_half_even(px[i] * K[0] / z + K[2]), vf = round_half_even(py[i] * K[4] / z + K[5]);
    if (!(std::fabs(uf) < 1.0e9) || !(std::fabs(vf) < 1.0e9)) return false;   // (also false for NaN)
    const int32_t u = (int32_t)uf, v = (int32_t)vf;
    if (vu) { vu[2 * i] = v; vu[2 * i + 1] = u; }
    umin = u < umin ? u : umin; umax = u > umax ? u : umax;
    vmin = v < vmin ? v : vmin; vmax = v > vmax ? v : vmax;
  }
  win[0] = umin; win[1] = vmin; win[2] = umax; win[3] = vmax;
  return true;
}

// crop window (left, top, right, bottom) intersected with the frame; false: they do not meet (rect = {0, 0, 0, 0})
inline bool window_rect(const int32_t win[4], int H, int W, int32_t rect[4]) {
  const int32_t x0 = win[0] > 0 ? win[0] : 0, x1 = win[2] < W ? win[2] : W;
  const int32_t y0 = win[1] > 0 ? win[1] : 0, y1 = win[3] < H ? win[3] : H;
  if (x1 <= x0 || y1 <= y0) { rect[0] = rect[1] = rect[2] = rect[3] = 0; return false; }
  rect[0] = x0; rect[1] = y0; rect[2] = x1; rect[3] = y1;
  return true;
}

// One (pose, frame) pair of a tracking call
struct TrackWindow {
  int32_t winB[4];      // predict.py:231-235: bbox of the previous pose -> crop window of image B (and of image A on SE3TN_ROUTE_FRAME)
  int32_t winA[4];      // :201-206: the same with the y axis flipped -> the window renderer's window
  int32_t vu[8];        // compute_bbox's corners
  // the part of the frame winB covers, rows / columns [y0, y0 + sh) x [x0, x0 + sw): only this sub-image is staged (and, on
  // SE3TN_ROUTE_FRAME, rendered).  crop_bbox's canvas is zero outside the frame (Utils.py:327-342): outside the sub-image too
  int32_t x0, y0, sw, sh;
  bool miss;            // winB misses the frame: the sub-image is ONE zero pixel that winB does not touch
  size_t off_rgb, off_d;   // byte offsets of the sub-image's rgb / depth in the staging buffer (64-byte aligned)
};

enum class PlanStatus { OK, NOT_IN_FRONT, EMPTY_WINDOW };

// The windows of one pair and its sub-image, placed at `bytes` in the staging buffer (advanced past it).  An object at or behind the
// camera plane has no crop window (the reference's compute_bbox divides by z and its crop comes out empty or mirrored; predict.py never
// gets there): the callers refuse instead of running the frame
inline PlanStatus plan_window(const double pose[16], const double K[9], double width_mm, int H, int W, size_t& bytes, TrackWindow& t) {
  if (!(pose[11] > 0) || !bbox_window(pose, K, width_mm, 1000.0, t.winB, t.vu) || !bbox_window(pose, K, width_mm, -1000.0, t.winA, nullptr))
    return PlanStatus::NOT_IN_FRONT;
  if (t.winB[2] <= t.winB[0] || t.winB[3] <= t.winB[1]) return PlanStatus::EMPTY_WINDOW;
  int32_t r[4];
  t.miss = !window_rect(t.winB, H, W, r);
  if (t.miss) { t.x0 = t.winB[0] - 8; t.y0 = t.winB[1] - 8; t.sw = t.sh = 1; }
  else { t.x0 = r[0]; t.y0 = r[1]; t.sw = r[2] - r[0]; t.sh = r[3] - r[1]; }
  const size_t px = (size_t)t.sw * t.sh;
  t.off_rgb = bytes; bytes += (px * 3 + 63) & ~(size_t)63;
  t.off_d = bytes;   bytes += (px * 2 + 63) & ~(size_t)63;
  return PlanStatus::OK;
}

// The sub-image of frame `rgb` / `depth` ([H,W,3] / [H,W], W columns) into the (pinned) staging buffer: a row-wise gather, or the
// zero pixel of a miss.  depth == nullptr: the rgb part only (the live-camera calls fill their depth on the device).  swap_rb: the
// frame is BGR, the staged pixels are RGB (predict_ros.py:45-46)
inline void stage_window(const TrackWindow& t, const uint8_t* rgb, const uint16_t* depth, int W, uint8_t* host, bool swap_rb = false) {
  uint8_t* h_rgb = host + t.off_rgb;
  uint8_t* h_d = host + t.off_d;
  if (t.miss) { std::memset(h_rgb, 0, 3); if (depth) std::memset(h_d, 0, 2); return; }
  for (int y = 0; y < t.sh; ++y) {
    const uint8_t* src = rgb + ((size_t)(t.y0 + y) * W + t.x0) * 3;
    uint8_t* dst = h_rgb + (size_t)y * t.sw * 3;
    if (swap_rb)
      for (int x = 0; x < t.sw; ++x, src += 3, dst += 3) { dst[0] = src[2]; dst[1] = src[1]; dst[2] = src[0]; }
    else
      std::memcpy(dst, src, (size_t)t.sw * 3);
    if (depth) std::memcpy(h_d + (size_t)y * t.sw * 2, depth + (size_t)(t.y0 + y) * W + t.x0, (size_t)t.sw * 2);
  }
}

// The staging buffer of a live-camera call for n objects of one frame (se3tn_on_track_objects_live), from `begin` (the end of the
// poses and the mean / std table) on:
//   every object's colour window | one zero pixel | the WHOLE raw depth frame, once | every object's FILLED depth window
// The first three travel (up to upload_bytes; up to raw_off when no fill runs); the depth windows exist on the device only, written
// by the n-rectangle pass.  An object whose window misses the frame reads the zero pixel for its depth.  Every region starts on a
// 64-byte boundary.  Re-places off_rgb / off_d of windows that plan_window has planned; crop_pair takes them unchanged.
struct LiveLayout {
  size_t zero_off;       // the zero pixel (64 bytes reserved)
  size_t raw_off;        // the raw depth frame, H * W uint16
  size_t upload_bytes;   // end of the raw frame = end of the upload
  size_t total;          // end of the last depth window = the size the buffers need
  int fills;             // objects whose window meets the frame (= rectangles of the fill)
};
inline LiveLayout plan_live(int n, TrackWindow* t, int H, int W, size_t begin) {
  auto a64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
  LiveLayout L{};
  size_t bytes = a64(begin);
  for (int i = 0; i < n; ++i) { t[i].off_rgb = bytes; bytes += a64((size_t)t[i].sw * t[i].sh * 3); }
  L.zero_off = bytes; bytes += 64;
  L.raw_off = bytes;
  L.upload_bytes = L.raw_off + (size_t)H * W * 2;
  bytes = a64(L.upload_bytes);
  for (int i = 0; i < n; ++i) {
    if (t[i].miss) { t[i].off_d = L.zero_off; continue; }
    t[i].off_d = bytes; bytes += a64((size_t)t[i].sw * t[i].sh * 2);
    ++L.fills;
  }
  L.total = bytes;
  return L;
}

// Where a pair's image A lies on the device
struct ImageA {
  const uint8_t* rgb;      // SE3TN_ROUTE_WINDOW: the 176 x 176 render.  SE3TN_ROUTE_FRAME: the rendered rectangle, sw x sh as the
  const uint16_t* depth;   // staged sub-image
  const uint8_t* zero;     // SE3TN_ROUTE_FRAME: 64 zero bytes, the 1 x 1 image A of a miss (rgb at 0, depth at 32); else nullptr
};

// Both crops of a pair (data_augmentation.py:124-189 with poseA's z): image B = the staged sub-image at b_base under winB shifted by the
// sub-image's origin; image A = the whole render, or (SE3TN_ROUTE_FRAME, predict.py:209-213) the rendered rectangle under the SAME window
inline void crop_pair(const TrackWindow& t, double z_mm, const ImageA& A, const uint8_t* b_base, se3tn_crop& ca, se3tn_crop& cb) {
  cb.rgb = b_base + t.off_rgb; cb.depth = (const uint16_t*)(b_base + t.off_d); cb.H = t.sh; cb.W = t.sw;
  cb.left = t.winB[0] - t.x0; cb.top = t.winB[1] - t.y0; cb.right = t.winB[2] - t.x0; cb.bottom = t.winB[3] - t.y0;
  cb.z_offset_mm = z_mm; cb.stats = 1; cb._pad = 0;
  if (A.zero) {
    ca = cb;
    ca.rgb = t.miss ? A.zero : A.rgb; ca.depth = t.miss ? (const uint16_t*)(A.zero + 32) : A.depth;
  } else {
    ca.rgb = A.rgb; ca.depth = A.depth; ca.H = SE3TN_RES; ca.W = SE3TN_RES;
    ca.left = 0; ca.top = 0; ca.right = SE3TN_RES; ca.bottom = SE3TN_RES; ca.z_offset_mm = z_mm; ca._pad = 0;
  }
  ca.stats = 0;
}

// The scene descriptor of a pair (the scene-aware crop records, fit_rule.h): the frame-sized composed depth of the tracked objects,
// device [H,W], under the UN-shifted winB -- the frame position image B's staged sub-image shows under the shifted one
inline void crop_scene(const TrackWindow& t, const uint16_t* scene, int H, int W, se3tn_crop& cs) {
  cs = se3tn_crop{};
  cs.depth = scene; cs.H = H; cs.W = W;
  cs.left = t.winB[0]; cs.top = t.winB[1]; cs.right = t.winB[2]; cs.bottom = t.winB[3];
}

}  // namespace se3tn
