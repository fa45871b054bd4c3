// Host-only: the mip pyramid se3tn_mesh_set_texture uploads and raster.hip's sample_bilinear reads.  No HIP in here, so a plain
// host program can include it (tests/c_abi/pyramid_host.cpp compares it with oracle/raster_oracle.py: mip_pyramid).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#define SE3TN_TEX_MAX_LEVELS 16

// 2x2 box filter per level (what glGenerateMipmap implementations do), rounded to nearest; level l is max(tw >> l, 1) x max(th >> l, 1)
// (an odd size drops its last column / row), RGB uint8, levels back to back in `pyr`.  tex_off[l]: byte offset of level l.
// Returns the number of levels.
inline int se3tn_build_mip_pyramid(const uint8_t* rgb, int tw, int th, std::vector<uint8_t>& pyr, unsigned tex_off[SE3TN_TEX_MAX_LEVELS]) {
  pyr.assign(rgb, rgb + (size_t)tw * th * 3);
  int w = tw, h = th, levels = 1;
  size_t off = 0;
  tex_off[0] = 0;
  while ((w > 1 || h > 1) && levels < SE3TN_TEX_MAX_LEVELS) {
    const int nw = w > 1 ? w / 2 : 1, nh = h > 1 ? h / 2 : 1;
    const size_t noff = off + (size_t)w * h * 3;
    pyr.resize(noff + (size_t)nw * nh * 3);
    const uint8_t* src = pyr.data() + off;
    uint8_t* dst = pyr.data() + noff;
    for (int y = 0; y < nh; ++y)
      for (int x = 0; x < nw; ++x)
        for (int ch = 0; ch < 3; ++ch) {
          const int x0 = 2 * x < w ? 2 * x : w - 1, x1 = 2 * x + 1 < w ? 2 * x + 1 : w - 1;
          const int y0 = 2 * y < h ? 2 * y : h - 1, y1 = 2 * y + 1 < h ? 2 * y + 1 : h - 1;
          const int sum = src[((size_t)y0 * w + x0) * 3 + ch] + src[((size_t)y0 * w + x1) * 3 + ch] +
                          src[((size_t)y1 * w + x0) * 3 + ch] + src[((size_t)y1 * w + x1) * 3 + ch];
          dst[((size_t)y * nw + x) * 3 + ch] = (uint8_t)((sum + 2) >> 2);
        }
    tex_off[levels] = (unsigned)noff;
    off = noff; w = nw; h = nh; ++levels;
  }
  return levels;
}
