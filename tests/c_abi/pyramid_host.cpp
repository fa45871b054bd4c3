// Host-only program around se3tn_build_mip_pyramid (csrc/tex_pyramid.h), the pyramid se3tn_mesh_set_texture uploads:
//   pyramid_host in.rgb th tw out.bin   ->   int32 levels, uint32 tex_off[16], then the pyramid's bytes
// tests/test_texture_filter_oracle.py compares them with oracle/raster_oracle.py: mip_pyramid.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tex_pyramid.h"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int th = std::atoi(argv[2]), tw = std::atoi(argv[3]);
  if (th < 1 || tw < 1) return 2;
  std::vector<uint8_t> rgb((size_t)th * tw * 3);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size()) return 3;
  std::fclose(f);
  std::vector<uint8_t> pyr;
  unsigned tex_off[SE3TN_TEX_MAX_LEVELS] = {};
  const int32_t levels = se3tn_build_mip_pyramid(rgb.data(), tw, th, pyr, tex_off);
  f = std::fopen(argv[4], "wb");
  if (!f) return 4;
  std::fwrite(&levels, sizeof(levels), 1, f);
  std::fwrite(tex_off, sizeof(unsigned), SE3TN_TEX_MAX_LEVELS, f);
  std::fwrite(pyr.data(), 1, pyr.size(), f);
  std::fclose(f);
  std::printf("levels=%d bytes=%zu\n", (int)levels, pyr.size());
  return 0;
}
