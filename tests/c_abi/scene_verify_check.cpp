// csrc/fit_rule.h on the host, built with AddressSanitizer + UBSan by tests/test_scene_verify_host.py: the scene-aware classifier over
// the boundary set of the rule.  For tol in {1, 10}: every model depth of M, every observed depth of the set around it and every scene
// depth of the set around it go through fit_classify_scene; the counts are printed, one line per tol, and the test compares them with
// the per-pixel loop of tests/scene_verify_oracle.py.  The program itself holds the rule to its invariants:
//   model == hidden + (the pixels fit_classify counts as model without them),  seen == inlier + front + behind,
//   a hidden pixel carries FC_MODEL and FC_HIDDEN and nothing else, and with s = 0 the classifier is fit_classify, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fit_rule.h"

using namespace se3tn;

static void require(bool ok, const char* what, int m, int o, int s, int tol) {
  if (ok) return;
  std::fprintf(stderr, "scene_verify_check: %s fails at m = %d, o = %d, s = %d, tol = %d\n", what, m, o, s, tol);
  std::exit(1);
}

static std::vector<int> around(int m, int tol, bool with_below) {
  std::vector<int> v = {0, 100, 101, 1999, 2000, 65535, m, m + tol, m + tol + 1};
  if (with_below) { v.push_back(m - tol); v.push_back(m - tol - 1); }
  std::vector<int> out;
  for (int d : v)
    if (d >= 0 && d <= 65535) out.push_back(d);   // a depth is a uint16
  return out;
}

int main() {
  const int M[] = {0, 100, 101, 102, 111, 600, 1988, 1989, 1998, 1999, 2000, 65535};
  for (int tol : {1, 10}) {
    unsigned long long cnt[FC_COUNTS + 1] = {0, 0, 0, 0, 0, 0}, sum_abs = 0;
    for (int m : M)
      for (int o : around(m, tol, true))
        for (int s : around(m, tol, false)) {
          unsigned ad = 77u, ad0 = 77u, ad1 = 77u;
          const unsigned bits = fit_classify_scene(m, o, s, tol, ad);
          const unsigned plain = fit_classify(m, o, tol, ad0);
          require(fit_classify_scene(m, o, 0, tol, ad1) == plain && ad1 == ad0, "s = 0 is fit_classify", m, o, s, tol);
          const bool hid = (bits >> FC_HIDDEN) & 1u;
          require(hid == fit_hidden(m, s, tol), "the hidden bit is fit_hidden", m, o, s, tol);
          if (hid) require(bits == ((1u << FC_MODEL) | (1u << FC_HIDDEN)) && ad == 0u, "hidden enters model and hidden only", m, o, s, tol);
          else require(bits == plain && ad == ad0, "not hidden: as fit_classify", m, o, s, tol);
          require(((bits >> FC_MODEL) & 1u) == (unsigned)depth_valid(m), "model is valid(m)", m, o, s, tol);
          const unsigned parts = ((bits >> FC_INLIER) & 1u) + ((bits >> FC_FRONT) & 1u) + ((bits >> FC_BEHIND) & 1u);
          require(parts == ((bits >> FC_SEEN) & 1u), "seen == inlier + front + behind", m, o, s, tol);
          require(ad == 0u || ((bits >> FC_INLIER) & 1u), "|o - m| of inliers only", m, o, s, tol);
          for (int k = 0; k <= FC_COUNTS; ++k) cnt[k] += (bits >> k) & 1u;
          sum_abs += ad;
        }
    std::printf("tol=%d model_px=%llu seen_px=%llu inlier_px=%llu front_px=%llu behind_px=%llu sum_abs_mm=%llu hidden_px=%llu\n", tol, cnt[FC_MODEL],
                cnt[FC_SEEN], cnt[FC_INLIER], cnt[FC_FRONT], cnt[FC_BEHIND], sum_abs, cnt[FC_HIDDEN]);
  }
  std::printf("scene_verify_check: ok\n");
  return 0;
}
