"""(no GPU) The plan of tests/test_gpu_pose_family_limits.py: the sizes at which the pose-search family (score / rank / grid / align /
errors and their _scene and _host forms) is run on the device, up to the largest include/se3tracknet.h admits, and why these.

tests/pose_family_limits.py holds the AUDIT table: every expression of pose_search.hip, pose_grid.hip, pose_align.hip, pose_errors.hip,
record_reduce.h, pose_point_rule.h, the four *_plan.h headers and the launchers and staging code of api.cpp that grows with a size of
the call and is formed in 32 bits, cast, used as a grid extent, packed into a field of the rank key or added into a fixed-width sum,
restated in Python integers with its file:line.  Here
  * every entry is evaluated at the admitted limits and at every size the GPU file runs, and must stay inside its type (grids inside
    HIP's extents): a kernel change that moves a bound fails here, before anything runs at that size;
  * the sizes the table asks for (a dimension at its limit; the frame's element index passing 2^24 and 2^31, its byte offset 2^32)
    must be among the GPU file's;
  * the table is held to the source text: every blockIdx, gridDim, (int) and (unsigned) of the four .hip files and of
    pose_point_rule.h is named by an entry or by the does-not-grow list, and every file:line an entry names exists;
  * narrowing an expression that the source forms in 64 bits must make the table fail at a size the GPU file runs -- what a device
    run of such a build would show, without running one."""
import os
import re

import numpy as np
import pytest

import pose_family_limits as PL
import pose_search_oracle as PSO

ROOT = os.path.join(os.path.dirname(__file__), "..")
CSRC = PL.C
AUDITED = ["pose_search.hip", "pose_grid.hip", "pose_align.hip", "pose_errors.hip", "pose_point_rule.h"]
TABLE_FILES = AUDITED + ["record_reduce.h", "pose_search_plan.h", "pose_grid_plan.h", "pose_align_plan.h", "pose_errors_plan.h",
                         "pose_align_math.h", "api.cpp"]


def lines_of(where):
    """{(path, line)} a `where` string names: "path:12, :14-16; other:3" """
    out, path = set(), None
    for part in re.split(r"[;,]\s*", where):
        m = re.fullmatch(r"(?:(\S+?))?:(\d+)(?:-(\d+))?", part.strip())
        assert m, (where, part)
        path = m.group(1) or path
        lo, hi = int(m.group(2)), int(m.group(3) or m.group(2))
        out |= {(path, n) for n in range(lo, hi + 1)}
    return out


def source(path):
    return open(os.path.join(ROOT, path)).read().split("\n")


def test_limits_are_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    macro = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))   # noqa: E731
    assert PL.LIMITS == dict(P=macro("SE3TN_POSE_ERRORS_MAX_POINTS"), n=macro("SE3TN_POSE_SEARCH_MAX_POSES"), k=macro("SE3TN_POSE_RANK_MAX"),
                             n_align=macro("SE3TN_POSE_ALIGN_MAX_POSES"), iters=macro("SE3TN_POSE_ALIGN_MAX_ITERS"),
                             chunk=macro("SE3TN_POSE_ERRORS_CHUNK"), scene_px=macro("SE3TN_SCENE_MAX_PIXELS"))
    plan = lambda f: open(os.path.join(ROOT, CSRC, f)).read()   # noqa: E731
    for f, name, want in (("pose_search_plan.h", "PS_THREADS", PL.PS_THREADS), ("pose_grid_plan.h", "PG_THREADS", PL.PG_THREADS),
                          ("pose_grid_plan.h", "PG_PT", PL.PG_PT), ("pose_grid_plan.h", "PG_TT", PL.PG_TT),
                          ("pose_errors_plan.h", "PE_THREADS", PL.PE_THREADS), ("pose_errors_plan.h", "PE_REF_TILE", PL.PE_REF_TILE)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, plan(f)).group(1)) == want, name
    assert "#define SE3TN_PA_THREADS 256" in plan("pose_align_plan.h") and "PE_QUERY_TILE = PE_THREADS * PE_QPT" in plan("pose_errors_plan.h")
    assert re.search(r"constexpr int PE_QPT = (\d+);", plan("pose_errors_plan.h")).group(1) == "4"


def test_every_expression_stays_in_its_type_at_the_limits_and_at_the_sizes_run():
    assert PL.evaluate(PL.limit_sizes()) == {}
    assert PL.evaluate(PL.gpu_sizes()) == {}
    # and the sizes run are admitted ones
    L = PL.LIMITS
    for s in PL.gpu_sizes():
        assert 1 <= s["n"] <= L["n"] and 1 <= s["P"] <= L["P"] and s["n_rot"] * s["n_trans"] <= L["n"] and 1 <= s["k"] <= min(L["k"], s["n"])
        assert 1 <= s["n_align"] <= L["n_align"] and 1 <= s["iters"] <= L["iters"] and s["n_err"] >= 1 and s["H"] >= 1 and s["W"] >= 1
    r, t = PL.GRID_REFUSED
    assert r * t > L["n"] and (r - 1, t) in PL.GRID_FACTORS


def test_the_gpu_sizes_contain_the_derived_ones():
    sizes = PL.gpu_sizes()
    lack = [why for why, ok in PL.derived_requirements().items() if not any(ok(s) for s in sizes)]
    assert not lack, lack
    # a list with a case taken out is named
    short = [s for s in sizes if (s["H"], s["W"]) != PL.FRAME_31]
    assert [why for why, ok in PL.derived_requirements().items() if not any(ok(s) for s in short)] == ["frame: element 2^31, byte 2^32"]
    # every other byte offset of the family stays below 2^31 at the limits: no size between the small ones and a limit is asked for
    L = PL.LIMITS
    assert max(L["n"] * 128, L["n"] * 32, L["P"] * 24, L["n_align"] * 224, L["n"] * 72, L["chunk"] * 1024 * 16) < PL.P31


def test_the_table_covers_the_source_text():
    named = set()
    for _, where, _, _ in PL.AUDIT:
        named |= lines_of(where)
    named |= {next(iter(lines_of(w))) for w in PL.DOES_NOT_GROW}
    pat = re.compile(r"blockIdx|gridDim|\(int\)|\(unsigned\)")
    lack = []
    for f in AUDITED:
        for no, text in enumerate(source(CSRC + f), 1):
            code = text.split("//")[0]
            if pat.search(code) and (CSRC + f, no) not in named:
                lack.append("%s:%d: %s" % (f, no, text.strip()))
    assert not lack, "neither in AUDIT nor in DOES_NOT_GROW:\n" + "\n".join(lack)
    # every line the table names exists, lies in a file of the family and is not blank
    for path, no in sorted(named):
        assert path.startswith(CSRC) and path[len(CSRC):] in TABLE_FILES, path
        src = source(path)
        assert 1 <= no <= len(src) and src[no - 1].strip(), (path, no)


# what each entry's line must say: the expression has not moved since it was restated
ANCHORS = {
    "pose_search.hip:26": "blockIdx.x", "pose_search.hip:33": "j += PS_THREADS", "pose_search.hip:69": "+ 1ull", "pose_search.hip:94": "dim3(n)",
    "pose_grid.hip:42": "(int)blockIdx.x", "pose_grid.hip:50": "p0 += PG_PT", "pose_grid.hip:95": "pg_candidate", "pose_grid.hip:104": "(unsigned)pg_grid",
    "pose_grid_plan.h:38": "(size_t)r * (size_t)n_trans", "pose_grid_plan.h:30": "(long long)n_rot", "pose_search_plan.h:35": "(in << 40)",
    "pose_align.hip:35": "blockIdx.x", "pose_align.hip:53": "j += pa_stride()", "pose_align.hip:108": "pose * PA_SUMS", "pose_align_math.h:28": "256.0",
    "pose_errors.hip:36": "blockIdx.y", "pose_errors.hip:98": "blockIdx.x * PE_THREADS", "pose_errors.hip:114": "dim3(tiles, count)",
    "pose_errors_plan.h:38": "(long long)n", "pose_point_rule.h:51": "(size_t)(int)vf * (size_t)f.W + (size_t)(int)uf",
    "api.cpp:442": "int grow(size_t bytes)", "api.cpp:1910": "const int n = n_rot * n_trans", "api.cpp:2548": "const int n = n_rot * n_trans",
}


def test_the_named_lines_say_what_was_restated():
    for where, text in ANCHORS.items():
        f, no = where.split(":")
        assert text in source(CSRC + f)[int(no) - 1], (where, source(CSRC + f)[int(no) - 1])


def entry(what):
    e = [a for a in PL.AUDIT if a[0] == what]
    assert len(e) == 1, what
    return e[0]


def first_bad(value, kind, sizes):
    for s in sizes:
        if not 0 <= value(s) < PL.BOUND[kind]:
            return s
    return None


def test_the_audit_fires_on_narrowed_expressions():
    """Three builds the source does NOT contain, judged on the table instead of on the device:
      * pixel_of's index q formed in int: out of range on the 32,769 x 65,536 frame and on no smaller size run.  Such a build reads
        before the frame there, so it is not run on a device; this is the statement that the FRAME_31 case is what holds the cast;
      * pg_candidate computed in int: r * n_trans + t <= 2^20 - 1 at every admitted grid, so the narrowed form is in range -- an
        int there is equivalent at the sizes the header admits, and no test, old or new, can tell the two builds apart;
      * the `+ 1ull` of the rank key dropped (with the `- 1ull` that undoes it): the key 0 -- no inliers, behind >= 2^20 - 1, index
        2^20 - 1 -- becomes "none yet".  That record is the LAST of 2^20 in the order, winner 2^20 of a call; k <= 64 < n never
        reaches it, so within the admitted k the two builds rank alike.  The convention is exercised by the record being present
        and k = 64 winners all lying above it (test_rank_at_the_field_limits of the GPU file)."""
    sizes = PL.gpu_sizes()
    q = entry("pixel: q = vf * W + uf elements")[3]
    bad = first_bad(q, "int", sizes)
    assert bad is not None and (bad["H"], bad["W"]) == PL.FRAME_31
    assert first_bad(q, "int", [s for s in sizes if (s["H"], s["W"]) != PL.FRAME_31]) is None
    assert first_bad(entry("pixel: depth[q] / scene[q], as bytes")[3], "unsigned", sizes) is not None
    assert q(dict(H=PL.FRAME_25[0], W=PL.FRAME_25[1])) == 2 ** 25 - 1
    cand = entry("grid: pg_candidate r * n_trans + t")[3]
    assert first_bad(cand, "int", sizes + PL.limit_sizes()) is None and max(cand(s) for s in PL.limit_sizes()) == PL.P20 - 1
    # the smallest key is 0 and belongs to index 2^20 - 1 alone; 2^20 - 1 records lie above it
    assert PSO.key(0, PL.P20 - 1, PL.P20 - 1) == 0 and PSO.key(0, 3000000, PL.P20 - 1) == 0 and PSO.key(0, PL.P20 - 1, PL.P20 - 2) == 1
    assert PL.LIMITS["k"] < PL.P20
    # the largest key + 1 fits 64 bits with room, the fields do not overlap
    assert PL.KEY_MAX + 1 < 2 ** 61 and PSO.key(PL.P20, 0, 0) == PL.KEY_MAX
    # the alignment's sums: 2^20 points at the clamp reach 2^60, eight times below the int64 limit; one more doubling of P or of the clamp holds too
    s_max = entry("align: int64 sums at the clamp, 256 * 2^32 per point")[3]
    assert s_max(dict(P=PL.P20)) == 2 ** 60 and s_max(dict(P=8 * PL.P20)) == PL.P63


def test_rank_fast_is_the_oracle_s_rank():
    """the lexsort the GPU file ranks 2^20 records with equals PSO.rank (a Python sort by the tuple) on records drawn from the field
    extremes, ties down to the index included.  inlier_pts above 2^20 -- which se3tn_score_poses never writes -- count as 2^20
    (csrc/pose_search_plan.h ps_key; include/se3tracknet.h): PSO.rank is asked about the clamped records."""
    rng = np.random.default_rng(20)
    for n in (1, 2, 257, 5000):
        fit = np.zeros(n, PSO.DTYPE)
        fit["inlier_pts"] = rng.choice(PL.INLIER_EXTREMES, n)
        fit["behind_pts"] = rng.choice(PL.BEHIND_EXTREMES, n)
        clamped = fit.copy()
        clamped["inlier_pts"] = np.minimum(fit["inlier_pts"], PL.P20)
        for k in sorted({1, min(n, 64), n}):
            assert np.array_equal(PL.rank_fast(clamped["inlier_pts"], fit["behind_pts"], k), PSO.rank(clamped, k)), (n, k)
        order = PSO.rank(clamped, n)
        keys = [PSO.key(clamped["inlier_pts"][i], clamped["behind_pts"][i], i) for i in order]
        assert keys == sorted(keys, reverse=True) and len(set(keys)) == n


@pytest.mark.parametrize("n,pool", [(PL.P20, 64), (4096, 65), (65537, 8), (3, 64), (64, 64)])
def test_slot_assignment(n, pool):
    idx = PL.slot_assignment(n, pool, seed=n)
    assert len(idx) == n and idx.min() >= 0 and idx.max() < pool and idx[0] != idx[-1]
    if n >= pool:
        assert len(set(idx[:pool].tolist())) == pool
    assert np.array_equal(idx, PL.slot_assignment(n, pool, seed=n))
