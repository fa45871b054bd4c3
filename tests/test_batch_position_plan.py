"""(no GPU) The plan of tests/test_gpu_batch_positions.py: which batch sizes it runs, how it fills a call's slots, and why.

The batch size n is the only free shape of the network kernels.  RULES restates, in plain Python, every launch-time selection that is a
function of n -- each with the file:line it restates -- per configuration of the position sweep.  A rule maps n to a value (a kernel, a
tile shape, a strip length, a number of persistent rounds).  The tests assert that the size list of a configuration
  * holds n - 1 and n wherever a rule's value changes between them (both neighbours of every switch in 6..256),
  * reaches every value a rule takes in 6..256,
  * (default configuration) holds every residue of n mod 8 and n mod 10 above 72 -- the max-pool's `n / 8 * 8` remap and
    fc_finish_kernel's ten pairs per workgroup -- and a fixed list of named sizes (NAMED),
and that the seeded slot assignment puts different pool pairs `d` slots apart for every d up to 64.
A kernel pull request that moves a switch edits the rule here; the size lists follow from the failing assertion."""
import numpy as np
import pytest

CUS = 256                       # compute units of an MI355X (se3tn_ctx::num_cus)
LO, HI = 6, 256                 # the sweep: above the batch 1-5 kernel family, up to what bench.py's sweep runs
POOL = 12                       # pool pairs with float64 references
PART_BYTES = 16 * 1024 * 121 * 16 * 4   # csrc/api.cpp:412 (split-K workspace)
S2, S3, S4 = 44, 22, 11         # csrc/se3tn_internal.h:14-16
TILE6_MIN = 14                  # include/se3tracknet.h SE3TN_WINOGRAD_TILE6_MIN_BATCH
CONFIGS = ("default", "keep", "F4", "F6", "direct", "f16x3")


def cdiv(a, b):
    return -(-a // b)


# ---- the selection rules -----------------------------------------------------------------------------------------------------------
def pool_rows(n):
    """csrc/stem7x7_mfma.hip:355 pool_rows: the longest strip that still gives 256 workgroups"""
    for r in (44, 22, 11, 4, 2, 1):
        if n * (S2 // r) >= 256:
            return r
    return 1


def pool_remap(n):
    """csrc/stem7x7_mfma.hip:309 maxpool3x3s2_kernel: images below n / 8 * 8 are remapped image = 8 k + xcd, the n % 8 behind them not"""
    return "tail images" if n % 8 else "all remapped"


def stem_grid(n):
    """csrc/stem7x7_mfma.hip:269 launch_stem: min(31 n, 128) persistent workgroups per branch"""
    return min(31 * n, 128)


def trunk_fused(n, groups, tmin=8, tfill=55):
    """csrc/infer_plan.h wino64_pays: the fused F(2x2) trunk kernel where the rounds of its 4 n groups workgroups are tfill % full"""
    if tmin <= 0 or n < tmin:
        return False
    wgs = 4 * n * groups
    return 100 * wgs >= tfill * cdiv(wgs, CUS) * CUS


def pick_slices(M, hw, cin, cout, groups, big_rows, bn_big):
    """csrc/infer_plan.h pick_slices (0: the big-tile kernel)"""
    if cdiv(M, big_rows) * (cout // bn_big) * groups >= 200:
        return 0
    bn = 128 if cout >= 128 else 64
    rows = hw if M <= 2 * hw else M
    base = cdiv(rows, 128) * (cout // bn) * groups
    ks, best = cin // 32 * 9, 0
    for sl in range(1, ks + 1):
        if ks % sl or ks // sl < 3:
            continue
        if groups * M * cout * 4 * sl > PART_BYTES:
            break
        if best > 0 and base * sl > 512:
            break
        best = sl
    return best


def direct(n, cin, cout, groups, ho, stride):
    """csrc/infer_plan.h plan_conv above 5 pairs: split-K (slices) | slab (one tile per workgroup | persistent, :732) at
    stride 1 | gather (8 | 4 waves, :758-761) at stride 2; f16x3 takes the 4-wave gather always"""
    M, bn = n * ho * ho, (128 if cout >= 128 else 64)
    sl = pick_slices(M, ho * ho, cin, cout, groups, 256 if stride == 1 else 128, bn)
    if sl:
        return "split-K %d" % sl
    tiles_n = cout // bn
    if stride == 1:
        return "slab persistent" if cdiv(M, 256) * tiles_n * groups > 256 else "slab"
    t256 = cdiv(M, 256) * tiles_n * groups
    return "gather 8" if 200 <= t256 <= 256 else "gather 4"


def direct_f16(n, cin, cout, groups, ho, stride):
    v = direct(n, cin, cout, groups, ho, stride)
    return "gather 4" if v == "gather 8" else v     # launch_gather: MM == MM_F32 only (:760)


def gemm(T, cout, groups, nf, split=False):
    """csrc/infer_plan.h plan_gemm: the persistent 128 x 256 kernel (F(6x6) planes, >= 2 tiles per CU; value: the
    virtual-tile rounds a workgroup walks, :679) | 96- or 128-row tiles, whichever queue is shorter"""
    per_b = (cout // 128) * groups * nf
    q128 = cdiv(cdiv(T, 128) * per_b, 256) * 16
    q96 = cdiv(cdiv(T, 96) * per_b, 256) * 12
    if not split and cout % 256 == 0 and (groups * nf) % 8 == 0 and nf == 64:
        tiles = (cout // 256) * cdiv(T, 128) * groups * nf
        if tiles >= 2 * CUS:
            return "persistent x%d" % cdiv(tiles, CUS // 8 * 8)
    return "96 rows" if q96 < q128 else "128 rows"


def tile(cfg, n, which):
    """csrc/infer_plan.h tile_for (rot_normalizer 5 degrees: AUTO takes F(6x6) for the heads too)"""
    if cfg == "F4" or cfg == "f16x3":
        return 4
    if cfg == "F6":
        return 6
    return 4 if n < TILE6_MIN else 6


def wino_gemm(cfg, n, which):
    t = tile(cfg, n, which)
    hin, cout, groups = ((S3, 256, 1), (S4, 512, 2))[which]
    th = cdiv(hin, t)
    return "F%d %s" % (t, gemm(n * th * th, cout, groups, (t + 2) ** 2, split=cfg == "f16x3"))


def ragged(cfg, n, which):
    """the last row tile of a Winograd GEMM is cut (csrc/wino_mfma.hip:633 mlast) | fits"""
    t = tile(cfg, n, which)
    th = cdiv((S3, S4)[which], t)
    rows = 96 if wino_gemm(cfg, n, which).endswith("96 rows") else 128
    return "ragged" if (n * th * th) % rows else "exact"


def fc_finish_grid(n):
    """csrc/wino_mfma.hip:1236 fc_finish_kernel: ten pairs per workgroup; value: the last workgroup is full | cut"""
    return "full" if n % 10 == 0 else "cut"


def _trunk(cfg, groups):
    if cfg == "direct":
        return lambda n: direct(n, 64, 64, groups, S2, 1)
    if cfg == "f16x3":
        return lambda n: direct_f16(n, 64, 64, groups, S2, 1)
    return lambda n: "fused F(2x2)" if trunk_fused(n, groups) else direct(n, 64, 64, groups, S2, 1)


def rules(cfg):
    """[(name, fn, kind)]: kind "switch" -- both neighbours of every change and every value; "value" -- every value (a property that
    alternates with n, like a ragged last tile: nothing to be on both sides of)"""
    d = direct_f16 if cfg == "f16x3" else direct
    r = [("max-pool strip rows", pool_rows, "switch"),
         ("max-pool remap", pool_remap, "value"),
         ("stem workgroups per branch", stem_grid, "switch"),
         ("trunk A2|B2", _trunk(cfg, 2), "switch"),
         ("trunk B3", _trunk(cfg, 1), "switch"),
         ("convAB1 s2", lambda n: d(n, 128, 256, 1, S3, 2), "switch"),
         ("heads conv1 s2", lambda n: d(n, 256, 1024, 1, S4, 2), "switch")]
    if cfg == "direct":
        r += [("convAB2", lambda n: direct(n, 256, 256, 1, S3, 1), "switch"),
              ("heads conv2", lambda n: direct(n, 512, 512, 2, S4, 1), "switch")]
    else:
        if cfg == "f16x3":    # the 256-channel block stays on the direct f16x3 kernels (csrc/api.cpp:986)
            r += [("convAB2", lambda n: direct_f16(n, 256, 256, 1, S3, 1), "switch")]
        else:
            r += [("convAB2 GEMM", lambda n: wino_gemm(cfg, n, 0), "switch"), ("convAB2 GEMM last tile", lambda n: ragged(cfg, n, 0), "value")]
        r += [("heads GEMM", lambda n: wino_gemm(cfg, n, 1), "switch"), ("heads GEMM last tile", lambda n: ragged(cfg, n, 1), "value"),
              ("fc_finish last workgroup", fc_finish_grid, "value")]
    return r


def switches(fn):
    """[n]: fn(n - 1) != fn(n), LO < n <= HI"""
    return [n for n in range(LO + 1, HI + 1) if fn(n - 1) != fn(n)]


# ---- the size lists ----------------------------------------------------------------------------------------------------------------
NAMED = [6, 7, 11, 12, 13, 14, 15, 23, 24, 56, 57, 63, 65, 70, 71, 100, 127, 128, 129, 131, 133, 190, 254, 255, 256]   # fixed by the specification of the sweep
KEPT = [127, 128, 255, 256]     # in every configuration: the max-pool's 11 | 22 | 44-row strips
_SHARED = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 18, 22, 23, 24, 25, 26, 27, 32, 33, 34, 35, 36, 37, 48, 49, 50, 51, 52, 53, 56, 57, 63, 64,
           65, 67, 68, 70, 71, 96, 97, 127, 128, 129, 160, 161, 192, 193, 224, 225, 255, 256]
# literal lists: test_sizes_cover_the_rules fails when a rule moves, and names the sizes to add
SIZES = {
    "default": sorted(set(_SHARED + NAMED + [250])),     # 250: the one residue mod 8 (2) the others leave out above 72
    "keep": _SHARED,
    # F(4x4) at every n: the 96- | 128-row choice of plan_gemm (csrc/infer_plan.h) alternates 38 (convAB2) + 18 (heads) times up to 256
    "F4": [7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29, 32, 33, 34, 35, 36, 45, 46, 49, 50, 51, 52, 53,
           54, 56, 57, 60, 61, 63, 64, 65, 67, 68, 70, 71, 72, 74, 75, 85, 86, 93, 94, 99, 100, 104, 105, 113, 114, 122, 123, 124, 125, 127,
           128, 130, 131, 138, 139, 141, 142, 143, 149, 150, 160, 161, 163, 164, 170, 171, 174, 175, 178, 179, 184, 185, 188, 189, 192, 193,
           197, 198, 199, 200, 202, 203, 208, 209, 213, 214, 216, 217, 227, 228, 234, 235, 238, 239, 245, 246, 252, 253, 255, 256],
    "F6": _SHARED,
    "direct": [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 22, 23, 24, 25, 26, 27, 33, 34, 50, 51, 52, 53, 63, 64, 67, 68, 127, 128, 255, 256],
    "f16x3": [7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 21, 22, 23, 24, 25, 26, 27, 28, 29, 33, 34, 52, 53, 54, 56, 57, 63, 64, 65, 67, 68, 71,
              72, 85, 86, 113, 114, 127, 128, 138, 139, 142, 143, 170, 171, 184, 185, 192, 193, 199, 200, 202, 203, 227, 228, 255, 256],
}


def slot_assignment(n, seed=0):
    """pool pair of every slot of a call of n pairs: a seeded draw in which neighbouring slots differ, the first min(n, POOL) slots hold
    distinct pairs (every pool pair that fits occurs, a first occurrence is never far from slot 0, the later copies sit at every kind of
    position); redrawn until the shift condition holds (short calls: the few slot pairs of the largest shifts)"""
    for attempt in range(64):
        rng = np.random.default_rng([seed, n, attempt])
        idx = list(rng.permutation(POOL)[:min(n, POOL)])
        while len(idx) < n:
            k = int(rng.integers(POOL))
            if k != idx[-1]:
                idx.append(k)
        idx = np.asarray(idx, dtype=np.int64)
        if shift_condition(idx) == 0:
            return idx
    raise AssertionError("no slot assignment for n = %d" % n)


def other_assignment(idx):
    """the call before the checked one: every slot holds another pool pair"""
    return (idx + 1 + (np.arange(len(idx)) % (POOL - 1))) % POOL


def shift_condition(idx):
    """for every shift d in 1 .. min(n - 1, 64): at least half of the slots j hold another pool pair than slot j + d"""
    n = len(idx)
    for d in range(1, min(n - 1, 64) + 1):
        if 2 * int((idx[:-d] != idx[d:]).sum()) < n - d:
            return d
    return 0


# ---- the assertions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS)
def test_sizes_cover_the_rules(cfg):
    sizes = SIZES[cfg]
    assert sizes == sorted(set(sizes)) and LO <= sizes[0] and sizes[-1] == HI and set(KEPT) <= set(sizes)
    missing = {}
    for name, fn, kind in rules(cfg):
        values = {fn(n) for n in range(LO, HI + 1)}
        reached = {fn(n) for n in sizes}
        if values - reached:
            missing[name + " (values)"] = sorted(values - reached)
        if kind == "switch":
            lack = sorted({m for n in switches(fn) for m in (n - 1, n)} - set(sizes))
            if lack:
                missing[name + " (switch neighbours)"] = lack
    assert not missing, "%s: the size list lacks %s" % (cfg, missing)


def test_default_sizes_hold_the_named_sizes_and_every_residue():
    s = set(SIZES["default"])
    assert set(NAMED) <= s
    above = [n for n in SIZES["default"] if n > 72]
    assert {n % 8 for n in above} == set(range(8)) and {n % 10 for n in above} == set(range(10))
    # what the named pairs are, from the rules
    assert [(pool_rows(a), pool_rows(b)) for a, b in ((11, 12), (23, 24), (63, 64), (127, 128), (255, 256))] == \
        [(1, 2), (2, 4), (4, 11), (11, 22), (22, 44)]
    assert (wino_gemm("default", 56, 0), wino_gemm("default", 57, 0)) == ("F6 96 rows", "F6 persistent x2")
    b3 = _trunk("default", 1)
    assert b3(64) == "fused F(2x2)" and all(b3(n) != "fused F(2x2)" for n in range(65, 71)) and b3(71) == "fused F(2x2)"


def test_rules_agree_with_the_route_table():
    """the rules here and tests/test_gpu_routes.py's `expected` restate the same launch code: they must name the same algorithm family"""
    import test_gpu_routes as RT
    base = dict(wmin=6, tile=RT.TILE_AUTO, tmin=8, tfill=55, small=True, keep=False, f16=False, tn=0.03, rn=5 * RT.DEG, fuse=True,
                tail_parts=True, ovr=[0, 0])
    cfgs = {"default": base, "keep": dict(base, keep=True), "F4": dict(base, tile=4), "F6": dict(base, wmin=1, tile=6),
            "direct": dict(base, wmin=0, tmin=0, tfill=0), "f16x3": dict(base, f16=True)}
    for cfg, c in cfgs.items():
        r = {name: fn for name, fn, _ in rules(cfg)}
        for n in range(LO, HI + 1):
            want = RT.expected(c, n)[0]
            assert (r["trunk A2|B2"](n) == "fused F(2x2)") == (want["trunk1"] == "trunk F2"), (cfg, n)
            assert (r["trunk B3"](n) == "fused F(2x2)") == (want["trunk3"] == "trunk F2"), (cfg, n)
            if "heads GEMM" in r:
                assert want["h2.2"] == r["heads GEMM"](n)[:2] + " block", (cfg, n)
            if "convAB2 GEMM" in r:
                assert want["ab2.1"] == r["convAB2 GEMM"](n)[:2] + " block", (cfg, n)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_slot_assignment_meets_the_shift_condition(cfg):
    for n in SIZES[cfg]:
        idx = slot_assignment(n)
        assert len(idx) == n and 0 <= idx.min() and idx.max() < POOL
        assert len(set(idx[:POOL].tolist())) == min(n, POOL)
        assert (idx[1:] != idx[:-1]).all()
        d = shift_condition(idx)
        assert d == 0, "n = %d: more than half of the slots hold the same pool pair %d slots apart" % (n, d)
        assert (other_assignment(idx) != idx).all()
