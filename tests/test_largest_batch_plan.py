"""(no GPU) The plan of tests/test_gpu_largest_batch.py: the batch sizes above the 6 .. 256 sweep, up to the largest max_batch
se3tn_create accepts (SE3TN_MAX_BATCH_LIMIT), and why these and no others.

Every other shape of the network is fixed, so above 256 pairs nothing new happens to a kernel's tile map -- what grows is the SIZE of
whole tensors, and with it every index formed from the base of one.  Three tables, each entry with the file:line it restates:
  * TENSORS: bytes per pair of every tensor a forward pass touches.  LARGE_SIZES[cfg] holds floor(2^31 / B) and the size after it, the
    same pair for 2^32, for every tensor B the configuration's route really writes, inside 257 .. LIMIT, and LIMIT itself;
  * AUDIT: every expression of the network kernels and their launchers that grows with n and is formed in 32 bits, evaluated in Python
    integers at EVERY n of 257 .. LIMIT for the routes that reach it: below 2^31 where it is an `int`, below 2^32 where it is only an
    unsigned byte offset, grids inside HIP's limits.  This is what the limit is derived from: the first n at which an entry breaks
    must be LIMIT + 1.  A kernel change that moves a bound fails here, before anything runs at that size;
  * the selection rules of tests/test_batch_position_plan.py applied to 257 .. LIMIT, reduced to kernel families: the lists reach
    every family that occurs (the 96- | 128-row alternation is held by the 6 .. 256 sweep, its neighbours are not asked for again).
The lists are literal; test_large_sizes_are_the_derived_ones recomputes them and names what a changed buffer shape adds."""
import re

import pytest

import test_batch_position_plan as PLAN

LIMIT = 1982                    # include/se3tracknet.h:61 SE3TN_MAX_BATCH_LIMIT (test_limit_is_the_header_s checks it)
LO, HI = PLAN.HI + 1, LIMIT     # 257 .. 1982
S1, S2, S3, S4 = 88, PLAN.S2, PLAN.S3, PLAN.S4      # csrc/infer_plan.h:17-20
IN_P = 176 + 2 * 3              # csrc/se3tn_internal.h:101-102
CONFIGS = PLAN.CONFIGS
P31, P32 = 2 ** 31, 2 ** 32


def cdiv(a, b):
    return -(-a // b)


# ---- which route a configuration takes above 256 pairs -----------------------------------------------------------------------------
def block_tile(cfg, n, which):
    """Winograd tile of the fused block `which` (0: convAB2, 1: the heads), or 0 where the block runs on the direct kernels
    (csrc/infer_plan.h:212-217 block_fused: never in the `direct` configuration, never the 256-channel block under f16x3)"""
    if cfg == "direct" or (cfg == "f16x3" and which == 0):
        return 0
    return PLAN.tile(cfg, n, which)


def planes_bytes(tile, which):
    """bytes per pair of ONE of the V / M workspaces of a Winograd conv: [groups][nf][T = n th th][C] floats
    (csrc/se3tn_internal.h:149-150; nf, th, T: csrc/api.cpp:838-840; C x groups = 256 | 2 x 512)"""
    hin, ch = ((S3, 256), (S4, 1024))[which]
    return (tile + 2) ** 2 * cdiv(hin, tile) ** 2 * ch * 4


# name -> (bytes per pair, what it restates, written(cfg, n))
always = lambda cfg, n: True
TENSORS = {
    "inA / inB": (IN_P * IN_P * 4 * 4, "csrc/api.cpp:502-503 (mb IN_P + slack rows) IN_P 4", always),
    "stem": (S1 * S1 * 128 * 4, "csrc/api.cpp:504 mb S1 S1 128", always),
    "pool / t64 / q64": ((S2 + 2) ** 2 * 128 * 4, "csrc/api.cpp:504-505 padded(S2, 128)", always),
    "ab": ((S3 + 2) ** 2 * 256 * 4, "csrc/api.cpp:506 padded(S3, 256)", always),
    "ab_t": ((S3 + 2) ** 2 * 256 * 4, "csrc/api.cpp:506; csrc/infer_plan.h:344", lambda cfg, n: cfg == "keep" or not block_tile(cfg, n, 0)),
    "head / head_f": ((S4 + 2) ** 2 * 1024 * 4, "csrc/api.cpp:507-508 padded(S4, 1024); csrc/infer_plan.h:348",
                      lambda cfg, n: cfg == "keep" or not block_tile(cfg, n, 1)),
    "head_t": ((S4 + 2) ** 2 * 1024 * 4, "csrc/api.cpp:507; csrc/infer_plan.h:345", lambda cfg, n: cfg == "keep" or not block_tile(cfg, n, 1)),
    "logits": (6 * 4, "csrc/api.cpp:509 mb 6", always),
    "fcpart": (192 * 4, "csrc/api.cpp:509 mb 192", always),
    "caller's A / B": (4 * 176 * 176 * 4, "include/se3tracknet.h:44 SE3TN_NCHW [N,4,176,176]", always),
    "caller's poseA / poseB": (16 * 8, "csrc/se3tn_internal.h:174-175 [n,16] float64", always),
}
for _t in (2, 4, 6):
    for _w, _nm in ((0, "256-channel block"), (1, "heads")):
        TENSORS["V / M F(%dx%d) %s" % (_t, _t, _nm)] = (
            planes_bytes(_t, _w), "csrc/se3tn_internal.h:149-150, csrc/api.cpp:838-840",
            (lambda t, w: lambda cfg, n: block_tile(cfg, n, w) == t)(_t, _w))
WS_BYTES = max(16 * 36 * 1024, 16 * 121 * 256) * 4      # csrc/api.cpp:264-267 wino_ws_floats per pair: what V and M are allocated with


def derived_sizes(cfg):
    """{n: [why]} of the sizes at which a tensor the configuration writes passes 2^31 or 2^32 bytes, and the limit"""
    out = {LIMIT: ["the limit"]}
    for name, (b, _, written) in TENSORS.items():
        for p, pn in ((P31, "2^31"), (P32, "2^32")):
            for n, side in ((p // b, "last below"), (p // b + 1, "first above")):
                if LO <= n <= HI and written(cfg, n):
                    out.setdefault(n, []).append("%s: %s %s bytes" % (name, side, pn))
    return out


# ---- the rules of the position plan, as kernel families ----------------------------------------------------------------------------
def family(v):
    """a rule's value without its count: the persistent GEMM's rounds, the split-K slices.  (96 | 128 rows, gather 4 | 8, the strip
    rows of the max-pool and the workgroups of the stem are kernels or tile shapes, not counts of one.)"""
    if isinstance(v, str):
        v = re.sub(r" x\d+$", "", v)
        v = re.sub(r"^split-K \d+$", "split-K", v)
    return v


def families(cfg, ns):
    return {name: {family(fn(n)) for n in ns} for name, fn, _ in PLAN.rules(cfg)}


# ---- the size lists ----------------------------------------------------------------------------------------------------------------
# literal: test_large_sizes_are_the_derived_ones / test_large_sizes_reach_every_family name what to add when a buffer or a rule moves.
# 541 | 542, 1083 | 1084: `stem` passes 2^31, 2^32 bytes; 1618 | 1619: the F(4x4) V / M planes pass 2^31; 1982: the three 46 x 46 x 128
# trunk maps end 200,704 bytes below 2^31.  1920 = 8 x 240 = 10 x 192 = 128 x 15: the max-pool remaps every image, fc_finish's last
# workgroup is full and the last row tile of both GEMMs fits -- the values of those rules that the sizes above leave out.
_BASE = [541, 542, 1083, 1084, 1920, 1982]
LARGE_SIZES = {
    "default": _BASE,
    "keep": _BASE,
    "F4": sorted(_BASE + [1618, 1619]),
    "F6": _BASE,
    "direct": _BASE,
    "f16x3": sorted(_BASE + [1618, 1619]),
}


# ---- the 32-bit index audit --------------------------------------------------------------------------------------------------------
def rule(cfg, name):
    return {nm: fn for nm, fn, _ in PLAN.rules(cfg)}.get(name)


def gather_pvoff(n, hin, in_ld):
    """the gather kernels' DMA byte offset of the LAST output row's tap (0, 0): (((n Hp + s ho) Wp + s wo) in_ld + 4 c4) 4, stride 2"""
    hp, ho = hin + 2, (hin - 1) // 2 + 1
    return ((((n - 1) * hp + 2 * (ho - 1)) * hp + 2 * (ho - 1)) * in_ld + 7 * 4) * 4


def gemm_T(cfg, n, which):
    t = block_tile(cfg, n, which)
    return n * cdiv((S3, S4)[which], t) ** 2 if t else 0


def gemm_kind(cfg, n, which):
    return PLAN.wino_gemm(cfg, n, which) if block_tile(cfg, n, which) else ""


def gemm_grid(cfg, n, which):
    """csrc/wino_mfma.hip:924 (Cout / 128) ceil(T / BM) groups nf | csrc/infer_plan.h:268 the persistent kernel's (cus / 8) 8"""
    t, kind = block_tile(cfg, n, which), gemm_kind(cfg, n, which)
    if "persistent" in kind:
        return 256
    cout, groups = ((256, 1), (512, 2))[which]
    return (cout // 128) * cdiv(gemm_T(cfg, n, which), 96 if kind.endswith("96 rows") else 128) * groups * (t + 2) ** 2


def gemm_tiles(cfg, n, which):
    """csrc/infer_plan.h:260 tiles of the persistent 128 x 256 kernel (formed for every Winograd conv, used by the persistent one)"""
    t = block_tile(cfg, n, which)
    cout, groups = ((256, 1), (512, 2))[which]
    return (cout // 256) * cdiv(gemm_T(cfg, n, which), 128) * groups * (t + 2) ** 2


def transform_threads(cfg, n, which):
    """csrc/wino_mfma.hip:170-171, 269-270 idx = blockIdx.x 256 + threadIdx.x < T (C / VEC), VEC = 2 (:31, :1052)"""
    c = (256, 512)[which]
    return cdiv(gemm_T(cfg, n, which) * (c // 2), 256) * 256


fused_block = lambda which: lambda cfg, n: block_tile(cfg, n, which) != 0
trunk_fused = lambda cfg, n: rule(cfg, "trunk A2|B2")(n) == "fused F(2x2)" or rule(cfg, "trunk B3")(n) == "fused F(2x2)"
trunk_slab = lambda cfg, n: str(rule(cfg, "trunk A2|B2")(n)).startswith("slab") or str(rule(cfg, "trunk B3")(n)).startswith("slab")
any_split_k = lambda cfg, n: any(str(fn(n)).startswith("split-K") for _, fn, _ in PLAN.rules(cfg))
plain_tail = lambda cfg, n: not block_tile(cfg, n, 1)
gather4 = lambda name: lambda cfg, n: rule(cfg, name)(n) == "gather 4"

# (what, where, kind, reached(cfg, n), value(cfg, n)).  kind: "int" < 2^31 | "unsigned" < 2^32 | "grid x" < 2^31 | "grid yz" <= 65535 |
# "threads" (grid x block) < 2^32 | "never": no configuration reaches it in 257 .. LIMIT (its bound lies below: the 6 .. 256 sweep).
# Every pvoff[] is FORMED in int and cast to unsigned afterwards, so it is held to 2^31; the offsets that are unsigned from the start
# (sv_even / sv_odd, wvoff, lvoff, uvoff, the fused trunk's patch offsets) are relative to a tile and do not grow with n: no entry.
AUDIT = [
    # the one the limit comes from
    ("gather pvoff[] on q64 (convAB1)", "csrc/mfma_common.h:154", "int", always, lambda cfg, n: gather_pvoff(n, S2, 128)),
    ("gather pvoff[] on ab (heads conv1)", "csrc/mfma_common.h:154", "int", always, lambda cfg, n: gather_pvoff(n, S3, 256)),
    ("split-K pvoff[] / conv_reduce total", "csrc/mfma_common.h:154; csrc/conv3x3_mfma.hip:499", "never", any_split_k, lambda cfg, n: n),
    # host: the counts the argument blocks carry as int
    ("ConvArgs.M, trunk", "csrc/api.cpp:820", "int", always, lambda cfg, n: n * S2 * S2),
    ("WinoArgs.T, 256-channel block", "csrc/api.cpp:840", "int", fused_block(0), lambda cfg, n: gemm_T(cfg, n, 0)),
    ("WinoArgs.T, heads", "csrc/api.cpp:840", "int", fused_block(1), lambda cfg, n: gemm_T(cfg, n, 1)),
    ("plan_gemm tiles, 256-channel block", "csrc/infer_plan.h:260", "int", fused_block(0), lambda cfg, n: gemm_tiles(cfg, n, 0)),
    ("plan_gemm tiles, heads", "csrc/infer_plan.h:260", "int", fused_block(1), lambda cfg, n: gemm_tiles(cfg, n, 1)),
    # pixel indices formed in int (multiplied by the row length in size_t afterwards)
    ("padded_index, 46 x 46 maps", "csrc/mfma_common.h:202-205", "int", always, lambda cfg, n: n * (S2 + 2) ** 2),
    ("slab lo + 8 j pixels / ntiles", "csrc/conv3x3_mfma.hip:108, :121-122", "int", trunk_slab, lambda cfg, n: n * (S2 + 2) ** 2 + 8 * 58),
    ("stem ntiles", "csrc/stem7x7_mfma.hip:88, :257", "int", always, lambda cfg, n: n * 31),
    ("max-pool padded row (img 46 + po + 1)", "csrc/stem7x7_mfma.hip:318", "int", always, lambda cfg, n: n * (S2 + 2)),
    ("wino64 patch row (img 46 + y0)", "csrc/wino64_fused.hip:116, :337", "int", trunk_fused, lambda cfg, n: n * (S2 + 2)),
    ("Winograd pixel (n Hp + Y) Wp + X, 24 x 24", "csrc/wino_mfma.hip:191, :219, :288, :329, :713", "int", fused_block(0),
     lambda cfg, n: n * (S3 + 2) ** 2 + 8 * (S3 + 2)),
    ("Winograd pixel (n Hp + Y) Wp + X, 13 x 13", "csrc/wino_mfma.hip:191, :219, :804, :834", "int", fused_block(1),
     lambda cfg, n: n * (S4 + 2) ** 2 + 8 * (S4 + 2)),
    ("mid / tail tile t = n NT + tile", "csrc/wino_mfma.hip:663, :791", "int", fused_block(0), lambda cfg, n: gemm_T(cfg, n, 0)),
    ("fc_finish logits i 6 + k", "csrc/wino_mfma.hip:888, :898", "int", fused_block(1), lambda cfg, n: 6 * (cdiv(n, 10) * 10)),
    # DMA byte offsets from the base of ONE plane of V
    ("GEMM pvoff[], 256-channel block", "csrc/wino_mfma.hip:422, :551", "int", fused_block(0),
     lambda cfg, n: ((gemm_T(cfg, n, 0) - 1) * 256 + 7 * 4) * 4),
    ("GEMM pvoff[], heads", "csrc/wino_mfma.hip:422, :551", "int", fused_block(1), lambda cfg, n: ((gemm_T(cfg, n, 1) - 1) * 512 + 7 * 4) * 4),
    # element counts of the one-thread-per-element passes
    ("to_padded_input total / idx", "csrc/kernels_misc.hip:33, :55", "int", always, lambda cfg, n: cdiv(n * 176 * 176, 256) * 256),
    ("padded_nhwc_to_nchw total / idx (se3tn_get_feature)", "csrc/kernels_misc.hip:414, :430; csrc/api.cpp:1048", "int", always,
     lambda cfg, n: cdiv(n * S3 * S3 * 256, 256) * 256),
    ("Winograd transform idx, 256-channel block", "csrc/wino_mfma.hip:170-171, :269-270", "int", fused_block(0),
     lambda cfg, n: transform_threads(cfg, n, 0)),
    ("Winograd transform idx, heads", "csrc/wino_mfma.hip:170-171, :269-270", "int", fused_block(1), lambda cfg, n: transform_threads(cfg, n, 1)),
    # grids
    ("stem grid", "csrc/stem7x7_mfma.hip:258-260", "grid x", always, lambda cfg, n: 2 * min(31 * n, 128)),
    ("max-pool grid", "csrc/stem7x7_mfma.hip:355", "grid x", always, lambda cfg, n: n * (S2 // PLAN.pool_rows(n))),
    ("fused trunk grid", "csrc/wino64_fused.hip:363", "grid x", trunk_fused, lambda cfg, n: n * 4 * 2),
    ("slab grid", "csrc/conv3x3_mfma.hip:466-470", "grid x", trunk_slab, lambda cfg, n: min(cdiv(n * S2 * S2, 256) * 2, 256)),
    ("gather grid, convAB1", "csrc/conv3x3_mfma.hip:482-483", "grid x", always,
     lambda cfg, n: cdiv(n * S3 * S3, 128 if gather4("convAB1 s2")(cfg, n) else 256) * 2),
    ("gather grid, heads conv1", "csrc/conv3x3_mfma.hip:482-483", "grid x", always,
     lambda cfg, n: cdiv(n * S4 * S4, 128 if gather4("heads conv1 s2")(cfg, n) else 256) * 8),
    ("GEMM grid, 256-channel block", "csrc/wino_mfma.hip:924; csrc/infer_plan.h:268", "grid x", fused_block(0), lambda cfg, n: gemm_grid(cfg, n, 0)),
    ("GEMM grid, heads", "csrc/wino_mfma.hip:924; csrc/infer_plan.h:268", "grid x", fused_block(1), lambda cfg, n: gemm_grid(cfg, n, 1)),
    ("Winograd transform grid x", "csrc/wino_mfma.hip:1002-1006, :1034-1038", "grid x", fused_block(1),
     lambda cfg, n: max(transform_threads(cfg, n, 0), transform_threads(cfg, n, 1)) // 256),
    ("Winograd transform threads", "csrc/wino_mfma.hip:1002-1006, :1034-1038", "threads", fused_block(1),
     lambda cfg, n: max(transform_threads(cfg, n, 0), transform_threads(cfg, n, 1))),
    ("mid / tail grid x = n", "csrc/wino_mfma.hip:979, :1025", "grid x", fused_block(1), lambda cfg, n: n),
    ("mid grid y = C / CS, z = groups", "csrc/wino_mfma.hip:979 (CS >= 16)", "grid yz", fused_block(1), lambda cfg, n: 512 // 16),
    ("fc_finish grid", "csrc/wino_mfma.hip:1031", "grid x", fused_block(1), lambda cfg, n: cdiv(n, 10)),
    ("tail grid", "csrc/kernels_misc.hip:261", "grid x", plain_tail, lambda cfg, n: n * 16),
    ("to_padded_input grid", "csrc/kernels_misc.hip:56", "grid x", always, lambda cfg, n: cdiv(n * 176 * 176, 256)),
    ("padded_nhwc_to_nchw grid", "csrc/kernels_misc.hip:431", "grid x", always, lambda cfg, n: cdiv(n * S3 * S3 * 256, 256)),
]
BOUND = {"int": P31, "unsigned": P32, "grid x": P31, "grid yz": 65536, "threads": P32}


def first_failure(entry, cfg, ns):
    """the first n of ns at which the entry is reached and out of its bound, or None"""
    _, _, kind, reached, value = entry
    for n in ns:
        if reached(cfg, n) and (kind == "never" or not 0 <= value(cfg, n) < BOUND[kind]):
            return n
    return None


CHUNK = 128     # slots of a stage map compared at a time


def chunks(n, size=CHUNK):
    return [(lo, min(lo + size, n)) for lo in range(0, n, size)]


# ---- the assertions ----------------------------------------------------------------------------------------------------------------
def test_limit_is_the_header_s():
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "se3tracknet.h")).read()
    assert int(re.search(r"#define SE3TN_MAX_BATCH_LIMIT (\d+)", hdr).group(1)) == LIMIT


def test_tensor_table():
    """the figures the sizes follow from, and that the one V / M allocation holds every route's planes"""
    b = {k: v[0] for k, v in TENSORS.items()}
    assert (b["stem"], b["pool / t64 / q64"], b["ab"], b["head / head_f"], b["inA / inB"]) == (3964928, 1083392, 589824, 692224, 529984)
    assert [b["V / M F(%dx%d) %s" % (t, t, w)] for t in (2, 4, 6) for w in ("256-channel block", "heads")] == \
        [1982464, 2359296, 1327104, 1327104, 1048576, 1048576]
    assert WS_BYTES == 2359296 == max(v for k, v in b.items() if k.startswith("V / M"))
    # (tensor, last n below 2^31 bytes, last n below 2^32 bytes)
    assert [(P31 // b[k], P32 // b[k]) for k in ("stem", "V / M F(2x2) heads", "V / M F(2x2) 256-channel block", "V / M F(4x4) heads",
                                                 "pool / t64 / q64")] == [(541, 1083), (910, 1820), (1083, 2166), (1618, 3236), (1982, 3964)]
    # every other tensor passes 2^31 bytes above the limit only
    for k, v in b.items():
        if k not in ("stem", "pool / t64 / q64") and not k.startswith("V / M F(2x2)") and not k.startswith("V / M F(4x4)"):
            assert P31 // v > LIMIT, k
    # no configuration of the sweep runs the conv-by-conv F(2x2) route: its planes are in the table for the allocation's sake
    for cfg in CONFIGS:
        assert {block_tile(cfg, n, w) for n in range(LO, HI + 1) for w in (0, 1)} <= {0, 4, 6}


@pytest.mark.parametrize("cfg", CONFIGS)
def test_large_sizes_are_the_derived_ones(cfg):
    sizes = LARGE_SIZES[cfg]
    assert sizes == sorted(set(sizes)) and LO <= sizes[0] and sizes[-1] == LIMIT
    want = derived_sizes(cfg)
    lack = {n: why for n, why in want.items() if n not in sizes}
    assert not lack, "%s: the size list lacks %s" % (cfg, lack)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_large_sizes_reach_every_family(cfg):
    occur, reached = families(cfg, range(LO, HI + 1)), families(cfg, LARGE_SIZES[cfg])
    lack = {}
    for name, fn, _ in PLAN.rules(cfg):
        for fam in sorted(occur[name] - reached[name], key=str):
            lack["%s = %s" % (name, fam)] = [n for n in range(LO, HI + 1) if family(fn(n)) == fam][:4]
    assert not lack, "%s: no size of the list takes (family: the first sizes that do) %s" % (cfg, lack)
    # nothing in the lists beyond what a tensor size or a family asks for
    need = set(derived_sizes(cfg))
    for n in LARGE_SIZES[cfg]:
        if n not in need:
            rest = families(cfg, [m for m in LARGE_SIZES[cfg] if m != n])
            assert any(occur[k] - rest[k] for k in occur), "%s: %d is in the list for no tensor size and no family" % (cfg, n)


def test_families_are_what_the_reduction_is_meant_to_keep():
    assert family("F6 persistent x62") == "F6 persistent" and family("split-K 12") == "split-K"
    assert [family(v) for v in ("F4 96 rows", "F4 128 rows", "gather 4", "gather 8", "slab persistent", "fused F(2x2)", 44, 128)] == \
        ["F4 96 rows", "F4 128 rows", "gather 4", "gather 8", "slab persistent", "fused F(2x2)", 44, 128]
    # the persistent GEMM walks 2 .. 8 virtual tiles per workgroup up to 256 pairs, 62 at the limit
    rounds = lambda n: int(PLAN.wino_gemm("default", n, 0).split("x")[-1])
    assert (rounds(57), rounds(256), rounds(LIMIT)) == (2, 8, 62)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_every_32_bit_index_stays_in_its_bound(cfg):
    bad = {}
    for e in AUDIT:
        n = first_failure(e, cfg, range(LO, HI + 1))
        if n is not None:
            bad["%s (%s, %s)" % e[:3]] = "n = %d: %s" % (n, "reached" if e[2] == "never" else e[4](cfg, n))
    assert not bad, "%s: %s" % (cfg, bad)


def test_the_limit_is_the_first_index_to_break():
    """one size above the limit the stride-2 gather's DMA offset into the 46 x 46 x 128 map passes 2^31, and nothing else does up to
    the next bound (the F(6x6) planes' 2^31 bytes at 2048 are a size_t product; the heads' gather offset breaks at 3642)"""
    broken = {e[0]: first_failure(e, "default", range(LO, 4000)) for e in AUDIT}
    broken = {k: v for k, v in broken.items() if v is not None}
    assert broken == {"gather pvoff[] on q64 (convAB1)": LIMIT + 1, "gather pvoff[] on ab (heads conv1)": 3642}
    assert gather_pvoff(LIMIT, S2, 128) == 2147210352 and gather_pvoff(LIMIT + 1, S2, 128) == 2147210352 + 1083392 > P31


def test_the_audit_fires_on_a_narrowed_expression():
    """the stem's store offset ((img S1 S1 + p) 128 + br 64 + c) floats is formed in size_t (csrc/stem7x7_mfma.hip:234).  Restated as a
    32-bit BYTE offset it must fail at 542 pairs, the first size of LARGE_SIZES above 2^31 bytes of `stem`; as an unsigned one at 1084"""
    off = lambda cfg, n: (((n - 1) * S1 * S1 + S1 * S1 - 1) * 128 + 64 + 60) * 4 + 15
    assert first_failure(("stem store", "csrc/stem7x7_mfma.hip:234", "int", always, off), "default", range(LO, HI + 1)) == 542
    assert first_failure(("stem store", "csrc/stem7x7_mfma.hip:234", "unsigned", always, off), "default", range(LO, HI + 1)) == 1084
    assert all(n in LARGE_SIZES[cfg] for cfg in CONFIGS for n in (541, 542, 1083, 1084))
    # and a size taken out of a list is named
    short = dict(LARGE_SIZES, F4=[n for n in LARGE_SIZES["F4"] if n != 1619])
    assert [n for n in derived_sizes("F4") if n not in short["F4"]] == [1619]


@pytest.mark.parametrize("cfg", CONFIGS)
def test_slot_assignment_meets_the_shift_condition(cfg):
    for n in LARGE_SIZES[cfg]:
        idx = PLAN.slot_assignment(n)
        assert len(idx) == n and 0 <= idx.min() and idx.max() < PLAN.POOL
        assert len(set(idx[:PLAN.POOL].tolist())) == PLAN.POOL
        assert (idx[1:] != idx[:-1]).all()
        d = PLAN.shift_condition(idx)
        assert d == 0, "n = %d: more than half of the slots hold the same pool pair %d slots apart" % (n, d)
        assert (PLAN.other_assignment(idx) != idx).all()


def test_chunks_tile_the_slots():
    """the stage maps are compared 128 slots at a time (`stem` alone is 7.9 GB at the limit): the chunks are disjoint and cover every slot"""
    for n in sorted({n for v in LARGE_SIZES.values() for n in v} | {6, 127, 128, 129, 256}):
        ch = chunks(n)
        assert [j for lo, hi in ch for j in range(lo, hi)] == list(range(n)) and all(0 < hi - lo <= CHUNK for lo, hi in ch)
