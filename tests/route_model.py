"""The route model of se3tn_infer in plain Python: what a configuration must run for a call of n pairs (`expected`), and how the launch
names of a profiled call read as a route (`actual`).  An independent statement of the rule, not generated from csrc/infer_plan.h:
tests/test_gpu_routes.py holds the device to it, tests/test_host_abi.py the host-side plan (no GPU)."""
import re

CUS = 256    # compute units of an MI355X: the fused trunk kernel runs only in rounds of them that are full enough
TILE_AUTO, TILE_6_4, TILE6_MIN, HEADS6_MAX_ROT = 46, 64, 14, 0.2   # include/se3tracknet.h (checked against _lib in the fixture)
LAYERS = [("trunk1", "conv64 A2.conv1|B2.conv1"), ("trunk2", "conv64 A2.conv2|B2.conv2"), ("trunk3", "conv64 B3.conv1"),
          ("trunk4", "conv64 B3.conv2"), ("ab1", "convAB1 s2"), ("ab2.1", "convAB2.conv1"), ("ab2.2", "convAB2.conv2"),
          ("h1", "trans|rot conv1 s2"), ("h2.1", "trans|rot conv2.conv1"), ("h2.2", "trans|rot conv2.conv2")]


# ---- the route table: what se3tn_infer must run for a configuration ----------------------------------------------------------------
def _tile_for(cfg, n, which):
    """Winograd tile of the 256-channel block (which 0) / the heads (1): include/se3tracknet.h, se3tn_set_winograd"""
    t = cfg["tile"]
    if t in (2, 4):
        return t
    if cfg["f16"]:
        return 4
    if t == 6:
        return 6
    if t == TILE_6_4:
        return 6 if which == 0 else 4
    if cfg["ovr"][which]:
        return cfg["ovr"][which]
    if n < TILE6_MIN:
        return 4
    return 6 if which == 0 or cfg["rn"] <= HEADS6_MAX_ROT else 4


def expected(cfg, n):
    """(algorithm per conv + "stem" + "tail", {stage: written}) of one call of n pairs"""
    f16 = cfg["f16"]
    small = cfg["small"] and not f16 and n <= 5
    plain = "small" if small else ("f16x3" if f16 else "direct")
    wino = cfg["wmin"] > 0 and n >= cfg["wmin"]
    r = {"stem": "small" if small and not cfg["keep"] else "big"}
    for key, groups in zip(("trunk1", "trunk2", "trunk3", "trunk4"), (2, 2, 1, 1)):
        wgs = 4 * n * groups
        fused = not f16 and cfg["tmin"] > 0 and n >= cfg["tmin"] and 100 * wgs >= cfg["tfill"] * -(-wgs // CUS) * CUS
        r[key] = "trunk F2" if fused else plain
    r["ab1"] = r["h1"] = plain
    block = {}
    for which, convs in ((0, ("ab2.1", "ab2.2")), (1, ("h2.1", "h2.2"))):
        t = _tile_for(cfg, n, which)
        block[which] = cfg["fuse"] and wino and (t == 4 or (t == 6 and not f16)) and not (which == 0 and f16)
        for k in convs:
            r[k] = ("F%d block" % t) if block[which] else (("F%d" % t) if wino and not f16 else plain)
    r["tail"] = "fused" if block[1] else ("parts" if r["h2.2"] == "small" and cfg["tail_parts"] and not cfg["keep"] else "tail")
    written = {"stem": r["stem"] == "big", "pool": True, "t64": True, "q64": True, "ab": True,
               "ab_t": not block[0] or cfg["keep"], "head_t": not block[1] or cfg["keep"],
               "head": (block[1] and cfg["keep"]) or (not block[1] and r["tail"] != "parts")}
    return r, written


def _tag(name):
    if "[fused F(2x2)]" in name:
        return "trunk F2"
    m = re.search(r"\[F\((\d)x\1\)\]", name)
    if m:
        return ("F%s block" % m.group(1)) if "fused block" in name else "F" + m.group(1)
    m = re.search(r"\[(conv64 small|slices|split-K|slab|gather)( f16x3)?\]", name)
    if m is None:
        return "untagged: " + name
    return "f16x3" if m.group(2) else ("small" if m.group(1) in ("conv64 small", "slices") else "direct")


def actual(names):
    """the route of a profiled call, from its launch names"""
    r = {}
    for key, prefix in LAYERS:
        hits = [nm for nm in names if nm == prefix or nm.startswith(prefix + " ")]
        assert len(hits) == 1, (key, names)
        r[key] = _tag(hits[0])
    r["stem"] = "small" if any(nm.startswith("stem7x7 + maxpool") for nm in names) else "big"
    r["tail"] = ("parts" if any(nm.startswith("tail slices") for nm in names) else
                 "tail" if any(nm.startswith("tail avgpool") for nm in names) else "fused")
    return r
