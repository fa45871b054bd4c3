"""GPU: every route se3tn_infer can take, against a FLOAT64 evaluation of the network.

se3tn_infer picks an algorithm per layer from the public switches (se3tn_set_winograd / _trunk_winograd / _small_kernels /
_keep_intermediates / _precision / _normalizers / _enable_graphs) and the create-time developer switches (SE3TN_WINOGRAD_FUSE,
SE3TN_TAIL_PARTS, SE3TN_WINOGRAD_AUTO_TILE_AB2 / _HEADS).  Each case of CASES is one combination, run at the
batch sizes around its switch points.  Per (case, n):
  * one call on another window of the 72-pair pool first, so that a route which reads the previous call's buffers fails;
  * the checked call: EVERY pair's logits against float64 within the case's tolerance class, every composed pose within 1e-5;
  * the profile names of that call: the algorithm the route table (`expected`) names ran for each conv and for the tail;
  * every stage se3tn_debug_buffer hands out against the float64 intermediates (first and last pair of the call), and the stages it
    refuses are exactly the ones the route does not write.  SE3TN_PREC_F16X3 stores `pool`, `t64`, `q64`, `ab`, `ab_t` and `head_t` as
    split rows (f16 hi | f16 lo, tests/split_rows.py; the `head_t` the fused head block keeps on request is float32): those are
    decoded and held to the same float64 maps with the same bounds, every stored (hi, lo) pair of every slot must be one a split
    store writes, the raw border words must be zero bits, and `inA` / `inB` must hold the split of the call's input pixels.
Bit identity: graph replay (non-default stream, third call) against the eager call.
The last test prints the worst error per stage of the f16x3 cases beside the float32 direct route's on the same pairs."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f16x3_range_cases as R
import split_rows as SR
from oracle import fixtures as Fx
from oracle import se3_oracle as O
# the route model (tests/route_model.py; other test modules import these names from here)
from route_model import CUS, HEADS6_MAX_ROT, LAYERS, TILE6_MIN, TILE_6_4, TILE_AUTO, _tag, _tile_for, actual, expected   # noqa: F401

POOL = 72
POSE_TOL = 1e-5
ACT_RTOL = 2e-5
# logit bound against float64 per route class, fixed before the first measurement: upper bounds taken from the documented rounding of
# each algorithm (e.g. 1.3e-5 logit rounding of F(6x6) heads, tile_for in csrc/infer_plan.h), all well inside the 1e-4 north star
CLASS_TOL = {"f32 direct": 1e-5, "F(2x2)/F(4x4)": 2e-5, "F(6x6)": 5e-5, "f16x3": 5e-5}
# activations: |err| <= ACT_RTOL |ref| + scale x max |ref|, scale per algorithm (tests/test_gpu_parity.py's bounds)
STAGE_SCALE = {"small": 5e-6, "direct": 5e-6, "f16x3": 5e-6, "trunk F2": 2e-5, "F2": 2e-5, "F4": 6e-5, "F6": 1.5e-4}
WORST = {}   # class -> worst |d logit| against float64 over the cases run (printed by the last test)
STAGE_ERR = {}   # (case id, n, stage) -> (max |err| / max |ref| against float64 over the pairs compared, its bound as such a ratio)
FAMILIES = {}    # case id -> the f16x3 kernel families its profile names showed ("split-K", "slab", "gather", "F4 block")
DEG = np.pi / 180
STAGES = ("stem", "pool", "t64", "q64", "ab", "ab_t", "head", "head_t")
# SE3TN_PREC_F16X3: the stages that hold split rows.  `stem` is float32 (written by the f16x3 stem kernel from split pixels and split
# weights), `head` is the float32 map of the last head conv (csrc/infer_plan.h BUF_HEAD_OUT).  `head_t` holds split rows where a conv
# kernel stores it; the fused F(4x4) head block keeps it in LDS as float32 and, asked to keep the intermediates, stores THAT
# (csrc/wino_mfma.hip wino_mid_kernel, `keep`): float32 words then -- see split_stages
SPLIT_STAGES = ("pool", "t64", "q64", "ab", "ab_t", "head_t")
IN_PAD = 3       # zero border of `inA` / `inB` [n,182,182,4] (include/se3tracknet.h, se3tn_debug_buffer)
N_BIG = R.smallest_all_big_tile()   # the smallest batch at which every f16x3 conv outside a block runs a big-tile kernel
S15 = [1, 2, 3, 4, 5]
EVERY_N = [1, 2, 3, 4, 5, 6, 7, 13, 14, 15, 17, 18, 33, 34, 64, 72]   # 5/6: batch 1-5 family | Winograd; 14: AUTO -> F(6x6); 18/34: trunk


def case(cid, ns, env=None, ops=(), graph=False):
    return dict(id=cid, ns=ns, env=env or {}, ops=list(ops), graph=graph)


CASES = [case("default", EVERY_N),
         case("small-off", S15, ops=[("small", 0)]),
         case("keep", S15 + [6, 14], ops=[("keep", 1)])]
CASES += [case("wino1-F%s-keep%d" % (name, keep), S15 + [6, 14], ops=[("wino", 1, tile), ("keep", keep)])
          for name, tile in (("2", 2), ("4", 4), ("6", 6), ("6_4", TILE_6_4), ("auto", TILE_AUTO)) for keep in (0, 1)]
CASES += [case("fuse0-F%d" % tile, [1, 3, 5, 8, 20], env={"SE3TN_WINOGRAD_FUSE": "0"}, ops=[("wino", 1, tile)]) for tile in (4, 6)]
CASES += [case("tail-parts%s" % v, S15, env={"SE3TN_TAIL_PARTS": v}) for v in ("0", "2")]
CASES += [case("wino-off", [6, 9, 13], ops=[("wino", 0, 0)]),
          case("trunk1-fill0", S15 + [8], ops=[("trunk", 1, 0)]),
          case("direct", EVERY_N, ops=[("wino", 0, 0), ("trunk", 0, 0)]),
          case("auto-rot0.3", [14], ops=[("norm", 0.03, 0.3)]),
          case("auto-rot0.1", [14], ops=[("norm", 0.03, 0.1)]),
          case("auto-tile-ab2-4-heads-6", [6, 14], env={"SE3TN_WINOGRAD_AUTO_TILE_AB2": "4", "SE3TN_WINOGRAD_AUTO_TILE_HEADS": "6"}),
          case("f16x3", [1, 5, 6, 14, 64], ops=[("f16",)]),
          case("f16x3-keep", [1, 5, 6, 14], ops=[("f16",), ("keep", 1)]),        # the fused split F(4x4) head block stores head, head_t
          case("f16x3-wino-off", [6, 14, N_BIG, 64], ops=[("wino", 0, 0), ("f16",)]),   # heads conv by conv; split-K | slab, gather
          case("f16x3-fuse0", [8], env={"SE3TN_WINOGRAD_FUSE": "0"}, ops=[("f16",)]),
          case("graph-f16x3", [5, 6], ops=[("f16",)], graph=True),
          case("graph-wino1-F2", [1, 3, 5], ops=[("wino", 1, 2)], graph=True),
          case("graph-tail-parts", [1, 3, 5], graph=True)]


def tol_class(cfg, r):
    if cfg["f16"]:
        return "f16x3"
    tags = " ".join(r.values())
    if "F6" in tags:
        return "F(6x6)"
    return "F(2x2)/F(4x4)" if ("F2" in tags or "F4" in tags) else "f32 direct"


# ---- reference ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    L = se3tracknet_amd._lib
    assert (L.WINOGRAD_TILE_AUTO, L.WINOGRAD_TILE_6_4, L.WINOGRAD_TILE6_MIN_BATCH) == (TILE_AUTO, TILE_6_4, TILE6_MIN)
    assert L.WINOGRAD_HEADS_TILE6_MAX_ROT == HEADS6_MAX_ROT
    return se3tracknet_amd


@pytest.fixture(scope="module")
def ref():
    """one seeded state dict, 72 input pairs, their logits in float64 (the yardstick) and in float32 (its noise floor)"""
    sd = O.make_state_dict(21)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    A, B = Fx.net_inputs(2100, POOL)
    lg64, lg32 = [], []
    for i in range(0, POOL, 8):
        o64 = O.forward(sd64, A[i:i + 8].double(), B[i:i + 8].double())
        o32 = O.forward(sd, A[i:i + 8], B[i:i + 8])
        lg64.append(torch.cat([o64["trans_logit"], o64["rot_logit"]], 1))
        lg32.append(torch.cat([o32["trans_logit"], o32["rot_logit"]], 1))
    lg64, lg32 = torch.cat(lg64).numpy(), torch.cat(lg32).numpy()
    floor = float(np.abs(lg32 - lg64).max())
    print("float32 oracle vs float64: max |d logit| %.2e over %d pairs (the noise floor of the float32 yardstick)" % (floor, POOL))
    return dict(sd=sd, sd64=sd64, A=A, B=B, Ac=A.cuda(), Bc=B.cuda(), lg64=lg64, floor=floor, poseA=Fx.pose(9, (0.03, -0.02, 0.7)),
                stages={})


def _stage_ref(ref, i):
    """float64 stage maps of pair i in the layout of se3tn_debug_buffer's channels (NCHW)"""
    if i not in ref["stages"]:
        o = O.forward(ref["sd64"], ref["A"][i:i + 1].double(), ref["B"][i:i + 1].double(), intermediates=True)
        cat = lambda a, b: torch.cat([o[a], o[b]], 1)
        ref["stages"][i] = {"stem": cat("stemA", "stemB"), "pool": cat("poolA", "poolB"), "t64": cat("A2_t", "B3_t"), "q64": o["cat"],
                            "ab": o["feature"], "ab_t": o["ab_t"], "head": cat("trans_c2", "rot_c2"), "head_t": cat("trans_t", "rot_t")}
    return ref["stages"][i]


def _close(name, got, want, rtol, atol, scale_atol=0.0, record=None):
    """record = (dict, key): (max |err| / max |ref|, the bound's absolute part as such a ratio) is noted there before the assertion,
    the larger of this call's and what the key holds"""
    got = got.double(); want = want.double()
    err = (got - want).abs()
    tol = atol + scale_atol * float(want.abs().max()) + rtol * want.abs()
    worst = float((err - tol).max())
    if record is not None:
        m = float(want.abs().max())
        new = (float(err.max()) / m, (atol + scale_atol * m) / m)
        record[0][record[1]] = max(record[0].get(record[1], new), new)
    if worst > 0:
        where = tuple(int(v) for v in np.unravel_index(int((err - tol).argmax()), err.shape))
        over = (err > tol)
        assert False, "%s: max abs err %.3e (max |ref| %.3e), exceeds tol by %.3e at %s; %d of %d elements over" % (
            name, float(err.max()), float(want.abs().max()), worst, where, int(over.sum()), over.numel())


def _words(t):
    return t.contiguous().view(torch.int32)


def split_stages(cfg, r):
    """the stages a call of route r (`expected`) leaves as split rows"""
    if not cfg["f16"]:
        return ()
    return tuple(s for s in SPLIT_STAGES if not (s == "head_t" and r["h2.1"] == "F4 block"))


def _stage_values(split, s, t):
    """the float32 values of stage map t [n,H,W,C]: the stages in `split` (split_stages) hold split rows, decoded here
    (tests/split_rows.py)"""
    return SR.decode_map(t) if s in split else t


def _check_split_map(name, t):
    """a split map, whole and raw: every (hi, lo) pair is one a split store writes; the one-pixel border is zero BITS"""
    bad = SR.count_ill_formed(t)
    assert bad == 0, "%s: %d (hi, lo) pairs no split store writes (first at %s)" % (
        name, bad, SR.ill_formed(*SR.map_halves(t)).nonzero()[0].tolist())
    w = _words(t)
    assert not bool(w[:, 0].any() | w[:, -1].any()) and not bool(w[:, :, 0].any() | w[:, :, -1].any()), name + ": border words not zero bits"


def _check_split_inputs(name, eng, n, A, B, nchw):
    """`inA` / `inB` after an f16x3 call on the caller's tensors A, B [n,...] (device): interior = split_pixel of every input pixel
    (csrc/kernels_misc.hip), compared as decoded values bit for bit, every pair well formed; the 3-pixel border zero bits"""
    for which, x in (("inA", A), ("inB", B)):
        t = eng.debug_buffer(which, n)
        assert tuple(t.shape) == (n, 176 + 2 * IN_PAD, 176 + 2 * IN_PAD, 4), (which, tuple(t.shape))
        assert SR.well_formed(t, pixels=True), "%s %s: a (hi, lo) pair no split store writes" % (name, which)
        inner = t[:, IN_PAD:-IN_PAD, IN_PAD:-IN_PAD]
        px = (x[:n].permute(0, 2, 3, 1) if nchw else x[:n]).contiguous().cpu().numpy()
        want = SR.decode_pixels(torch.from_numpy(SR.encode_pixels(px)))
        got = SR.decode_pixels(inner).cpu()
        assert torch.equal(_words(got), _words(want)), "%s %s: %d decoded pixels differ from the split of the input" % (
            name, which, int((_words(got) != _words(want)).any(-1).sum()))
        w = _words(t).clone()
        w[:, IN_PAD:-IN_PAD, IN_PAD:-IN_PAD] = 0
        assert not bool(w.any()), "%s %s: border words not zero bits" % (name, which)


def _f16x3_families(names, want_r, n, hold):
    """the f16x3 kernel family of every conv of a profiled call, from the [split-K|slab|gather f16x3] tag of its launch name (`actual`
    folds them into "f16x3"); hold: each must be the one the plan rule names for that conv at n pairs (f16x3_range_cases.f16x3_family)"""
    out = set()
    for key, prefix in LAYERS:
        if want_r[key] == "F4 block":
            out.add("F4 block")
            continue
        if want_r[key] != "f16x3":
            continue
        nm = [x for x in names if x == prefix or x.startswith(prefix + " ")]
        fam = [f for f in ("split-K", "slab", "gather") if "[%s f16x3]" % f in nm[0]]
        assert len(nm) == 1 and len(fam) == 1, (key, names)
        if hold:
            assert fam[0] == R.f16x3_family(key, n), (key, n, fam[0], R.f16x3_family(key, n), names)
        out.add(fam[0])
    return out


def _nchw(t, border):
    if border:
        assert float(t[:, 0].abs().max()) == 0 and float(t[:, -1].abs().max()) == 0            # borders stay zero
        assert float(t[:, :, 0].abs().max()) == 0 and float(t[:, :, -1].abs().max()) == 0
        t = t[:, border:-border, border:-border]
    return t.permute(0, 3, 1, 2).contiguous()


def _windows(n):
    """(previous call, checked call): pool indices; slot j of the two calls never holds the same pair"""
    s = (11 * n + 5) % (POOL - n + 1)
    chk = list(range(s, s + n))
    return [POOL - 1 - i for i in chk], chk


class _Runner:
    """se3tn_infer on pool pairs through fixed buffers (a captured graph replays with the same pointers)"""
    def __init__(self, se3, eng, ref, n_max):
        self.se3, self.eng, self.ref = se3, eng, ref
        self.A = torch.empty((n_max, 4, 176, 176), device="cuda")
        self.B = torch.empty_like(self.A)
        self.trans = torch.empty((n_max, 3), device="cuda")
        self.rot = torch.empty_like(self.trans)
        self.pA = torch.from_numpy(np.tile(ref["poseA"].reshape(1, 16), (n_max, 1))).cuda()
        self.pB = torch.empty_like(self.pA)

    def __call__(self, idx):
        n = len(idx)
        ii = torch.tensor(idx, device="cuda")
        self.A[:n].copy_(self.ref["Ac"][ii]); self.B[:n].copy_(self.ref["Bc"][ii])
        self.eng.infer(self.A, self.B, n, self.se3.NCHW, self.trans, self.rot, self.pA, self.pB)
        return self.eng.logits(n).cpu().numpy(), self.pB[:n].cpu().numpy().reshape(n, 4, 4)


def _cfg_op(cfg, op):
    """one switch call in the test's own record of the configuration (what `expected` reads)"""
    if op[0] == "wino":
        cfg["wmin"] = op[1]
        cfg["tile"] = op[2] or cfg["tile"]
    elif op[0] == "trunk":
        cfg["tmin"], cfg["tfill"] = op[1], op[2]
    elif op[0] == "small":
        cfg["small"] = bool(op[1])
    elif op[0] == "keep":
        cfg["keep"] = bool(op[1])
    elif op[0] == "norm":
        cfg["tn"], cfg["rn"] = op[1], op[2]
    elif op[0] == "f16":                    # ("f16",) selects f16x3, ("f16", 0) goes back to float32
        cfg["f16"] = bool(op[1]) if len(op) > 1 else True
    else:
        raise ValueError(op)


def _eng_op(se3, eng, op):
    """the same switch call on the context"""
    if op[0] == "wino":
        eng.set_winograd(op[1], op[2])
    elif op[0] == "trunk":
        eng.set_trunk_winograd(op[1], op[2])
    elif op[0] == "small":
        eng.set_small_kernels(bool(op[1]))
    elif op[0] == "keep":
        eng.keep_intermediates(bool(op[1]))
    elif op[0] == "norm":
        eng.set_normalizers(op[1], op[2])
    elif op[0] == "f16":
        eng.set_precision(se3._lib.PREC_F16X3 if (len(op) == 1 or op[1]) else se3._lib.PREC_F32)
    else:
        raise ValueError(op)


def _engine(se3, ref, env, ops, n_max):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                  # read by se3tn_create
    try:
        eng = se3.Engine(0, n_max)
        eng.load_state_dict(ref["sd"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    wmin, tile = eng.get_winograd()
    tmin, tfill = eng.get_trunk_winograd()
    ovr = [int(env.get(k, "0")) for k in ("SE3TN_WINOGRAD_AUTO_TILE_AB2", "SE3TN_WINOGRAD_AUTO_TILE_HEADS")]
    cfg = dict(wmin=wmin, tile=tile, tmin=tmin, tfill=tfill, small=eng.get_small_kernels(), keep=False, f16=False, tn=0.03, rn=5 * DEG,
               fuse=env.get("SE3TN_WINOGRAD_FUSE", "1") != "0", tail_parts=env.get("SE3TN_TAIL_PARTS", "1") != "0",
               ovr=[v if v in (4, 6) else 0 for v in ovr])
    for op in ops:
        _eng_op(se3, eng, op)
        _cfg_op(cfg, op)
    return eng, cfg


def _readable(se3, eng, n):
    """stage -> the device map [n,H,W,C] se3tn_debug_buffer hands out, or None where it refuses"""
    out = {}
    for s in STAGES:
        try:
            out[s] = eng.debug_buffer(s, n)
        except se3._lib.Se3tnError as e:
            assert "not written" in str(e), (s, str(e))
            out[s] = None
    return out


def _check(se3, eng, run, ref, cfg, n, cid):
    pre, chk = _windows(n)
    run(pre)
    eng.profile_enable(1)
    try:
        lg, pose = run(chk)
        names = [nm for nm, _ in eng.profile_launches(0)]
    finally:
        eng.profile_enable(0)
    got_w = _check_call(se3, eng, ref, cfg, n, chk, lg, pose, names, cid, WORST, stage_err=STAGE_ERR)
    if cfg["f16"]:
        _check_split_inputs("%s n=%d" % (cid, n), eng, n, run.A, run.B, True)
        FAMILIES.setdefault(cid, set()).update(_f16x3_families(names, expected(cfg, n)[0], n, hold=cid == "f16x3-wino-off"))
    return lg, pose, got_w


def _check_call(se3, eng, ref, cfg, n, chk, lg, pose, names, cid, worst, stage_err=None):
    """one profiled call on pool pairs `chk`, after the fact: logits and poses against float64, the route from its launch names, the
    stages se3tn_debug_buffer hands out (f16x3: split rows decoded, and checked whole as split rows); -> {stage: readable}"""
    want_r, written = expected(cfg, n)
    cls = tol_class(cfg, want_r)
    err = np.abs(lg.astype(np.float64) - ref["lg64"][chk])
    e = float(err.max())
    worst[cls] = max(worst.get(cls, 0.0), e)
    assert e <= CLASS_TOL[cls], "%s n=%d: max |d logit| vs float64 %.3e > %.0e (%s), pair %d" % (
        cid, n, e, CLASS_TOL[cls], cls, chk[int(err.max(1).argmax())])
    for j, i in enumerate(chk):
        want = O.process_predict(ref["poseA"], np.tanh(ref["lg64"][i, :3]), np.tanh(ref["lg64"][i, 3:]), cfg["tn"], cfg["rn"])
        d = float(np.abs(pose[j] - want).max())
        assert d <= POSE_TOL, "%s n=%d pair %d: |d pose| %.3e" % (cid, n, i, d)
    got_r = actual(names)
    assert got_r == want_r, "%s n=%d: route %s, expected %s (%s)" % (cid, n, got_r, want_r, names)
    # the stages: handed out exactly where this call wrote them, and then equal to float64
    maps = _readable(se3, eng, n)
    got_w = {s: maps[s] is not None for s in STAGES}
    assert got_w == written, "%s n=%d: readable stages %s, written by the route %s" % (cid, n, got_w, written)
    sc = lambda keys: max(STAGE_SCALE[want_r[k].replace(" block", "")] for k in keys)
    sc_trunk, sc_all = sc(("trunk1", "trunk2", "trunk3", "trunk4")), sc([k for k, _ in LAYERS])
    split = split_stages(cfg, want_r)
    for s, t in maps.items():
        if t is None:
            continue
        if s in split:    # f16x3 split rows: the whole map of all n slots, raw
            _check_split_map("%s n=%d %s" % (cid, n, s), t)
        for j in sorted({0, n - 1}):
            got = _nchw(_stage_values(split, s, t[j:j + 1]).cpu(), 0 if s == "stem" else 1)
            want = _stage_ref(ref, chk[j])[s]
            _close("%s n=%d %s pair %d" % (cid, n, s, chk[j]), got, want, ACT_RTOL, 1e-5 if s in ("stem", "pool") else 0,
                   sc_trunk if s in ("stem", "pool", "t64", "q64") else sc_all,
                   record=None if stage_err is None else (stage_err, (cid, n, s)))
    return got_w


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_route_vs_float64(se3, ref, case):
    n_max = max(case["ns"])
    eng, cfg = _engine(se3, ref, case["env"], case["ops"], n_max)
    try:
        run = _Runner(se3, eng, ref, n_max)
        for n in case["ns"]:
            lg, pose, got_w = _check(se3, eng, run, ref, cfg, n, case["id"])
            if case["graph"]:   # graph replay: first call eager, second captured, third replayed -- the eager bits
                eager = _readable(se3, eng, n)
                pre, chk = _windows(n)
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    eng.enable_graphs(True)
                    try:
                        run(pre)
                        run(chk[::-1])
                        lg_g, pose_g = run(chk)
                        replayed = _readable(se3, eng, n)
                        w_g = {k: v is not None for k, v in replayed.items()}
                    finally:
                        eng.enable_graphs(False)
                torch.cuda.synchronize()
                assert np.array_equal(lg_g, lg) and np.array_equal(pose_g, pose), (case["id"], n)
                assert w_g == got_w, (case["id"], n, w_g, got_w)
                if cfg["f16"]:      # every handed-out stage word for word, raw (split rows included, nothing decoded)
                    for s_, t in replayed.items():
                        assert t is None or torch.equal(_words(t), _words(eager[s_])), (case["id"], n, s_)
        if case["id"] == "f16x3-wino-off":   # both sides of each conv's split-K -> slab | gather switch ran
            assert FAMILIES[case["id"]] >= {"split-K", "slab", "gather"}, FAMILIES[case["id"]]
            for key in R.GEOM:
                assert {R.f16x3_family(key, n) for n in case["ns"]} == {"split-K", "slab" if R.GEOM[key][1] == 1 else "gather"}, key
    finally:
        eng.close()


def test_f16x3_input_adapter_splits_both_layouts(se3, ref):
    """se3tn_infer's copy of the caller's tensors into `inA` / `inB` in f16x3 mode (to_padded_input_kernel), NCHW and NHWC: the split
    of every input pixel; 3 pairs, one of them holding the values where the split is delicate"""
    eng, cfg = _engine(se3, ref, {}, [("f16",)], 4)
    try:
        n = 3
        A, B = ref["Ac"][:n].clone(), ref["Bc"][7:7 + n].clone()
        edge = torch.tensor([0.0, -0.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 65000.0, -65000.0, 1e-6, 2049.0, 1.0 + 2.0 ** -13,
                             2.0 ** -3], device="cuda")
        A[2].view(-1)[:edge.numel()] = edge
        B[0].view(-1)[-edge.numel():] = edge
        trans, rot = torch.empty((n, 3), device="cuda"), torch.empty((n, 3), device="cuda")
        for layout, nchw in ((se3.NCHW, True), (se3.NHWC, False)):
            a, b = (A, B) if nchw else (A.permute(0, 2, 3, 1).contiguous(), B.permute(0, 2, 3, 1).contiguous())
            eng.infer(a, b, n, layout, trans, rot)
            _check_split_inputs("layout %d" % layout, eng, n, a, b, nchw)
    finally:
        eng.close()


class _Render:
    """synthetic image A per render call (kept for the oracle)"""
    def __init__(self):
        self.log = []

    def render(self, ob2cam, K, window):
        self.log.append(Fx.synthetic_render(130 + len(self.log), ob2cam[2, 3]))
        return self.log[-1]


def test_tracker_on_track_and_batch_with_winograd_tile2_from_one_pair(se3):
    """Tracker.on_track / on_track_batch(3) on a context with se3tn_set_winograd(1, 2): the per-frame batch runs the F(2x2) blocks
    conv by conv and the plain tail (at the parent commit the tail read stale partial sums here)."""
    sd = O.make_state_dict(0, head_gain=0.01)
    mean, std = Fx.mean_std(0)
    rend = _Render()
    trk = se3.Tracker(Fx.DATASET_INFO, mean, std, {"state_dict": sd}, renderer=rend, max_samples=3)
    trk.engine.set_winograd(1, 2)
    tol = CLASS_TOL["F(2x2)/F(4x4)"]
    args = (trk.K, trk.object_width, mean, std, trk.trans_normalizer, trk.rot_normalizer)
    P = Fx.pose(3)
    for f in range(3):
        rgb, depth = Fx.synthetic_frame(30 + f)
        got = trk.on_track(P, rgb, depth)
        want, o = O.on_track(sd, P, rgb, depth, *rend.log[-1], *args)
        lp = trk.last_prediction
        assert np.abs(lp["trans"][0] - o["trans"]).max() < tol and np.abs(lp["rot"][0] - o["rot"]).max() < tol, f
        assert np.abs(got - want).max() < POSE_TOL, f
        P = got
    poses = [Fx.pose(40 + i, (0.03 * i - 0.03, 0.01, 0.7 + 0.05 * i)) for i in range(3)]
    frames = [Fx.synthetic_frame(50 + i) for i in range(3)]
    k0 = len(rend.log)
    bat = trk.on_track_batch(poses, [f[0] for f in frames], [f[1] for f in frames])
    lp = trk.last_prediction
    for i in range(3):
        want, o = O.on_track(sd, poses[i], *frames[i], *rend.log[k0 + i], *args)
        assert np.abs(lp["trans"][i] - o["trans"]).max() < tol and np.abs(lp["rot"][i] - o["rot"]).max() < tol, i
        assert np.abs(bat[i] - want).max() < POSE_TOL, i


def test_zz_report_worst_logit_error_per_class(ref):
    """(runs last) the worst |d logit| against float64 per tolerance class over the cases above, beside the float32 oracle's own error"""
    print("float32 oracle vs float64: %.2e" % ref["floor"])
    for cls, bound in CLASS_TOL.items():
        print("%-14s worst |d logit| vs float64 %s (bound %.0e)" % (cls, "%.2e" % WORST[cls] if cls in WORST else "not run", bound))
        assert WORST.get(cls, 0.0) <= bound


def test_zz_report_f16x3_stage_errors_beside_float32_direct():
    """(runs last) per f16x3 case and stage: the worst max |err| / max |ref| against float64 over the sizes and pairs compared, the
    bound as the same ratio, and what the float32 direct route ("direct": the same pool pairs at the same n) left on that stage at the
    sizes both ran -- what "float32-class" is measured against.  Then the f16x3 kernel families the profile names showed."""
    f16 = sorted({cid for cid, _, _ in STAGE_ERR if "f16x3" in cid})
    print("\ncase             stage    f16x3 err/max  (at n)  bound/max   f32 direct err/max (same n)")
    for cid in f16:
        for s in STAGES:
            rows = {n: v for (c, n, s_), v in STAGE_ERR.items() if c == cid and s_ == s}
            if not rows:
                continue
            n = max(rows, key=lambda k: rows[k][0])
            d = STAGE_ERR.get(("direct", n, s))
            both = [k for k in rows if ("direct", k, s) in STAGE_ERR]
            d_worst = max((STAGE_ERR[("direct", k, s)][0] for k in both), default=None)
            print("%-16s %-7s  %.2e       %4d    %.2e    %s (worst over n in %s: %s)" % (
                cid, s, rows[n][0], n, rows[n][1], "%.2e" % d[0] if d else "-", both, "%.2e" % d_worst if both else "-"))
    for cid in sorted(FAMILIES):
        print("%-16s f16x3 kernel families in the profile names: %s" % (cid, sorted(FAMILIES[cid])))
    if FAMILIES:
        ran = set().union(*FAMILIES.values())
        assert ran >= {"split-K", "slab", "gather", "F4 block"} or not {"f16x3", "f16x3-wino-off"} <= set(FAMILIES), ran
