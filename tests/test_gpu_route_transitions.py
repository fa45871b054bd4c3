"""GPU: se3tn_infer across switch changes on ONE live context.

tests/test_gpu_routes.py builds a fresh context per configuration.  The state se3tn_ctx keeps between calls -- which Winograd planes
wino_u holds (wino_tile_derived), the f16x3 split rows of those planes (wino_us), workspaces allocated late, the pixel format left in
the activation buffers (last_fast, head_f), the arrival counters and partial sums three tails share, the stage mask and the graph
cache -- is exercised only when a switch changes on a context that has already run another route.  Each SEQUENCE here is a fixed,
named list of steps on one context; a step is a list of switch calls and a batch size n.  Per step:
  * one call on another window of the 24-pair pool, then the checked call with profiling on;
  * BIT identity with a twin -- a context created, given the same weights and put directly into this configuration: logits, trans,
    rot, poseB, se3tn_get_feature and every stage se3tn_debug_buffer hands out (whole maps, borders included, compared as words);
  * float64: logits per tolerance class, poses, stage maps -- test_gpu_routes' bounds, nothing new;
  * the route from the profile names equals the route table's; the readable stages are the ones the route writes, borders zero.
Every sequence but the random walk runs again with graphs enabled on a non-default stream through persistent buffers: three calls
per step (eager, capture, replay -- on a key seen before, three replays), each bit-equal to the twin's eager result.
test_sequences_cover_the_transitions (no GPU) replays the sequences through the route table and asserts what they reach."""
import numpy as np
import pytest
import torch

from oracle import fixtures as Fx
from oracle import se3_oracle as O
from test_gpu_routes import (CLASS_TOL, DEG, STAGES, TILE_6_4, TILE_AUTO, _cfg_op, _check_call, _eng_op, _engine, _readable, _Runner,
                             actual, expected, tol_class)

POOL = 24
N_MAX = 18
MAX_TWINS = 24    # twin contexts alive at a time (a context with every plane set holds ~1 GB): the least recently used one is closed
WORST = {}        # class -> worst |d logit| against float64 over all transition steps (printed by the last test)


# ---- the sequences -----------------------------------------------------------------------------------------------------------------
def W(min_batch, tile):
    return ("wino", min_batch, tile)


def step(ops, n):
    return dict(ops=list(ops), n=n)


F16, F32 = ("f16", 1), ("f16", 0)
TILE_WALK = [4, 2, 4, 6, 2, TILE_AUTO, TILE_6_4, 2, 6]


def _random_walk(seed, steps):
    """fixed walk over the operations of the other sequences (an LCG of its own: the same walk under every numpy / python)"""
    state = [seed]

    def draw(k):
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (state[0] >> 33) % k
    ops = ([W(mb, t) for mb in (1, 6) for t in (2, 4, 6, TILE_AUTO, TILE_6_4)] + [W(0, 0), W(6, 0)] +
           [("trunk", 1, 0), ("trunk", 0, 0), ("trunk", 8, 55), ("small", 0), ("small", 1), ("keep", 0), ("keep", 1),
            ("norm", 0.03, 5 * DEG), ("norm", 0.03, 0.3), ("norm", 0.03, 0.1), F16, F32, F16, F32])
    ns = [1, 2, 5, 6, 13, 14, 18]
    return [step([ops[draw(len(ops))] for _ in range(1 + draw(2))], ns[draw(len(ns))]) for _ in range(steps)]


def seq(name, steps, env=None, max_batch=N_MAX, graph=True):
    return dict(name=name, steps=steps, env=env or {}, max_batch=max_batch, graph=graph)


_TAILS = [step([], 3),                                   # tail slices (tail_parts_kernel: 64 | 32 workgroups per pair)
          step([("keep", 1)], 3),                        # tail avgpool (tail_kernel: 16 workgroups per pair)
          step([("keep", 0), W(1, 4)], 3),               # the fused heads' tail (fc_finish_kernel)
          step([W(6, 0)], 3),                            # slices
          step([W(1, 4)], 3),                            # fused
          step([W(6, 0), ("small", 0)], 3),              # avgpool
          step([("small", 1)], 3)]                       # slices
SEQUENCES = [
    seq("planes", [step([W(6, t)], n) for n in (6, 14) for t in TILE_WALK] + [step([W(1, t)], 3) for t in TILE_WALK]),
    seq("late-workspace", [step([], 5), step([W(1, 4)], 5), step([W(1, 6)], 5), step([W(1, 2)], 5), step([W(0, 0)], 5),
                           step([W(1, TILE_AUTO)], 5)], max_batch=5),
    seq("precision", [step(ops, n) for n in (1, 6, 14) for ops in ([F32], [F16], [F32], [F16])] +
        [step([("keep", 1)], 14), step([("keep", 0)], 14), step([("keep", 1)], 6), step([("keep", 0)], 6),
         step([F32, W(0, 0)], 6), step([F16], 6), step([F32], 6),                    # ... with the direct kernels as the float32 route
         step([W(6, 0), ("refuse",)], 6),      # own input buffers filled under float32, f16x3 selected: refused; then a valid call
         step([F32], 6)]),
    seq("split-planes", [step([W(6, 2), F16], 6),                        # f16x3 while wino_u holds F(2x2): wino_us not derivable
                         step([W(6, 4)], 6),                             # -> the fused F(4x4) head block on split planes derived now
                         step([W(6, 2)], 6), step([W(6, 4)], 6),         # wino_us kept, wino_u overwritten and re-derived
                         step([W(6, 2), ("load", 1), W(6, 4)], 6),       # new weights while F(2x2) is loaded, then F(4x4)
                         step([("load", 0)], 6),
                         step([W(6, TILE_AUTO)], 14), step([F32], 14)]),
    seq("tails", _TAILS),
    seq("tails-parts2", _TAILS, env={"SE3TN_TAIL_PARTS": "2"}),
    seq("descending-n", [step([], n) for n in (18, 5, 1, 14, 2, 17, 6)] +
        [step([("trunk", 1, 0)], 2), step([("trunk", 0, 0)], 2), step([("trunk", 1, 0)], 8), step([("trunk", 0, 0)], 8),
         step([("trunk", 8, 55)], 18)]),
    seq("normalisers", [step([W(6, TILE_AUTO)], 14), step([("norm", 0.03, 0.3)], 14), step([("norm", 0.03, 0.1)], 14),
                        step([("norm", 0.03, 0.3)], 14)]),
    seq("random-walk", _random_walk(20261, 30), graph=False)]
RUNS = [(s, g) for s in SEQUENCES for g in ((False, True) if s["graph"] else (False,))]
# eviction: 17 graph keys at n <= 5 out of n x small x keep x two normaliser pairs (the cache holds 16)
_EVICT_ALL = [(n, small, keep, norm) for norm in ((0.03, 5 * DEG), (0.05, 0.3)) for keep in (0, 1) for small in (1, 0) for n in (1, 2, 3, 4, 5)]
EVICT_KEYS = [_EVICT_ALL[(7 * i) % len(_EVICT_ALL)] for i in range(17)]


def _cfg0(env, max_batch):
    """the record test_gpu_routes._engine keeps of a context just created (include/se3tracknet.h's defaults; checked against the
    context in _Live)"""
    ovr = [int(env.get(k, "0")) for k in ("SE3TN_WINOGRAD_AUTO_TILE_AB2", "SE3TN_WINOGRAD_AUTO_TILE_HEADS")]
    return dict(wmin=6, tile=TILE_AUTO, tmin=8, tfill=55, small=True, keep=False, f16=False, tn=0.03, rn=5 * DEG,
                fuse=env.get("SE3TN_WINOGRAD_FUSE", "1") != "0", tail_parts=env.get("SE3TN_TAIL_PARTS", "1") != "0",
                ovr=[v if v in (4, 6) else 0 for v in ovr])


def _walk(s):
    """the sequence through the route table alone: per step (cfg after its switch calls, n, weights, planes in wino_u before / after)"""
    cfg, sd, out = _cfg0(s["env"], s["max_batch"]), 0, []
    planes = lambda p: (2 if cfg["tile"] == 2 else 4) if 0 < cfg["wmin"] <= s["max_batch"] else p   # wino_prepare (csrc/api.cpp)
    u = planes(0)
    for st in s["steps"]:
        u0, flips = u, []
        for op in st["ops"]:
            if op[0] == "load":
                sd = op[1]
            elif op[0] == "refuse":
                cfg["f16"] = True
            else:
                _cfg_op(cfg, op)
            if planes(u) != u:
                flips.append((u, planes(u), cfg["f16"]))
            u = planes(u)
        out.append(dict(cfg=dict(cfg), n=st["n"], sd=sd, u=(u0, u), flips=flips))
    return out


def _family(r):
    tags = set(r.values())
    return "small" if r["ab1"] == "small" else "F6 block" if "F6 block" in tags else "F4 block" if "F4 block" in tags else "direct"


def test_sequences_cover_the_transitions():
    """(no GPU) what the fixed sequences reach, from the route table: the condition that keeps an edit from hollowing them out"""
    walks = {s["name"]: _walk(s) for s in SEQUENCES}
    routes = {k: [expected(w["cfg"], w["n"])[0] for w in v] for k, v in walks.items()}
    for k, v in walks.items():
        assert all(1 <= w["n"] <= min(N_MAX, next(s for s in SEQUENCES if s["name"] == k)["max_batch"]) for w in v), k
    # every ordered pair of tail kinds back to back, for both workgroup counts of the slices tail
    for name in ("tails", "tails-parts2"):
        kinds = [r["tail"] for r in routes[name]]
        assert set(zip(kinds, kinds[1:])) >= {(a, b) for a in ("parts", "tail", "fused") for b in ("parts", "tail", "fused") if a != b}, kinds
        assert all(w["n"] == 3 for w in walks[name])
    # wino_u overwritten F2 -> F4 and F4 -> F2, each under both precisions, and followed by a call that runs on those planes
    flips = {f for v in walks.values() for w in v for f in w["flips"]}
    assert flips >= {(2, 4, False), (2, 4, True), (4, 2, False), (4, 2, True)}, flips
    used = set()
    for k, v in walks.items():
        for w, r in zip(v, routes[k]):
            if w["u"][0] != w["u"][1] and w["u"][0]:
                used.add((w["u"][1], w["cfg"]["f16"], r["h2.2"]))
    assert used >= {(4, False, "F4 block"), (2, False, "F2"), (4, True, "F4 block"), (2, True, "f16x3")}, used
    # F(6x6) -> F(2x2) -> F(6x6) (wino_u6 stays resident while wino_u changes)
    ab = [r["ab2.1"] for r in routes["planes"]]
    assert any(a.startswith("F6") and b == "F2" and c.startswith("F6") for a, b, c in zip(ab, ab[1:], ab[2:])), ab
    # the late workspace: nothing allocated at create time, then every plane set
    late = walks["late-workspace"]
    assert late[0]["u"] == (0, 0) and [r["h2.2"] for r in routes["late-workspace"]] == ["small", "F4 block", "F6 block", "F2", "small", "F4 block"]
    # both precision flips with each float32 family on the float32 side, and both f16x3 head routes on the other
    to16, to32, f16_before, f16_after = set(), set(), set(), set()
    for k, v in walks.items():
        for (w0, r0), (w1, r1) in zip(zip(v, routes[k]), zip(v[1:], routes[k][1:])):
            if not w0["cfg"]["f16"] and w1["cfg"]["f16"]:
                to16.add(_family(r0)); f16_after.add(r1["h2.2"])
            if w0["cfg"]["f16"] and not w1["cfg"]["f16"]:
                to32.add(_family(r1)); f16_before.add(r0["h2.2"])
    every = {"small", "direct", "F4 block", "F6 block"}
    assert to16 >= every and to32 >= every, (to16, to32)
    assert f16_before >= {"f16x3", "F4 block"} and f16_after >= {"f16x3", "F4 block"}, (f16_before, f16_after)
    assert any("refuse" in [op[0] for op in st["ops"]] for st in SEQUENCES[2]["steps"])
    assert any(w["sd"] == 1 and w["cfg"]["f16"] and w["flips"] == [(4, 2, True), (2, 4, True)] for w in walks["split-planes"])
    # descending n: every consecutive pair of calls changes the route, and the trunk visits its three families both ways
    desc = routes["descending-n"]
    assert [w["n"] for w in walks["descending-n"]][:7] == [18, 5, 1, 14, 2, 17, 6]
    trunk = [r["trunk1"] for r in desc]
    assert set(zip(trunk, trunk[1:])) >= {("trunk F2", "small"), ("small", "direct"), ("direct", "small"), ("small", "trunk F2"),
                                          ("trunk F2", "direct"), ("direct", "trunk F2")}, trunk
    assert {r["stem"] for r in desc} == {"small", "big"}
    # the normalisers move the heads F(6x6) <-> F(4x4) under AUTO
    assert [r["h2.2"] for r in routes["normalisers"]] == ["F6 block", "F4 block", "F6 block", "F4 block"]
    # the random walk: 30 steps, n from the set, both precisions, every family
    rw = walks["random-walk"]
    assert len(rw) == 30 and {w["n"] for w in rw} <= {1, 2, 5, 6, 13, 14, 18} and {w["cfg"]["f16"] for w in rw} == {False, True}
    assert {_family(r) for r in routes["random-walk"]} == every
    # eviction: more keys than the graph cache holds
    assert len(set(EVICT_KEYS)) >= 17 and all(1 <= k[0] <= 5 for k in EVICT_KEYS)
    assert len({k[1] for k in EVICT_KEYS}) == 2 and len({k[2] for k in EVICT_KEYS}) == 2 and len({k[3] for k in EVICT_KEYS}) == 2


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def _make_ref(seed, A, B, rows):
    """a seeded state dict and the float64 logits of pool pairs `rows` (stage maps: test_gpu_routes._stage_ref, on demand)"""
    sd = O.make_state_dict(seed)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    lg64 = np.full((POOL, 6), np.nan)
    for i in range(0, len(rows), 8):
        ii = rows[i:i + 8]
        o64 = O.forward(sd64, A[ii].double(), B[ii].double())
        lg64[ii] = torch.cat([o64["trans_logit"], o64["rot_logit"]], 1).numpy()
    return dict(sd=sd, sd64=sd64, A=A, B=B, Ac=A.cuda(), Bc=B.cuda(), lg64=lg64, poseA=Fx.pose(9, (0.03, -0.02, 0.7)), stages={})


def _windows(n, k):
    """(previous call, checked call) of step k: pool indices; slot j of the two calls never holds the same pair"""
    s = (11 * n + 5 + 7 * (k % 2)) % (POOL - n + 1)
    chk = list(range(s, s + n))
    return [POOL - 1 - i for i in chk], chk


@pytest.fixture(scope="module")
def refs():
    """[the state dict every sequence starts with, the second one of split-planes (only the pairs its one call checks)]"""
    A, B = Fx.net_inputs(2400, POOL)
    k = next(i for i, st in enumerate(SEQUENCES[3]["steps"]) if ("load", 1) in st["ops"])
    return [_make_ref(21, A, B, list(range(POOL))), _make_ref(22, A, B, _windows(6, k)[1])]


class _Twins:
    """contexts created, given the weights and put directly into one configuration, which run nothing else; one per configuration"""
    def __init__(self, se3, refs):
        self.se3, self.refs, self.live = se3, refs, {}

    def get(self, env, max_batch, sd, cfg):
        key = (tuple(sorted(env.items())), max_batch, sd) + tuple(cfg[k] for k in ("wmin", "tile", "tmin", "tfill", "small", "keep", "f16", "tn", "rn"))
        if key in self.live:
            self.live[key] = self.live.pop(key)          # (most recently used last)
            return self.live[key]
        while len(self.live) >= MAX_TWINS:
            self.live.pop(next(iter(self.live)))[0].close()
        ops = [("trunk", cfg["tmin"], cfg["tfill"]), ("small", cfg["small"]), ("keep", cfg["keep"]), ("norm", cfg["tn"], cfg["rn"]),
               W(cfg["wmin"], cfg["tile"])] + ([F16] if cfg["f16"] else [])
        eng, got = _engine(self.se3, self.refs[sd], env, ops, max_batch)
        assert got == cfg, (got, cfg)
        self.live[key] = (eng, _Runner(self.se3, eng, self.refs[sd], max_batch))
        return self.live[key]

    def close(self):
        for eng, _ in self.live.values():
            eng.close()
        self.live = {}


@pytest.fixture(scope="module")
def twins(se3, refs):
    t = _Twins(se3, refs)
    yield t
    t.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _snapshot(se3, eng, run, n):
    """everything a call leaves behind that a caller can read, on the device"""
    out = dict(logits=eng.logits(n), trans=run.trans[:n].clone(), rot=run.rot[:n].clone(), poseB=run.pB[:n].clone(), feature=eng.feature(n))
    for s, t in _readable(se3, eng, n).items():
        out["stage " + s] = t
    return out


def _assert_same(got, want, what):
    for k in want:
        assert (got[k] is None) == (want[k] is None), "%s: \"%s\" readable %s, on the twin %s" % (what, k, got[k] is not None, want[k] is not None)
        if want[k] is None:
            continue
        a, b = _bits(got[k]), _bits(want[k])
        if not torch.equal(a, b):
            bad = (a != b).reshape(a.shape[0], -1).sum(1).cpu().tolist()
            d = float((got[k].double() - want[k].double()).abs().max()) if not k.startswith("stage ") else float("nan")   # (split rows)
            raise AssertionError("%s: %s differs from the twin's in %s words per pair (max |d| %.3e)" % (what, k, bad, d))


def _borders_zero(snap, what):
    for k, t in snap.items():
        if t is None or not k.startswith("stage ") or k == "stage stem":
            continue
        for name, edge in (("top", t[:, 0]), ("bottom", t[:, -1]), ("left", t[:, :, 0]), ("right", t[:, :, -1])):
            assert int((_bits(edge) & 0x7fffffff).max()) == 0, "%s: %s border of %s not zero" % (what, name, k)


def _refuse(se3, eng, n):
    """the context's own input buffers filled by se3tn_preprocess under float32, f16x3 selected, se3tn_infer on those buffers"""
    mean, std = Fx.mean_std(0)
    eng.set_normalization(mean, std)
    rgb, depth = Fx.synthetic_frame(7)
    crop = dict(rgb=torch.from_numpy(rgb).cuda(), depth=torch.from_numpy(depth.view(np.int16)).cuda(), window=(200, 150, 376, 326),
                z_offset_mm=800.0, stats=1)
    eng.preprocess([crop] * n, eng.input_buffer_ptr(0))
    eng.preprocess([crop] * n, eng.input_buffer_ptr(1))
    eng.set_precision(se3._lib.PREC_F16X3)
    with pytest.raises(se3._lib.Se3tnError, match="different precision mode"):
        eng.infer(eng.input_buffer_ptr(0), eng.input_buffer_ptr(1), n)


class _Live:
    """the one context of a sequence, the record of its switches and the trail of steps taken"""
    def __init__(self, se3, refs, twins, env, max_batch):
        self.se3, self.refs, self.twins, self.env, self.max_batch = se3, refs, twins, env, max_batch
        self.eng, self.cfg = _engine(se3, refs[0], env, [], max_batch)
        assert self.cfg == _cfg0(env, max_batch), (self.cfg, _cfg0(env, max_batch))
        self.sd, self.trail = 0, []
        self.run = _Runner(se3, self.eng, refs[0], max_batch)   # (persistent buffers: a captured graph replays with the same pointers)

    def switch(self, ops, n):
        for op in ops:
            if op[0] == "load":
                self.sd = op[1]
                self.eng.load_state_dict(self.refs[self.sd]["sd"])
            elif op[0] == "refuse":
                _refuse(self.se3, self.eng, n)
                self.cfg["f16"] = True
            else:
                _eng_op(self.se3, self.eng, op)
                _cfg_op(self.cfg, op)

    def twin_of(self, chk):
        eng, run = self.twins.get(self.env, self.max_batch, self.sd, self.cfg)
        run(chk)
        return _snapshot(self.se3, eng, run, len(chk))

    def step(self, k, st, graph):
        se3, eng, cfg, n = self.se3, self.eng, self.cfg, st["n"]
        self.trail.append("%2d  %s  n=%d" % (k, " ".join("%s%s" % (op[0], tuple(op[1:])) for op in st["ops"]) or "-", n))
        self.switch(st["ops"], n)
        ref, run = self.refs[self.sd], self.run
        pre, chk = _windows(n, k)
        want_r, written = expected(cfg, n)
        what = "%s n=%d" % ("f16x3" if cfg["f16"] else "f32", n)
        if graph:
            want = self.twin_of(chk)
            for it in ("1 (eager)", "2 (capture)", "3 (replay)"):     # (a key met before: three replays)
                lg, pose = run(chk)
                snap = _snapshot(se3, eng, run, n)
                _assert_same(snap, want, "%s, graphs on, call %s" % (what, it))
            got_w = {s: snap["stage " + s] is not None for s in STAGES}
            assert got_w == written, "after the replay: readable stages %s, written by the route %s" % (got_w, written)
            _borders_zero(snap, what)
            e = float(np.abs(lg.astype(np.float64) - ref["lg64"][chk]).max())
            assert e <= CLASS_TOL[tol_class(cfg, want_r)], "%s: max |d logit| vs float64 %.3e" % (what, e)
        else:
            run(pre)
            eng.profile_enable(1)
            try:
                lg, pose = run(chk)
                names = [nm for nm, _ in eng.profile_launches(0)]
            finally:
                eng.profile_enable(0)
            snap = _snapshot(se3, eng, run, n)
            assert actual(names) == want_r, "%s: route %s, expected %s (%s)" % (what, actual(names), want_r, names)
            _assert_same(snap, self.twin_of(chk), what)
            _borders_zero(snap, what)
            _check_call(se3, eng, ref, cfg, n, chk, lg, pose, names, what, WORST)
        if cfg["f16"]:
            assert not eng.overflow(), what + ": the overflow flag is set"


def _run_sequence(se3, refs, twins, s, graph):
    live = _Live(se3, refs, twins, s["env"], s["max_batch"])
    stream = torch.cuda.Stream() if graph else torch.cuda.current_stream()
    try:
        with torch.cuda.stream(stream):
            if graph:
                live.eng.enable_graphs(True)
            for k, st in enumerate(s["steps"]):
                try:
                    live.step(k, st, graph)
                except AssertionError as e:
                    raise AssertionError("%s%s, step %d: %s\nthe sequence up to here (switch calls, n):\n%s" % (
                        s["name"], " (graphs)" if graph else "", k, e, "\n".join(live.trail))) from None
        torch.cuda.synchronize()
    finally:
        live.eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s,graph", RUNS, ids=[s["name"] + ("-graphs" if g else "") for s, g in RUNS])
def test_sequence_on_one_context(se3, refs, twins, s, graph):
    _run_sequence(se3, refs, twins, s, graph)


@pytest.mark.gpu
def test_graph_cache_eviction(se3, refs, twins):
    """17 keys through a cache of 16 entries: every key three times (eager, capture, replay); back to the first, which was evicted and
    is captured again; then the others, each of which the one before it has pushed out.  Every call bit-equal to the twin."""
    live = _Live(se3, refs, twins, {}, 5)
    visits = EVICT_KEYS + EVICT_KEYS[:1] + EVICT_KEYS[1:]
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            live.eng.enable_graphs(True)
            for k, (n, small, keep, norm) in enumerate(visits):
                try:
                    live.step(k, step([("small", small), ("keep", keep), ("norm",) + norm], n), True)
                except AssertionError as e:
                    raise AssertionError("visit %d: %s\nthe visits up to here:\n%s" % (k, e, "\n".join(live.trail))) from None
        torch.cuda.synchronize()
    finally:
        live.eng.close()


@pytest.mark.gpu
def test_zz_report_worst_transition_logit_error_per_class():
    """(runs last) the worst |d logit| against float64 per tolerance class over all transition steps, beside the bound"""
    for cls, bound in CLASS_TOL.items():
        print("transitions: %-14s worst |d logit| vs float64 %s (bound %.0e)" % (cls, "%.2e" % WORST[cls] if cls in WORST else "not run", bound))
        assert WORST.get(cls, 0.0) <= bound
