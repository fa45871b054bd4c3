"""GPU: every pair of a call against its reference, at the batch sizes where an index map changes (6 .. 256 pairs).

The batch size is the only free shape of the network kernels, and every index map that is easy to get wrong -- the max-pool's strip
length and its `n / 8 * 8` remap, the persistent Winograd GEMM's virtual-tile walk, the 8- / 4-wave stride-2 gather, the trunk
kernel's full-rounds rule, the 96- / 128-row GEMM tiles, fc_finish_kernel's ten pairs per workgroup, the ragged last tile of every
flattened-pixel GEMM -- is a function of it.  tests/test_batch_position_plan.py derives the sizes from those rules (no GPU).

A pool of 12 input pairs has float64 logits and float64 stage maps.  Slot j of a call holds pool pair idx[j] (a seeded draw: for every
shift d up to 64 most slots hold another pair than the slot d further on) and its OWN poseA; the call before the checked one holds
other pool pairs in every slot.  Per (configuration, n), on one live context per configuration with max_batch = 256:
  (a) every slot's logits against float64 within the route's class tolerance (tests/test_gpu_routes.py's, nothing new);
  (b) the route read from the profile names is the route table's; the readable stages are the ones that route writes;
  (c) every slot's poseB within POSE_TOL of processPredict(poseA[j], tanh(float64 logits)), within 1e-12 of processPredict applied
      to the device's own (trans, rot), last row exactly (0, 0, 0, 1);
  (d) BIT identity across slots: for every stage se3tn_debug_buffer hands out and for the logits, all slots that hold the same pool
      pair are equal word for word -- whole maps, borders included, compared on the device.  Every kernel accumulates a row's K in an
      order that does not depend on the row's position (tests/test_gpu_parity.py asserts it at 64 pairs); a tile map that sends one
      slot's rows elsewhere, or reads another slot's, breaks this at the slot it happens in;
  (e) the first occurrence of each pool pair against its float64 stage maps (test_gpu_routes' _close and scales), borders zero --
      with (d) that holds every pixel of every slot to float64;
  (f) se3tn_get_feature equals the interior of `ab`, transposed, bit for bit, for every slot.
f16x3 keeps `pool`, `t64`, `q64`, `ab`, `ab_t` and (conv by conv) `head_t` as split rows (f16 hi | f16 lo, tests/split_rows.py).  (d) compares their raw
words like any other map; (e) decodes the first occurrence of each pool pair and holds it to the same float64 maps with the same
bounds, its raw border words zero bits, and every stored (hi, lo) pair of every slot must be one a split store writes; (f) holds the
library's decode (se3tn_get_feature) to the test's decode of `ab`; and the range guard stays silent.
check_every_slot_of_a_call holds the checks; tests/test_gpu_largest_batch.py runs it at 541 .. 1982 pairs on contexts of that size."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fixtures as Fx
from oracle import se3_oracle as O
import split_rows as SR
import test_batch_position_plan as PLAN
import test_gpu_routes as RT

N_MAX = PLAN.HI
OPS = {"default": [], "keep": [("keep", 1)], "F4": [("wino", 6, 4)], "F6": [("wino", 1, 6)],
       "direct": [("wino", 0, 0), ("trunk", 0, 0)], "f16x3": [("f16",)]}
CASES = [(cfg, n) for cfg in PLAN.CONFIGS for n in PLAN.SIZES[cfg]]
WORST = {}      # class -> worst |d logit| against float64 over the sweep
SECONDS = {}    # (cfg, n) -> wall time of the case
T0 = [None]


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


_ORACLE = {}    # the float64 part of make_ref: computed once per session, shared with tests/test_gpu_largest_batch.py, never changed


def make_ref(n_poses):
    """12 pool pairs of one seeded state dict: float64 logits and stage maps (computed once, never changed), n_poses distinct poses"""
    if not _ORACLE:
        _ORACLE.update(_oracle())
    poses = np.stack([Fx.pose(500 + j, (0.002 * (j % 37) - 0.03, 0.001 * (j % 41) - 0.02, 0.5 + 0.003 * j)) for j in range(n_poses)])
    return dict(_ORACLE, poses=poses)


def _oracle():
    sd = O.make_state_dict(23)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    A, B = Fx.net_inputs(2300, PLAN.POOL)
    lg64, stages = [], {s: [] for s in RT.STAGES}
    for i in range(PLAN.POOL):
        o = O.forward(sd64, A[i:i + 1].double(), B[i:i + 1].double(), intermediates=True)
        lg64.append(torch.cat([o["trans_logit"], o["rot_logit"]], 1))
        cat = lambda a, b: torch.cat([o[a], o[b]], 1)
        one = {"stem": cat("stemA", "stemB"), "pool": cat("poolA", "poolB"), "t64": cat("A2_t", "B3_t"), "q64": o["cat"],
               "ab": o["feature"], "ab_t": o["ab_t"], "head": cat("trans_c2", "rot_c2"), "head_t": cat("trans_t", "rot_t")}
        for s in RT.STAGES:
            stages[s].append(one[s])
    return dict(sd=sd, Ac=A.cuda(), Bc=B.cuda(), lg64=torch.cat(lg64).numpy(), stages={s: torch.cat(v).cuda() for s, v in stages.items()})


@pytest.fixture(scope="module")
def ref():
    """the 12 pool pairs and 256 poses"""
    T0[0] = time.time()
    return make_ref(N_MAX)


class _Buffers:
    """the caller's tensors of every call of the module"""
    def __init__(self, n_max=N_MAX):
        self.A = torch.empty((n_max, 4, 176, 176), device="cuda")
        self.B = torch.empty_like(self.A)
        self.trans = torch.empty((n_max, 3), device="cuda")
        self.rot = torch.empty_like(self.trans)
        self.pA = torch.empty((n_max, 16), dtype=torch.float64, device="cuda")
        self.pB = torch.empty_like(self.pA)


def live_contexts(se3, ref, n_max):
    """cfg -> (context, the route table's record of it): ONE context alive at a time, kept across the sizes of its configuration"""
    state = {"cfg": None, "eng": None, "rec": None, "buf": _Buffers(n_max)}

    def get(cfg):
        if state["cfg"] != cfg:
            if state["eng"] is not None:
                state["eng"].close()
            state["eng"], state["rec"] = RT._engine(se3, ref, {}, OPS[cfg], n_max)
            state["cfg"] = cfg
        return state["eng"], state["rec"], state["buf"]
    yield get
    if state["eng"] is not None:
        state["eng"].close()


@pytest.fixture(scope="module")
def live(se3, ref):
    yield from live_contexts(se3, ref, N_MAX)


def _call(se3, eng, buf, ref, idx, poses):
    n = len(idx)
    ii = torch.from_numpy(np.asarray(idx)).cuda()
    buf.A[:n].copy_(ref["Ac"][ii]); buf.B[:n].copy_(ref["Bc"][ii])
    buf.pA[:n].copy_(torch.from_numpy(poses[:n].reshape(n, 16)))
    buf.pB.zero_()
    eng.infer(buf.A, buf.B, n, se3.NCHW, buf.trans, buf.rot, buf.pA, buf.pB)


_words = RT._words


def check_every_slot_of_a_call(se3, ref, live, cfg, n, worst, seconds, chunk=None):
    """checks (a) .. (f) of the module's docstring on one call of n pairs.  chunk: the stage maps are compared that many slots at a
    time (None: all at once)"""
    t_start = time.time()
    eng, rec, buf = live(cfg)
    spans = [(lo, min(lo + (chunk or n), n)) for lo in range(0, n, chunk or n)]
    assert [j for lo, hi in spans for j in range(lo, hi)] == list(range(n))     # the chunks tile the slots: none skipped, none twice
    idx = PLAN.slot_assignment(n)
    for d in range(1, min(n - 1, 64) + 1):      # a kernel that reads the slot d further on hits other data in most slots
        assert 2 * int((idx[:-d] != idx[d:]).sum()) >= n - d, (n, d)
    pre = PLAN.other_assignment(idx)
    assert (pre != idx).all()
    poses = ref["poses"]
    _call(se3, eng, buf, ref, pre, poses[::-1].copy())      # stale buffers: other pairs, other poses
    eng.profile_enable(1)
    try:
        _call(se3, eng, buf, ref, idx, poses)
        names = [nm for nm, _ in eng.profile_launches(0)]
    finally:
        eng.profile_enable(0)
    lg_d = eng.logits(n)
    lg = lg_d.cpu().numpy()
    trans, rot = buf.trans[:n].cpu().numpy(), buf.rot[:n].cpu().numpy()
    poseB = buf.pB[:n].cpu().numpy().reshape(n, 4, 4)
    tag = "%s n=%d" % (cfg, n)

    # (b) the route
    want_r, written = RT.expected(rec, n)
    got_r = RT.actual(names)
    assert got_r == want_r, "%s: route %s, expected %s (%s)" % (tag, got_r, want_r, names)
    maps = RT._readable(se3, eng, n)
    got_w = {s: maps[s] is not None for s in RT.STAGES}
    assert got_w == written, "%s: readable stages %s, written by the route %s" % (tag, got_w, written)

    # (a) every slot's logits
    cls = RT.tol_class(rec, want_r)
    err = np.abs(lg.astype(np.float64) - ref["lg64"][idx])
    e = float(err.max())
    worst[cls] = max(worst.get(cls, 0.0), e)
    print("%s: max |d logit| vs float64 %.3e (%s, bound %.0e)" % (tag, e, cls, RT.CLASS_TOL[cls]))
    assert e <= RT.CLASS_TOL[cls], "%s: max |d logit| vs float64 %.3e > %.0e (%s), slot %d = pool pair %d" % (
        tag, e, RT.CLASS_TOL[cls], cls, int(err.max(1).argmax()), idx[int(err.max(1).argmax())])

    # (c) every slot's pose, composed with the slot's own poseA
    for j in range(n):
        l64 = ref["lg64"][idx[j]]
        want = O.process_predict(poses[j], np.tanh(l64[:3]), np.tanh(l64[3:]), rec["tn"], rec["rn"])
        d = float(np.abs(poseB[j] - want).max())
        assert d <= RT.POSE_TOL, "%s slot %d (pool pair %d): |d pose| vs float64 %.3e" % (tag, j, idx[j], d)
        own = O.process_predict(poses[j], trans[j], rot[j], rec["tn"], rec["rn"])
        d = float(np.abs(poseB[j] - own).max())
        assert d < 1e-12, "%s slot %d: |d pose| vs processPredict of the device's own trans / rot %.3e" % (tag, j, d)
        assert (poseB[j, 3] == np.array([0, 0, 0, 1.0])).all(), (tag, j)

    # (d) bit identity across the slots that hold the same pool pair (f16x3: the split rows as they are stored, raw)
    first = {}
    for j, k in enumerate(idx.tolist()):
        first.setdefault(k, j)
    src = torch.tensor([first[k] for k in idx.tolist()], device="cuda")
    assert len(first) == min(n, PLAN.POOL)
    assert torch.equal(_words(lg_d), _words(lg_d[src])), "%s: logits differ between slots of one pool pair: slots %s" % (
        tag, (_words(lg_d) != _words(lg_d[src])).any(1).nonzero().flatten().tolist())
    checked = {s: t for s, t in maps.items() if t is not None}
    for s, t in checked.items():
        bad = []
        for lo, hi in spans:    # whole maps, borders included: every word of every slot
            same = (_words(t[lo:hi]) == _words(t[src[lo:hi]])).flatten(1).all(1)
            bad += (lo + (~same).nonzero().flatten()).tolist()
        assert not bad, "%s %s: slots %s differ from the first slot of their pool pair (%s)" % (
            tag, s, bad[:16], [(j, int(src[j])) for j in bad[:4]])

    # (e) the first occurrence of each pool pair against float64, borders zero (f16x3: that one slot of a split map decoded, at most
    # 12 slots per map; the raw split rows of ALL slots checked span by span)
    sc = lambda keys: max(RT.STAGE_SCALE[want_r[k].replace(" block", "")] for k in keys)
    sc_trunk, sc_all = sc(("trunk1", "trunk2", "trunk3", "trunk4")), sc([k for k, _ in RT.LAYERS])
    split = RT.split_stages(rec, want_r)
    for s, t in checked.items():
        if s in split:
            for lo, hi in spans:
                RT._check_split_map("%s %s slots %d..%d" % (tag, s, lo, hi - 1), t[lo:hi])
        for k, j in first.items():
            got = RT._nchw(RT._stage_values(split, s, t[j:j + 1]), 0 if s == "stem" else 1)
            RT._close("%s %s slot %d (pool pair %d)" % (tag, s, j, k), got, ref["stages"][s][k:k + 1], RT.ACT_RTOL,
                      1e-5 if s in ("stem", "pool") else 0, sc_trunk if s in ("stem", "pool", "t64", "q64") else sc_all)

    # (f) se3tn_get_feature: the interior of `ab`, transposed (f16x3: the library's decode kernel against the test's, span by span)
    feat = eng.feature(n)
    for lo, hi in spans:
        ab = RT._stage_values(split, "ab", maps["ab"][lo:hi])
        assert torch.equal(_words(feat[lo:hi]), _words(ab[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2))), (tag, lo)
    if rec["f16"]:
        assert not eng.overflow(), tag
    torch.cuda.synchronize()
    seconds[(cfg, n)] = time.time() - t_start


@pytest.mark.parametrize("cfg,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_every_slot_of_a_call(se3, ref, live, cfg, n):
    check_every_slot_of_a_call(se3, ref, live, cfg, n, WORST, SECONDS)


def test_create_refuses_a_max_batch_above_the_limit_on_the_device(se3):
    """the refusal comes before any allocation (the bound itself: tests/test_largest_batch_plan.py derives it from the kernels' 32-bit
    expressions, tests/test_gpu_largest_batch.py runs 541 .. 1982 pairs on contexts of that size; every case passes)"""
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(se3._lib.Se3tnError, match="SE3TN_MAX_BATCH_LIMIT"):
        se3.Engine(0, se3._lib.MAX_BATCH_LIMIT + 1)
    assert torch.cuda.mem_get_info()[0] == free0
    eng = se3.Engine(0, 2)
    assert eng.lib.se3tn_max_batch(eng._h) == 2
    eng.close()


def test_zz_report_worst_logit_error_per_class_over_the_positions():
    """(runs last) the worst |d logit| against float64 per tolerance class over the sweep, beside its bound; the slowest case"""
    for cls, bound in RT.CLASS_TOL.items():
        print("%-14s worst |d logit| vs float64 %s (bound %.0e)" % (cls, "%.2e" % WORST[cls] if cls in WORST else "not run", bound))
        assert WORST.get(cls, 0.0) <= bound
    if SECONDS:
        slow = max(SECONDS, key=SECONDS.get)
        print("%d cases, slowest %s-%d %.2f s, sum %.1f s, module %.1f s since the reference was started" % (
            len(SECONDS), slow[0], slow[1], SECONDS[slow], sum(SECONDS.values()), time.time() - T0[0]))
