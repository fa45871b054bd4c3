"""GPU: the range guard of SE3TN_PREC_F16X3 at every split store of se3tn_infer, and the range in which the mode is float32-class.

The header's promise: a split-row store outside the f16 range raises the flag se3tn_overflow reads and clears, and the caller reruns in
SE3TN_PREC_F32.  tests/f16x3_range_cases.py builds, per split store, a network whose first out-of-range stored value occurs at that
store (tests/test_f16x3_range_cases.py proves it in float64).  Each case runs at the smallest batches that reach the f16x3 kernel
families -- split-K with its reduce epilogue, the fused F(4x4) head block, the big-tile slab / gather epilogues; the sizes follow from
the plan rule (f16x3_family) and tests/route_model.py, and the profile names of every call are held to both:

  over range   the flag is up after the call and down on the second read; the same call in SE3TN_PREC_F32 then meets the float32 class
               bound of its route against float64 (the hot channel is dead downstream, so every pair is compared);
  in range     the flag stays down and every pair's logits meet CLASS_TOL["f16x3"] against float64;
  input site   65000 and -65000 raise nothing, nextafter(65000), inf and NaN do: both layouts of se3tn_infer, se3tn_preprocess;
  life cycle   the flag outlives clean calls and precision switches until read, is raised by a replayed graph, never in PREC_F32,
               and belongs to one context;
  the edges    measured and printed (high side: the F(4x4) planes of the fused head route; low side: f16 subnormals of small
               activations), asserting only that nothing in range raises the flag.

Measured (MI355X, seed 31, n = 6), max |d logit| against float64; PREC_F32 direct on the same weights: 3e-7 .. 7e-7 in every row:
  high side: the head conv1 stage scaled by 2^k.  Fused head route: no flag up to k = 6 (stage maximum 5.4e3, largest F(4x4) plane
      5.6e4, error 3.6e-7), flag from k = 7 (1.09e4 / 1.12e5; the unflagged result would be off by 0.6).  The planes run 10.3 x above
      the map here (bound 49 x).  Heads conv by conv: no flag up to k = 9 (4.3e4, error 4.1e-7), flag at k = 10 (8.7e4).
  low side: a stage scaled by 2^-k, no flag at any k.  head conv1 (fused | conv by conv): k = 0 .. 8 (maximum >= 0.5) 4.7e-7 | 4.5e-7,
      k = 12 (3.9e-2) 1.1e-6 | 9.0e-7, k = 16 (2.4e-3) 1.3e-5 | 8.8e-6, k = 20 (1.5e-4) 3.5e-4 | 2.0e-4: outside the 5e-5 class,
      k = 24 (9.5e-6) 5.2e-3 | 4.9e-3, k = 28 0.15 | 0.11.  head_t: the same picture (k = 16: 7.1e-6 | 8.1e-6, k = 20: 3.0e-4 | 1.0e-4).

With one atomicOr(overflow) removed from the library at a time, this file fails in: to_padded_input -> the input-site test (layouts);
preprocess -> the input-site test (preprocess); conv3x3 store_tiles (big tiles) and reduce_element (split-K) -> over:A2_t, B2_t, B2, B3_t,
A2, B3, ab1, ab_t, ab, head, head_t each; wino_input_kernel -> over:V_in; the mid transform -> over:V_mid; the max-pool -> over:poolA, poolB.
wino_output_kernel's split form is launched only for a fused block without the tail, i.e. the 256-channel block, which plan_infer never
fuses in f16x3 mode (csrc/infer_plan.h: `!(which == 0 && fast)`): unreachable, and its removal goes unnoticed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f16x3_range_cases as R
from route_model import LAYERS, actual, expected
from test_gpu_routes import CLASS_TOL, _cfg_op, _eng_op, _engine, tol_class

N_MAX = 64


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


class _Ctx:
    """one context in f16x3 mode, its switch record, fixed input / output buffers"""
    def __init__(self, se3, sd):
        self.se3 = se3
        self.eng, self.cfg = _engine(se3, {"sd": sd}, {}, [("f16",)], N_MAX)
        self.wino = self.eng.get_winograd()
        self.A = torch.empty((N_MAX, 4, 176, 176), device="cuda")
        self.B = torch.empty_like(self.A)
        self.trans = torch.empty((N_MAX, 3), device="cuda")
        self.rot = torch.empty_like(self.trans)

    def op(self, *op):
        _eng_op(self.se3, self.eng, op)
        _cfg_op(self.cfg, op)

    def load(self, sd):
        self.eng.load_state_dict(sd)

    def fill(self, A2, B2, n):
        """the batch: the case's two pairs, repeated"""
        idx = torch.arange(n) % A2.shape[0]
        self.A[:n].copy_(A2[idx]); self.B[:n].copy_(B2[idx])
        return idx.numpy()

    def call(self, n, names=False):
        """one se3tn_infer on the buffers; -> (logits [n,6], launch names | None)"""
        if names:
            self.eng.profile_enable(1)
        try:
            self.eng.infer(self.A, self.B, n, self.se3.NCHW, self.trans, self.rot)
            nm = [x for x, _ in self.eng.profile_launches(0)] if names else None
        finally:
            if names:
                self.eng.profile_enable(0)
        return self.eng.logits(n).cpu().numpy().astype(np.float64), nm

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def ctx(se3):
    c = _Ctx(se3, R.base()["sd"])
    yield c
    c.close()


def _sizes(ctx):
    """(first batch whose heads run as the fused F(4x4) block, first batch at which every conv runs a big-tile kernel)"""
    cfg = dict(ctx.cfg, f16=True, wmin=ctx.wino[0], tile=ctx.wino[1])
    n_fused = next(n for n in range(1, N_MAX + 1) if expected(cfg, n)[0]["h2.1"] == "F4 block")
    return n_fused, R.smallest_all_big_tile(N_MAX)


def _runs(ctx, routes):
    """(n, Winograd blocks on) per head route: split-K and big-tile epilogues under each"""
    n_fused, n_big = _sizes(ctx)
    assert n_fused > 1 and all(R.f16x3_family(k, n_fused) == "split-K" for k in R.GEOM)
    out = []
    if "fused" in routes:
        out += [(n_fused, True), (n_big, True)]
    if "plain" in routes:
        out += [(n_fused - 1, True), (n_big, False)]
    return out


def _set_route(ctx, wino_on, f16):
    ctx.op("wino", ctx.wino[0] if wino_on else 0, ctx.wino[1])
    ctx.op("f16", 1 if f16 else 0)


def _family(names, key):
    nm = [x for x in names if x == dict(LAYERS)[key] or x.startswith(dict(LAYERS)[key] + " ")]
    assert len(nm) == 1, (key, names)
    for fam in ("split-K", "slab", "gather"):
        if "[%s f16x3]" % fam in nm[0]:
            return fam
    return "block" if "fused block" in nm[0] else nm[0]


def _check_route(ctx, n, names, stage, fused):
    """the profile names: the route table's algorithms, every conv in the kernel family the plan rule names, the target's store present"""
    want, _ = expected(ctx.cfg, n)
    assert actual(names) == want, (n, actual(names), want, names)
    assert (want["h2.1"] == "F4 block") == fused, (n, want)
    for key in R.GEOM:
        fam = _family(names, key)
        assert fam == ("block" if fused and key.startswith("h2") else R.f16x3_family(key, n)), (key, n, fam, names)
    if stage in ("inA", "inB"):
        assert "to_padded_input" in names
    if stage in ("poolA", "poolB"):
        assert "maxpool3x3s2" in names, names


def _f32_bound(ctx, n):
    cfg = dict(ctx.cfg)
    assert not cfg["f16"]
    return CLASS_TOL[tol_class(cfg, expected(cfg, n)[0])]


@pytest.mark.parametrize("cid", R.OVER_IDS)
def test_over_range_raises_the_flag_and_f32_is_the_remedy(ctx, cid):
    c = R.build(cid)
    ctx.load(c["sd"])
    A2, B2 = c["A"].cuda(), c["B"].cuda()
    for n, wino_on in _runs(ctx, c["routes"]):
        what = "%s n=%d wino=%d" % (cid, n, wino_on)
        idx = ctx.fill(A2, B2, n)
        _set_route(ctx, wino_on, True)
        assert not ctx.eng.overflow(), what + ": flag up before the call"
        _, names = ctx.call(n, names=True)
        _check_route(ctx, n, names, c["stage"], fused=wino_on and n >= _sizes(ctx)[0])
        assert ctx.eng.overflow(), "%s: %s reaches %.4g and no flag was raised" % (what, c["stage"], c["maxima"][c["stage"]])
        assert not ctx.eng.overflow(), what + ": the read did not clear the flag"
        # the remedy: the same call in float32
        _set_route(ctx, wino_on, False)
        lg, _ = ctx.call(n)
        err = float(np.abs(lg - c["lg64"][idx]).max())
        bound = _f32_bound(ctx, n)
        print("%s: PREC_F32 max |d logit| vs float64 %.2e (bound %.0e)" % (what, err, bound))
        assert err <= bound, (what, err, bound)
        assert not ctx.eng.overflow(), what + ": flag raised in PREC_F32"
    _set_route(ctx, True, True)


@pytest.mark.parametrize("cid", R.IN_IDS)
def test_in_range_stays_silent_and_float32_class(ctx, cid):
    c = R.build(cid)
    ctx.load(c["sd"])
    A2, B2 = c["A"].cuda(), c["B"].cuda()
    for n, wino_on in _runs(ctx, c["routes"]):
        what = "%s n=%d wino=%d" % (cid, n, wino_on)
        idx = ctx.fill(A2, B2, n)
        _set_route(ctx, wino_on, True)
        lg, names = ctx.call(n, names=True)
        _check_route(ctx, n, names, c["stage"], fused=wino_on and n >= _sizes(ctx)[0])
        err = float(np.abs(lg - c["lg64"][idx]).max())
        print("%s: %s max %.4g, f16x3 max |d logit| vs float64 %.2e" % (what, c["stage"], c["maxima"][c["stage"]], err))
        assert not ctx.eng.overflow(), "%s: flag raised with every stored value <= %.0f" % (what, R.IN_RANGE[1])
        assert err <= CLASS_TOL["f16x3"], (what, err)
    _set_route(ctx, True, True)


# ---- the input site, exactly ---------------------------------------------------------------------------------------------------------
EDGE = np.nextafter(np.float32(R.GUARD), np.float32(np.inf))
INPUT_VALUES = [(R.GUARD, False), (-R.GUARD, False), (float(EDGE), True), (float("inf"), True), (float("nan"), True)]


def test_input_site_threshold_both_layouts(ctx):
    """one element of one image at the value, everything else 0: se3tn_infer's copy into the padded buffers (NCHW and NHWC)"""
    se3 = ctx.se3
    ctx.load(R.base()["sd"])
    _set_route(ctx, True, True)
    assert float(EDGE) > R.GUARD and not ctx.eng.overflow()
    for layout, shape in ((se3.NCHW, (1, 4, 176, 176)), (se3.NHWC, (1, 176, 176, 4))):
        for which in (0, 1):
            for pos in (0, -1):              # the first and the last element of the tensor
                for v, flagged in INPUT_VALUES:
                    x = [torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")]
                    x[which].view(-1)[pos] = v
                    ctx.eng.infer(x[0], x[1], 1, layout, ctx.trans, ctx.rot)
                    got = ctx.eng.overflow()
                    assert got == flagged, "layout %d image %s element %d value %r: flag %s" % (layout, "AB"[which], pos, v, got)
                    assert not ctx.eng.overflow()


def test_input_site_threshold_preprocess(ctx):
    """se3tn_preprocess into the context's own buffers: a std that puts ONE normalised value at 65000 / -65000 (no flag) and one
    float32 step beyond (flag).  (x - mean) / std is formed in float64 and rounded to float32 once (kernels_misc.hip)."""
    eng = ctx.eng
    _set_route(ctx, True, True)
    depth = torch.zeros((176, 176), dtype=torch.int16, device="cuda")      # invalid everywhere -> 2000, normalised to 0 below
    for stats in (0, 1):
        for sign in (1, -1):
            for target, flagged in ((R.GUARD, False), (float(EDGE), True)):
                # sign +: background 0, one pixel 130, mean 0.  sign -: background 255, one pixel 125, mean 255: -130 / std
                bg, px, mu = (0, 130, 0.0) if sign > 0 else (255, 125, 255.0)
                std = 130.0 / target
                assert np.float32((px - mu) / std) == np.float32(sign * target) and (bg - mu) / std == 0
                rgb = torch.full((176, 176, 3), bg, dtype=torch.uint8)
                rgb[5, 7, 0] = px
                mean = np.zeros(8); sd_ = np.ones(8)
                mean[4 * stats], sd_[4 * stats], mean[4 * stats + 3] = mu, std, 2000.0
                eng.set_normalization(mean, sd_)
                crop = dict(rgb=rgb.cuda(), depth=depth, window=(0, 0, 176, 176), z_offset_mm=0.0, stats=stats)
                eng.preprocess([crop], eng.input_buffer_ptr(stats))
                got = eng.overflow()
                assert got == flagged, "stats %d value %r: flag %s" % (stats, sign * target, got)
                assert not eng.overflow()


# ---- life cycle ------------------------------------------------------------------------------------------------------------------------
def test_flag_life_cycle(ctx):
    """over:inA -- its state dict with clean inputs is an ordinary call, with the hot depth channel an over-range one"""
    se3, eng = ctx.se3, ctx.eng
    c = R.build("over:inA")
    clean_A, hot_A, B2 = R.base()["A"].cuda(), c["A"].cuda(), c["B"].cuda()
    ctx.load(c["sd"])
    _set_route(ctx, True, True)
    n = 2
    clean = lambda: (ctx.fill(clean_A, B2, n), ctx.call(n))
    hot = lambda: (ctx.fill(hot_A, B2, n), ctx.call(n))
    clean()
    assert not eng.overflow()
    # survives later clean calls until it is read
    hot(); clean(); clean()
    assert eng.overflow() and not eng.overflow()
    # survives a precision switch and back
    hot()
    ctx.op("f16", 0); ctx.op("f16", 1)
    assert eng.overflow() and not eng.overflow()
    # never raised in PREC_F32 on the same inputs
    ctx.op("f16", 0)
    hot()
    assert not eng.overflow()
    ctx.op("f16", 1)
    # raised by a replayed graph after the buffers' contents change
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.enable_graphs(True)
        try:
            for _ in range(3):       # eager, captured, replayed
                clean()
            s.synchronize()
            assert not eng.overflow()
            hot()                    # the same pointers: a replay
            s.synchronize()
            assert eng.overflow() and not eng.overflow()
        finally:
            eng.enable_graphs(False)
    torch.cuda.synchronize()
    # not shared between two contexts
    other = _Ctx(se3, c["sd"])
    try:
        hot()
        other.fill(clean_A, B2, n); other.call(n)
        assert not other.eng.overflow()
        assert eng.overflow()
        other.fill(hot_A, B2, n); other.call(n)
        assert not eng.overflow()
        assert other.eng.overflow() and not other.eng.overflow()
    finally:
        other.close()


# ---- the two edges, measured -------------------------------------------------------------------------------------------------------
def _three_ways(ctx, c, n):
    """-> (flag, err f16x3 fused heads, err f16x3 heads conv by conv, err PREC_F32 direct kernels), errors = max |d logit| vs float64"""
    idx = ctx.fill(c["A"].cuda(), c["B"].cuda(), n)
    out = []
    _set_route(ctx, True, True)
    lg, names = ctx.call(n, names=True)
    assert expected(ctx.cfg, n)[0]["h2.1"] == "F4 block" and actual(names) == expected(ctx.cfg, n)[0]
    flag = ctx.eng.overflow()
    out.append(float(np.abs(lg - c["lg64"][idx]).max()))
    _set_route(ctx, False, True)
    lg, _ = ctx.call(n)
    flag_plain = ctx.eng.overflow()
    out.append(float(np.abs(lg - c["lg64"][idx]).max()))
    _set_route(ctx, False, False)
    ctx.op("trunk", 0, 0)
    try:
        lg, names = ctx.call(n, names=True)
        assert tol_class(ctx.cfg, actual(names)) == "f32 direct", names
    finally:
        ctx.op("trunk", *ctx.trunk0)
    out.append(float(np.abs(lg - c["lg64"][idx]).max()))
    assert not ctx.eng.overflow()
    _set_route(ctx, True, True)
    return flag, flag_plain, out


def test_high_side_edge_measured(ctx):
    """Fused head route: the head conv1 stage scaled by 2^k.  The guard tests the F(4x4) planes of the map (B^T d B: rows of B^T with
    absolute sums up to 7, so up to 49 x the map), and raises the flag for maps well inside 65000.  Prints the table; asserts only that
    no flag rises while every stored value -- planes included -- is at or below OTHERS_MAX."""
    ctx.trunk0 = ctx.eng.get_trunk_winograd()
    n = _sizes(ctx)[0]
    BT = R.base()["BT"]
    assert np.abs(BT).sum(1).max() == 7.0
    print("\n k  max|head|   max|V_in|  flag fused  flag plain  err fused   err plain   err f32 direct")
    first = None
    for k in range(4, 11):
        c = R.build("scaled:head:%d" % k)
        ctx.load(c["sd"])
        flag, flag_plain, (e_f, e_p, e_32) = _three_ways(ctx, c, n)
        mx = c["maxima"]
        print("%2d  %.3e  %.3e  %-10s  %-10s  %.2e   %.2e   %.2e" % (k, mx["head"], mx["V_in"], flag, flag_plain, e_f, e_p, e_32))
        if max(mx[s] for s in R.stored(True)) <= R.OTHERS_MAX:
            assert not flag, k
        if max(mx[s] for s in R.stored(False)) <= R.OTHERS_MAX:
            assert not flag_plain, k
        if flag and first is None:
            first = (k, mx["head"], mx["V_in"])
        if flag_plain:
            break
    print("fused head route: first flag at 2^%d, stage maximum %.4g, largest plane %.4g" % first if first else "no flag")


@pytest.mark.parametrize("stage", ["head", "head_t"])
def test_low_side_edge_measured(ctx, stage):
    """A stage scaled by 2^-k (its reader's weights by 2^k): only the weights are scaled per row, so the lo half of small activations
    falls into f16 subnormals (granularity 2^-24 absolute) and f16x3 leaves the float32 class without any flag.  Prints the table
    against float64 beside the PREC_F32 direct route on the same weights; asserts only that no flag rises."""
    ctx.trunk0 = ctx.eng.get_trunk_winograd()
    n = _sizes(ctx)[0]
    print("\n  k  max|%s|  err fused   err plain   err f32 direct   (class bound %.0e)" % (stage, CLASS_TOL["f16x3"]))
    out_of_class = None
    for k in range(0, 29, 4):
        c = R.build("scaled:%s:%d" % (stage, -k))
        ctx.load(c["sd"])
        flag, flag_plain, (e_f, e_p, e_32) = _three_ways(ctx, c, n)
        print("%3d  %.3e  %.2e   %.2e   %.2e" % (k, c["maxima"][stage], e_f, e_p, e_32))
        assert not flag and not flag_plain, k
        if out_of_class is None and max(e_f, e_p) > CLASS_TOL["f16x3"]:
            out_of_class = k
    print("%s: f16x3 first exceeds the class bound at 2^-%s" % (stage, out_of_class))
