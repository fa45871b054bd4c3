"""se3tn_on_track_objects / MultiTracker: several DIFFERENT objects (own weights, mean / std, normalisers, mesh) in one camera frame per
call.  The contract: every object gets exactly the bits se3tn_on_track on its own model context gives it -- whatever n, the chunking
into launches of <= 5, the order or the company -- because the batch 1-5 kernel family works image by image and each image reads its
own model's parameters.  Models: the two trained stand-ins (tests/golden/synth_tracker.npz, 30-degree regime, and
synth_tracker_5deg.npz, 5-degree regime: different weights, mean / std and normalisers) and a random-init third one; meshes: the
synthetic ellipsoid of oracle/synth_track.py and an icosphere of another size and face count (the repository's bunny has no faces)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import closed_loop as CL
from oracle import fixtures as Fx
from oracle import free_run as FR
from oracle import se3_oracle as O
from oracle import synth_track as ST
from oracle import ycbv_fixtures as YF

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -2


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


@pytest.fixture(scope="module")
def models():
    """name -> (state_dict, mean, std, trans_normalizer, rot_normalizer)"""
    out = {}
    for name, regime in (("30deg", "ycbineoat_30deg"), ("5deg", "ycb_video_5deg")):
        sd, mean, std, _ = FR.load_synth_weights(FR.default_synth_weights(regime))
        out[name] = (sd, mean, std) + tuple(CL.REGIMES[regime])
    mean, std = Fx.mean_std(3)
    out["random"] = (O.make_state_dict(5, head_gain=CL.HEAD_GAIN), mean, std, 0.05, 12 * np.pi / 180)
    return out


MESHES = {"ellipsoid": ST.make_object(4), "sphere": Fx.icosphere(3, 0.05, 1)}
YF_WIDTH = 120.0


def make_tracker(se3, models, model, mesh, width=ST.OBJECT_WIDTH_MM):
    sd, mean, std, tn, rn = models[model]
    trk = se3.Tracker(dict(Fx.DATASET_INFO, object_width=width), mean, std, {"state_dict": sd}, trans_normalizer=tn,
                      rot_normalizer=rn, max_samples=1)
    trk.renderer = se3.HipRenderer(trk.engine, MESHES[mesh])
    trk.spec = (model, mesh, width)          # (test bookkeeping)
    return trk


@pytest.fixture(scope="module")
def trackers(se3, models):
    specs = [("30deg", "ellipsoid", 150.0), ("5deg", "sphere", 120.0), ("random", "ellipsoid", 140.0), ("5deg", "ellipsoid", 150.0),
             ("30deg", "sphere", 110.0), ("random", "sphere", 130.0), ("30deg", "ellipsoid", 160.0)]
    return [make_tracker(se3, models, *s) for s in specs]


def frame_and_poses(n, seed=0):
    rgb, depth = Fx.structured_frame(400 + seed)
    poses = [Fx.pose(50 + 7 * seed + i, (0.09 * np.cos(1.3 * i + seed), 0.06 * np.sin(0.9 * i + seed), 0.7 + 0.04 * i)) for i in range(n)]
    return rgb, depth, poses


def single(trk, P, rgb, depth):
    """what se3tn_on_track on the object's own context gives: pose, trans, rot, bbox, image A"""
    pose = trk.on_track(P, rgb, depth)
    lp = trk.last_prediction
    return dict(pose=pose, trans=lp["trans"].reshape(3).copy(), rot=lp["rot"].reshape(3).copy(), bbox=lp["bbox"].copy(),
                rgbA=trk.renderer.rgb.cpu().numpy().copy(), depthA=trk.renderer.depth.cpu().numpy().copy())


def multi(se3, trks, poses, rgb, depth):
    mt = se3.MultiTracker(trks)
    n = len(trks)
    bb = np.empty((n, 4, 2), np.int32)
    out = mt.on_track(np.stack(poses), rgb, depth, bbox_out=bb)
    lp = mt.last_prediction
    res = [dict(pose=out[i], trans=lp["trans"][i], rot=lp["rot"][i], bbox=bb[i], rgbA=lp["rgbA"][i].cpu().numpy(),
                depthA=lp["depthA"][i].cpu().numpy()) for i in range(n)]
    mt.close()
    return res


def assert_same(got, want, what):
    for k in ("pose", "trans", "rot", "bbox", "rgbA", "depthA"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7])
def test_each_object_gets_the_bits_of_its_own_single_object_call(se3, trackers, n):
    rgb, depth, poses = frame_and_poses(n, seed=n)
    trks = trackers[:n]
    got = multi(se3, trks, poses, rgb, depth)
    for i, t in enumerate(trks):
        assert_same(got[i], single(t, poses[i], rgb, depth), (n, i, t.spec))
    if n > 1:   # mixed models really differ: the same inputs through another model give other outputs
        assert not np.array_equal(got[0]["trans"], single(trks[1], poses[0], rgb, depth)["trans"])


def test_order_and_company_do_not_matter(se3, trackers):
    rgb, depth, poses = frame_and_poses(5, seed=11)
    trks = trackers[:5]
    base = multi(se3, trks, poses, rgb, depth)
    perm = [3, 0, 4, 2, 1]
    got = multi(se3, [trks[p] for p in perm], [poses[p] for p in perm], rgb, depth)
    for j, p in enumerate(perm):
        assert_same(got[j], base[p], ("permuted", j))
    # the same object (tracker = model + mesh) listed twice, with the same pose and with another one, and in another company
    got = multi(se3, [trks[1], trks[2], trks[1], trks[1]], [poses[1], poses[2], poses[1], poses[4]], rgb, depth)
    assert_same(got[0], base[1], "twice a")
    assert_same(got[2], base[1], "twice b")
    assert_same(got[1], base[2], "company")
    assert_same(got[3], single(trks[1], poses[4], rgb, depth), "other pose")


def test_a_model_context_off_the_default_one_pair_route(se3, models):
    """The bit-equality contract holds while the model context runs one pair through the batch 1-5 family (its default): under
    se3tn_set_winograd(1, 2) se3tn_on_track on that context takes the F(2x2) blocks and the plain tail -- other bits, the same
    tolerance -- while se3tn_on_track_objects still runs the family (the bits of the default route).  At the parent commit the
    single-object call under this setting read stale partial sums in its tail (wrong trans / rot / pose)."""
    rgb, depth, poses = frame_and_poses(2, seed=23)
    trks = [make_tracker(se3, models, "random", "sphere", 130.0), make_tracker(se3, models, "5deg", "ellipsoid", 150.0)]
    base = [single(t, poses[i], rgb, depth) for i, t in enumerate(trks)]
    trks[0].engine.set_winograd(1, 2)
    got = multi(se3, trks, poses, rgb, depth)
    for i in range(2):
        assert_same(got[i], base[i], ("default-route bits", i))
    off = single(trks[0], poses[0], rgb, depth)
    assert not np.array_equal(off["trans"], base[0]["trans"]) or not np.array_equal(off["rot"], base[0]["rot"])
    for k in ("trans", "rot"):
        assert np.abs(off[k] - base[0][k]).max() < 3e-5, k
    assert np.abs(off["pose"] - base[0]["pose"]).max() < 1e-5
    sd, mean, std, tn, rn = models["random"]
    want, aux = O.on_track(sd, poses[0], rgb, depth, off["rgbA"], off["depthA"].view(np.uint16), trks[0].K, trks[0].object_width, mean,
                           std, tn, rn)
    assert np.abs(off["trans"] - aux["trans"]).max() < 2e-5 and np.abs(off["rot"] - aux["rot"]).max() < 2e-5
    assert np.abs(off["pose"] - want).max() < 1e-5


def test_against_the_oracle_per_object(se3, trackers, models):
    rgb, depth, poses = frame_and_poses(5, seed=3)
    trks = trackers[:5]
    got = multi(se3, trks, poses, rgb, depth)
    for i, t in enumerate(trks):
        sd, mean, std, tn, rn = models[t.spec[0]]
        want, aux = O.on_track(sd, poses[i], rgb, depth, got[i]["rgbA"], got[i]["depthA"].view(np.uint16), t.K, t.object_width, mean,
                               std, tn, rn)
        assert np.abs(got[i]["trans"] - aux["trans"]).max() < 1e-4 and np.abs(got[i]["rot"] - aux["rot"]).max() < 1e-4, (i, t.spec)
        assert np.abs(got[i]["pose"] - want).max() < 1e-5, (i, t.spec)


def test_closed_loop_of_two_composited_sequences_equals_two_separate_loops(se3, models):
    frames = 50
    K = np.array([[Fx.DATASET_INFO["camera"]["focalX"], 0, Fx.DATASET_INFO["camera"]["centerX"]],
                  [0, Fx.DATASET_INFO["camera"]["focalY"], Fx.DATASET_INFO["camera"]["centerY"]], [0, 0, 1.0]])
    regimes = (("30deg", "ycbineoat_30deg", 2), ("5deg", "ycb_video_5deg", 5))
    seqs = [ST.make_sequence(seed, frames + 1, K, regime=reg) for _, reg, seed in regimes]
    bg = ST.backgrounds()

    def frame(f):   # the second object pasted over a frame that shows the first
        rgb, depth = ST.compose_frame(bg[f % len(bg)], seqs[0].patches[f])
        return ST.compose_frame((rgb, depth), seqs[1].patches[f])

    solo = [make_tracker(se3, models, name, "ellipsoid") for name, _, _ in regimes]
    together = [make_tracker(se3, models, name, "ellipsoid") for name, _, _ in regimes]
    mt = se3.MultiTracker(together)
    P_solo = [ST.gt_pose(seed, 0, reg) for _, reg, seed in regimes]
    P_multi = [p.copy() for p in P_solo]
    moved = 0.0
    for f in range(1, frames + 1):
        rgb, depth = frame(f)
        P_solo = [t.on_track(P, rgb, depth) for t, P in zip(solo, P_solo)]
        P_multi = list(mt.on_track(np.stack(P_multi), rgb, depth))
        for k in range(2):
            assert np.array_equal(P_multi[k], P_solo[k]), (f, k)
        moved = max(moved, float(np.abs(P_multi[0][:3, 3] - ST.gt_pose(2, 0, "ycbineoat_30deg")[:3, 3]).max()))
    assert moved > 1e-3      # (the loop does move)
    mt.close()


def _call(se3, ctx, objs, poses, rgb, depth, K):
    lib = se3._lib.load()
    n = len(objs)
    arr = (se3._lib.Object * max(n, 1))(*objs)
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    out = np.zeros((max(n, 1), 16))
    Kc = np.ascontiguousarray(K, np.float64)
    return lib.se3tn_on_track_objects(ctx._h, n, arr, C.c_void_p(P.ctypes.data), Kc.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.c_void_p(rgb.ctypes.data), C.c_void_p(depth.ctypes.data), rgb.shape[0], rgb.shape[1], None, None,
                                      C.c_void_p(out.ctypes.data), None, None, None, None), out


def test_refusals_leave_the_context_usable(se3, trackers, models):
    rgb, depth, poses = frame_and_poses(2, seed=21)
    t0, t1 = trackers[0], trackers[1]
    K = t0.K
    ctx = se3.Engine(0, 2)
    obj = lambda t, mesh=None: se3._lib.Object(t.engine._h.value, mesh if mesh is not None else t.renderer._m.value, float(t.object_width))
    ok = [obj(t0), obj(t1)]
    # SE3TN_E_ARG: n out of range, a null mesh, a textured mesh, poses with z <= 0 / not finite
    assert _call(se3, ctx, [], [], rgb, depth, K)[0] == E_ARG
    assert _call(se3, ctx, ok + [obj(t0)], poses + [poses[0]], rgb, depth, K)[0] == E_ARG
    assert _call(se3, ctx, [ok[0], se3._lib.Object(t1.engine._h.value, None, 120.0)], poses, rgb, depth, K)[0] == E_ARG
    m = MESHES["sphere"]
    tex = se3.HipRenderer(t1.engine, dict(m, uv=np.zeros((len(m["vertices"]), 2)), texture=np.full((4, 4, 3), 200, np.uint8)),
                          mode="pyrender", frame_size=rgb.shape[:2])
    assert _call(se3, ctx, [ok[0], obj(t1, tex._m.value)], poses, rgb, depth, K)[0] == E_ARG
    for bad in (0.0, -0.5, np.nan, np.inf):
        P = [poses[0], poses[1].copy()]
        P[1][2, 3] = bad
        assert _call(se3, ctx, ok, P, rgb, depth, K)[0] == E_ARG, bad
    # SE3TN_E_STATE: models without weights / normalisation, other rules; ctx in f16x3, small kernels off, keep_intermediates
    bare = se3.Engine(0, 1)
    assert _call(se3, ctx, [ok[0], se3._lib.Object(bare._h.value, t1.renderer._m.value, 120.0)], poses, rgb, depth, K)[0] == E_STATE
    sd, mean, std, tn, rn = models["5deg"]
    no_norm = se3.Engine(0, 1)
    no_norm.load_state_dict(sd)
    assert _call(se3, ctx, [ok[0], se3._lib.Object(no_norm._h.value, t1.renderer._m.value, 120.0)], poses, rgb, depth, K)[0] == E_STATE
    t1.engine.set_offset_rule("numpy2")
    assert _call(se3, ctx, ok, poses, rgb, depth, K)[0] == E_STATE
    t1.engine.set_offset_rule("numpy1")
    t1.engine.set_raster_rule(8)
    assert _call(se3, ctx, ok, poses, rgb, depth, K)[0] == E_STATE
    t1.engine.set_raster_rule(4)
    ctx.set_precision(se3._lib.PREC_F16X3)
    assert _call(se3, ctx, ok, poses, rgb, depth, K)[0] == E_STATE
    ctx.set_precision(se3._lib.PREC_F32)
    ctx.set_small_kernels(False)
    assert _call(se3, ctx, ok, poses, rgb, depth, K)[0] == E_STATE
    ctx.set_small_kernels(True)
    ctx.keep_intermediates(True)
    assert _call(se3, ctx, ok, poses, rgb, depth, K)[0] == E_STATE
    ctx.keep_intermediates(False)
    # the same context then serves a valid call, with the right results
    rc, out = _call(se3, ctx, ok, poses, rgb, depth, K)
    assert rc == 0
    for i, t in enumerate((t0, t1)):
        assert np.array_equal(out[i].reshape(4, 4), single(t, poses[i], rgb, depth)["pose"]), i
    for e in (ctx, bare, no_norm):
        e.close()


def test_ycbv_objects_driver_writes_the_files_of_the_per_class_driver(se3, models, tmp_path):
    """get_results_ycb_objects on a tree where sequence 0048 shows a second class: byte-identical files to two get_results_ycb runs"""
    import shutil
    tree = YF.make_tree(str(tmp_path / "ycbv"))
    c1, c2 = YF.CLASS_ID, YF.CLASS_ID + 1
    src = os.path.join(tree, "data_organized", "0048", "pose_gt", str(c1))
    dst = os.path.join(tree, "data_organized", "0048", "pose_gt", str(c2))
    shutil.copytree(src, dst)
    for f in sorted(os.listdir(dst)):                         # the second object sits 2 cm to the side and 3 cm further away
        P = np.loadtxt(os.path.join(dst, f))
        P[:3, 3] += (0.02, -0.01, 0.03)
        np.savetxt(os.path.join(dst, f), P)
    t1 = make_tracker(se3, models, "30deg", "sphere", width=YF_WIDTH)
    t2 = make_tracker(se3, models, "5deg", "ellipsoid", width=YF_WIDTH)
    d = {c: str(tmp_path / ("multi%d" % c)) for c in (c1, c2)}
    done = se3.sequence.get_results_ycb_objects({c1: t1, c2: t2}, tree, d)
    e1, e2 = str(tmp_path / "one1"), str(tmp_path / "one2")
    assert done[c1] == se3.sequence.get_results_ycb(t1, tree, c1, e1)
    assert done[c2] == se3.sequence.get_results_ycb(t2, tree, c2, e2) == {48: 9}
    for c, e in ((c1, e1), (c2, e2)):
        for sdir in sorted(os.listdir(e)):
            names = sorted(os.listdir(os.path.join(e, sdir)))
            assert names == sorted(os.listdir(os.path.join(d[c], sdir)))
            for f in names:
                with open(os.path.join(e, sdir, f), "rb") as a, open(os.path.join(d[c], sdir, f), "rb") as b:
                    assert a.read() == b.read(), (c, sdir, f)

