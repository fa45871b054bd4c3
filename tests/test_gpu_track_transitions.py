"""GPU: the one-call tracking entry points across changes on ONE live Tracker / context.

Every other test of se3tn_on_track / _live / _batch / _objects / _objects_live runs on a Tracker made for it: one frame size, one mesh,
one route, one batch size.  What the context grows on demand and never shrinks (the fill_depth scratch addressed with the call's pixel
count, the z-buffers, the frame route's sub-image buffers addressed with the call's n x maxpx, the pinned / device staging two entry
points size with two formulas, the per-mesh batch buffers, the multi-object raster scratch the fit stage shares, the graph cache whose
key holds a pointer a frame-size change re-allocates) and what Tracker builds at its first call (_one_call_state, _batch_state,
_fit_imgs) is read as OLD state only by a call that follows a larger, a smaller or a different one.  Each SEQUENCE here is a fixed,
named list of such calls on one live Tracker created for the smallest camera.  Per step:
  * BIT identity with a twin: a Tracker created for this step's camera on a context and mesh handles of its own, put directly into
    this step's renderer, switches and fit tolerance, which runs this one call and is closed -- pose, trans, rot, bbox, image A of every
    pair, the filled depth frame, the fit records, estimate renders and last_fit_ratio, and which keys last_prediction holds;
  * on the window route the float oracle as well (O.on_track on the twin's image A, test_gpu_routes' bounds per route class; on live
    steps the depth it sees is fill_depth of the raw frame on a fresh context, which the fill tests hold to the depth oracle);
  * wherever the window meets the frame, image A covers more than 500 pixels.
frame_sizes, live_and_plain and switches run again on a Tracker(use_graphs=True): every call three times (eager, capture, replay).
test_sequences_cover_the_transitions (no GPU) asserts from the sequence data what the steps grow, under-use and follow."""
import ctypes as C
import hashlib
import time

import numpy as np
import pytest
import torch

from oracle import fixtures as Fx
from oracle import se3_oracle as O
from test_gpu_routes import CLASS_TOL, DEG, POSE_TOL, TILE_AUTO, _cfg_op, _eng_op, expected, tol_class

SIZES = dict(a=(120, 160), b=(97, 131), c=(240, 320), d=(480, 640))      # b: odd sizes (strides and 64-byte roundings differ)
WIDTH = 150.0
MAX_SAMPLES = 8
MESH_VF = dict(M1=(162, 320), M2=(642, 1280), M3=(42, 80), TEX=(162, 320))
MESH_SUBDIV = dict(M1=2, M2=3, M3=1)
# translations (metres) by where the crop window lies; the cameras are one camera scaled, so a pose lies alike at every size
POSE_T = dict(inside=(0.02, -0.01, 0.8), cross=((-0.2, -0.17, 0.75), (0.2, 0.14, 0.7)), miss=(0.6, 0.5, 0.9),
              far=(0.01, 0.0, 1.6), near=(0.0, 0.0, 0.4))      # far / near: a 25- / 100-pixel rectangle of the 160-column frame
KINDS = ("inside", "cross", "miss")
WORST = {}        # class -> worst |d logit| against the oracle over all steps run (printed by the last test)
TIMES = {}        # case id -> seconds


def cam(H, W):
    K = Fx.K_YCB.copy()
    K[0] *= W / 640
    K[1] *= H / 480
    return K


def info(size):
    H, W = SIZES[size]
    K = cam(H, W)
    return dict(Fx.DATASET_INFO, object_width=WIDTH,
                camera=dict(height=H, width=W, focalX=K[0, 0], focalY=K[1, 1], centerX=K[0, 2], centerY=K[1, 2]))


# ---- the sequences -----------------------------------------------------------------------------------------------------------------
def step(call, size, n=1, mesh="M1", fit=0, ops=(), kinds=None, **kw):
    """call: on_track | live | batch | objects | objects_live.  kinds: where the window of each pair lies (default: the three kinds in
    rotation with the step index and the pair).  ops: switch calls made before the step (test_gpu_routes' notation); fit: the fit
    tolerance in force (0 = off).  kw: depth_filled / extrapolate / blur (live), objs (objects: indices into the three trackers)."""
    return dict(call=call, size=size, n=n, mesh=mesh, fit=fit, ops=list(ops), kinds=kinds, **kw)


def seq(name, steps, graph=False, rot=0):
    out = []
    for k, st in enumerate(steps):
        st = dict(st, k=k)
        if st["kinds"] is None:
            st["kinds"] = [KINDS[(k + i + rot) % 3] for i in range(st["n"])]
        assert len(st["kinds"]) == st["n"]
        out.append(st)
    return dict(name=name, steps=out, graph=graph)


def W_(min_batch, tile):
    return ("wino", min_batch, tile)


def _switch_steps():
    """every switch followed by on_track, on_track_batch(3) and on_track_batch(7); a step undoes the one before it where the two would
    hide each other (Winograd from one pair leaves the small-kernels switch nothing to decide)"""
    configs = [([], 0),
               ([W_(1, 2)], 0),
               ([W_(1, 4)], 30),                                   # one pair: the fused heads' tail, which takes no completion word
               ([W_(6, TILE_AUTO), ("small", 0)], 30),
               ([("small", 1), ("keep", 1)], 30),
               ([("keep", 0), ("f16", 1)], 0),                     # (se3tn_on_track_objects refuses on this context: _objects_refusal)
               ([("f16", 0)], 0),                                  # ... and runs again here
               ([("trunk", 1, 0)], 30),
               ([("trunk", 8, 55), ("norm", 0.03, 0.3)], 30),
               ([("norm", 0.03, 5 * DEG)], 30)]                    # back to the defaults
    out = []
    for ops, fit in configs:
        out += [step("on_track", "a", fit=fit, ops=ops), step("batch", "a", 3, fit=fit), step("batch", "a", 7, fit=fit)]
    return out


_T = "TEX"
SEQUENCES = [
    seq("frame_sizes", [step("on_track", s) for s in "adbcda"], graph=True),
    seq("live_and_plain", [step("live", "a"), step("on_track", "d"), step("live", "d"), step("live", "b", depth_filled=True),
                           step("on_track", "b"), step("live", "c", extrapolate=True, blur="gaussian"), step("on_track", "a")],
        graph=True, rot=1),
    seq("batch_sizes", [step("batch", "a", 2), step("batch", "c", 7), step("batch", "d", 1), step("batch", "d", 8), step("batch", "b", 3),
                        step("on_track", "d"), step("batch", "a", 5)], rot=2),
    seq("meshes", [step("on_track", "a", mesh="M1"), step("batch", "a", 4, mesh="M2"), step("batch", "a", 6, mesh="M1", fit=30),
                   step("on_track", "a", mesh="M3", fit=30), step("batch", "a", 8, mesh="M3", fit=30),
                   step("batch", "a", 3, mesh="M2", fit=30), step("on_track", "a", mesh="M1", fit=30),   # (the fit stage: larger after smaller, and back)
                   step("batch", "a", 2, mesh="M2")]),
    seq("objects", [step("objects", "a", 1, objs=[2]), step("objects", "c", 2, objs=[0, 1]),
                    step("objects_live", "a", 4, objs=[1, 1, 0, 2]), step("objects", "a", 2, objs=[2, 2], fit=30),
                    step("objects", "a", 1, objs=[1], fit=30)]),
    seq("frame_route", [step("on_track", "a", mesh=_T, kinds=["far"]), step("on_track", "a", mesh=_T, kinds=["near"]),
                        step("on_track", "a", mesh=_T, kinds=["miss"]), step("on_track", "c", mesh=_T, kinds=["near"]),
                        step("batch", "c", 3, mesh=_T, kinds=["far"] * 3), step("batch", "c", 2, mesh=_T, kinds=["near", "cross"]),
                        step("batch", "a", 5, mesh=_T, kinds=["far", "near", "miss", "cross", "inside"]),
                        step("batch", "a", 3, mesh=_T, kinds=["miss"] * 3), step("batch", "c", 1, mesh=_T, kinds=["near"]),
                        step("on_track", "c", mesh="M1", kinds=["inside"]),      # a window-route renderer on the same Tracker ...
                        step("on_track", "c", mesh=_T, kinds=["near"]),          # ... and the full-frame one back
                        step("on_track", "a", mesh="M1", kinds=["cross"])]),
    seq("switches", _switch_steps(), graph=True)]
RUNS = [(s, g) for s in SEQUENCES for g in ((False, True) if s["graph"] else (False,))]


def _cfg0():
    """the switches of a context just created (include/se3tracknet.h's defaults), in test_gpu_routes' record"""
    return dict(wmin=6, tile=TILE_AUTO, tmin=8, tfill=55, small=True, keep=False, f16=False, tn=0.03, rn=5 * DEG, fuse=True, tail_parts=True,
                ovr=[0, 0])


def _pose_of(st, i):
    kind = st["kinds"][i]
    t = POSE_T[kind]
    if kind == "cross":
        t = t[(st["k"] + i) % 2]
    return Fx.pose(300 + 8 * st["k"] + i, t)


def _is_live(st):
    return st["call"] in ("live", "objects_live")


def _walk(s):
    """the sequence from its data alone: per step the sizes of what the context keeps between calls, and for each whether this call is
    the first to use it, exceeds every earlier use or stays under one (per component)"""
    import se3tracknet_amd as se3
    seen, out, cfg = {}, [], _cfg0()
    for st in s["steps"]:
        H, W_px = SIZES[st["size"]]
        dims = {"frame px": (H * W_px,)}
        if _is_live(st):
            dims["live frame px"] = (H * W_px,)
        if st["call"] in ("batch", "objects", "objects_live"):
            dims["n"] = (st["n"],)
        if st["call"].startswith("objects"):
            vf = [MESH_VF["M%d" % (o + 1)] for o in st["objs"]]
            dims["object list"] = (st["n"], max(v for v, _ in vf), max(f for _, f in vf))
        elif st["fit"]:
            dims["mesh"] = MESH_VF[st["mesh"]]          # (the fit stage renders into the raster scratch every entry point shares)
        if st["mesh"] == _T:
            rects = [se3.frame_rect(_pose_of(st, i), cam(H, W_px), WIDTH, H, W_px) for i in range(st["n"])]
            dims["frame route n x maxpx"] = (st["n"] * max([(r[2] - r[0]) * (r[3] - r[1]) if r else 0 for r in rects]),)
        pos = {}
        for d, v in dims.items():
            if d not in seen:
                pos[d] = {"first"}
            else:
                pos[d] = ({"growth"} if any(x > m for x, m in zip(v, seen[d]["max"])) else set()) | \
                         ({"shrink"} if seen[d]["grown"] and any(x < m for x, m in zip(v, seen[d]["max"])) else set())
            e = seen.setdefault(d, dict(max=v, grown=False))
            e["grown"] = e["grown"] or "growth" in pos[d]
            e["max"] = tuple(max(x, m) for x, m in zip(v, e["max"]))
        for op in st["ops"]:
            _cfg_op(cfg, op)
        out.append(dict(st=st, dims=dims, pos=pos, cfg=dict(cfg)))
    return out


ENTRY = dict(on_track="on_track", live="on_track_live", batch="on_track_batch", objects="on_track_objects", objects_live="on_track_objects_live")


def test_sequences_cover_the_transitions():
    """(no GPU) what the fixed sequences reach, from their data: the condition that keeps an edit from hollowing them out"""
    walks = {s["name"]: _walk(s) for s in SEQUENCES}
    for m, sub in MESH_SUBDIV.items():
        ico = Fx.icosphere(sub)
        assert (len(ico["vertices"]), len(ico["faces"])) == MESH_VF[m]
    tex = Fx.textured_sphere()
    assert (len(tex["vertices"]), len(tex["faces"])) == MESH_VF[_T]
    # every kept size is exceeded after its first use and under-used after a growth
    for d in ("frame px", "live frame px", "n", "mesh", "object list", "frame route n x maxpx"):
        got = set().union(*[w["pos"].get(d, set()) for v in walks.values() for w in v])
        assert got >= {"first", "growth", "shrink"}, (d, got)
    # ... and every entry point makes a call of each kind
    for call, name in ENTRY.items():
        got = set().union(*[p for v in walks.values() for w in v if w["st"]["call"] == call for p in w["pos"].values()])
        assert got >= {"first", "growth", "shrink"}, (name, got)
    # the live Tracker is created for camera a, the smallest: every other size grows something
    assert all(v[0]["st"]["size"] == "a" for v in walks.values())
    assert SIZES["b"][0] * SIZES["b"][1] < SIZES["a"][0] * SIZES["a"][1] < SIZES["c"][0] * SIZES["c"][1] < SIZES["d"][0] * SIZES["d"][1]
    # at every frame size the three kinds of window, and they lie where they are said to
    import se3tracknet_amd as se3
    kinds = {}
    for v in walks.values():
        for w in v:
            st = w["st"]
            H, W_px = SIZES[st["size"]]
            for i, kind in enumerate(st["kinds"]):
                l, t, r, b = se3.crop_window(se3.compute_bbox(_pose_of(st, i), cam(H, W_px), WIDTH))
                where = "miss" if (r <= 0 or b <= 0 or l >= W_px or t >= H) else "cross" if (l < 0 or t < 0 or r > W_px or b > H) else "inside"
                assert where == {"far": "inside", "near": "inside"}.get(kind, kind), (st, i, where)
                kinds.setdefault(st["size"], set()).add(where)
    assert all(kinds[s] == set(KINDS) for s in SIZES), kinds
    # frame_sizes is a, d, b, c, d, a; the two formulas of the staging size alternate in live_and_plain
    assert [w["st"]["size"] for w in walks["frame_sizes"]] == list("adbcda")
    lp = [(w["st"]["call"], w["st"]["size"]) for w in walks["live_and_plain"]]
    assert lp == [("live", "a"), ("on_track", "d"), ("live", "d"), ("live", "b"), ("on_track", "b"), ("live", "c"), ("on_track", "a")]
    # batch sizes on both sides of the Winograd threshold of the default switches
    bs = [(w["st"]["n"], expected(w["cfg"], w["st"]["n"])[0]["h2.2"]) for w in walks["batch_sizes"] if w["st"]["call"] == "batch"]
    assert bs == [(2, "small"), (7, "F4 block"), (1, "small"), (8, "F4 block"), (3, "small"), (5, "small")], bs
    # the fit stage meets a larger mesh after a smaller one and the reverse
    fm = [MESH_VF[w["st"]["mesh"]][0] for w in walks["meshes"] if w["st"]["fit"]]
    assert any(a < b for a, b in zip(fm, fm[1:])) and any(a > b for a, b in zip(fm, fm[1:])), fm
    ms = [MESH_VF[w["st"]["mesh"]][0] for w in walks["meshes"]]
    assert any(a < b for a, b in zip(ms, ms[1:])) and any(a > b for a, b in zip(ms, ms[1:]))
    # the frame route: small and large rectangles, a miss, all missing; and the renderer kind swapped both ways on the live Tracker
    fr = walks["frame_route"]
    px = [w["dims"].get("frame route n x maxpx", (None,))[0] for w in fr]
    assert 0 in px and any(w["st"]["call"] == "batch" and w["st"]["kinds"] == ["miss"] * 3 for w in fr)
    routes = [w["st"]["mesh"] == _T for w in fr]
    assert (True, False) in set(zip(routes, routes[1:])) and (False, True) in set(zip(routes, routes[1:]))
    # every switch is followed by a one-pair and a multi-pair call before the next one; the fused tail at one pair is among the routes
    sw = walks["switches"]
    idx = [i for i, w in enumerate(sw) if w["st"]["ops"]] + [len(sw)]
    assert len(idx) == 10
    for a, b in zip(idx, idx[1:]):
        ns = [w["st"]["n"] for w in sw[a:b]]
        assert 1 in ns and any(n > 1 for n in ns), (a, ns)
    ops = {op[:2] if op[0] != "norm" else op for w in sw for op in w["st"]["ops"]}
    assert ops >= {("wino", 1), ("small", 0), ("keep", 1), ("f16", 1), ("f16", 0), ("trunk", 1), ("norm", 0.03, 0.3)}, ops
    assert {w["st"]["ops"][0] for w in sw if w["st"]["ops"]} >= {W_(1, 2), W_(1, 4)}
    tails = {expected(w["cfg"], 1)[0]["tail"] for w in sw if w["st"]["n"] == 1}
    assert tails == {"parts", "tail", "fused"}, tails
    assert sw[-1]["cfg"] == _cfg0()
    assert [w["st"]["fit"] for w in sw if w["st"]["n"] == 1] == [0, 0, 30, 30, 30, 0, 0, 30, 30, 30]
    assert {(a, b) for a, b in zip([w["st"]["fit"] for w in sw], [w["st"]["fit"] for w in sw[1:]])} >= {(0, 30), (30, 0)}


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


_CACHE = dict(sd={}, mesh={}, frame={}, raw={}, filled={}, twin={}, oracle={})


def _sd(seed):
    if seed not in _CACHE["sd"]:
        _CACHE["sd"][seed] = O.make_state_dict(seed, head_gain=0.01)
    return _CACHE["sd"][seed]


def _mesh(name):
    if name not in _CACHE["mesh"]:
        if name == _T:
            m = Fx.textured_sphere()
            _CACHE["mesh"][name] = dict(vertices=m["vertices"], faces=m["faces"], colors=m["colors"], uv=m["uv"], texture=m["texture"], kd=m["kd"])
        else:
            _CACHE["mesh"][name] = Fx.icosphere(MESH_SUBDIV[name])
    return _CACHE["mesh"][name]


def _frame(seed, size):
    key = (seed, size)
    if key not in _CACHE["frame"]:
        if len(_CACHE["frame"]) > 40:
            _CACHE["frame"].clear()
        _CACHE["frame"][key] = Fx.synthetic_frame(seed, *SIZES[size])
    return _CACHE["frame"][key]


def _raw(seed, size):
    key = (seed, size)
    if key not in _CACHE["raw"]:
        _CACHE["raw"][key] = Fx.depth_frame_with_holes(seed, *SIZES[size])
    return _CACHE["raw"][key]


def _fill_opts(st):
    return (2.0, bool(st.get("extrapolate", False)), st.get("blur", "bilateral"))


def _filled(se3, seed, size, opts):
    """engine.fill_depth of the whole raw frame on a context that does nothing else"""
    key = (seed, size, opts)
    if key not in _CACHE["filled"]:
        eng = se3.Engine(0, 1)
        try:
            _CACHE["filled"][key] = eng.fill_depth(_raw(seed, size), *opts)
        finally:
            eng.close()
    return _CACHE["filled"][key]


def _inputs(st):
    """poses and frames of a step: other frames and rotations at every step, so that nothing left by the call before passes for this one"""
    n, k = st["n"], st["k"]
    one_frame = st["call"].startswith("objects")
    seeds = [1000 + 16 * k + (0 if one_frame else i) for i in range(n)]
    frames = [_frame(s, st["size"]) for s in seeds]
    return dict(poses=[_pose_of(st, i) for i in range(n)], rgb=[f[0] for f in frames], seeds=seeds,
                depth=[_raw(s, st["size"]) if _is_live(st) else f[1] for s, f in zip(seeds, frames)])


def _new_tracker(se3, size, sd_seed=0, use_graphs=False):
    mean, std = Fx.mean_std(sd_seed)
    return se3.Tracker(info(size), mean, std, {"state_dict": _sd(sd_seed)}, max_samples=MAX_SAMPLES, use_graphs=use_graphs)


def _new_renderer(se3, eng, mesh, size):
    if mesh == _T:
        return se3.HipRenderer(eng, _mesh(mesh), mode="pyrender", frame_size=SIZES[size])
    return se3.HipRenderer(eng, _mesh(mesh))


def _close(trk):
    r, trk.renderer = trk.renderer, None
    if r is not None:
        r.__del__()              # the mesh handle goes before its context
    trk.engine.close()


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _record(trk, out, n, filled):
    """everything a call leaves behind that a caller can read"""
    torch.cuda.synchronize()
    lp = trk.last_prediction
    if "rgbA" not in lp:
        rgbA, depthA = trk.renderer.rgb[None], trk.renderer.depth[None]
    elif torch.is_tensor(lp["rgbA"]):
        rgbA, depthA = lp["rgbA"][None], lp["depthA"][None]
    else:
        rgbA, depthA = torch.stack(list(lp["rgbA"])), torch.stack(list(lp["depthA"]))
    rec = dict(pose=np.array(out, np.float64).reshape(n, 4, 4), trans=np.array(lp["trans"], np.float32).reshape(n, 3),
               rot=np.array(lp["rot"], np.float32).reshape(n, 3), bbox=np.array(lp["bbox"], np.int32).reshape(n, 4, 2),
               rgbA=rgbA.cpu().numpy(), depthA=depthA.cpu().numpy().view(np.uint16), keys=sorted(lp.keys()),
               logits=trk.engine.logits(n).cpu().numpy())
    assert rec["rgbA"].shape == (n, 176, 176, 3) and rec["depthA"].shape == (n, 176, 176)
    if filled is not None:
        rec["filled"] = filled.cpu().numpy().view(np.uint16)
    if "fit" in lp:
        rec.update(fit=np.frombuffer(np.ascontiguousarray(lp["fit"]).tobytes(), np.uint8), pred_rgb=lp["pred_rgb"][:n].cpu().numpy(),
                   pred_depth=lp["pred_depth"][:n].cpu().numpy().view(np.uint16), fit_ratio=np.atleast_1d(np.asarray(trk.last_fit_ratio, np.float64)),
                   model_px=np.asarray(lp["fit"]["model_px"]).copy())
        assert len(lp["fit"]) == n and rec["fit_ratio"].shape == (n,)
    else:
        assert trk.last_fit_ratio is None
    return rec


def _call(trk, st, inp):
    n, filled = st["n"], None
    if st["call"] == "on_track":
        out = trk.on_track(inp["poses"][0], inp["rgb"][0], inp["depth"][0])
    elif st["call"] == "live":
        if st.get("depth_filled"):
            filled = torch.zeros(SIZES[st["size"]], dtype=torch.int16, device="cuda")
        max_depth, extrapolate, blur = _fill_opts(st)
        out = trk.on_track_live(inp["poses"][0], inp["rgb"][0], inp["depth"][0], bgr=False, max_depth=max_depth, extrapolate=extrapolate,
                                blur_type=blur, depth_filled=filled)
    else:
        out = trk.on_track_batch(inp["poses"], inp["rgb"], inp["depth"])
    return _record(trk, out, n, filled)


def _assert_same(got, want, what):
    assert got["keys"] == want["keys"], "%s: last_prediction holds %s, on the twin %s" % (what, got["keys"], want["keys"])
    assert set(got) == set(want), "%s: the call left %s, on the twin %s" % (what, sorted(got), sorted(want))
    for k in want:
        if k == "keys" or _bytes_equal(got[k], want[k]):
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape:
            raise AssertionError("%s: %s has shape %s, on the twin %s" % (what, k, a.shape, b.shape))
        bad = (a != b).reshape(a.shape[0], -1).sum(1).tolist() if a.ndim > 1 else int((a != b).sum())
        raise AssertionError("%s: %s differs from the twin's bit for bit; differing elements per pair %s, max |d| %.3e" % (
            what, k, bad, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())))


def _cfg_ops(cfg):
    return [("trunk", cfg["tmin"], cfg["tfill"]), ("small", cfg["small"]), ("keep", cfg["keep"]), ("norm", cfg["tn"], cfg["rn"]),
            W_(cfg["wmin"], cfg["tile"])] + ([("f16", 1)] if cfg["f16"] else [])


def _twin(se3, st, cfg):
    """the step on a Tracker of its own: created for this camera, this renderer on mesh handles of its own, the switches and the fit
    tolerance applied directly, this one call, closed.  Cached per step (the graph rerun of a sequence asks for the same steps)."""
    key = repr((st["call"], st["size"], st["n"], st["mesh"], st["fit"], st["kinds"], st["k"], _fill_opts(st), st.get("depth_filled"),
                sorted((k, v) for k, v in cfg.items() if k != "ovr")))
    if key not in _CACHE["twin"]:
        trk = _new_tracker(se3, st["size"])
        try:
            trk.renderer = _new_renderer(se3, trk.engine, st["mesh"], st["size"])
            if cfg != _cfg0():
                for op in _cfg_ops(cfg):
                    _eng_op(se3, trk.engine, op)
            if st["fit"]:
                trk.fit_check = st["fit"]
            _CACHE["twin"][key] = _call(trk, st, _inputs(st))
        finally:
            _close(trk)
    return _CACHE["twin"][key]


def _oracle(sd_seed, P, rgb, depth, rgbA, depthA, K, tn, rn):
    key = (sd_seed, P.tobytes(), K.tobytes(), tn, rn, hashlib.sha1(rgb.tobytes() + depth.tobytes() + rgbA.tobytes() + depthA.tobytes()).hexdigest())
    if key not in _CACHE["oracle"]:
        mean, std = Fx.mean_std(sd_seed)
        _CACHE["oracle"][key] = O.on_track(_sd(sd_seed), P, rgb, depth, rgbA, depthA, K, WIDTH, mean, std, tn, rn)
    return _CACHE["oracle"][key]


def _anchor(se3, st, inp, got, want, cfg, what, sd_seeds=None, n_route=None):
    """window-route steps: O.on_track on the twin's own image A; test_gpu_routes' bounds, nothing new"""
    n = st["n"]
    r, _ = expected(cfg, n_route or n)
    cls = tol_class(cfg, r)
    K = cam(*SIZES[st["size"]])
    for i in range(n):
        depth = _filled(se3, inp["seeds"][i], st["size"], _fill_opts(st)) if _is_live(st) else inp["depth"][i]
        pose, o = _oracle(sd_seeds[i] if sd_seeds else 0, inp["poses"][i], inp["rgb"][i], depth, want["rgbA"][i], want["depthA"][i], K, cfg["tn"], cfg["rn"])
        e_lg = float(np.abs(got["logits"][i].astype(np.float64) - np.concatenate([o["trans_logit"], o["rot_logit"]])).max())
        WORST[cls] = max(WORST.get(cls, 0.0), e_lg)
        e = max(float(np.abs(got["trans"][i] - o["trans"]).max()), float(np.abs(got["rot"][i] - o["rot"]).max()))
        assert e <= CLASS_TOL[cls], "%s pair %d: max |d (trans, rot)| vs the oracle %.3e > %.0e (%s); |d logit| %.3e" % (what, i, e, CLASS_TOL[cls], cls, e_lg)
        d = float(np.abs(got["pose"][i] - pose).max())
        assert d <= POSE_TOL, "%s pair %d: |d pose| vs the oracle %.3e" % (what, i, d)
        assert np.array_equal(got["bbox"][i], o["bbox"]), "%s pair %d: bbox" % (what, i)


def _covered(st, got, what):
    for i, kind in enumerate(st["kinds"]):
        px = int((got["depthA"][i] != 0).sum())
        if kind != "miss":
            assert px > 500, "%s pair %d (%s window): image A covers %d pixels" % (what, i, kind, px)
        elif st["mesh"] == _T:      # the full-frame route renders what the frame shows: nothing
            assert px == 0, "%s pair %d: a window that misses the frame shows %d pixels" % (what, i, px)


class _Live:
    """the one Tracker of a sequence (created for camera a), its renderers (mesh handles on ITS context), the record of its switches and
    the trail of steps taken"""
    def __init__(self, se3, graph):
        self.se3, self.graph = se3, graph
        self.trk = _new_tracker(se3, "a", use_graphs=graph)
        self.renderers, self.cfg, self.trail = {}, _cfg0(), []

    def close(self):
        for r in self.renderers.values():
            r.__del__()
        self.trk.renderer = None
        self.trk.engine.close()

    def step(self, st):
        se3, trk = self.se3, self.trk
        self.trail.append("%2d  %-8s %s (%d x %d) n=%d mesh %s fit %d  %s%s" % (
            st["k"], st["call"], st["size"], *SIZES[st["size"]], st["n"], st["mesh"], st["fit"], ",".join(st["kinds"]),
            "".join("  %s%s" % (op[0], tuple(op[1:])) for op in st["ops"])))
        for op in st["ops"]:
            _eng_op(se3, trk.engine, op)
            _cfg_op(self.cfg, op)
        trk.K = cam(*SIZES[st["size"]])
        rkey = (st["mesh"], st["size"] if st["mesh"] == _T else None)
        if rkey not in self.renderers:
            self.renderers[rkey] = _new_renderer(se3, trk.engine, st["mesh"], st["size"])
        trk.renderer = self.renderers[rkey]
        if (trk.fit_check or 0) != st["fit"]:
            trk.fit_check = st["fit"] or None
        inp = _inputs(st)
        want = _twin(se3, st, self.cfg)
        what = "%s %s n=%d" % (st["call"], st["size"], st["n"])
        for it in (("call 1 (eager)", "call 2 (capture)", "call 3 (replay)") if self.graph else ("",)):
            got = _call(trk, st, inp)
            _assert_same(got, want, (what + ", graphs on, " + it) if it else what)
        _covered(st, got, what)
        if st["mesh"] != _T:
            _anchor(se3, st, inp, got, want, self.cfg, what)
        if "filled" in got:
            assert np.array_equal(got["filled"], _filled(se3, inp["seeds"][0], st["size"], _fill_opts(st))), what + ": the filled frame is not engine.fill_depth's"
        if st["fit"]:
            assert all(m > 0 for m, kind in zip(got["model_px"], st["kinds"]) if kind == "inside"), (what, got["model_px"])
        if self.cfg["f16"]:
            assert not trk.engine.overflow(), what + ": the overflow flag is set"
            if st["call"] == "on_track":
                self.objects_refusal(st, inp, refuse=True)
        elif st["ops"] == [("f16", 0)]:
            self.objects_refusal(st, inp, refuse=False, want=got)

    def objects_refusal(self, st, inp, refuse, want=None):
        """se3tn_on_track_objects with this Tracker's context as the executing one: refused under f16x3 before anything is launched
        (SE3TN_E_STATE), and the bits of on_track again once float32 is back"""
        trk, L = self.trk, self.se3._lib
        objs = (L.Object * 1)(L.Object(trk.engine._h.value, trk.renderer._m.value, float(trk.object_width)))
        res = _objects_call(trk.engine, objs, 1, inp, st, None)
        if refuse:
            with pytest.raises(L.Se3tnError, match=r"rc=-2.*ctx is in SE3TN_PREC_F16X3"):
                res()
        else:
            got = res()
            for k in ("pose", "trans", "rot", "bbox", "rgbA", "depthA"):
                assert _bytes_equal(got[k], want[k]), "se3tn_on_track_objects after f16x3 was switched off: " + k


def _objects_call(eng, objs, n, inp, st, fit_imgs):
    """se3tn_on_track_objects / _objects_live on the executing Engine `eng`, called as MultiTracker._on_track calls it"""
    import se3tracknet_amd as se3
    L, _stream_ptr = se3._lib, se3.engine._stream_ptr
    H, W_px = SIZES[st["size"]]
    K = np.ascontiguousarray(cam(H, W_px))
    poses = np.ascontiguousarray(np.stack(inp["poses"]).reshape(n, 16))
    rgb, dep = np.ascontiguousarray(inp["rgb"][0]), np.ascontiguousarray(inp["depth"][0], dtype=np.uint16)
    rA = torch.zeros((n, 176, 176, 3), dtype=torch.uint8, device="cuda")
    dA = torch.zeros((n, 176, 176), dtype=torch.int16, device="cuda")
    out, tr, ro, bb = np.empty((n, 16)), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty((n, 4, 2), np.int32)
    outs = (C.c_void_p(rA.data_ptr()), C.c_void_p(dA.data_ptr()), C.c_void_p(out.ctypes.data), C.c_void_p(tr.ctypes.data),
            C.c_void_p(ro.ctypes.data), C.c_void_p(bb.ctypes.data))

    def run():
        if _is_live(st):
            max_depth, extrapolate, blur = _fill_opts(st)
            L.check(eng.lib.se3tn_on_track_objects_live(
                eng._h, n, objs, C.c_void_p(poses.ctypes.data), K.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(rgb.ctypes.data),
                L.COLOR_RGB, C.c_void_p(dep.ctypes.data), H, W_px, C.c_double(max_depth), int(extrapolate), L.BLUR_BILATERAL, None, *outs,
                _stream_ptr()), "se3tn_on_track_objects_live")
        else:
            L.check(eng.lib.se3tn_on_track_objects(
                eng._h, n, objs, C.c_void_p(poses.ctypes.data), K.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(rgb.ctypes.data),
                C.c_void_p(dep.ctypes.data), H, W_px, *outs, _stream_ptr()), "se3tn_on_track_objects")
        torch.cuda.synchronize()
        rec = dict(pose=out.reshape(n, 4, 4), trans=tr, rot=ro, bbox=bb, rgbA=rA.cpu().numpy(), depthA=dA.cpu().numpy().view(np.uint16))
        if eng.get_fit_check():
            fit = eng.last_fit(n)
            eng.last_fit_images(n, fit_imgs[0], fit_imgs[1])
            rec.update(fit=np.frombuffer(np.ascontiguousarray(fit).tobytes(), np.uint8), pred_rgb=fit_imgs[0][:n].cpu().numpy(),
                       pred_depth=fit_imgs[1][:n].cpu().numpy().view(np.uint16))
        return rec
    return run


def _run_objects(se3, s):
    """one executing Engine(0, 4); three Trackers (M1 / M2 / M3, weights of seeds 0 / 1 / 2) created for camera a.  Object i of a call
    must have exactly the bits trackers[i].on_track / on_track_live gives it (include/se3tracknet.h)"""
    L = se3._lib
    trks = [_new_tracker(se3, "a", sd_seed=i) for i in range(3)]
    for i, t in enumerate(trks):
        t.renderer = _new_renderer(se3, t.engine, "M%d" % (i + 1), "a")
    eng = se3.Engine(0, 4)
    fit_imgs = (torch.empty((4, 176, 176, 3), dtype=torch.uint8, device="cuda"), torch.empty((4, 176, 176), dtype=torch.int16, device="cuda"))
    trail = []
    try:
        for st in s["steps"]:
            trail.append("%2d  %-12s %s objects %s fit %d  %s" % (st["k"], st["call"], st["size"], [o + 1 for o in st["objs"]], st["fit"], ",".join(st["kinds"])))
            try:
                n, inp = st["n"], _inputs(st)
                what = "%s %s %s" % (st["call"], st["size"], [o + 1 for o in st["objs"]])
                eng.set_fit_check(st["fit"] or None)
                objs = (L.Object * n)(*[L.Object(trks[o].engine._h.value, trks[o].renderer._m.value, float(trks[o].object_width)) for o in st["objs"]])
                got = _objects_call(eng, objs, n, inp, st, fit_imgs)()
                _covered(st, got, what)
                one = dict(st, call="live" if _is_live(st) else "on_track", n=1)
                for i, o in enumerate(st["objs"]):
                    t = trks[o]
                    t.K = cam(*SIZES[st["size"]])
                    t.fit_check = st["fit"] or None
                    sub = dict(one, kinds=[st["kinds"][i]])
                    inp_i = dict(poses=[inp["poses"][i]], rgb=[inp["rgb"][0]], depth=[inp["depth"][0]], seeds=[inp["seeds"][0]])
                    want = _call(t, sub, inp_i)
                    for k in ("pose", "trans", "rot", "bbox", "rgbA", "depthA") + (("fit", "pred_rgb", "pred_depth") if st["fit"] else ()):
                        assert _bytes_equal(got[k][i:i + 1] if k != "fit" else got[k].reshape(n, -1)[i], want[k] if k != "fit" else want[k]), \
                            "%s: object %d (tracker %d): %s is not what the tracker's own %s gives" % (what, i, o + 1, k, ENTRY[sub["call"]])
                    _anchor(se3, sub, inp_i, want, want, _cfg0(), what + " object %d" % i, sd_seeds=[o])
            except AssertionError as e:
                raise AssertionError("objects, step %d: %s\nthe sequence up to here:\n%s" % (st["k"], e, "\n".join(trail))) from None
    finally:
        eng.close()
        for t in trks:
            _close(t)


def _run_sequence(se3, s, graph):
    live = _Live(se3, graph)
    try:
        for st in s["steps"]:
            try:
                live.step(st)
            except AssertionError as e:
                raise AssertionError("%s%s, step %d: %s\nthe sequence up to here (call, frame size, n, mesh, fit tolerance, windows, switch calls):\n%s" % (
                    s["name"], " (graphs)" if graph else "", st["k"], e, "\n".join(live.trail))) from None
        torch.cuda.synchronize()
    finally:
        live.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s,graph", RUNS, ids=[s["name"] + ("-graphs" if g else "") for s, g in RUNS])
def test_sequence_on_one_tracker(se3, s, graph):
    t0 = time.perf_counter()
    try:
        if s["name"] == "objects":
            _run_objects(se3, s)
        else:
            _run_sequence(se3, s, graph)
    finally:
        TIMES[s["name"] + ("-graphs" if graph else "")] = time.perf_counter() - t0


@pytest.mark.gpu
def test_zz_report_worst_logit_error_per_class_and_times():
    """(runs last) the worst |d logit| against the oracle per tolerance class over all steps, beside the bound; seconds per sequence"""
    for cls, bound in CLASS_TOL.items():
        print("track transitions: %-14s worst |d logit| vs the oracle %s (bound %.0e)" % (cls, "%.2e" % WORST[cls] if cls in WORST else "not run", bound))
        assert WORST.get(cls, 0.0) <= bound
    for name, t in TIMES.items():
        print("track transitions: %-24s %.2f s" % (name, t))
    print("track transitions: module %.2f s" % sum(TIMES.values()))
