"""Drop-in for the reference's ``predict.Tracker`` (predict.py:127-296): same constructor
arguments, ``on_track`` signature / return value and the attributes callers read (``K``,
``object_cloud``, ``object_width``, ``dataset`` with processData / processPredict, callable ``model``).  The arithmetic of on_track runs on the GPU
through the C ABI: se3tn_render (image A, predict.py:193-215) -> se3tn_preprocess -> se3tn_infer (network + pose update); only
compute_bbox is host float64 exactly as the reference.  Given a model file the constructor builds the HIP rasteriser itself
(``HipRenderer``: byte-identical to the reference's VispyRenderer on the GL implementation the goldens were rendered on); a
renderer object with the reference's protocol can be injected instead (``renderer.render(ob_in_cam, K, window) -> rgb u8,
depth u16`` or the full-frame ``render([ob_in_cam])`` of offscreen_renderer.Renderer)."""
import numpy as np
import torch

from . import utils as U
from .dataset import TrackDataset
from .engine import Engine, NHWC
from .se3_tracknet import Se3TrackNet


def _depth_u16(depth, rgb):
    """HxW depth in millimetres as the int16-viewed uint16 array the engine takes.  The reference casts with
    .astype(np.uint16) (predict.py:410-412 callers); a wider dtype must be CONVERTED, never byte-reinterpreted."""
    d = np.asarray(depth)
    if d.shape != np.asarray(rgb).shape[:2]:
        raise ValueError("depth %s does not match rgb %s" % (d.shape, np.asarray(rgb).shape))
    return np.ascontiguousarray(d, dtype=np.uint16).view(np.int16)


def _is_full_frame_renderer(renderer):
    """offscreen_renderer.Renderer protocol (predict.py:209-213): ``render([ob2cam]) -> (rgb HxWx3, depth HxW metres)``.
    Detected structurally -- the reference's class has no marker attribute: an explicit ``full_frame`` attribute wins,
    otherwise a ``render`` that takes exactly ONE positional argument (the pose list) is the full-frame protocol, one that
    takes (ob2cam, K, window) is the window protocol."""
    flag = getattr(renderer, "full_frame", None)
    if flag is not None:
        return bool(flag)
    import inspect
    try:
        params = [p for p in inspect.signature(renderer.render).parameters.values()
                  if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
    except (TypeError, ValueError):
        return False
    required = [p for p in params if p.default is p.empty]
    return len(required) == 1 and len(params) < 3


class Tracker:
    def __init__(self, dataset_info, images_mean, images_std, ckpt_dir, model_path=None,
                 trans_normalizer=0.03, rot_normalizer=5 * np.pi / 180, renderer=None, device=0,
                 max_samples=8, use_graphs=False):
        self.dataset_info = dataset_info
        self.image_size = (dataset_info['resolution'], dataset_info['resolution'])
        self.object_cloud = None
        self._normals = None         # object_normals: (model_path, vertices) until first read, then the array or None
        if model_path is not None:
            pts = U.load_model_points(model_path)
            self.object_cloud = U.PointCloud(U.voxel_down_sample(pts, 0.005))
            self._normals = (model_path, pts)
        if 'object_width' not in dataset_info:
            if self.object_cloud is None:
                raise ValueError("dataset_info has no 'object_width' and no model_path was given")
            object_max_width = U.compute_obj_max_width(self.object_cloud.points)
            self.object_width = object_max_width + dataset_info['boundingbox'] / 100 * object_max_width
        else:
            self.object_width = dataset_info['object_width']
        self.mean = np.asarray(images_mean, np.float64)
        self.std = np.asarray(images_std, np.float64)
        cam = dataset_info['camera']
        self.K = np.array([cam['focalX'], 0, cam['centerX'], 0, cam['focalY'], cam['centerY'], 0, 0, 1]).reshape(3, 3)

        # checkpoint surface: torch.load(path)['state_dict'] (predict.py:151-156) or a dict
        checkpoint = torch.load(ckpt_dir, map_location="cpu") if isinstance(ckpt_dir, str) else ckpt_dir
        sd = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint
        self.engine = Engine(device, max_samples)
        self.engine.load_state_dict(sd)
        self.engine.set_normalization(self.mean, self.std)
        # start-up reservation for this camera: full-frame z-buffer / fill_depth scratch, Winograd planes -- no stream-ordered
        # call allocates afterwards (se3tn_reserve)
        self.engine.reserve(int(cam['height']), int(cam['width']))
        self.trans_normalizer = float(trans_normalizer)
        self.rot_normalizer = float(rot_normalizer)
        self.engine.set_normalizers(self.trans_normalizer, self.rot_normalizer)
        # predict.py:270-271 `prediction = self.model(dataA, dataB)`: float32 CUDA [N,4,176,176] -> the reference's dict
        self.model = Se3TrackNet.from_engine(self.engine)
        # predict.py:189-191: the inner pre / post boundary (processData / processPredict)
        self.dataset = TrackDataset(self.engine, self.mean, self.std, dataset_info, self.trans_normalizer,
                                    self.rot_normalizer)
        self.renderer = renderer
        if renderer is None and model_path is not None and dataset_info.get('renderer') == 'pyrenderer':
            # predict.py:161-164: textured .obj through the pyrender-style full-frame renderer
            assert '.obj' in model_path
            from .renderer import HipRenderer
            self.renderer = HipRenderer(self.engine, model_path, mode="pyrender", frame_size=(cam['height'], cam['width']))
        elif renderer is None and model_path is not None and model_path.endswith(".ply"):
            # the reference builds a VispyRenderer from the .ply here (predict.py:180-182); ours is the
            # HIP rasteriser -- only if the file has faces (the repo's bunny fixture has none)
            from .renderer import HipRenderer
            mesh = U.load_ply_mesh(model_path)
            if len(mesh["faces"]) > 0:
                self.renderer = HipRenderer(self.engine, mesh)
        self.prev_rgb = None
        self.prev_depth = None
        self.frame_cnt = 0
        self._one_call_state = None
        self._batch_state = None
        self.one_call = True     # on_track through se3tn_on_track when the built-in rasteriser renders image A, window or full-frame
                                 # route (False: step by step)
        self.errs = []
        dev = "cuda:%d" % device
        self._dev = dev
        self._poseA = torch.empty((max_samples, 16), dtype=torch.float64, device=dev)
        # poseB | trans | rot live in ONE device buffer: what predict.py:275-276 reads back per frame is one D2H copy + one sync
        ms = int(max_samples)
        self._out = torch.zeros(ms * (128 + 12 + 12), dtype=torch.uint8, device=dev)
        self._poseB = self._out[:ms * 128].view(torch.float64).view(ms, 16)
        self._trans = self._out[ms * 128:ms * 140].view(torch.float32).view(ms, 3)
        self._rot = self._out[ms * 140:ms * 152].view(torch.float32).view(ms, 3)
        self._model_points = None    # pose_errors: object_cloud on the device, uploaded at first use
        self.last_prediction = None
        self.last_recover = None     # recover(): what the last search found (dict)
        self.last_acquire = None     # acquire(): every hypothesis of the last search and what became of it (dict)
        self._facing_points = None   # recover(facing=True) / acquire: object_cloud with object_normals on the device, at first use
        self.last_fit_ratio = None   # fit_check set: inlier_px / model_px of the last call (float; on_track_batch: [n] array)
        self._fit_imgs = None
        # optional hipGraph replay of the ~20 dependent launches of a frame on a dedicated stream (the
        # null stream cannot be captured).  Off by default: measured 0.213 ms/frame with vs 0.194 without
        # (profiles/EXPERIMENTS.md item 54: the kernels are 5-15 us each and the eager launches already run ahead of the device)
        self._stream = torch.cuda.Stream(device=dev) if use_graphs else None
        if use_graphs:
            self.engine.enable_graphs(True)

    def pose_errors(self, preds, gts):
        """ADD / ADD-S (metres) of n (pred, gt) pose pairs against ``object_cloud`` in one device call (Engine.pose_errors) ->
        (add[n], adds[n]).  The cloud is uploaded on the first call and kept."""
        if self.object_cloud is None:
            raise ValueError("pose_errors: this tracker has no object_cloud (no model_path was given)")
        if self._model_points is None:
            self._model_points = self.engine.model_points(self.object_cloud)
        return self.engine.pose_errors(self._model_points, preds, gts)

    def recover(self, prev_pose, rgb, depth, trans_radius=0.05, trans_step=0.01, rot_deg=(15.0,), tol_mm=10, top=None, refine=1,
                points=None, extra=None, facing=False, align=0, colour=False, colour_within=0.9, color=None, color_within=None):
        """Extension: look for a lost object near where it was last seen.  The reference re-initialises from an external detector
        (predict.py:539-541); this searches the observed depth frame instead and hands the track back:
          1. the lattice of candidates around prev_pose (recover.pose_lattice; `extra`: a list of poses appended after it) is scored
             against `depth` (HxW uint16 mm) in ONE device call with its `top` best picked (Engine.score_poses);
          2. refine >= 1: the top poses go through on_track_batch(top_poses, [rgb] * k, [depth] * k), `refine` times -- the network
             pulls a nearby hypothesis in;
          3. [refined..., unrefined...] are scored once more and the pose with the largest key wins (recover.pose_key: more
             inliers, then fewer seen-through points, then the lower index -- ties prefer the refined pose).
        So the result never scores below the lattice's best.  refine=0 returns the top lattice candidate with no network call.
        points: model points ([P,3], an object with .points, or a ModelPoints handle); default ``object_cloud``.  top defaults to
        min(8, engine.max_batch).  ``last_recover`` keeps n, top_idx, top_fit, refined, final_fit, chosen and inlier_frac
        (= inlier_pts / points of the returned pose).  With fit_check set, last_fit_ratio is whatever on_track_batch left.
        facing=True: only the model points whose normal faces the camera are counted (the rule of se3tn_score_pose_grid), in both
        scorings, so inlier_frac is the share of the VISIBLE surface the sensor confirms and means the same for every object.  The
        lattice then travels as its factors (recover.lattice_factors through Engine.score_pose_grid) and [refined, unrefined] are
        rescored as the diagonal of a 2k x 2k grid.  Needs normals: ``object_normals``, or a ModelPoints handle that carries them
        as `points`; `extra` cannot be combined with it (extra poses are no product): ValueError.
        align = iters > 0: the top lattice candidates are first aligned to the depth frame (align(): up to `iters` point-to-plane
        steps of the facing points, Engine.align_poses) and the network, if any, starts from the aligned poses; the final pool is
        [refined..., aligned..., unaligned...] (refine=0: [aligned..., unaligned...]), scored as before, so the result never scores
        below the one without alignment.  Needs ``object_normals`` (or a handle with normals as `points`) with or without facing --
        the scoring of the plain search stays plain.  ``last_recover`` then also keeps aligned and align_rec.
        colour=True (or color=True; off by default, and then not one call more is made): the final pool and its depth keys are
        formed as above and D is their winner; the pool members with inlier_pts >= colour_within * inlier_pts[D] go through
        verify() and the highest colour score wins (a tie: the larger depth key; every score 0: D).  Depth alone cannot tell a
        near-symmetric object from its half turn; its colours can.  colour_within is a design choice, not a measured value.
        ``last_recover`` then also keeps depth_chosen, color_fit, color_score and candidates."""
        colour = bool(colour or color)
        colour_within = colour_within if color_within is None else color_within
        if facing:
            if extra is not None and len(extra):
                raise ValueError("recover: extra poses cannot be combined with facing=True (the lattice is scored as a product)")
            return self._recover_facing(prev_pose, rgb, depth, trans_radius, trans_step, rot_deg, tol_mm, top, refine, points, align,
                                        colour, colour_within)
        from .engine import ModelPoints
        from .recover import pose_key, pose_lattice
        if points is None:
            if self.object_cloud is None:
                raise ValueError("recover: this tracker has no object_cloud (no model_path was given) and no points were passed")
            if self._model_points is None:
                self._model_points = self.engine.model_points(self.object_cloud)
            handle, own = self._model_points, False
        elif isinstance(points, ModelPoints):
            handle, own = points, False
        else:
            handle, own = self.engine.model_points(points), True
        try:
            if int(align) > 0:   # the alignment reads normals: the tracker's facing handle, or the caller's own when it carries them
                with_normals = isinstance(points, ModelPoints) and points.normals is not None
                facing_handle = points if with_normals else self._facing_handle(None, "recover")
            k = min(8, self.engine.max_batch) if top is None else int(top)
            cands = pose_lattice(prev_pose, trans_radius, trans_step, rot_deg)
            if extra is not None and len(extra):
                cands = np.concatenate([cands, np.asarray(extra, np.float64).reshape(-1, 4, 4)])
            dep = np.ascontiguousarray(depth, dtype=np.uint16)
            top_idx, top_fit = self.engine.score_poses(handle, cands, dep, self.K, tol_mm, top=k)
            unrefined = cands[top_idx]
            info = dict(n=len(cands), top_idx=top_idx, top_fit=top_fit, refined=None)
            aligned = None
            if int(align) > 0:
                aligned, align_rec = self.engine.align_poses(facing_handle, unrefined, dep, self.K, iters=int(align))
                info.update(aligned=aligned, align_rec=align_rec)
            if int(refine) < 1 and aligned is None:
                info.update(final_fit=top_fit[:1].copy(), chosen=0, inlier_frac=float(top_fit["inlier_pts"][0]) / float(top_fit["points"][0]))
                if colour:   # the pool is the ranked top of the lattice
                    info.update(final_fit=top_fit.copy())
                    self._choose_by_colour(info, unrefined, top_fit, rgb, dep, tol_mm, colour_within)
                self.last_recover = info
                return unrefined[info["chosen"]].copy()
            refined = unrefined if aligned is None else aligned
            for _ in range(int(refine)):
                refined = np.asarray(self.on_track_batch(list(refined), [rgb] * k, [dep] * k), np.float64)
            final = np.concatenate(([refined] if int(refine) >= 1 else []) + ([] if aligned is None else [aligned]) + [unrefined])
            final_fit = self.engine.score_poses(handle, final, dep, self.K, tol_mm)
            keys = pose_key(final_fit)
            chosen = int(np.argmax(keys))             # keys are unique: the lower index wins a tie, and the refined poses come first
            info.update(refined=refined if int(refine) >= 1 else None, final_fit=final_fit, chosen=chosen,
                        inlier_frac=float(final_fit["inlier_pts"][chosen]) / float(final_fit["points"][chosen]))
            if colour:
                chosen = self._choose_by_colour(info, final, final_fit, rgb, dep, tol_mm, colour_within)
            self.last_recover = info
            return final[chosen].copy()
        finally:
            if own:
                handle.close()

    @property
    def object_normals(self):
        """One normal per point of ``object_cloud`` (float64 [P,3], not of unit length), or None without a model: the normals the
        .ply stores, else utils.vertex_normals of the model's triangles, down-sampled with the cloud
        (utils.voxel_down_sample_normals: the mean normal of each voxel).  None for a model that has neither normals nor triangles.
        Computed at first read -- only recover(facing=True) and acquire need them.  Assignable."""
        if isinstance(self._normals, tuple):
            model_path, pts = self._normals
            nrm = U.load_model_normals(model_path, pts)
            self._normals = None if nrm is None else U.voxel_down_sample_normals(pts, nrm, 0.005)[1]
        return self._normals

    @object_normals.setter
    def object_normals(self, normals):
        self._normals = None if normals is None else np.asarray(normals, np.float64).reshape(-1, 3)
        self._facing_points = None

    def _facing_handle(self, points, who):
        """the ModelPoints handle with normals a facing search scores against"""
        from .engine import ModelPoints
        if points is None:
            if self.object_cloud is None or self.object_normals is None:
                raise ValueError("%s: this tracker has no object_normals (no model_path, or a model without normals and triangles) "
                                 "and no ModelPoints handle with normals was passed" % who)
            if self._facing_points is None:
                self._facing_points = self.engine.model_points(self.object_cloud, self.object_normals)
            return self._facing_points
        if not isinstance(points, ModelPoints) or points.normals is None:
            raise ValueError("%s: with facing=True `points` must be a ModelPoints handle that carries normals "
                             "(Engine.model_points(pts, normals))" % who)
        return points

    def _score_diagonal(self, handle, poses, dep, tol_mm):
        """the facing records of m poses: the diagonal of the m x m grid of their rotations and translations (one device call)"""
        poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        m = len(poses)
        fit = self.engine.score_pose_grid(handle, poses[:, :3, :3], poses[:, :3, 3], dep, self.K, tol_mm, facing=True)
        return fit[np.arange(m) * m + np.arange(m)]

    def _refine_and_choose(self, handle, unrefined, rgb, dep, tol_mm, refine, aligned=None):
        """steps 2 and 3 of recover under the facing rule -> (final poses, refined, final_fit, chosen).  With `aligned` (the
        unrefined poses after align()) the network starts from those and the pool is [refined..., aligned..., unrefined...];
        refine < 1 leaves the refined part out (refined is then None)."""
        from .recover import pose_key
        k = len(unrefined)
        refined = unrefined if aligned is None else aligned
        for _ in range(int(refine)):
            refined = np.asarray(self.on_track_batch(list(refined), [rgb] * k, [dep] * k), np.float64)
        if int(refine) < 1:
            refined = None
        final = np.concatenate(([] if refined is None else [refined]) + ([] if aligned is None else [aligned]) + [unrefined])
        final_fit = self._score_diagonal(handle, final, dep, tol_mm)
        return final, refined, final_fit, int(np.argmax(pose_key(final_fit)))   # ties prefer the earlier part of the pool: the lower index

    def verify(self, poses, rgb, depth, tol_mm=10, min_px=64, scene=None):
        """Extension: which of these n pose hypotheses ([n,4,4]) does the frame (rgb HxWx3 uint8, depth HxW uint16 mm) confirm --
        by colour, where depth cannot tell: per pose the model rendered in its own compute_bbox window against that window of the
        frame, compared at the pixels where the two depths agree within tol_mm -> (fit [n], color [n], score [n]): the depth
        records (as fit_stats), the colour records (_lib.COLOR_FIT_DTYPE) and utils.color_score of each (the zero-mean normalised
        cross-correlation, mean of R, G, B; 0 below min_px compared pixels).  With the built-in HIP renderer ONE library call
        (se3tn_verify_poses_host); with an injected renderer render_window per pose plus Engine.color_stats.
        scene: the composed depth of the tracked objects of the frame, uint16 [H,W] as an array or a cuda 16-bit tensor
        (Engine.scene_fit(..., scene=True); MultiTracker.verify composes it from its own objects) -- the scene-aware rule
        (se3tn_verify_poses_scene_host, utils.fit_stats(scene=)): a pixel with a tracked surface at or in front of the model's is
        hidden_px and not compared, so an object lying on this one does not lend it its colours; fit is then
        _lib.SCENE_CROP_FIT_DTYPE."""
        from .renderer import HipRenderer
        poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        n = len(poses)
        if n > self.engine.max_batch:
            raise ValueError("verify: %d poses > max_samples=%d given to Tracker()" % (n, self.engine.max_batch))
        if n == 0:
            from ._lib import COLOR_FIT_DTYPE, FIT_DTYPE, SCENE_CROP_FIT_DTYPE
            return np.zeros(0, FIT_DTYPE if scene is None else SCENE_CROP_FIT_DTYPE), np.zeros(0, COLOR_FIT_DTYPE), np.zeros(0, np.float64)
        if self.one_call and isinstance(self.renderer, HipRenderer):
            dep = _depth_u16(depth, rgb).view(np.uint16)   # the shape check and the reference's cast; the host call takes the uint16 itself
            fit, color, _ = self.engine.verify_poses(self.renderer, poses, rgb, dep, self.K, self.object_width, tol_mm, scene=scene)
        else:
            fit, color = self._verify_stepwise(poses, rgb, depth, tol_mm, scene)
        return fit, color, np.atleast_1d(U.color_score(color, min_px))

    def _verify_stepwise(self, poses, rgb, depth, tol_mm, scene=None):
        """verify on the step-by-step path: per pose render_window against the uploaded frame under the pose's own crop window,
        through Engine.color_stats -- the records the one-call path gets from the library (scene: the frame-sized scene under the
        same window)"""
        rgb_d = torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8)).to(self._dev)
        dep_d = torch.from_numpy(_depth_u16(depth, rgb)).to(self._dev)
        if scene is not None and not torch.is_tensor(scene):
            scene = torch.from_numpy(np.ascontiguousarray(scene, dtype=np.uint16).view(np.int16)).to(self._dev)
        model, observed, hiding = [], [], []
        for pose in poses:
            rgbA, depA = self.render_window(pose)
            model.append(dict(rgb=torch.from_numpy(np.ascontiguousarray(rgbA, dtype=np.uint8)).to(self._dev),
                              depth=torch.from_numpy(np.ascontiguousarray(depA).astype(np.uint16).view(np.int16)).to(self._dev)))
            bb = U.compute_bbox(pose, self.K, self.object_width, scale=(1000, 1000, 1000))
            observed.append(dict(rgb=rgb_d, depth=dep_d, window=U.crop_window(bb)))
            hiding.append(dict(depth=scene, window=U.crop_window(bb)))
        return self.engine.color_stats(model, observed, tol_mm, scene=None if scene is None else hiding)

    def _choose_by_colour(self, info, final, final_fit, rgb, dep, tol_mm, within, min_px=64, scene=None):
        """colour=True of acquire / recover: D = the depth winner (info['chosen']); the candidates are the pool members whose
        inlier_pts reach `within` times D's -- colour never buys a pose the depth frame does not support; among them the highest
        verify score wins, a tie goes to the larger depth key, and if every candidate scores 0, D stays.  `dep` is the uint16 frame
        the depth stages of the caller read; scene: verify's (MultiTracker.recover: the kept scene of its search).  Updates info;
        returns the chosen index."""
        from ._lib import COLOR_FIT_DTYPE
        from .recover import pose_key
        d = int(info["chosen"])
        keys = pose_key(final_fit)
        cand = np.flatnonzero(final_fit["inlier_pts"].astype(np.float64) >= float(within) * float(final_fit["inlier_pts"][d]))
        score = np.zeros(len(final), np.float64)
        color = np.zeros(len(final), COLOR_FIT_DTYPE)
        mb = self.engine.max_batch
        for i0 in range(0, len(cand), mb):   # (a pool of 3 x top poses may exceed the engine's batch)
            part = cand[i0:i0 + mb]
            _, col, sc = self.verify(final[part], rgb, dep, tol_mm, min_px) if scene is None else \
                self.verify(final[part], rgb, dep, tol_mm, min_px, scene=scene)
            color[part], score[part] = col, sc
        chosen = d
        if np.any(score[cand] != 0.0):
            best = cand[score[cand] == score[cand].max()]
            chosen = int(best[np.argmax(keys[best])])
        info.update(depth_chosen=d, color_fit=color, color_score=score, candidates=cand, chosen=chosen,
                    inlier_frac=self._frac(final_fit[chosen]))
        return chosen

    def align(self, poses, depth, **kw):
        """Align n pose hypotheses ([n,4,4]) to the depth frame (HxW uint16 mm): Engine.align_poses on ``object_cloud`` with
        ``object_normals`` (uploaded at first use and kept) and this tracker's K -> (poses [n,4,4], records [n]); the keywords
        (gate_mm, iters, min_pairs, damping, stop, sums) are Engine.align_poses'.  Needs ``object_normals``: ValueError otherwise.
        scene=..., scene_tol_mm=10 (Engine.align_poses'): the composed depth of the tracked objects, uint16 [H,W] as an array or a cuda
        16-bit tensor -- points hidden by it are not paired and the records are _lib.SCENE_ALIGN_REC_DTYPE (MultiTracker.align
        composes that scene from its own objects)."""
        handle = self._facing_handle(None, "align")
        dep = depth if torch.is_tensor(depth) else np.ascontiguousarray(depth, dtype=np.uint16)
        return self.engine.align_poses(handle, poses, dep, self.K, **kw)

    @staticmethod
    def _compose(rots, trans, idx):
        """candidates idx (r * n_trans + t) of the product rots x trans as [k,4,4] poses"""
        idx = np.asarray(idx, np.int64)
        out = np.tile(np.eye(4), (len(idx), 1, 1))
        out[:, :3, :3] = rots[idx // len(trans)]
        out[:, :3, 3] = trans[idx % len(trans)]
        return out

    @staticmethod
    def _frac(rec):
        return float(rec["inlier_pts"]) / float(rec["points"]) if int(rec["points"]) else 0.0

    def _recover_facing(self, prev_pose, rgb, depth, trans_radius, trans_step, rot_deg, tol_mm, top, refine, points, align=0,
                        colour=False, colour_within=0.9):
        from .recover import lattice_factors
        handle = self._facing_handle(points, "recover")
        k = min(8, self.engine.max_batch) if top is None else int(top)
        rots, trans = lattice_factors(prev_pose, trans_radius, trans_step, rot_deg)
        dep = np.ascontiguousarray(depth, dtype=np.uint16)
        top_idx, top_fit = self.engine.score_pose_grid(handle, rots, trans, dep, self.K, tol_mm, facing=True, top=k)
        unrefined = self._compose(rots, trans, top_idx)
        info = dict(n=len(rots) * len(trans), top_idx=top_idx, top_fit=top_fit, refined=None, facing=True)
        aligned = None
        if int(align) > 0:
            aligned, align_rec = self.engine.align_poses(handle, unrefined, dep, self.K, iters=int(align))
            info.update(aligned=aligned, align_rec=align_rec)
        if int(refine) < 1 and aligned is None:
            info.update(final_fit=top_fit[:1].copy(), chosen=0, inlier_frac=self._frac(top_fit[0]))
            if colour:   # the pool is the ranked top of the lattice
                info.update(final_fit=top_fit.copy())
                self._choose_by_colour(info, unrefined, top_fit, rgb, dep, tol_mm, colour_within)
            self.last_recover = info
            return unrefined[info["chosen"]].copy()
        final, refined, final_fit, chosen = self._refine_and_choose(handle, unrefined, rgb, dep, tol_mm, refine, aligned)
        info.update(refined=refined, final_fit=final_fit, chosen=chosen, inlier_frac=self._frac(final_fit[chosen]))
        if colour:
            chosen = self._choose_by_colour(info, final, final_fit, rgb, dep, tol_mm, colour_within)
        self.last_recover = info
        return final[chosen].copy()

    def acquire(self, rgb, depth, roi=None, views=40, inplane=12, stride=16, behind_m=0.03, tol_mm=10, top=None, refine=1, align=0,
                colour=False, colour_within=0.9, color=None, color_within=None):
        """Extension with no reference counterpart (the reference takes its first pose from a file, from ground truth or from
        PoseCNN): find the object in a frame with NO pose to start from.
          1. recover.rotation_grid(views, inplane) x recover.depth_seeds(depth, K, stride, behind_m, roi) -- rotations that cover
             SO(3) times one translation per valid pixel of a stride grid, pushed behind_m behind the seen surface -- scored as a
             product in ONE device call counting only the points that face the camera (Engine.score_pose_grid(facing=True)), the
             `top` best kept (default min(8, engine.max_batch)).  At most 2^20 candidates: ValueError otherwise (raise `stride`,
             or pass a `roi` = (left, top, right, bottom));
          2. around each of them the default lattice of recover(facing=True), its best candidate kept;
          3. refine >= 1: those go through on_track_batch `refine` times; [refined..., unrefined...] are scored once more and the
             pose with the largest key is returned (refine=0: the best of step 2, no network call).
        Depth alone fixes WHERE the object is, not which way a near-symmetric object is turned: a box scores the same after half a
        turn, and the true rotation may come second or fourth.  That is why ``last_acquire`` keeps ALL `top` hypotheses and not
        just the winner: n, n_rot, n_trans, stage1_idx, stage1_fit, hypotheses (their poses), local, local_idx, local_fit (step 2),
        refined, final_fit, chosen, inlier_frac (= inlier_pts / facing points of the returned pose).  Use colour, the network's
        own fit check (fit_check) or a few tracked frames to tell them apart.  Needs ``object_normals``.
        align = iters > 0: the hypotheses of step 2 are aligned to the depth frame before step 3 (align(): up to `iters`
        point-to-plane steps each, one device call for all of them); the network, if any, starts from the aligned poses and the
        pool of step 3 is [refined..., aligned..., unaligned...] (refine=0: [aligned..., unaligned...]).  ``last_acquire`` then
        also keeps aligned and align_rec.  The lattices end 10 mm and 15 degrees apart; alignment ends on the surface.
        colour=True (or color=True; off by default, and then not one call more is made): the pool of step 3 and its depth keys
        are formed as above and D is their winner; the pool members with inlier_pts >= colour_within * inlier_pts[D] go through
        verify() -- the model rendered at each against `rgb` -- and the highest colour score wins (a tie: the larger depth key;
        every score 0: D).  Colour never buys a pose the depth frame does not support.  colour_within is a design choice, not a
        measured value.  ``last_acquire`` then also keeps depth_chosen, color_fit, color_score and candidates."""
        colour = bool(colour or color)
        colour_within = colour_within if color_within is None else color_within
        from .recover import depth_seeds, lattice_factors, pose_key, rotation_grid
        from ._lib import POSE_SEARCH_MAX_POSES, POINT_FIT_DTYPE
        handle = self._facing_handle(None, "acquire")
        dep = np.ascontiguousarray(depth, dtype=np.uint16)
        rots = rotation_grid(views, inplane)
        seeds = depth_seeds(dep, self.K, stride, behind_m, roi)
        if len(seeds) == 0:
            raise ValueError("acquire: no valid depth pixel (100 < d < 2000 mm) on the stride grid of the region searched")
        n = len(rots) * len(seeds)
        if n > POSE_SEARCH_MAX_POSES:
            raise ValueError("acquire: %d rotations x %d seeds = %d candidates > 2^20: raise stride (now %d) or narrow roi"
                             % (len(rots), len(seeds), n, int(stride)))
        k = min(min(8, self.engine.max_batch) if top is None else int(top), n)
        idx1, fit1 = self.engine.score_pose_grid(handle, rots, seeds, dep, self.K, tol_mm, facing=True, top=k)
        hyps = self._compose(rots, seeds, idx1)
        local, local_idx, local_fit = np.empty_like(hyps), np.empty(k, np.int32), np.zeros(k, POINT_FIT_DTYPE)
        for i in range(k):
            lr, lt = lattice_factors(hyps[i])
            li, lf = self.engine.score_pose_grid(handle, lr, lt, dep, self.K, tol_mm, facing=True, top=1)
            local[i], local_idx[i], local_fit[i] = self._compose(lr, lt, li)[0], li[0], lf[0]
        info = dict(n=n, n_rot=len(rots), n_trans=len(seeds), stage1_idx=idx1, stage1_fit=fit1, hypotheses=hyps, local=local,
                    local_idx=local_idx, local_fit=local_fit, refined=None)
        aligned = None
        if int(align) > 0:
            aligned, align_rec = self.engine.align_poses(handle, local, dep, self.K, iters=int(align))
            info.update(aligned=aligned, align_rec=align_rec)
        if int(refine) < 1 and aligned is None:
            chosen = int(np.argmax(pose_key(local_fit)))
            info.update(final_fit=local_fit.copy(), chosen=chosen, inlier_frac=self._frac(local_fit[chosen]))
            if colour:
                chosen = self._choose_by_colour(info, local, local_fit, rgb, dep, tol_mm, colour_within)
            self.last_acquire = info
            return local[chosen].copy()
        final, refined, final_fit, chosen = self._refine_and_choose(handle, local, rgb, dep, tol_mm, refine, aligned)
        info.update(refined=refined, final_fit=final_fit, chosen=chosen, inlier_frac=self._frac(final_fit[chosen]))
        if colour:
            chosen = self._choose_by_colour(info, final, final_fit, rgb, dep, tol_mm, colour_within)
        self.last_acquire = info
        return final[chosen].copy()

    @property
    def fit_check(self):
        """None (default) | tol_mm: every on_track / on_track_live / on_track_batch also scores its estimate against the observed
        depth (se3tn_set_fit_check): the model rendered at the estimate in the window of the previous pose, compared with the depth
        image B was cropped from.  last_prediction then carries ``fit`` (the records: structured array with model_px, seen_px,
        inlier_px, front_px, behind_px, sum_abs_mm, tol_mm), ``pred_rgb`` / ``pred_depth`` (device tensors [n,176,176,3] /
        [n,176,176]: `pred_color`, `pred_depth` of predict.py:284, in the previous pose's window) and last_fit_ratio is
        inlier_px / model_px."""
        return self.engine.get_fit_check()

    @fit_check.setter
    def fit_check(self, tol_mm):
        self.engine.set_fit_check(tol_mm)
        if not tol_mm:
            self.last_fit_ratio = None

    def _fit_from_call(self, n, single):
        """fit_check set: the records and estimate renders the library call just left (se3tn_last_fit / _images) into last_prediction"""
        if not self.engine.get_fit_check():
            self.last_fit_ratio = None
            return
        fit = self.engine.last_fit(n)
        if self._fit_imgs is None or self._fit_imgs[0].shape[0] < n:
            self._fit_imgs = (torch.empty((n, 176, 176, 3), dtype=torch.uint8, device=self._dev),
                              torch.empty((n, 176, 176), dtype=torch.int16, device=self._dev))
        self.engine.last_fit_images(n, self._fit_imgs[0], self._fit_imgs[1])
        self.last_prediction.update(fit=fit, pred_rgb=self._fit_imgs[0][:n], pred_depth=self._fit_imgs[1][:n])
        r = U.fit_ratio(fit)
        self.last_fit_ratio = float(r[0]) if single else r

    def _fit_stepwise(self, prev_poses, ests, frame_depths, bboxes, single):
        """fit_check set on the step-by-step path: per pair a render at the ESTIMATE in the window of the PREVIOUS pose
        (render_window(est, window_of=prev)) against the uploaded frame under image B's window, through Engine.fit_stats -- the
        records the one-call path gets from the library's own stage."""
        tol = self.engine.get_fit_check()
        if not tol:
            self.last_fit_ratio = None
            return
        model, observed, rgbs = [], [], []
        for prev, est, dep_d, bb in zip(prev_poses, ests, frame_depths, bboxes):
            rgbP, depP = self.render_window(est, window_of=prev)
            rgbs.append(torch.from_numpy(np.ascontiguousarray(rgbP)).to(self._dev))
            model.append(torch.from_numpy(np.ascontiguousarray(depP).astype(np.uint16).view(np.int16)).to(self._dev))
            observed.append(dict(depth=dep_d, window=U.crop_window(bb)))
        fit = self.engine.fit_stats(model, observed, tol)
        self.last_prediction.update(fit=fit, pred_rgb=torch.stack(rgbs), pred_depth=torch.stack(model))
        r = U.fit_ratio(fit)
        self.last_fit_ratio = float(r[0]) if single else r

    def _read_back(self, n):
        """(poseB [n,4,4] float64, trans [n,3], rot [n,3] float32) of the last engine call: one device-to-host copy."""
        ms = self.engine.max_batch
        host = self._out.cpu().numpy()
        poseB = host[:ms * 128].view(np.float64).reshape(ms, 4, 4)[:n].copy()
        trans = host[ms * 128:ms * 140].view(np.float32).reshape(ms, 3)[:n].copy()
        rot = host[ms * 140:ms * 152].view(np.float32).reshape(ms, 3)[:n].copy()
        return poseB, trans, rot

    def render_window(self, ob2cam, window_of=None):
        """predict.py:193-215.  window_of (extension): the pose whose bbox gives the window (default: ob2cam itself, as the
        reference) -- the fit check renders the estimate in the previous pose's window.  Three renderer protocols, in the
        reference's order:
          * VispyRenderer-like objects (``update_cam_mat`` + ``render_image``): driven exactly as
            predict.py:201-208 does -- y-flipped bbox (scale (1000,-1000,1000)), ``update_cam_mat(K, left,
            right, bottom, top)``, ``render_image(ob2cam_gl)``;
          * the HIP rasteriser and any injected ``render(ob2cam, K, window)`` object: the same y-flipped
            window (left, top, right, bottom) is passed (round 1 passed the plain crop window: INTEGRATION.md);
          * full-frame renderers in the style of offscreen_renderer.Renderer (``render([ob2cam])`` ->
            rgb HxWx3, depth HxW metres; predict.py:209-213): depth -> uint16 mm, then the crop + NEAREST
            resize of crop_bbox on the device (se3tn_crop_raw)."""
        if self.renderer is None:
            raise RuntimeError("Tracker.render_window: no renderer injected (rendering is outside the HIP hot path)")
        from .renderer import HipRenderer
        ob2cam = np.asarray(ob2cam, np.float64)
        wpose = ob2cam if window_of is None else np.asarray(window_of, np.float64)
        if isinstance(self.renderer, HipRenderer) and self.renderer.full_frame:     # predict.py:209-213
            rgb_d, dep_d = self.renderer.render_frame_device(ob2cam, self.K)
            bbox = U.compute_bbox(wpose, self.K, self.object_width, scale=(1000, 1000, 1000))
            return self.engine.crop_raw(rgb_d, dep_d, U.crop_window(bbox))
        win = HipRenderer.gl_window(wpose, self.K, self.object_width)      # left, top, right, bottom (GL image)
        if hasattr(self.renderer, "update_cam_mat") and hasattr(self.renderer, "render_image"):
            glcam_in_cvcam = np.diag([1.0, -1.0, -1.0, 1.0])
            self.renderer.update_cam_mat(self.K, win[0], win[2], win[3], win[1])
            return self.renderer.render_image(np.linalg.inv(glcam_in_cvcam).dot(ob2cam))
        if _is_full_frame_renderer(self.renderer):
            rgb, depth = self.renderer.render([ob2cam])
            depth = (np.asarray(depth) * 1000).astype(np.uint16)
            bbox = U.compute_bbox(wpose, self.K, self.object_width, scale=(1000, 1000, 1000))
            return self.engine.crop_raw(rgb, depth, U.crop_window(bbox))
        return self.renderer.render(ob2cam, self.K, win)

    def on_track(self, prev_pose, current_rgb, current_depth, gt_A_in_cam=None, gt_B_in_cam=None,
                 debug=False, samples=1):
        """predict.py:217-296.  current_rgb HxWx3 uint8 RGB, current_depth HxW uint16 mm,
        prev_pose 4x4 object-in-camera (metres).  Returns the 4x4 float64 pose estimate."""
        if self._stream is not None and torch.cuda.current_stream() != self._stream:
            with torch.cuda.stream(self._stream):
                return self.on_track(prev_pose, current_rgb, current_depth, gt_A_in_cam, gt_B_in_cam, debug, samples)
        prev_pose = np.asarray(prev_pose, np.float64)
        from .renderer import HipRenderer
        if self.one_call and isinstance(self.renderer, HipRenderer) and int(samples) <= 1:
            return self._on_track_one_call(prev_pose, current_rgb, current_depth)
        bb = U.compute_bbox(prev_pose, self.K, self.object_width, scale=(1000, 1000, 1000))
        dev = self._dev
        winA = (0, 0, self.image_size[0], self.image_size[0])
        if isinstance(self.renderer, HipRenderer) and self.renderer.full_frame:
            # pyrender route: the full rendered frame stays on the device and is cropped by the same kernel (and the
            # same bbox) as the camera frame -- predict.py:209-213 without the host round trip
            rgbA_d, depA_d = self.renderer.render_frame_device(prev_pose, self.K)
            winA = U.crop_window(bb)
        elif isinstance(self.renderer, HipRenderer):   # rendered A never leaves the device
            rgbA_d, depA_d = self.renderer.render_device(
                prev_pose, self.K, HipRenderer.gl_window(prev_pose, self.K, self.object_width))
        else:
            rgbA, depthA = self.render_window(prev_pose)
            rgbA_d = torch.from_numpy(np.ascontiguousarray(rgbA)).to(dev, non_blocking=True)
            depA_d = torch.from_numpy(np.ascontiguousarray(depthA).astype(np.uint16).view(np.int16)).to(dev, non_blocking=True)
        rgb_d = torch.from_numpy(np.ascontiguousarray(current_rgb)).to(dev, non_blocking=True)
        dep_d = torch.from_numpy(_depth_u16(current_depth, current_rgb)).to(dev, non_blocking=True)
        z_mm = float(prev_pose[2, 3]) * 1000
        # the reference evaluates `samples` IDENTICAL hypotheses (only i == 0 sets sample_pose, predict.py:229-231)
        # and returns the first: any count beyond the engine's batch capacity adds nothing -- clamp, never overrun
        n = max(1, min(int(samples), self.engine.max_batch))
        cropA = dict(rgb=rgbA_d, depth=depA_d, window=winA, z_offset_mm=z_mm, stats=0)
        cropB = dict(rgb=rgb_d, depth=dep_d, window=U.crop_window(bb), z_offset_mm=z_mm, stats=1)
        self.engine.preprocess([cropA] * n, self.engine.input_buffer_ptr(0))
        self.engine.preprocess([cropB] * n, self.engine.input_buffer_ptr(1))
        self._poseA[:n].copy_(torch.from_numpy(np.tile(prev_pose.reshape(1, 16), (n, 1))), non_blocking=True)
        self.engine.infer(self.engine.input_buffer_ptr(0), self.engine.input_buffer_ptr(1), n, NHWC,
                          self._trans, self._rot, self._poseA, self._poseB)
        poseB, trans_h, rot_h = self._read_back(n)               # one D2H + sync, as predict.py:275-276
        self.last_prediction = dict(trans=trans_h, rot=rot_h, bbox=bb)
        self._fit_stepwise([prev_pose], [poseB[0]], [dep_d], [bb], True)
        self.prev_rgb = current_rgb
        self.prev_depth = current_depth
        self.frame_cnt += 1
        return poseB[0]

    def _on_track_one_call(self, prev_pose, current_rgb, current_depth):
        """The whole frame in ONE library call (se3tn_on_track): compute_bbox, image A, both crops in one launch, network, pose
        update, read-back; the camera frame goes up as the window's rows / columns only, through pinned memory, together with the
        pose.  Same arithmetic as the step-by-step path below (tests/test_tracker_surface.py compares the two)."""
        rgb = current_rgb if (type(current_rgb) is np.ndarray and current_rgb.dtype == np.uint8 and current_rgb.flags.c_contiguous) \
            else np.ascontiguousarray(current_rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("rgb must be HxWx3 uint8")
        dep = current_depth if (type(current_depth) is np.ndarray and current_depth.dtype == np.uint16 and current_depth.flags.c_contiguous
                                and current_depth.shape == rgb.shape[:2]) else _depth_u16(current_depth, rgb)
        st = self._one_call_args()
        C = st["C"]
        st["P"][...] = prev_pose
        r = self.renderer
        rgbA, depthA = (st["rgbA"], st["depthA"]) if st["full_frame"] else (r.rgb, r.depth)
        st["check"](st["fn"](self.engine._h, r._m, st["p_P"], st["p_K"], C.c_double(float(self.object_width)), C.c_void_p(rgb.ctypes.data),
                             C.c_void_p(dep.ctypes.data), int(rgb.shape[0]), int(rgb.shape[1]), C.c_void_p(rgbA.data_ptr()),
                             C.c_void_p(depthA.data_ptr()), st["p_pose"], st["p_tr"], st["p_ro"], st["p_bb"], st["stream"]()),
                    "se3tn_on_track")
        return self._one_call_result(st, rgbA, depthA, current_rgb, current_depth)

    def _one_call_args(self):
        """argument objects of se3tn_on_track / se3tn_on_track_live: built once, not per frame.  ``K`` and ``renderer`` are public
        attributes the step-by-step path reads on every call, so the camera matrix is copied into the argument buffer and the
        renderer's route is looked up per call (no allocation unless a full-frame renderer is met for the first time)."""
        st = self._one_call_state
        if st is None:
            import ctypes as C
            from ._lib import check
            from .engine import _stream_ptr
            st = self._one_call_state = dict(
                C=C, check=check, stream=_stream_ptr, fn=self.engine.lib.se3tn_on_track, P=np.empty((4, 4), np.float64),
                K=np.empty((3, 3), np.float64), pose=np.empty((4, 4), np.float64), tr=np.empty(3, np.float32),
                ro=np.empty(3, np.float32), bb=np.empty((4, 2), np.int32))
            for k, t in (("P", C.c_double), ("K", C.c_double), ("pose", C.c_double), ("tr", C.c_float), ("ro", C.c_float), ("bb", C.c_int32)):
                st["p_" + k] = st[k].ctypes.data_as(C.POINTER(t))
        st["K"][...] = self.K
        st["full_frame"] = bool(self.renderer.full_frame)
        if st["full_frame"] and "rgbA" not in st:
            # pyrender route: the renderer's own buffers hold a whole frame; image A (the 176 x 176 crop of the render, what
            # render_window returns) goes to buffers of the tracker
            st["rgbA"] = torch.empty((176, 176, 3), dtype=torch.uint8, device=self._dev)
            st["depthA"] = torch.empty((176, 176), dtype=torch.int16, device=self._dev)
        return st

    def _one_call_result(self, st, rgbA, depthA, current_rgb, current_depth):
        self.last_prediction = dict(trans=st["tr"].reshape(1, 3).copy(), rot=st["ro"].reshape(1, 3).copy(), bbox=st["bb"].copy())
        if st["full_frame"]:
            self.last_prediction.update(rgbA=rgbA, depthA=depthA)
        self._fit_from_call(1, True)
        self.prev_rgb = current_rgb
        self.prev_depth = current_depth
        self.frame_cnt += 1
        return st["pose"].copy()

    def on_track_live(self, prev_pose, color, depth_raw, bgr=False, max_depth=2.0, extrapolate=False, blur_type="bilateral",
                      depth_filled=None):
        """predict_ros.py:38-60 for one camera frame: fill_depth of the RAW depth frame (HxW uint16 mm with holes), the colour
        frame's channel order (bgr=True: what CvBridge 'bgr8' delivers) and on_track.  With the built-in rasteriser this is ONE
        library call (se3tn_on_track_live): the raw depth frame goes up whole, only the crop window's part of it is blurred and
        converted, and the filled frame never visits the host.  depth_filled (optional cuda int16/uint16 [H,W]) receives the whole
        filled frame.  With an injected renderer (or one_call = False) it composes engine.fill_depth + on_track.  Returns the 4x4
        float64 pose; prev_rgb / prev_depth keep the frames as given."""
        if self._stream is not None and torch.cuda.current_stream() != self._stream:
            with torch.cuda.stream(self._stream):
                return self.on_track_live(prev_pose, color, depth_raw, bgr, max_depth, extrapolate, blur_type, depth_filled)
        prev_pose = np.asarray(prev_pose, np.float64)
        from . import _lib
        from .renderer import HipRenderer
        if not (self.one_call and isinstance(self.renderer, HipRenderer)):
            filled = self.engine.fill_depth(np.asarray(depth_raw).astype(np.uint16), max_depth, extrapolate, blur_type)
            if depth_filled is not None:
                depth_filled.copy_(torch.from_numpy(filled.view(np.int16)).view(depth_filled.dtype))
            rgb = np.ascontiguousarray(np.asarray(color)[:, :, ::-1]) if bgr else color
            return self.on_track(prev_pose, rgb, filled)
        col = color if (type(color) is np.ndarray and color.dtype == np.uint8 and color.flags.c_contiguous) \
            else np.ascontiguousarray(color, dtype=np.uint8)
        if col.ndim != 3 or col.shape[2] != 3:
            raise ValueError("color must be HxWx3 uint8")
        raw = depth_raw if (type(depth_raw) is np.ndarray and depth_raw.dtype == np.uint16 and depth_raw.flags.c_contiguous
                            and depth_raw.shape == col.shape[:2]) else _depth_u16(depth_raw, col)
        H, W = int(col.shape[0]), int(col.shape[1])
        if depth_filled is not None:
            assert depth_filled.is_cuda and depth_filled.element_size() == 2 and depth_filled.is_contiguous() \
                and tuple(depth_filled.shape) == (H, W)
        st = self._one_call_args()
        C = st["C"]
        st["P"][...] = prev_pose
        r = self.renderer
        rgbA, depthA = (st["rgbA"], st["depthA"]) if st["full_frame"] else (r.rgb, r.depth)
        blur = blur_type if isinstance(blur_type, int) else \
            {"bilateral": _lib.BLUR_BILATERAL, "gaussian": _lib.BLUR_GAUSSIAN}.get(blur_type, _lib.BLUR_NONE)
        order = bgr if (isinstance(bgr, int) and not isinstance(bgr, bool)) else (_lib.COLOR_BGR if bgr else _lib.COLOR_RGB)
        st["check"](self.engine.lib.se3tn_on_track_live(
            self.engine._h, r._m, st["p_P"], st["p_K"], C.c_double(float(self.object_width)), C.c_void_p(col.ctypes.data), int(order),
            C.c_void_p(raw.ctypes.data), H, W, C.c_double(float(max_depth)), 1 if extrapolate else 0, int(blur),
            C.c_void_p(depth_filled.data_ptr()) if depth_filled is not None else None, C.c_void_p(rgbA.data_ptr()),
            C.c_void_p(depthA.data_ptr()), st["p_pose"], st["p_tr"], st["p_ro"], st["p_bb"], st["stream"]()), "se3tn_on_track_live")
        return self._one_call_result(st, rgbA, depthA, color, depth_raw)

    def on_track_batch(self, prev_poses, rgbs, depths):
        """Extension: n independent (pose, frame) pairs of the SAME object in one engine call -- several
        sequences / cameras / hypotheses (frames of one track are serial, so this is where batch > 1
        comes from).  Same arithmetic per pair as on_track; returns [n,4,4] float64.
        With the built-in rasteriser the whole step is ONE library call (se3tn_on_track_batch: image A of all n poses in four
        launches, the frames' crop windows staged through pinned memory in one copy, no per-pair Python)."""
        from .renderer import HipRenderer
        n = len(prev_poses)
        if n > self.engine.max_batch:
            raise ValueError("on_track_batch: %d pairs > max_samples=%d given to Tracker()" % (n, self.engine.max_batch))
        if self.one_call and isinstance(self.renderer, HipRenderer) and n > 0:
            return self._on_track_batch_one_call(prev_poses, rgbs, depths)
        return self._on_track_batch_stepwise(prev_poses, rgbs, depths)

    def _on_track_batch_one_call(self, prev_poses, rgbs, depths):
        import ctypes as C
        from ._lib import check
        from .engine import _stream_ptr
        n = len(prev_poses)
        poses = np.ascontiguousarray(np.stack([np.asarray(p, np.float64) for p in prev_poses]).reshape(n, 16))
        frames_rgb, frames_dep = [], []
        for i in range(n):
            rgb = rgbs[i]
            if not (type(rgb) is np.ndarray and rgb.dtype == np.uint8 and rgb.flags.c_contiguous):
                rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
            if rgb.ndim != 3 or rgb.shape[2] != 3:
                raise ValueError("rgb must be HxWx3 uint8")
            dep = depths[i]
            if not (type(dep) is np.ndarray and dep.dtype == np.uint16 and dep.flags.c_contiguous and dep.shape == rgb.shape[:2]):
                dep = _depth_u16(dep, rgb)
            if rgb.shape != frames_rgb[0].shape if frames_rgb else False:
                raise ValueError("on_track_batch: the frames of one call must have one size")
            frames_rgb.append(rgb); frames_dep.append(dep)
        H, W = int(frames_rgb[0].shape[0]), int(frames_rgb[0].shape[1])
        st = self._batch_state
        if st is None or st["n"] < n:
            dev = self._dev
            st = self._batch_state = dict(
                n=n, rgbA=torch.empty((n, 176, 176, 3), dtype=torch.uint8, device=dev),
                depthA=torch.empty((n, 176, 176), dtype=torch.int16, device=dev), K=np.empty((3, 3), np.float64))
        st["K"][...] = self.K      # (a public attribute: the camera of THIS call, as the step-by-step path reads it)
        out = np.empty((n, 16), np.float64)
        tr, ro, bb = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty((n, 4, 2), np.int32)
        prgb = (C.c_void_p * n)(*[f.ctypes.data for f in frames_rgb])
        pdep = (C.c_void_p * n)(*[f.ctypes.data for f in frames_dep])
        check(self.engine.lib.se3tn_on_track_batch(
            self.engine._h, self.renderer._m, n, C.c_void_p(poses.ctypes.data), st["K"].ctypes.data_as(C.POINTER(C.c_double)),
            C.c_double(float(self.object_width)), prgb, pdep, H, W, C.c_void_p(st["rgbA"].data_ptr()), C.c_void_p(st["depthA"].data_ptr()),
            C.c_void_p(out.ctypes.data), C.c_void_p(tr.ctypes.data), C.c_void_p(ro.ctypes.data), C.c_void_p(bb.ctypes.data), _stream_ptr()),
            "se3tn_on_track_batch")
        self.last_prediction = dict(trans=tr, rot=ro, bbox=bb, rgbA=list(st["rgbA"][:n]), depthA=list(st["depthA"][:n]))
        self._fit_from_call(n, False)
        self.frame_cnt += 1
        return out.reshape(n, 4, 4)

    def _on_track_batch_stepwise(self, prev_poses, rgbs, depths):
        """on_track_batch step by step (injected renderers, one_call = False): per pair a render and two uploads"""
        from .renderer import HipRenderer
        n = len(prev_poses)
        dev = self._dev
        cropsA, cropsB, keep, bboxes = [], [], [], []
        poses = np.stack([np.asarray(p, np.float64) for p in prev_poses])
        for i in range(n):
            bb = U.compute_bbox(poses[i], self.K, self.object_width, scale=(1000, 1000, 1000))
            bboxes.append(bb)
            if isinstance(self.renderer, HipRenderer) and not self.renderer.full_frame:
                rgbA_d = torch.empty((176, 176, 3), dtype=torch.uint8, device=dev)
                depA_d = torch.empty((176, 176), dtype=torch.int16, device=dev)
                self.renderer.render_device(poses[i], self.K, HipRenderer.gl_window(poses[i], self.K, self.object_width),
                                            rgbA_d, depA_d)
            else:
                rgbA, depthA = self.render_window(poses[i])
                rgbA_d = torch.from_numpy(np.ascontiguousarray(rgbA)).to(dev)
                depA_d = torch.from_numpy(np.ascontiguousarray(depthA).astype(np.uint16).view(np.int16)).to(dev)
            rgb_d = torch.from_numpy(np.ascontiguousarray(rgbs[i])).to(dev, non_blocking=True)
            dep_d = torch.from_numpy(_depth_u16(depths[i], rgbs[i])).to(dev, non_blocking=True)
            keep += [rgbA_d, depA_d, rgb_d, dep_d]
            z_mm = float(poses[i, 2, 3]) * 1000
            cropsA.append(dict(rgb=rgbA_d, depth=depA_d, window=(0, 0, 176, 176), z_offset_mm=z_mm, stats=0))
            cropsB.append(dict(rgb=rgb_d, depth=dep_d, window=U.crop_window(bb), z_offset_mm=z_mm, stats=1))
        self.engine.preprocess(cropsA, self.engine.input_buffer_ptr(0))
        self.engine.preprocess(cropsB, self.engine.input_buffer_ptr(1))
        self._poseA[:n].copy_(torch.from_numpy(poses.reshape(n, 16)), non_blocking=True)
        self.engine.infer(self.engine.input_buffer_ptr(0), self.engine.input_buffer_ptr(1), n, NHWC,
                          self._trans, self._rot, self._poseA, self._poseB)
        out, trans_h, rot_h = self._read_back(n)
        # what on_track keeps in last_prediction / renderer.rgb, per pair (callers that log or check the step)
        self.last_prediction = dict(trans=trans_h, rot=rot_h, bbox=np.stack(bboxes), rgbA=keep[0::4], depthA=keep[1::4])
        self._fit_stepwise(poses, out, keep[3::4], bboxes, False)
        self.frame_cnt += 1
        return out


class MultiTracker:
    """Extension: several DIFFERENT objects in one camera frame, one library call per frame.  se(3)-TrackNet is trained per object
    (every YCB-Video class has its own weights, mean / std, normalisers and mesh: one ``Tracker`` each); a frame shows several of
    them.  ``on_track(prev_poses, rgb, depth)`` advances all of them through se3tn_on_track_objects: image A of every object in four
    rasteriser launches, the frame's crop windows in one upload, the network in chunks of <= 5 objects on the batch 1-5 kernel family
    with every object reading its own tracker's weights -- object i gets exactly the bits ``trackers[i].on_track`` gives it.
    The trackers are used as they are (their weights, normalisation and meshes stay where they live; nothing is copied); they must
    render image A with the built-in rasteriser (``HipRenderer``), ALL on the window route (vertex-colour meshes) or ALL on the
    full-frame route (``dataset_info['renderer'] == 'pyrenderer'``: textured .obj models, or un-textured ones with a Kd) -- one
    rasteriser mode per launch.  On the full-frame route ``last_prediction["rgbA"/"depthA"]`` hold the raw 176 x 176 crops of the
    renders, what ``Tracker.render_window`` returns there.  The MultiTracker owns one executing ``Engine`` of
    max_batch = len(trackers) (workspaces, staging).  The trackers' K, object widths and context / mesh handles are snapshotted
    HERE: unlike ``Tracker``, which reads its ``K`` and ``renderer`` on every call, a later assignment to a tracker's attributes does
    not reach a MultiTracker built before it."""

    def __init__(self, trackers, device=0):
        from .renderer import HipRenderer
        import ctypes as C
        from ._lib import Object
        trackers = list(trackers)
        if not trackers:
            raise ValueError("MultiTracker: no trackers")
        for i, t in enumerate(trackers):
            if not isinstance(t.renderer, HipRenderer):
                raise ValueError("MultiTracker: tracker %d does not render image A with the built-in rasteriser (an injected "
                                 "renderer): track it with its own on_track" % i)
            if bool(t.renderer.full_frame) != bool(trackers[0].renderer.full_frame):
                raise ValueError("MultiTracker: tracker %d renders image A on the %s route, tracker 0 on the %s route (one rasteriser "
                                 "mode per call: all window-route or all full-frame trackers)"
                                 % (i, *[("full-frame" if x.renderer.full_frame else "window") for x in (t, trackers[0])]))
            if int(t.engine.device) != int(device):
                raise ValueError("MultiTracker: tracker %d lives on device %d, not %d" % (i, t.engine.device, device))
            if not np.array_equal(np.asarray(t.K, np.float64), np.asarray(trackers[0].K, np.float64)):
                raise ValueError("MultiTracker: tracker %d has another camera matrix than tracker 0 (one camera frame per call)" % i)
        self.trackers = trackers
        self.n = len(trackers)
        self.full_frame = bool(trackers[0].renderer.full_frame)
        self.engine = Engine(device, self.n)
        self.K = np.ascontiguousarray(trackers[0].K, np.float64)
        self._dev = "cuda:%d" % device
        self._objs = (Object * self.n)(*[Object(t.engine._h.value, t.renderer._m.value, float(t.object_width)) for t in trackers])
        self._rgbA = torch.empty((self.n, 176, 176, 3), dtype=torch.uint8, device=self._dev)
        self._depthA = torch.empty((self.n, 176, 176), dtype=torch.int16, device=self._dev)
        self._C = C
        self.last_prediction = None
        self.last_recover = None     # recover(): what the last search found (dict)
        self.last_fit_ratio = None   # fit_check set: inlier_px / model_px per object of the last call ([n] array)
        self._pred_rgb = self._pred_depth = None
        # scene_check (extension): None (default) -- not one call more than before -- or tol_mm: every on_track / on_track_live is
        # followed by ONE scene call at the estimates (scene_fit below)
        self.scene_check = None
        self.scene_ids = False           # scene_check set: also keep the id image of the frame in last_prediction["ids"]
        self.last_scene_ratio = None     # scene_check set: inlier_px / visible_px per object ([n] array, NaN where nothing is visible)
        self.last_visible_share = None   # scene_check set: visible_px / model_px per object ([n] array, NaN where model_px == 0)
        self._filled = None              # scene_check on the live path: the filled frame, when the caller brought no depth_filled
        self.frame_cnt = 0

    def scene_fit(self, poses, depth, tol_mm=10, ids=False):
        """The tracked objects as ONE scene (Engine.scene_fit with this tracker's meshes, widths and camera): every object's mesh
        rendered at poses[i] inside its frame rectangle, composed through a shared depth test and scored against `depth` (numpy uint16
        [H,W]: the host entry; cuda 16-bit [H,W]: the device entry) over the pixels where it is the nearest TRACKED surface -- so an
        object behind another tracked object is "hidden" there, not "lost".  Returns the [n] records (_lib.SCENE_FIT_DTYPE), or
        (records, ids) with ids=True: the instance mask of the frame, uint8 [H,W], 0 = no tracked object, i + 1 = trackers[i].
        utils.scene_status reads the records."""
        rec, ids_img, _ = self.engine.scene_fit(self._objs, poses, depth, self.K, tol_mm=tol_mm, ids=ids)
        return (rec, ids_img) if ids else rec

    def align(self, i, poses, depth, occ_poses, occluders=None, scene_tol_mm=10, **kw):
        """Extension: align hypotheses of object i ([k,4,4]) to the depth frame AMONG the other objects.  The occluders (indices;
        default: every other object) are rendered at occ_poses ([len(occluders),4,4], in that order) and composed into a scene frame
        on the device (Engine.scene_fit(..., scene=True) on the uploaded frame, with scene_tol_mm as its tolerance); then
        Engine.align_poses(scene=...) runs on trackers[i]'s model: a facing point with a tracked surface at or in front of it is
        hidden, not paired.  depth: numpy uint16 [H,W] or a cuda 16-bit tensor.  Returns (poses [k,4,4], records [k] of
        _lib.SCENE_ALIGN_REC_DTYPE) as numpy; the further keywords are Engine.align_poses'."""
        i = int(i)
        occ = [j for j in range(self.n) if j != i] if occluders is None else [int(j) for j in occluders]
        if not 0 <= i < self.n or any(j < 0 or j >= self.n or j == i for j in occ) or not occ:
            raise ValueError("MultiTracker.align: object %d among occluders %s of %d objects" % (i, occ, self.n))
        t = self.trackers[i]
        handle = t._facing_handle(None, "MultiTracker.align")
        dep = depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(depth, dtype=np.uint16).view(np.int16)).to(self._dev)
        occ_objs = (type(self._objs[0]) * len(occ))(*[self._objs[j] for j in occ])
        _, _, scene = self.engine.scene_fit(occ_objs, occ_poses, dep, self.K, tol_mm=scene_tol_mm, scene=True)
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))).to(self._dev)
        out = t.engine.align_poses(handle, p, dep, self.K, scene=scene, scene_tol_mm=scene_tol_mm, **kw)
        from ._lib import SCENE_ALIGN_REC_DTYPE
        res = (out[0].cpu().numpy(), out[1].cpu().numpy().view(SCENE_ALIGN_REC_DTYPE).reshape(-1))
        return res + tuple(x.cpu().numpy() for x in out[2:])

    def verify(self, i, poses, rgb, depth, occ_poses, occluders=None, tol_mm=10, min_px=64):
        """Extension: which of these hypotheses of object i ([k,4,4]) does the frame confirm by colour, AMONG the other objects.
        The occluders (indices; default: every other object) are rendered at occ_poses ([len(occluders),4,4], in that order) and
        composed into a scene frame on the device (Engine.scene_fit(..., scene=True) on the uploaded depth frame, tol_mm as its
        tolerance); then trackers[i].verify(scene=...) runs: a pixel with a tracked surface at or in front of the model's is
        hidden_px and its colours are not compared.  rgb HxWx3 uint8, depth HxW uint16 mm (host arrays).  Returns (fit [k] of
        _lib.SCENE_CROP_FIT_DTYPE, color [k], score [k]) as Tracker.verify."""
        i = int(i)
        occ = [j for j in range(self.n) if j != i] if occluders is None else [int(j) for j in occluders]
        if not 0 <= i < self.n or any(j < 0 or j >= self.n or j == i for j in occ) or not occ:
            raise ValueError("MultiTracker.verify: object %d among occluders %s of %d objects" % (i, occ, self.n))
        dep = np.ascontiguousarray(depth, dtype=np.uint16)
        dep_d = torch.from_numpy(dep.view(np.int16)).to(self._dev)
        occ_objs = (type(self._objs[0]) * len(occ))(*[self._objs[j] for j in occ])
        _, _, scene = self.engine.scene_fit(occ_objs, occ_poses, dep_d, self.K, tol_mm=tol_mm, scene=True)
        return self.trackers[i].verify(poses, rgb, dep, tol_mm=tol_mm, min_px=min_px, scene=scene)

    def recover(self, prev_poses, rgb, depth, lost=None, lost_below=0.5, min_visible=0.2, trans_radius=0.05, trans_step=0.01,
                rot_deg=(15.0,), tol_mm=10, top=None, refine=1, align=0, scene_align=False, colour=False, colour_within=0.9, min_px=64):
        """Extension: re-acquire the lost objects of a frame AMONG the tracked ones.  Tracker.recover scores a candidate against the
        depth frame alone: it lays a lost model onto the visible face of a neighbour, and counts a tracked object in front of a
        candidate as an unknown obstacle.  Here the objects that are "tracked" explain their pixels (the rule of
        se3tn_score_pose_grid_scene): a point at or behind a tracked surface is hidden_pts and nothing else.
        prev_poses: [n,4,4], the poses to search around (lost objects) and to render at (occluders); rgb, depth: the frame.
        lost: a list of object indices; default: the objects utils.scene_status(last_prediction["scene_fit"], lost_below,
        min_visible) calls "lost" -- scene_check must have run (ValueError otherwise, also when `lost` is given: the occluders
        are chosen by the same records).  Occluders are the objects with status "tracked" that are not being searched, at their
        prev_poses; "occluded" and lost objects explain nothing.  With no occluder at all every lost object falls back to
        trackers[i].recover(..., facing=True) and last_recover[i]["fallback"] says so.
        Per lost object i, in index order: (1) recover.lattice_factors around prev_poses[i]; (2) ONE call,
        Engine.search_pose_grid_scene with facing=True on trackers[i]'s facing handle, whose composed scene is kept on the device;
        (3) align > 0: Engine.align_poses of the top nodes, refine >= 1: trackers[i].on_track_batch on them, as Tracker.recover
        does; (4) the pool [refined, aligned, unrefined] rescored under the scene-aware rule as the diagonal of a grid against the
        kept scene, and the largest recover.pose_key wins.  So the result never scores below the lattice's best under the scene
        rule.  The network stays scene-unaware, and so does the alignment by default; the choice is not.  scene_align=True (with
        align > 0): step (3) aligns the top nodes against the kept scene of step (2) (Engine.align_poses(scene=..., scene_tol_mm =
        tol_mm)): points hidden by a tracked object are not paired, so a neighbour's face or an object lying on the lost one no longer
        drags the hypotheses away; align_rec then has _lib.SCENE_ALIGN_REC_DTYPE (hidden_pts) and last_recover[i]["scene_align"]
        says which rule ran (False on the no-occluder fallback).  colour=True (off by default, and then not one call more is made
        and every bit is as before): after step (4) the choice goes through trackers[i]._choose_by_colour over the pool and its
        scene-rule records, against the kept scene of step (2) -- D is the depth winner, the candidates are the pool members with
        inlier_pts >= colour_within * inlier_pts[D], each verified under the scene-aware colour rule (Tracker.verify(scene=...): the
        pixels a tracked object hides or claims are not compared), the highest score wins, a tie goes to the larger depth key, and
        if every score is 0, D stays (with refine=0 and no alignment the pool is the ranked top of the lattice, as in
        Tracker.recover).  last_recover[i] then also keeps depth_chosen, color_fit, color_score and candidates; on the no-occluder
        fallback the switch is passed to trackers[i].recover.  A recovered object does NOT become an
        occluder for the next lost one within the same call: every search of a call sees the same occluders.
        Returns [n,4,4]: rows of objects that were not searched are prev_poses' rows.  last_recover: {i: dict} per searched object
        -- what Tracker.last_recover keeps (n, top_idx, top_fit, refined, final_fit, chosen, inlier_frac = inlier_pts / points;
        aligned, align_rec) plus occluders (indices), occ_fit (their scene records), hidden_pts and visible_frac = inlier_pts /
        (points - hidden_pts), NaN when that is 0."""
        from .recover import lattice_factors, pose_key
        poses = np.asarray(prev_poses, np.float64).reshape(-1, 4, 4)
        if poses.shape[0] != self.n:
            raise ValueError("MultiTracker.recover: %d poses for %d objects" % (poses.shape[0], self.n))
        rec = (self.last_prediction or {}).get("scene_fit")
        if rec is None:
            raise ValueError("MultiTracker.recover: no scene records -- set scene_check (tol_mm) and track a frame first: they say which "
                             "objects are lost and which are tracked and explain their pixels")
        status = U.scene_status(rec, lost_below, min_visible)
        lost = [i for i, s in enumerate(status) if s == "lost"] if lost is None else sorted(set(int(i) for i in lost))
        if any(i < 0 or i >= self.n for i in lost):
            raise ValueError("MultiTracker.recover: lost = %s names an object outside [0, %d)" % (lost, self.n))
        out = poses.copy()
        self.last_recover = {}
        if not lost:
            return out
        occ = [i for i, s in enumerate(status) if s == "tracked" and i not in lost]
        dep = np.ascontiguousarray(depth, dtype=np.uint16)
        if not occ:   # nothing explains anything: the single-object search
            for i in lost:
                out[i] = self.trackers[i].recover(poses[i], rgb, dep, trans_radius=trans_radius, trans_step=trans_step, rot_deg=rot_deg,
                                                  tol_mm=tol_mm, top=top, refine=refine, facing=True, align=align,
                                                  **(dict(colour=True, colour_within=colour_within) if colour else {}))
                self.last_recover[i] = dict(self.trackers[i].last_recover, occluders=[], fallback=True, scene_align=False)
            return out
        occ_objs = (type(self._objs[0]) * len(occ))(*[self._objs[j] for j in occ])
        for i in lost:
            t = self.trackers[i]
            handle = t._facing_handle(None, "MultiTracker.recover")
            k = min(8, t.engine.max_batch) if top is None else int(top)
            rots, trans = lattice_factors(poses[i], trans_radius, trans_step, rot_deg)
            top_idx, top_fit, occ_fit, scene = self.engine.search_pose_grid_scene(handle, rots, trans, dep, self.K, occ_objs, poses[occ],
                                                                                  tol_mm=tol_mm, facing=True, top=k, keep_scene=True)
            unrefined = t._compose(rots, trans, top_idx)
            info = dict(n=len(rots) * len(trans), top_idx=top_idx, top_fit=top_fit, refined=None, facing=True, occluders=list(occ),
                        occ_fit=occ_fit, fallback=False, scene_align=bool(scene_align) and int(align) > 0)
            aligned = None
            if int(align) > 0:
                if scene_align:
                    aligned, align_rec = t.engine.align_poses(handle, unrefined, dep, self.K, iters=int(align), scene=scene,
                                                              scene_tol_mm=tol_mm)
                else:
                    aligned, align_rec = t.engine.align_poses(handle, unrefined, dep, self.K, iters=int(align))
                info.update(aligned=aligned, align_rec=align_rec)
            if int(refine) < 1 and aligned is None:
                final, final_fit, chosen = unrefined, (top_fit.copy() if colour else top_fit[:1].copy()), 0   # (colour: the pool is the ranked top)
            else:
                refined = unrefined if aligned is None else aligned
                for _ in range(int(refine)):
                    refined = np.asarray(t.on_track_batch(list(refined), [rgb] * k, [dep] * k), np.float64)
                if int(refine) < 1:
                    refined = None
                final = np.concatenate(([] if refined is None else [refined]) + ([] if aligned is None else [aligned]) + [unrefined])
                m = len(final)
                grid = self.engine.score_pose_grid(handle, final[:, :3, :3], final[:, :3, 3], dep, self.K, tol_mm, facing=True, scene=scene)
                final_fit = grid[np.arange(m) * m + np.arange(m)]
                chosen = int(np.argmax(pose_key(final_fit)))   # ties prefer the earlier part of the pool: the lower index
                info.update(refined=refined)
            win = final_fit[chosen]
            shown = int(win["points"]) - int(win["hidden_pts"])
            info.update(final_fit=final_fit, chosen=chosen, inlier_frac=t._frac(win), hidden_pts=int(win["hidden_pts"]),
                        visible_frac=float(win["inlier_pts"]) / shown if shown > 0 else float("nan"))
            if colour:
                chosen = t._choose_by_colour(info, final, final_fit, rgb, dep, tol_mm, colour_within, min_px, scene=scene)
                win = final_fit[chosen]
                shown = int(win["points"]) - int(win["hidden_pts"])
                info.update(hidden_pts=int(win["hidden_pts"]), visible_frac=float(win["inlier_pts"]) / shown if shown > 0 else float("nan"))
            self.last_recover[i] = info
            out[i] = final[chosen]
        return out

    @property
    def fit_check(self):
        """None (default) | tol_mm, as Tracker.fit_check: every call also scores each object's estimate against the observed depth
        (the executing engine's se3tn_set_fit_check); last_prediction gains ``fit`` ([n] records), ``pred_rgb`` / ``pred_depth``
        ([n,176,176,3] / [n,176,176] device tensors) and last_fit_ratio is inlier_px / model_px per object."""
        return self.engine.get_fit_check()

    @fit_check.setter
    def fit_check(self, tol_mm):
        self.engine.set_fit_check(tol_mm)
        if not tol_mm:
            self.last_fit_ratio = None

    def on_track(self, prev_poses, rgb, depth, rgbA_out=None, depthA_out=None, bbox_out=None):
        """prev_poses: n 4x4 poses (object i = trackers[i]); rgb HxWx3 uint8, depth HxW millimetres: ONE camera frame.
        Returns [n,4,4] float64.  rgbA_out / depthA_out: optional device tensors uint8 [n,176,176,3] / 16-bit [n,176,176] that receive
        the images A (default: the MultiTracker's own, kept in last_prediction); bbox_out: optional host int32 [n,4,2] array that
        receives compute_bbox's corners."""
        return self._on_track(prev_poses, rgb, depth, None, rgbA_out, depthA_out, bbox_out)

    def on_track_live(self, prev_poses, color, depth_raw, bgr=False, max_depth=2.0, extrapolate=False, blur_type="bilateral",
                      depth_filled=None, rgbA_out=None, depthA_out=None, bbox_out=None):
        """predict_ros.py:38-60 for all n objects of one camera frame in ONE library call (se3tn_on_track_objects_live): color HxWx3
        uint8 in the camera's channel order (bgr=True: what CvBridge 'bgr8' delivers), depth_raw HxW uint16 millimetres WITH holes.
        The raw frame goes up once, fill_depth's chain runs once for the frame, only the crop windows' pixels are blurred and
        converted, and the filled frame never visits the host.  depth_filled (optional cuda int16/uint16 [H,W]) receives the whole
        filled frame.  Object i gets the bits ``trackers[i].on_track_live`` gives it = the bits of
        ``on_track(prev_poses, rgb, engine.fill_depth(depth_raw))``.  Return value, last_prediction and the other arguments as on_track."""
        from . import _lib
        blur = blur_type if isinstance(blur_type, int) else \
            {"bilateral": _lib.BLUR_BILATERAL, "gaussian": _lib.BLUR_GAUSSIAN}.get(blur_type, _lib.BLUR_NONE)
        order = bgr if (isinstance(bgr, int) and not isinstance(bgr, bool)) else (_lib.COLOR_BGR if bgr else _lib.COLOR_RGB)
        live = (int(order), float(max_depth), 1 if extrapolate else 0, int(blur), depth_filled)
        return self._on_track(prev_poses, color, depth_raw, live, rgbA_out, depthA_out, bbox_out)

    def _on_track(self, prev_poses, rgb, depth, live, rgbA_out, depthA_out, bbox_out):
        C = self._C
        from ._lib import check
        from .engine import _stream_ptr
        n = self.n
        poses = np.ascontiguousarray(np.asarray(prev_poses, np.float64).reshape(-1, 16))
        if poses.shape[0] != n:
            raise ValueError("MultiTracker.on_track: %d poses for %d objects" % (poses.shape[0], n))
        rgb = rgb if (type(rgb) is np.ndarray and rgb.dtype == np.uint8 and rgb.flags.c_contiguous) else np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("rgb must be HxWx3 uint8")
        dep = depth if (type(depth) is np.ndarray and depth.dtype == np.uint16 and depth.flags.c_contiguous
                        and depth.shape == rgb.shape[:2]) else _depth_u16(depth, rgb)
        rA, dA = self._rgbA, self._depthA
        if rgbA_out is not None:
            if tuple(rgbA_out.shape) != (n, 176, 176, 3) or rgbA_out.dtype != torch.uint8 or not rgbA_out.is_cuda or not rgbA_out.is_contiguous():
                raise ValueError("rgbA_out must be a contiguous device uint8 tensor [n,176,176,3]")
            rA = rgbA_out
        if depthA_out is not None:
            if tuple(depthA_out.shape) != (n, 176, 176) or depthA_out.element_size() != 2 or not depthA_out.is_cuda or not depthA_out.is_contiguous():
                raise ValueError("depthA_out must be a contiguous 16-bit device tensor [n,176,176]")
            dA = depthA_out
        bb = bbox_out if bbox_out is not None else np.empty((n, 4, 2), np.int32)
        if bb.shape != (n, 4, 2) or bb.dtype != np.int32 or not bb.flags.c_contiguous:
            raise ValueError("bbox_out must be a contiguous int32 array [n,4,2]")
        # the call runs under the trackers' offset / raster rules (the library refuses models whose rules differ from the executing ctx's)
        t0 = self.trackers[0].engine
        self.engine.set_offset_rule(t0.get_offset_rule())
        self.engine.set_raster_rule(t0.get_raster_rule())
        out = np.empty((n, 16), np.float64)
        tr, ro = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        outs = (C.c_void_p(rA.data_ptr()), C.c_void_p(dA.data_ptr()), C.c_void_p(out.ctypes.data), C.c_void_p(tr.ctypes.data),
                C.c_void_p(ro.ctypes.data), C.c_void_p(bb.ctypes.data), _stream_ptr())
        if live is None:
            check(self.engine.lib.se3tn_on_track_objects(
                self.engine._h, n, self._objs, C.c_void_p(poses.ctypes.data), self.K.ctypes.data_as(C.POINTER(C.c_double)),
                C.c_void_p(rgb.ctypes.data), C.c_void_p(dep.ctypes.data), H, W, *outs), "se3tn_on_track_objects")
        else:
            order, max_depth, extrapolate, blur, filled = live
            if filled is not None and not (filled.is_cuda and filled.element_size() == 2 and filled.is_contiguous()
                                           and tuple(filled.shape) == (H, W)):
                raise ValueError("depth_filled must be a contiguous 16-bit device tensor [H,W]")
            if filled is None and self.scene_check:   # the scene call reads the filled frame, which stays on the device
                if self._filled is None or tuple(self._filled.shape) != (H, W):
                    self._filled = torch.empty((H, W), dtype=torch.int16, device=self._dev)
                filled = self._filled
            check(self.engine.lib.se3tn_on_track_objects_live(
                self.engine._h, n, self._objs, C.c_void_p(poses.ctypes.data), self.K.ctypes.data_as(C.POINTER(C.c_double)),
                C.c_void_p(rgb.ctypes.data), order, C.c_void_p(dep.ctypes.data), H, W, C.c_double(max_depth), extrapolate, blur,
                C.c_void_p(filled.data_ptr()) if filled is not None else None, *outs), "se3tn_on_track_objects_live")
        self.last_prediction = dict(trans=tr, rot=ro, bbox=bb, rgbA=list(rA), depthA=list(dA))
        self.last_fit_ratio = None
        if self.engine.get_fit_check():
            if self._pred_rgb is None:
                self._pred_rgb = torch.empty((n, 176, 176, 3), dtype=torch.uint8, device=self._dev)
                self._pred_depth = torch.empty((n, 176, 176), dtype=torch.int16, device=self._dev)
            fit = self.engine.last_fit(n)
            self.engine.last_fit_images(n, self._pred_rgb, self._pred_depth)
            self.last_prediction.update(fit=fit, pred_rgb=self._pred_rgb, pred_depth=self._pred_depth)
            self.last_fit_ratio = U.fit_ratio(fit)
        self.last_scene_ratio = self.last_visible_share = None
        if self.scene_check:   # ONE scene call at the estimates: against the frame as given, or (live) the filled frame on the device
            rec, ids_img, _ = self.engine.scene_fit(self._objs, out, dep if live is None else filled, self.K, tol_mm=int(self.scene_check),
                                                    ids=bool(self.scene_ids))
            self.last_prediction["scene_fit"] = rec
            if self.scene_ids:
                self.last_prediction["ids"] = ids_img
            self.last_scene_ratio = U.scene_ratio(rec)
            self.last_visible_share = U.visible_share(rec)
        self.frame_cnt += 1
        return out.reshape(n, 4, 4)

    def close(self):
        self.engine.close()
