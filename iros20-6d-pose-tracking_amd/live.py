"""Live-camera front end: the reference's ``predict_ros.TrackerRos`` (predict_ros.py:19-66) without ROS.

The ROS node is transport (subscribers, tf broadcaster) around three pieces of arithmetic, kept here with the
reference's method names so that a rospy / ROS 2 / RealSense wrapper only has to forward messages:

    grab_depth(depth_mm)   uint16 mm frame -> hole-filled uint16 mm (fill_depth, predict_ros.py:38-41) -- se3tn_fill_depth
    grab_color(bgr)        BGR uint8 frame -> RGB (cv2.cvtColor(..., COLOR_BGR2RGB), :43-46)
    on_track()             Tracker.on_track on the latest pair, pose feedback (:48-60); returns what the node
                           publishes on tf: (translation [3], quaternion x,y,z,w, stamp) (:62-66)

``LiveTracker(..., one_call=True)`` with the built-in rasteriser: the two grabs only keep the camera's frames and on_track is ONE
library call (Tracker.on_track_live -> se3tn_on_track_live: fill_depth of the crop window's pixels, the BGR swap of the window and
on_track); ``depth`` is then fetched from the device when somebody reads it.

``LiveMultiTracker`` is the same surface over a ``MultiTracker``: several objects of one camera, one (trans, quaternion, stamp) per
object and frame; ``one_call=True`` makes on_track ONE library call for all of them (MultiTracker.on_track_live ->
se3tn_on_track_objects_live).
"""
import numpy as np


def quaternion_from_matrix(matrix):
    """Rotation part of a 4x4 homogeneous matrix -> unit quaternion (w, x, y, z) the way the `transformations`
    package does it by default (isprecise=False), which is what the reference calls at predict_ros.py:63: the
    eigenvector of the largest eigenvalue of the symmetric 4x4 matrix K built from the rotation (Bar-Itzhack 2000),
    sign chosen so that w >= 0.  Robust to the slightly non-orthonormal R_B the pose update produces (its Rodrigues
    factor is rounded to float32)."""
    M = np.asarray(matrix, dtype=np.float64)[:4, :4]
    m00, m01, m02 = M[0, 0], M[0, 1], M[0, 2]
    m10, m11, m12 = M[1, 0], M[1, 1], M[1, 2]
    m20, m21, m22 = M[2, 0], M[2, 1], M[2, 2]
    K = np.array([[m00 - m11 - m22, 0.0, 0.0, 0.0],
                  [m01 + m10, m11 - m00 - m22, 0.0, 0.0],
                  [m02 + m20, m12 + m21, m22 - m00 - m11, 0.0],
                  [m21 - m12, m02 - m20, m10 - m01, m00 + m11 + m22]]) / 3.0
    w, V = np.linalg.eigh(K)          # eigh reads the lower triangle
    q = V[[3, 0, 1, 2], np.argmax(w)]
    return -q if q[0] < 0.0 else q


class LiveTracker:
    """predict_ros.py:19-66 `TrackerRos` minus the ROS plumbing."""

    def __init__(self, tracker, pose_init, max_depth=2.0, extrapolate=False, blur_type="bilateral", one_call=False, recover_below=None):
        self.tracker = tracker
        self.color = None
        self._depth = None
        self.cur_time = None
        self.A_in_cam = np.asarray(pose_init, np.float64).copy()
        # recover_below (extension): None (default) -- not one call more than before -- or a fit ratio: a frame whose estimate scores
        # last_fit_ratio < recover_below is searched again (Tracker.recover around the pose the frame started from, the tracked
        # estimate among the candidates) and the recovered pose is adopted.  Needs the fit check: the ratio comes from it.
        if recover_below is not None and not tracker.fit_check:
            raise ValueError("LiveTracker: recover_below needs tracker.fit_check to be set (the fit ratio comes from it)")
        self.recover_below = recover_below
        self._fill = dict(max_depth=max_depth, extrapolate=extrapolate, blur_type=blur_type)
        from .renderer import HipRenderer
        # one library call per frame needs the built-in rasteriser (False by default: not measured on the MI355X yet)
        self.one_call = bool(one_call) and isinstance(tracker.renderer, HipRenderer)
        self._raw = None           # one_call: the camera's depth frame as it came
        self._filled_dev = None    # one_call: the filled frame of the last on_track, on the device
        self._filled_valid = False

    @property
    def fit_check(self):
        """The tracker's fit_check (None | tol_mm): with it set every on_track also scores the estimate against the observed depth;
        last_fit_ratio and tracker.last_prediction["fit" / "pred_rgb" / "pred_depth"] carry the result."""
        return self.tracker.fit_check

    @fit_check.setter
    def fit_check(self, tol_mm):
        self.tracker.fit_check = tol_mm

    @property
    def last_fit_ratio(self):
        return self.tracker.last_fit_ratio

    def reset(self, pose_init):
        self.color = None
        self._depth = None
        self._raw = None
        self._filled_valid = False
        self.cur_time = None
        self.A_in_cam = np.asarray(pose_init, np.float64).copy()

    @property
    def depth(self):
        """The hole-filled uint16 mm frame on_track reads.  one_call: fetched from the device on demand (of the last on_track; a
        frame grabbed since is filled here, off the per-frame path)."""
        if not self.one_call:
            return self._depth
        if self._raw is None:
            return None
        if self._filled_valid:
            return self._filled_dev.cpu().numpy().view(np.uint16)
        return self.tracker.engine.fill_depth(self._raw, **self._fill)

    @depth.setter
    def depth(self, value):
        self._depth = value

    def grab_depth(self, depth_mm):
        """depth_mm: HxW array in millimetres (what CvBridge 'passthrough' hands over, cast to uint16)."""
        if self.one_call:
            self._raw = np.ascontiguousarray(depth_mm, dtype=np.uint16) if np.asarray(depth_mm).dtype == np.uint16 \
                else np.asarray(depth_mm).astype(np.uint16)
            self._filled_valid = False
            return
        self._depth = self.tracker.engine.fill_depth(np.asarray(depth_mm).astype(np.uint16), **self._fill)

    def grab_color(self, bgr, stamp=0.0):
        """bgr: HxWx3 uint8 as CvBridge 'bgr8' delivers it; stored as RGB (one_call: kept as it came, swapped inside the call)."""
        self.cur_time = stamp
        self.color = np.ascontiguousarray(bgr, dtype=np.uint8) if self.one_call else np.ascontiguousarray(np.asarray(bgr)[:, :, ::-1])

    def _on_track_one_call(self):
        import torch
        if self._filled_dev is None or tuple(self._filled_dev.shape) != self._raw.shape:
            self._filled_dev = torch.empty(self._raw.shape, dtype=torch.int16, device="cuda:%d" % self.tracker.engine.device)
        self._filled_valid = False
        pose = self.tracker.on_track_live(self.A_in_cam, self.color, self._raw, bgr=True, depth_filled=self._filled_dev, **self._fill)
        self._filled_valid = True
        return pose

    def on_track(self):
        if self.color is None or (self._raw if self.one_call else self._depth) is None or self.cur_time is None:
            return None
        if self.one_call:
            ob_in_cam = self._on_track_one_call()
        else:
            ob_in_cam = self.tracker.on_track(self.A_in_cam, self.color.astype(np.uint8), self._depth,
                                              gt_A_in_cam=np.eye(4), gt_B_in_cam=np.eye(4), debug=False, samples=1)
        if self.recover_below is not None and self.tracker.last_fit_ratio is not None and self.tracker.last_fit_ratio < self.recover_below:
            # lost: search around the pose this frame started from; only here is the filled frame fetched on the one-call route
            rgb = np.ascontiguousarray(self.color[:, :, ::-1]) if self.one_call else self.color.astype(np.uint8)
            ob_in_cam = self.tracker.recover(self.A_in_cam, rgb, self.depth, extra=[ob_in_cam])
        self.A_in_cam = ob_in_cam.copy()
        trans = ob_in_cam[:3, 3]
        q_wxyz = quaternion_from_matrix(ob_in_cam)
        q_xyzw = [q_wxyz[1], q_wxyz[2], q_wxyz[3], q_wxyz[0]]
        return trans, q_xyzw, self.cur_time


class LiveMultiTracker:
    """`TrackerRos` for several objects seen by one camera: a ``MultiTracker`` instead of a ``Tracker``, n poses instead of one.
    The surface of ``LiveTracker``; on_track() returns a list of n (translation [3], quaternion x,y,z,w, stamp) and feeds the n
    poses back.  one_call=False composes engine.fill_depth + the channel swap + MultiTracker.on_track; one_call=True is ONE library
    call per frame (opt-in, as LiveTracker's; measured in profiles/EXPERIMENTS.md item 73).
    recover_lost: None (default; then not one call more is made) or a dict of utils.scene_status thresholds (lost_below,
    min_visible; further keys are MultiTracker.recover's keywords, align and scene_align among them, and "colour": True -- with colour_within / min_px -- for
    the scene-aware colour choice among the depth-equal hypotheses, which reads the frame's RGB image): after each frame the objects the scene records call "lost" go
    through MultiTracker.recover around the poses the frame started from, and the poses it finds are adopted.  Needs scene_check."""

    def __init__(self, multi_tracker, poses_init, max_depth=2.0, extrapolate=False, blur_type="bilateral", one_call=False,
                 recover_lost=None):
        self.tracker = multi_tracker
        self.recover_lost = None if recover_lost is None else dict(recover_lost)
        self.color = None
        self._depth = None
        self.cur_time = None
        self.A_in_cam = self._poses(poses_init)
        self._fill = dict(max_depth=max_depth, extrapolate=extrapolate, blur_type=blur_type)
        self.one_call = bool(one_call)
        self._raw = None           # one_call: the camera's depth frame as it came
        self._filled_dev = None    # one_call: the filled frame of the last on_track, on the device
        self._filled_valid = False

    def _poses(self, poses):
        p = np.asarray(poses, np.float64).reshape(-1, 4, 4).copy()
        if p.shape[0] != self.tracker.n:
            raise ValueError("LiveMultiTracker: %d poses for %d objects" % (p.shape[0], self.tracker.n))
        return p

    @property
    def fit_check(self):
        """The tracker's fit_check (None | tol_mm): with it set every on_track also scores the estimate against the observed depth;
        last_fit_ratio and tracker.last_prediction["fit" / "pred_rgb" / "pred_depth"] carry the result."""
        return self.tracker.fit_check

    @fit_check.setter
    def fit_check(self, tol_mm):
        self.tracker.fit_check = tol_mm

    @property
    def last_fit_ratio(self):
        return self.tracker.last_fit_ratio

    @property
    def scene_check(self):
        """The tracker's scene_check (None | tol_mm): with it set every on_track is followed by one scene call at the estimates, in
        which the tracked objects explain each other's occlusions; tracker.last_prediction["scene_fit"], last_scene_ratio and
        scene_status() carry the result.  (Acting on "lost": recover_lost, or MultiTracker.recover.)"""
        return self.tracker.scene_check

    @scene_check.setter
    def scene_check(self, tol_mm):
        self.tracker.scene_check = tol_mm

    @property
    def last_scene_ratio(self):
        return self.tracker.last_scene_ratio

    def scene_status(self, lost_below=0.5, min_visible=0.2):
        """"tracked" | "lost" | "occluded" per object from the last on_track's scene records (utils.scene_status); None when
        scene_check is off or no frame has been tracked."""
        from . import utils as U
        rec = (self.tracker.last_prediction or {}).get("scene_fit") if self.tracker.scene_check else None
        return None if rec is None else U.scene_status(rec, lost_below, min_visible)

    def reset(self, poses_init):
        self.color = None
        self._depth = None
        self._raw = None
        self._filled_valid = False
        self.cur_time = None
        self.A_in_cam = self._poses(poses_init)

    @property
    def depth(self):
        """The hole-filled uint16 mm frame on_track reads.  one_call: fetched from the device on demand (of the last on_track; a
        frame grabbed since is filled here, off the per-frame path)."""
        if not self.one_call:
            return self._depth
        if self._raw is None:
            return None
        if self._filled_valid:
            return self._filled_dev.cpu().numpy().view(np.uint16)
        return self.tracker.engine.fill_depth(self._raw, **self._fill)

    @depth.setter
    def depth(self, value):
        self._depth = value

    def grab_depth(self, depth_mm):
        """depth_mm: HxW array in millimetres (what CvBridge 'passthrough' hands over, cast to uint16)."""
        if self.one_call:
            self._raw = np.ascontiguousarray(np.asarray(depth_mm).astype(np.uint16, copy=False))
            self._filled_valid = False
            return
        self._depth = self.tracker.engine.fill_depth(np.asarray(depth_mm).astype(np.uint16), **self._fill)

    def grab_color(self, bgr, stamp=0.0):
        """bgr: HxWx3 uint8 as CvBridge 'bgr8' delivers it; stored as RGB (one_call: kept as it came, swapped inside the call)."""
        self.cur_time = stamp
        self.color = np.ascontiguousarray(bgr, dtype=np.uint8) if self.one_call else np.ascontiguousarray(np.asarray(bgr)[:, :, ::-1])

    def _on_track_one_call(self):
        import torch
        if self._filled_dev is None or tuple(self._filled_dev.shape) != self._raw.shape:
            self._filled_dev = torch.empty(self._raw.shape, dtype=torch.int16, device="cuda:%d" % self.tracker.engine.device)
        self._filled_valid = False
        poses = self.tracker.on_track_live(self.A_in_cam, self.color, self._raw, bgr=True, depth_filled=self._filled_dev, **self._fill)
        self._filled_valid = True
        return poses

    def _recover_lost(self, obs_in_cam):
        """recover_lost: the objects of this frame the scene records call "lost" searched among the tracked ones.  The lost objects
        are searched around the poses the frame started from, the occluders stand at this frame's estimates."""
        if not self.tracker.scene_check:
            raise ValueError("LiveMultiTracker: recover_lost needs scene_check (the scene records say which objects are lost)")
        kw = dict(self.recover_lost)
        status = self.scene_status(kw.get("lost_below", 0.5), kw.get("min_visible", 0.2))
        lost = [i for i, s in enumerate(status) if s == "lost"]
        if not lost:
            return obs_in_cam
        around = np.asarray(obs_in_cam, np.float64).copy()
        around[lost] = self.A_in_cam[lost]
        rgb = np.ascontiguousarray(self.color[:, :, ::-1]) if self.one_call else self.color.astype(np.uint8)
        return self.tracker.recover(around, rgb, self.depth, lost=lost, **kw)

    def on_track(self):
        if self.color is None or (self._raw if self.one_call else self._depth) is None or self.cur_time is None:
            return None
        if self.one_call:
            obs_in_cam = self._on_track_one_call()
        else:
            obs_in_cam = self.tracker.on_track(self.A_in_cam, self.color.astype(np.uint8), self._depth)
        if self.recover_lost is not None:
            obs_in_cam = self._recover_lost(obs_in_cam)
        self.A_in_cam = obs_in_cam.copy()
        out = []
        for ob_in_cam in obs_in_cam:
            q_wxyz = quaternion_from_matrix(ob_in_cam)
            out.append((ob_in_cam[:3, 3], [q_wxyz[1], q_wxyz[2], q_wxyz[3], q_wxyz[0]], self.cur_time))
        return out
