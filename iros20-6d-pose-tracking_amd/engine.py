"""Thin Python owner of one se3tn context (one per process / GPU).  PyTorch is used only for
device memory, streams and (in dist.py) torch.distributed -- all arithmetic is in the HIP library."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ALIGN_REC_DTYPE, SCENE_ALIGN_REC_DTYPE, SCENE_CROP_FIT_DTYPE, COLOR_FIT_DTYPE, CROP_DTYPE, FIT_DTYPE, POINT_FIT_DTYPE, SCENE_FIT_DTYPE, SCENE_POINT_FIT_DTYPE, NCHW, NHWC, RES, Crop, Se3tnError, check


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack_crops(rgb, depth, windows, z_offset_mm, stats):
    """Vectorised se3tn_crop descriptors for a batch of frames that live in ONE tensor each:
    rgb cuda u8 [n,H,W,3], depth cuda 2-byte [n,H,W], windows int [n,4] (left,top,right,bottom),
    z_offset_mm float [n], stats 0|1.  Returns a numpy record array accepted by Engine.preprocess."""
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.dim() == 4 and rgb.shape[3] == 3
    assert depth.is_cuda and depth.element_size() == 2 and depth.is_contiguous() and depth.shape == rgb.shape[:3]
    n, H, W = int(rgb.shape[0]), int(rgb.shape[1]), int(rgb.shape[2])
    rec = np.zeros(n, dtype=CROP_DTYPE)
    idx = np.arange(n, dtype=np.uint64)
    rec["rgb"] = np.uint64(rgb.data_ptr()) + idx * np.uint64(H * W * 3)
    rec["depth"] = np.uint64(depth.data_ptr()) + idx * np.uint64(H * W * 2)
    rec["H"] = H; rec["W"] = W
    win = np.asarray(windows, dtype=np.int64).reshape(n, 4)
    rec["left"], rec["top"], rec["right"], rec["bottom"] = win[:, 0], win[:, 1], win[:, 2], win[:, 3]
    rec["z_offset_mm"] = np.asarray(z_offset_mm, dtype=np.float64)
    rec["stats"] = int(stats)
    return rec


class ModelPoints:
    """se3tn_points: the model points of Engine.pose_errors on the device (uploaded once) with the scratch of one chunk of pairs.
    ``points`` keeps the host copy (float64 [P,3]), so the handle also serves the CPU evaluators of metrics.py.  ``normals``
    (optional float64 [P,3], one per point, any length) are what Engine.score_pose_grid(facing=True) reads
    (se3tn_points_set_normals); ``.normals`` keeps the host copy, or None."""

    def __init__(self, engine, pts, normals=None):
        self.points = np.ascontiguousarray(np.asarray(pts.points if hasattr(pts, "points") else pts, np.float64).reshape(-1, 3))
        self.normals = None
        self.engine = engine
        self._h = None
        h = C.c_void_p()
        check(engine.lib.se3tn_points_create(engine._h, C.c_void_p(self.points.ctypes.data), int(self.points.shape[0]), C.byref(h)),
              "se3tn_points_create")
        self._h = h
        if normals is not None:
            nrm = np.ascontiguousarray(np.asarray(normals, np.float64).reshape(-1, 3))
            if nrm.shape != self.points.shape:
                self.close()
                raise ValueError("ModelPoints: %d normals for %d points" % (nrm.shape[0], self.points.shape[0]))
            rc = engine.lib.se3tn_points_set_normals(self._h, C.c_void_p(nrm.ctypes.data))
            if rc != 0:
                self.close()
                check(rc, "se3tn_points_set_normals")
            self.normals = nrm

    def __len__(self):
        return int(self.points.shape[0])

    def close(self):
        if getattr(self, "_h", None):
            self.engine.lib.se3tn_points_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    def __init__(self, device=0, max_batch=64):
        self.lib = _lib.load()
        self.device = int(device)
        self.max_batch = int(max_batch)
        h = C.c_void_p()
        check(self.lib.se3tn_create(self.device, self.max_batch, C.byref(h)), "se3tn_create")
        self._h = h
        self._blob = None  # keeps a bound (caller-owned) weight blob alive
        self.has_weights = False
        self._fit_tol = None   # what set_fit_check last set (the per-frame paths read this, not the library)
        if self.device >= 0:
            torch.cuda.set_device(self.device)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.se3tn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, H, W):
        """Start-up reservation (se3tn_reserve): z-buffer / fill_depth scratch for H x W camera frames and the planes of the
        selected modes, so that no stream-ordered call allocates later (hipGraph capture, latency of the first frame)."""
        check(self.lib.se3tn_reserve(self._h, int(H), int(W)), "se3tn_reserve")

    def split_weights_device(self):
        """f16x3 mode: copy of the device-derived split panels as a CPU uint8 tensor (tests)."""
        n = int(self.lib.se3tn_split_weights_bytes(self._h))
        ptr = self.lib.se3tn_split_weights_device(self._h)
        if not ptr:
            raise Se3tnError("split panels not derived: select PREC_F16X3 with weights bound")
        out = torch.empty(n, dtype=torch.uint8, device="cuda:%d" % self.device)
        check(self.lib.se3tn_memcpy_d2d(C.c_void_p(out.data_ptr()), C.c_void_p(ptr), n, _stream_ptr()), "se3tn_memcpy_d2d")
        return out.cpu()

    def split_weights_host(self, packed_blob):
        """The host statement of the same derivation applied to a packed blob (CPU uint8 tensor)."""
        n = int(self.lib.se3tn_split_weights_bytes(self._h))
        blob = packed_blob.contiguous()
        out = torch.empty(n, dtype=torch.uint8)
        check(self.lib.se3tn_split_weights_host(C.c_void_p(blob.data_ptr()), blob.numel(), C.c_void_p(out.data_ptr()), n),
              "se3tn_split_weights_host")
        return out

    # ---- weights ---------------------------------------------------------------------------
    def pack_state_dict(self, state_dict):
        """Hand the reference checkpoint's state_dict (predict.py:151-156) to the library:
        BN folding + packing happen in C++.  Returns the packed blob as a CPU uint8 tensor."""
        n = 0
        for key, t in state_dict.items():
            if t.dtype != torch.float32:
                if key.endswith("num_batches_tracked"):
                    continue
                raise Se3tnError("state_dict[%s]: expected float32, got %s" % (key, t.dtype))
            t = t.detach().cpu().contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            check(self.lib.se3tn_set_tensor(self._h, key.encode(), C.c_void_p(t.data_ptr()), shape, t.dim()),
                  "se3tn_set_tensor(%s)" % key)
            n += 1
        check(self.lib.se3tn_pack_weights(self._h), "se3tn_pack_weights")
        nbytes = self.lib.se3tn_packed_bytes(self._h)
        host = self.lib.se3tn_packed_host(self._h)
        buf = (C.c_uint8 * nbytes).from_address(host)
        return torch.frombuffer(buf, dtype=torch.uint8).clone()

    def load_state_dict(self, state_dict):
        self.pack_state_dict(state_dict)
        check(self.lib.se3tn_upload_weights(self._h, _stream_ptr()), "se3tn_upload_weights")
        self.has_weights = True

    def packed_bytes(self):
        return int(self.lib.se3tn_packed_bytes(self._h))

    def bind_blob(self, blob_cuda):
        """Use a caller-owned CUDA uint8 tensor holding the packed blob (e.g. received through
        an RCCL broadcast)."""
        assert blob_cuda.is_cuda and blob_cuda.dtype == torch.uint8 and blob_cuda.is_contiguous()
        torch.cuda.current_stream().synchronize()
        check(self.lib.se3tn_bind_weights(self._h, C.c_void_p(blob_cuda.data_ptr()), blob_cuda.numel()),
              "se3tn_bind_weights")
        self._blob = blob_cuda
        self.has_weights = True

    # ---- constants -------------------------------------------------------------------------
    def set_normalization(self, mean, std):
        m = (C.c_double * 8)(*[float(x) for x in np.asarray(mean).reshape(8)])
        s = (C.c_double * 8)(*[float(x) for x in np.asarray(std).reshape(8)])
        check(self.lib.se3tn_set_normalization(self._h, m, s), "se3tn_set_normalization")

    def enable_graphs(self, on=True):
        """hipGraph replay of repeated se3tn_infer calls (needs a non-default stream)."""
        check(self.lib.se3tn_enable_graphs(self._h, 1 if on else 0), "se3tn_enable_graphs")

    def set_precision(self, mode):
        """_lib.PREC_F32 (default, exact) or _lib.PREC_F16X3 (split-f16 MFMA for the deep layers, n >= 32)."""
        check(self.lib.se3tn_set_precision(self._h, int(mode)), "se3tn_set_precision")

    def set_offset_rule(self, rule):
        """Rounding of OffsetDepth's `depth -= pose[2,3]*1000`: "numpy1" | _lib.OFFSET_RULE_NUMPY1 (default: one float32 operation, what
        every NumPy the reference runs on does) or "numpy2" | _lib.OFFSET_RULE_NUMPY2 (float64, rounded once)."""
        rule = {"numpy1": _lib.OFFSET_RULE_NUMPY1, "numpy2": _lib.OFFSET_RULE_NUMPY2}.get(rule, rule)
        check(self.lib.se3tn_set_offset_rule(self._h, int(rule)), "se3tn_set_offset_rule")

    def get_offset_rule(self):
        return "numpy2" if self.lib.se3tn_get_offset_rule(self._h) == _lib.OFFSET_RULE_NUMPY2 else "numpy1"

    def set_small_kernels(self, on=True):
        """Batches of 1-5 pairs through the batch-1 kernel family (conv64_small, conv_slices_small; the small-tile stem + pool at 1-2
        pairs) -- the default -- or through the general kernels (False): include/se3tracknet.h, se3tn_set_small_kernels."""
        check(self.lib.se3tn_set_small_kernels(self._h, 1 if on else 0), "se3tn_set_small_kernels")

    def get_small_kernels(self):
        return bool(self.lib.se3tn_get_small_kernels(self._h))

    def set_raster_rule(self, sub_bits):
        """Sub-pixel bits of the rasteriser's window coordinates: 4 (default: the software GL the goldens were rendered on, = the GL
        minimum) or 8 (what desktop GPUs report for GL_SUBPIXEL_BITS).  include/se3tracknet.h: se3tn_set_raster_rule."""
        check(self.lib.se3tn_set_raster_rule(self._h, int(sub_bits)), "se3tn_set_raster_rule")

    def get_raster_rule(self):
        return int(self.lib.se3tn_get_raster_rule(self._h))

    def set_winograd(self, min_batch, tile=0):
        """Batches of n >= min_batch run the 256/512-channel residual blocks as Winograd F(tile x tile,3x3) launch sequences (float32;
        tile 2 | 4 | 6 | _lib.WINOGRAD_TILE_6_4 = 6 for the 256-channel block + 4 for the heads | _lib.WINOGRAD_TILE_AUTO = 4 below 14
        pairs, from there 6 for the 256-channel block and -- while rot_normalizer <= 0.2 rad -- for the heads; 0 = keep the tile);
        min_batch 0 = always the direct kernels.  Defaults: SE3TN_WINOGRAD_DEFAULT_MIN_BATCH / _TILE of include/se3tracknet.h."""
        check(self.lib.se3tn_set_winograd(self._h, int(min_batch), int(tile)), "se3tn_set_winograd")

    def set_trunk_winograd(self, min_batch, min_fill_percent=None):
        """Launches of the 64-channel trunk at n >= min_batch take the fused Winograd F(2x2,3x3) kernel when their workgroups fill
        whole rounds of the CUs to >= min_fill_percent (None = SE3TN_TRUNK_WINOGRAD_DEFAULT_MIN_FILL, 0 = every such launch);
        min_batch 0 = always the direct kernels."""
        fill = _lib.TRUNK_WINOGRAD_DEFAULT_MIN_FILL if min_fill_percent is None else int(min_fill_percent)
        check(self.lib.se3tn_set_trunk_winograd(self._h, int(min_batch), fill), "se3tn_set_trunk_winograd")

    def get_trunk_winograd(self):
        """(min_batch, min_fill_percent) currently in force."""
        mb, fp = C.c_int(), C.c_int()
        check(self.lib.se3tn_get_trunk_winograd(self._h, C.byref(mb), C.byref(fp)), "se3tn_get_trunk_winograd")
        return mb.value, fp.value

    def get_winograd(self):
        """(min_batch, tile) currently in force."""
        mb, t = C.c_int(), C.c_int()
        check(self.lib.se3tn_get_winograd(self._h, C.byref(mb), C.byref(t)), "se3tn_get_winograd")
        return mb.value, t.value

    def keep_intermediates(self, on=True):
        """Make the fused Winograd blocks also store the activations they otherwise keep on chip ("ab_t", "head_t",
        "head" of debug_buffer); results are bit-identical either way -- except at 1-5 pairs, where the stem and the tail then take the
        general kernels that write "stem" / "head" (same tolerances, another summation order)."""
        check(self.lib.se3tn_keep_intermediates(self._h, 1 if on else 0), "se3tn_keep_intermediates")

    def overflow(self):
        """True if a split-row store left the f16 range since the last call (synchronises)."""
        f = C.c_int(0)
        check(self.lib.se3tn_overflow(self._h, C.byref(f)), "se3tn_overflow")
        return bool(f.value)

    def set_normalizers(self, trans_normalizer, rot_normalizer):
        check(self.lib.se3tn_set_normalizers(self._h, float(trans_normalizer), float(rot_normalizer)),
              "se3tn_set_normalizers")

    # ---- compute ---------------------------------------------------------------------------
    def input_buffer_ptr(self, which):
        return self.lib.se3tn_input_buffer(self._h, which)

    def preprocess(self, crops, out):
        """crops: list of dict(rgb=cuda u8 [H,W,3], depth=cuda u16-as-int16/uint16 [H,W],
        window=(left,top,right,bottom), z_offset_mm=float, stats=0|1), or the packed descriptor array
        returned by pack_crops() (no per-crop Python work).
        out: cuda float32 tensor [n,176,176,4] or a raw device pointer (int)."""
        if isinstance(crops, np.ndarray):
            assert crops.dtype == CROP_DTYPE and crops.flags.c_contiguous
            n = crops.shape[0]
            arr = crops.ctypes.data_as(C.POINTER(Crop))
        else:
            n = len(crops)
            arr = (Crop * n)()
            for i, c in enumerate(crops):
                rgb, depth = c["rgb"], c["depth"]
                assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.shape[2] == 3
                assert depth.is_cuda and depth.element_size() == 2 and depth.is_contiguous()
                arr[i].rgb = rgb.data_ptr(); arr[i].depth = depth.data_ptr()
                arr[i].H, arr[i].W = int(rgb.shape[0]), int(rgb.shape[1])
                arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = [int(v) for v in c["window"]]
                arr[i].z_offset_mm = float(c["z_offset_mm"])
                arr[i].stats = int(c["stats"])
        ptr = out.data_ptr() if torch.is_tensor(out) else int(out)
        check(self.lib.se3tn_preprocess(self._h, arr, n, C.c_void_p(ptr), _stream_ptr()), "se3tn_preprocess")

    def crop_raw(self, rgb, depth, window, device=False):
        """crop_bbox (Utils.py:320-359) alone: numpy rgb u8 [H,W,3] + depth u16 [H,W], window (left, top, right,
        bottom) -> numpy (rgb u8 [176,176,3], depth u16 [176,176]); device=True: the device tensors (uint8, uint16-as-int16)."""
        dev = "cuda:%d" % self.device
        rgb_d = rgb if torch.is_tensor(rgb) else torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8)).to(dev)
        dep_d = depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(depth, dtype=np.uint16).view(np.int16)).to(dev)
        assert rgb_d.is_cuda and dep_d.is_cuda and rgb_d.dtype == torch.uint8 and dep_d.element_size() == 2
        assert rgb_d.dim() == 3 and rgb_d.shape[2] == 3 and tuple(dep_d.shape) == tuple(rgb_d.shape[:2])
        c = Crop()
        c.rgb = rgb_d.data_ptr(); c.depth = dep_d.data_ptr()
        c.H, c.W = int(rgb_d.shape[0]), int(rgb_d.shape[1])
        c.left, c.top, c.right, c.bottom = [int(v) for v in window]
        out_rgb = torch.empty((RES, RES, 3), dtype=torch.uint8, device=dev)
        out_d = torch.empty((RES, RES), dtype=torch.int16, device=dev)
        check(self.lib.se3tn_crop_raw(self._h, C.byref(c), C.c_void_p(out_rgb.data_ptr()), C.c_void_p(out_d.data_ptr()),
                                      _stream_ptr()), "se3tn_crop_raw")
        if device:
            return out_rgb, out_d
        return out_rgb.cpu().numpy(), out_d.cpu().numpy().view(np.uint16)

    # ---- how well an estimate fits the observed depth -------------------------------------------
    def fit_stats(self, model, observed, tol_mm):
        """se3tn_fit_stats: model / observed = n descriptors each, dict(depth=cuda 16-bit [H,W], window=(left, top, right, bottom))
        (the crop window in that image, as preprocess takes it) or 176 x 176 device depth images (window = the whole image).
        Returns the n records as a structured array (_lib.FIT_DTYPE: model_px, seen_px, inlier_px, front_px, behind_px, sum_abs_mm,
        tol_mm); synchronises on the current stream."""
        n = len(model)
        if len(observed) != n:
            raise ValueError("fit_stats: %d model and %d observed descriptors" % (n, len(observed)))
        arrs = []
        for group in (model, observed):
            arr = (Crop * max(n, 1))()
            for i, c in enumerate(group):
                if torch.is_tensor(c):
                    c = dict(depth=c, window=(0, 0, int(c.shape[1]), int(c.shape[0])))
                depth = c["depth"]
                assert depth.is_cuda and depth.element_size() == 2 and depth.is_contiguous() and depth.dim() == 2
                arr[i].rgb = None; arr[i].depth = depth.data_ptr()
                arr[i].H, arr[i].W = int(depth.shape[0]), int(depth.shape[1])
                arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = [int(v) for v in c["window"]]
            arrs.append(arr)
        out = torch.empty((max(n, 1), 32), dtype=torch.uint8, device="cuda:%d" % self.device)
        check(self.lib.se3tn_fit_stats(self._h, arrs[0], arrs[1], n, int(tol_mm), C.c_void_p(out.data_ptr()), _stream_ptr()),
              "se3tn_fit_stats")
        return out.cpu().numpy().reshape(-1).view(FIT_DTYPE)[:n].copy()

    # ---- how well a hypothesis fits the observed colour ------------------------------------------
    def color_stats(self, model, observed, tol_mm, out=None, scene=None):
        """se3tn_color_stats: model / observed = n descriptors each, dict(rgb=cuda uint8 [H,W,3], depth=cuda 16-bit [H,W],
        window=(left, top, right, bottom)); window defaults to the whole image.  ONE pass gives both records: returns (fit, color),
        structured arrays of n records (_lib.FIT_DTYPE as fit_stats, _lib.COLOR_FIT_DTYPE: px, tol_mm, sum_m, sum_o, sum_mm, sum_oo,
        sum_mo, sum_abs with three words each); synchronises on the current stream.  out: a cuda uint8 [>= n,112] tensor -- the call
        is then only enqueued (capturable) and returns None; row-wise the first n * 32 bytes are the fit records, the n * 80 behind
        them the colour records (color_records reads them).
        scene: n more descriptors, as the observed ones but with depth alone, dict(depth=cuda 16-bit [H,W], window=...) -- the composed
        depth of the tracked objects under the window that shows the frame positions the observed crop shows
        (se3tn_color_stats_scene, the rule: utils.fit_stats(scene=)): pixels hidden by a tracked surface are counted as hidden_px and
        not compared; fit is then _lib.SCENE_CROP_FIT_DTYPE (color_records(..., scene=True) reads it so)."""
        n = len(model)
        if len(observed) != n:
            raise ValueError("color_stats: %d model and %d observed descriptors" % (n, len(observed)))
        if scene is not None and len(scene) != n:
            raise ValueError("color_stats: %d scene descriptors for %d pairs" % (len(scene), n))
        arrs = []
        for group in (model, observed):
            arr = (Crop * max(n, 1))()
            for i, c in enumerate(group):
                rgb, depth = c["rgb"], c["depth"]
                assert depth.is_cuda and depth.element_size() == 2 and depth.is_contiguous() and depth.dim() == 2
                assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.is_contiguous() and tuple(rgb.shape) == tuple(depth.shape) + (3,)
                arr[i].rgb = rgb.data_ptr(); arr[i].depth = depth.data_ptr()
                arr[i].H, arr[i].W = int(depth.shape[0]), int(depth.shape[1])
                win = c.get("window") or (0, 0, int(depth.shape[1]), int(depth.shape[0]))
                arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = [int(v) for v in win]
            arrs.append(arr)
        buf = out if out is not None else torch.empty((max(n, 1), 112), dtype=torch.uint8, device="cuda:%d" % self.device)
        assert buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous() and buf.numel() >= 112 * n
        if scene is None:
            check(self.lib.se3tn_color_stats(self._h, arrs[0], arrs[1], n, int(tol_mm), C.c_void_p(buf.data_ptr()),
                                             C.c_void_p(buf.data_ptr() + 32 * n), _stream_ptr()), "se3tn_color_stats")
            return None if out is not None else self.color_records(buf, n)
        arr = (Crop * max(n, 1))()
        for i, c in enumerate(scene):
            if torch.is_tensor(c):
                c = dict(depth=c)
            depth = c["depth"]
            assert depth.is_cuda and depth.element_size() == 2 and depth.is_contiguous() and depth.dim() == 2
            arr[i].rgb = None; arr[i].depth = depth.data_ptr()
            arr[i].H, arr[i].W = int(depth.shape[0]), int(depth.shape[1])
            win = c.get("window") or (0, 0, int(depth.shape[1]), int(depth.shape[0]))
            arr[i].left, arr[i].top, arr[i].right, arr[i].bottom = [int(v) for v in win]
        check(self.lib.se3tn_color_stats_scene(self._h, arrs[0], arrs[1], arr, n, int(tol_mm), C.c_void_p(buf.data_ptr()),
                                               C.c_void_p(buf.data_ptr() + 32 * n), _stream_ptr()), "se3tn_color_stats_scene")
        return None if out is not None else self.color_records(buf, n, scene=True)

    @staticmethod
    def color_records(buf, n, scene=False):
        """(fit, color) of the n pairs a color_stats(..., out=buf) call left in buf (scene=True: the call had a scene, fit reads as
        _lib.SCENE_CROP_FIT_DTYPE)"""
        host = buf.cpu().numpy().reshape(-1)
        return host[:32 * n].view(SCENE_CROP_FIT_DTYPE if scene else FIT_DTYPE).copy(), host[32 * n:112 * n].view(COLOR_FIT_DTYPE).copy()

    def verify_poses(self, mesh, poses, rgb, depth, K, object_width_mm, tol_mm=10, scene=None):
        """se3tn_verify_poses_host: "which of these n hypotheses does the frame confirm" in ONE call -- per pose its compute_bbox
        window, its own image A (the renderer of `mesh`: a HipRenderer or its se3tn_mesh handle) and the depth and colour records of
        that render against the frame's window.  poses [n,4,4]; rgb HxWx3 uint8, depth HxW uint16 mm (host arrays); K 3x3.
        Returns (fit [n], color [n], bbox [n,4,2]).  Synchronous on the default stream: refused (Se3tnError, rc = SE3TN_E_STATE) while
        the current stream is being captured -- here, since the library sees a capture only where the default stream takes part in it
        (a blocking stream), and torch captures on non-blocking ones.
        scene: the composed depth of the tracked objects of the frame, a cuda 16-bit [H,W] tensor (what scene_fit(..., scene=True) or
        search_pose_grid_scene(..., keep_scene=True) return; torch's current stream is waited for before the call, which runs on the
        default stream) or a host uint16 [H,W] array, which is uploaded -- se3tn_verify_poses_scene_host: pixels hidden by a tracked
        surface are hidden_px and not compared, fit is _lib.SCENE_CROP_FIT_DTYPE."""
        if torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing():
            raise Se3tnError("se3tn_verify_poses_host refused (rc=-2): the call is synchronous, it cannot be captured")
        p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        n = len(p)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        dep = np.ascontiguousarray(depth, dtype=np.uint16)
        if rgb.ndim != 3 or rgb.shape[2] != 3 or dep.shape != rgb.shape[:2]:
            raise ValueError("verify_poses: rgb must be HxWx3 uint8 and depth HxW")
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        fit_dtype = FIT_DTYPE if scene is None else SCENE_CROP_FIT_DTYPE
        fit, col, bb = np.zeros(max(n, 1), fit_dtype), np.zeros(max(n, 1), COLOR_FIT_DTYPE), np.zeros((max(n, 1), 4, 2), np.int32)
        front = (self._h, getattr(mesh, "_m", mesh), C.c_void_p(p.ctypes.data), n, Kc.ctypes.data_as(C.POINTER(C.c_double)),
                 C.c_double(float(object_width_mm)), C.c_void_p(rgb.ctypes.data), C.c_void_p(dep.ctypes.data))
        back = (int(rgb.shape[0]), int(rgb.shape[1]), int(tol_mm), C.c_void_p(fit.ctypes.data), C.c_void_p(col.ctypes.data),
                C.c_void_p(bb.ctypes.data))
        if scene is None:
            check(self.lib.se3tn_verify_poses_host(*front, *back), "se3tn_verify_poses_host")
        else:
            if torch.is_tensor(scene):
                sc = scene
                if not (sc.is_cuda and sc.element_size() == 2 and sc.is_contiguous() and tuple(sc.shape) == dep.shape):
                    raise ValueError("verify_poses: scene must be a contiguous cuda 16-bit tensor of the frame's shape")
                torch.cuda.current_stream(sc.device).synchronize()   # the scene is complete before the default stream reads it
            else:
                host = np.ascontiguousarray(scene, dtype=np.uint16)
                if host.shape != dep.shape:
                    raise ValueError("verify_poses: scene must have the frame's shape")
                sc = torch.from_numpy(host.view(np.int16) if host.flags.writeable else host.view(np.int16).copy()).to("cuda:%d" % self.device)
                torch.cuda.current_stream(sc.device).synchronize()
            check(self.lib.se3tn_verify_poses_scene_host(*front, C.c_void_p(sc.data_ptr()), *back), "se3tn_verify_poses_scene_host")
        return fit[:n], col[:n], bb[:n]

    def set_fit_check(self, tol_mm):
        """se3tn_set_fit_check: every one-call tracking call this engine executes also scores its estimates against the observed
        depth with this tolerance in millimetres (None / 0: off, the default)."""
        check(self.lib.se3tn_set_fit_check(self._h, int(tol_mm or 0)), "se3tn_set_fit_check")
        self._fit_tol = int(tol_mm) if tol_mm else None

    def get_fit_check(self):
        """The tolerance in force, or None when the check is off."""
        return self._fit_tol

    def last_fit(self, n):
        """The n records of the last tracking call this engine executed (structured array, _lib.FIT_DTYPE)."""
        out = np.zeros(int(n), FIT_DTYPE)
        check(self.lib.se3tn_last_fit(self._h, int(n), C.c_void_p(out.ctypes.data)), "se3tn_last_fit")
        return out

    def last_fit_images(self, n, rgb_out=None, depth_out=None):
        """Copies of the estimate renders of that call: device tensors uint8 [n,176,176,3], uint16-as-int16 [n,176,176]
        (stream-ordered copies into rgb_out / depth_out when given)."""
        rgb_p, dep_p = C.c_void_p(), C.c_void_p()
        check(self.lib.se3tn_last_fit_images(self._h, C.byref(rgb_p), C.byref(dep_p)), "se3tn_last_fit_images")
        dev = "cuda:%d" % self.device
        n = int(n)
        rgb = rgb_out if rgb_out is not None else torch.empty((n, RES, RES, 3), dtype=torch.uint8, device=dev)
        dep = depth_out if depth_out is not None else torch.empty((n, RES, RES), dtype=torch.int16, device=dev)
        check(self.lib.se3tn_memcpy_d2d(C.c_void_p(rgb.data_ptr()), rgb_p, n * RES * RES * 3, _stream_ptr()), "se3tn_memcpy_d2d")
        check(self.lib.se3tn_memcpy_d2d(C.c_void_p(dep.data_ptr()), dep_p, n * RES * RES * 2, _stream_ptr()), "se3tn_memcpy_d2d")
        return rgb, dep

    # ---- the objects of one frame as one scene ---------------------------------------------------
    def scene_stats(self, layers, rects, observed, tol_mm, ids=True, scene=True, out=None):
        """se3tn_scene_stats: n depth layers of one frame composed through a shared depth test (the rule: utils.scene_stats).
        layers: n cuda 16-bit tensors, layer i of rects[i][3]-rects[i][1] rows x rects[i][2]-rects[i][0] columns, contiguous (None for
        an empty rectangle); rects [n,4] (x0, y0, x1, y1); observed: cuda 16-bit [H,W].  ids / scene: also compute the id image (cuda
        uint8 [H,W]) / the composed depth (cuda int16 [H,W]).  Returns (records, ids, scene): records a structured array
        (_lib.SCENE_FIT_DTYPE), the images as numpy arrays (uint8, uint16) or None; synchronises on the current stream.
        out: where the n records go -- a cuda uint8 tensor of >= 48 n bytes, or the DEVICE address (int) of mapped pinned host memory;
        the call is then only enqueued (capturable), records is None and the images stay device tensors."""
        r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 4))
        n = len(r)
        if len(layers) != n:
            raise ValueError("scene_stats: %d layers and %d rectangles" % (len(layers), n))
        assert observed.is_cuda and observed.element_size() == 2 and observed.is_contiguous() and observed.dim() == 2
        H, W = int(observed.shape[0]), int(observed.shape[1])
        arr = (_lib.SceneLayer * max(n, 1))()
        for i in range(n):
            w, h = int(r[i, 2] - r[i, 0]), int(r[i, 3] - r[i, 1])
            arr[i].rect[:] = [int(v) for v in r[i]]
            if w > 0 and h > 0 and layers[i] is not None:
                d = layers[i]
                assert d.is_cuda and d.element_size() == 2 and d.is_contiguous() and d.numel() == w * h
                arr[i].depth = d.data_ptr()
        dev = "cuda:%d" % self.device
        ids_t = torch.empty((H, W), dtype=torch.uint8, device=dev) if ids else None
        scene_t = torch.empty((H, W), dtype=torch.int16, device=dev) if scene else None
        rec_t = None
        if out is None:
            rec_t = torch.empty((max(n, 1), 48), dtype=torch.uint8, device=dev)
            out_p = rec_t.data_ptr()
        else:
            out_p = out.data_ptr() if torch.is_tensor(out) else int(out)
        check(self.lib.se3tn_scene_stats(self._h, n, arr, C.c_void_p(observed.data_ptr()), H, W, int(tol_mm), C.c_void_p(out_p),
                                         C.c_void_p(ids_t.data_ptr()) if ids else None, C.c_void_p(scene_t.data_ptr()) if scene else None,
                                         _stream_ptr()), "se3tn_scene_stats")
        if rec_t is None:
            return None, ids_t, scene_t
        rec = rec_t.cpu().numpy().reshape(-1).view(SCENE_FIT_DTYPE)[:n].copy()
        return rec, (ids_t.cpu().numpy() if ids else None), (scene_t.cpu().numpy().view(np.uint16) if scene else None)

    @staticmethod
    def _scene_objects(objects):
        """an se3tn_object array from a ctypes array of them, or from (mesh | HipRenderer, object_width_mm) pairs; model stays NULL
        (the scene calls do not read it)"""
        if isinstance(objects, C.Array):
            return objects, len(objects)
        objs = (_lib.Object * max(len(objects), 1))()
        for i, (mesh, width) in enumerate(objects):
            m = getattr(mesh, "_m", mesh)
            objs[i].mesh = m.value if isinstance(m, C.c_void_p) else m
            objs[i].object_width_mm = float(width)
        return objs, len(objects)

    def scene_fit(self, objects, poses, depth, K, tol_mm=10, ids=False, scene=False):
        """se3tn_scene_fit / se3tn_scene_fit_host: render the objects' meshes at `poses` ([n,4,4]) into their se3tn_frame_rect
        rectangles (full-frame mode, whatever a mesh's route or material), compose them through a shared depth test and score every
        object over the pixels where it is the nearest tracked surface.  objects: a ctypes array of _lib.Object, or (mesh | HipRenderer,
        object_width_mm) pairs.  depth: a numpy uint16 [H,W] frame -> the host entry (one upload, one read-back, synchronous; refused
        while the current stream is being captured) with numpy results; a cuda 16-bit [H,W] tensor -> the device entry on the current
        stream with ids / scene as device tensors (uint8 / int16) and the records read back (which synchronises).
        Returns (records [n] of _lib.SCENE_FIT_DTYPE, ids | None, scene | None)."""
        objs, n = self._scene_objects(objects)
        p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        if len(p) != n:
            raise ValueError("scene_fit: %d poses for %d objects" % (len(p), n))
        Kp = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
        if torch.is_tensor(depth):
            assert depth.is_cuda and depth.element_size() == 2 and depth.is_contiguous() and depth.dim() == 2
            H, W = int(depth.shape[0]), int(depth.shape[1])
            rec_t = torch.empty((max(n, 1), 48), dtype=torch.uint8, device=depth.device)
            ids_t = torch.empty((H, W), dtype=torch.uint8, device=depth.device) if ids else None
            scene_t = torch.empty((H, W), dtype=torch.int16, device=depth.device) if scene else None
            check(self.lib.se3tn_scene_fit(self._h, n, objs, C.c_void_p(p.ctypes.data), Kp, C.c_void_p(depth.data_ptr()), H, W, int(tol_mm),
                                           C.c_void_p(rec_t.data_ptr()), C.c_void_p(ids_t.data_ptr()) if ids else None,
                                           C.c_void_p(scene_t.data_ptr()) if scene else None, _stream_ptr()), "se3tn_scene_fit")
            return rec_t.cpu().numpy().reshape(-1).view(SCENE_FIT_DTYPE)[:n].copy(), ids_t, scene_t
        if self.device >= 0 and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing():
            raise Se3tnError("se3tn_scene_fit_host refused (rc=-2): the call is synchronous, it cannot be captured")
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise ValueError("scene_fit: depth must be [H,W]")
        H, W = int(d.shape[0]), int(d.shape[1])
        rec = np.zeros(max(n, 1), SCENE_FIT_DTYPE)
        ids_a = np.zeros((H, W), np.uint8) if ids else None
        scene_a = np.zeros((H, W), np.uint16) if scene else None
        check(self.lib.se3tn_scene_fit_host(self._h, n, objs, C.c_void_p(p.ctypes.data), Kp, C.c_void_p(d.ctypes.data), H, W, int(tol_mm),
                                            C.c_void_p(rec.ctypes.data), C.c_void_p(ids_a.ctypes.data) if ids else None,
                                            C.c_void_p(scene_a.ctypes.data) if scene else None, _stream_ptr()), "se3tn_scene_fit_host")
        return rec[:n], ids_a, scene_a

    # ---- ADD / ADD-S of n pose pairs -------------------------------------------------------------
    def model_points(self, pts, normals=None):
        """Upload model points (float64 [P,3] metres, or an object with ``.points``) for pose_errors: a ModelPoints handle.
        normals (optional float64 [P,3]): one per point, for score_pose_grid(facing=True)."""
        return ModelPoints(self, pts, normals)

    def pose_errors(self, points, preds, gts, adds=True):
        """se3tn_pose_errors: ADD and ADD-S (Utils.py:72-98) of n (pred, gt) pose pairs against the model `points` (ModelPoints) in one
        call -> (add[n], adds[n]) in metres; adds=False skips the all-pairs loop and returns (add[n], None).
        preds / gts: [n,4,4] (or [n,16]) numpy arrays -> float64 numpy arrays, synchronous (se3tn_pose_errors_host); or cuda float64
        tensors -> cuda tensors, stream-ordered on the current stream, nothing allocated by the library (se3tn_pose_errors)."""
        if not isinstance(points, ModelPoints) or not points._h:
            raise Se3tnError("pose_errors: points must be an open ModelPoints handle (Engine.model_points)")
        if torch.is_tensor(preds) or torch.is_tensor(gts):
            if not (torch.is_tensor(preds) and torch.is_tensor(gts)):
                raise Se3tnError("pose_errors: preds and gts must both be tensors or both be arrays")
            for x in (preds, gts):
                assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and x.numel() % 16 == 0
            n = preds.numel() // 16
            assert gts.numel() == preds.numel()
            add = torch.empty((n,), dtype=torch.float64, device=preds.device)
            ads = torch.empty((n,), dtype=torch.float64, device=preds.device) if adds else None
            check(self.lib.se3tn_pose_errors(self._h, points._h, n, C.c_void_p(preds.data_ptr()), C.c_void_p(gts.data_ptr()),
                                             C.c_void_p(add.data_ptr()), C.c_void_p(ads.data_ptr()) if adds else None, _stream_ptr()),
                  "se3tn_pose_errors")
            return add, ads
        p = np.ascontiguousarray(np.asarray(preds, np.float64).reshape(-1, 16))
        g = np.ascontiguousarray(np.asarray(gts, np.float64).reshape(-1, 16))
        if p.shape != g.shape:
            raise ValueError("pose_errors: %d predicted and %d ground-truth poses" % (p.shape[0], g.shape[0]))
        n = int(p.shape[0])
        add = np.empty(n, np.float64)
        ads = np.empty(n, np.float64) if adds else None
        check(self.lib.se3tn_pose_errors_host(self._h, points._h, n, C.c_void_p(p.ctypes.data), C.c_void_p(g.ctypes.data),
                                              C.c_void_p(add.ctypes.data), C.c_void_p(ads.ctypes.data) if adds else None, _stream_ptr()),
              "se3tn_pose_errors_host")
        return add, ads

    # ---- n candidate poses against one depth frame ------------------------------------------------
    def score_poses(self, points, poses, depth, K, tol_mm, top=None):
        """se3tn_score_poses (+ se3tn_rank_poses): project the model `points` (ModelPoints) under each of n candidate poses into the
        depth frame (uint16 mm [H,W]) with the camera K (3x3) and count, per pose, the points in frame / seen / within tol_mm of the
        observed surface / behind something / seen through -- the rule of include/se3tracknet.h, every counter an integer.
        numpy in ([n,4,4] or [n,16] poses, [H,W] depth): top=None -> a structured array (_lib.POINT_FIT_DTYPE) of n records;
        top=k -> (idx[k] int32, records[k]): the k best candidates, best first (more inliers, then fewer seen-through points, then
        the lower index), ONE synchronous call (se3tn_search_poses_host: one upload, two launches, one read-back).
        cuda tensors in (float64 poses, 16-bit depth): an int32 tensor [n,8] of records (``.cpu().numpy().view(POINT_FIT_DTYPE)``), or
        with top=k (idx[k] int32, records[k,8]) -- stream-ordered on the current stream, nothing allocated by the library."""
        if not isinstance(points, ModelPoints) or not points._h:
            raise Se3tnError("score_poses: points must be an open ModelPoints handle (Engine.model_points)")
        Kh = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        Kp = Kh.ctypes.data_as(C.POINTER(C.c_double))
        if torch.is_tensor(poses) or torch.is_tensor(depth):
            if not (torch.is_tensor(poses) and torch.is_tensor(depth)):
                raise Se3tnError("score_poses: poses and depth must both be tensors or both be arrays")
            return self._score_poses_device(points, poses, depth, Kp, tol_mm, top)
        p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise ValueError("score_poses: depth must be [H,W]")
        n = int(p.shape[0])
        if top is None:   # all n records: the device entry point on uploaded copies (the host entry point returns the k best only)
            dev = "cuda:%d" % self.device
            fit = self._score_poses_device(points, torch.from_numpy(p).to(dev), torch.from_numpy(d.view(np.int16)).to(dev), Kp, tol_mm, None)
            return fit.cpu().numpy().view(POINT_FIT_DTYPE).reshape(n)
        k = int(top)
        idx = np.empty(max(k, 0), np.int32)
        fit = np.zeros(max(k, 0), POINT_FIT_DTYPE)
        check(self.lib.se3tn_search_poses_host(self._h, points._h, n, C.c_void_p(p.ctypes.data), C.c_void_p(d.ctypes.data), int(d.shape[0]),
                                               int(d.shape[1]), Kp, int(tol_mm), k, C.c_void_p(idx.ctypes.data), C.c_void_p(fit.ctypes.data),
                                               _stream_ptr()), "se3tn_search_poses_host")
        return idx, fit

    def _score_poses_device(self, points, poses, depth, Kp, tol_mm, top):
        assert poses.is_cuda and poses.dtype == torch.float64 and poses.is_contiguous() and poses.numel() % 16 == 0
        assert depth.is_cuda and depth.element_size() == 2 and depth.dim() == 2 and depth.is_contiguous()
        n = poses.numel() // 16
        fit = torch.empty((n, 8), dtype=torch.int32, device=poses.device)
        check(self.lib.se3tn_score_poses(self._h, points._h, n, C.c_void_p(poses.data_ptr()), C.c_void_p(depth.data_ptr()),
                                         int(depth.shape[0]), int(depth.shape[1]), Kp, int(tol_mm), C.c_void_p(fit.data_ptr()), _stream_ptr()),
              "se3tn_score_poses")
        if top is None:
            return fit
        idx = torch.empty((max(int(top), 0),), dtype=torch.int32, device=poses.device)
        check(self.lib.se3tn_rank_poses(self._h, n, C.c_void_p(fit.data_ptr()), int(top), C.c_void_p(idx.data_ptr()), _stream_ptr()),
              "se3tn_rank_poses")
        return idx, fit[idx.long()]

    def score_pose_grid(self, points, rots, trans, depth, K, tol_mm, facing=False, top=None, scene=None):
        """se3tn_score_pose_grid (+ se3tn_rank_poses): the n_rot x n_trans candidates [R_r | t_t] (candidate r * n_trans + t) of the
        rotations `rots` ([n_rot,3,3] or [n_rot,9]) and translations `trans` ([n_trans,3]) scored as score_poses scores composed
        poses, without materialising them.  facing=True counts only the points whose normal faces the camera (the handle must carry
        normals: Engine.model_points(pts, normals)); a record's ``points`` is then the number of facing points.  facing=False gives
        the words of score_poses on the composed poses.  Inputs and return values as score_poses: numpy in -> a structured array of
        n_rot * n_trans records, or with top=k (idx[k] int32, records[k]) from ONE synchronous call (se3tn_search_pose_grid_host);
        cuda tensors in (float64 rots / trans, 16-bit depth) -> int32 tensors, stream-ordered, nothing allocated by the library.
        scene (a cuda 16-bit [H,W] tensor, or a host uint16 array beside host inputs): the composed depth of the tracked objects
        (Engine.scene_fit(..., scene=True)) -> the scene-aware rule of se3tn_score_pose_grid_scene: a point at or behind a tracked
        surface is hidden_pts and nothing else.  The records then have dtype _lib.SCENE_POINT_FIT_DTYPE (word 7 = hidden_pts); with
        host inputs everything is uploaded and the device entry runs, top=k included (the one-call host search takes the occluders,
        not their scene: search_pose_grid_scene).  Without it nothing changes."""
        if not isinstance(points, ModelPoints) or not points._h:
            raise Se3tnError("score_pose_grid: points must be an open ModelPoints handle (Engine.model_points)")
        Kh = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        Kp = Kh.ctypes.data_as(C.POINTER(C.c_double))
        fc = 1 if facing else 0
        if scene is not None:
            return self._score_pose_grid_scene(points, rots, trans, depth, Kp, tol_mm, fc, top, scene)
        tensors = [torch.is_tensor(x) for x in (rots, trans, depth)]
        if any(tensors):
            if not all(tensors):
                raise Se3tnError("score_pose_grid: rots, trans and depth must all be tensors or all be arrays")
            return self._score_pose_grid_device(points, rots, trans, depth, Kp, tol_mm, fc, top)
        r = np.ascontiguousarray(np.asarray(rots, np.float64).reshape(-1, 9))
        t = np.ascontiguousarray(np.asarray(trans, np.float64).reshape(-1, 3))
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise ValueError("score_pose_grid: depth must be [H,W]")
        n_rot, n_trans = int(r.shape[0]), int(t.shape[0])
        if top is None:   # all records: the device entry point on uploaded copies (the host entry point returns the k best only)
            dev = "cuda:%d" % self.device
            fit = self._score_pose_grid_device(points, torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev),
                                               torch.from_numpy(d.view(np.int16)).to(dev), Kp, tol_mm, fc, None)
            return fit.cpu().numpy().view(POINT_FIT_DTYPE).reshape(n_rot * n_trans)
        k = int(top)
        idx = np.empty(max(k, 0), np.int32)
        fit = np.zeros(max(k, 0), POINT_FIT_DTYPE)
        check(self.lib.se3tn_search_pose_grid_host(self._h, points._h, n_rot, C.c_void_p(r.ctypes.data), n_trans, C.c_void_p(t.ctypes.data),
                                                   C.c_void_p(d.ctypes.data), int(d.shape[0]), int(d.shape[1]), Kp, int(tol_mm), fc, k,
                                                   C.c_void_p(idx.ctypes.data), C.c_void_p(fit.ctypes.data), _stream_ptr()),
              "se3tn_search_pose_grid_host")
        return idx, fit

    def _score_pose_grid_scene(self, points, rots, trans, depth, Kp, tol_mm, facing, top, scene):
        """score_pose_grid with a scene: tensors in -> tensors out; arrays in -> uploaded, the device entry, numpy out"""
        tensors = [torch.is_tensor(x) for x in (rots, trans, depth)]
        if any(tensors):
            if not (all(tensors) and torch.is_tensor(scene)):
                raise Se3tnError("score_pose_grid: rots, trans, depth and scene must all be tensors or all be arrays")
            return self._score_pose_grid_device(points, rots, trans, depth, Kp, tol_mm, facing, top, scene)
        dev = "cuda:%d" % self.device
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise ValueError("score_pose_grid: depth must be [H,W]")
        if torch.is_tensor(scene):   # (a scene kept on the device beside host candidates: MultiTracker.recover's rescoring)
            sc = scene
        else:
            sc = np.ascontiguousarray(scene, dtype=np.uint16)
            if sc.shape != d.shape:
                raise ValueError("score_pose_grid: scene must have the frame's shape")
            sc = torch.from_numpy(sc.view(np.int16)).to(dev)
        r = torch.from_numpy(np.ascontiguousarray(np.asarray(rots, np.float64).reshape(-1, 9))).to(dev)
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(trans, np.float64).reshape(-1, 3))).to(dev)
        out = self._score_pose_grid_device(points, r, t, torch.from_numpy(d.view(np.int16)).to(dev), Kp, tol_mm, facing, top, sc)
        if top is None:
            return out.cpu().numpy().view(SCENE_POINT_FIT_DTYPE).reshape(-1)
        return out[0].cpu().numpy(), out[1].cpu().numpy().view(SCENE_POINT_FIT_DTYPE).reshape(-1)

    def search_pose_grid_scene(self, points, rots, trans, depth, K, occluders, occ_poses, tol_mm=10, facing=True, top=8, keep_scene=False):
        """se3tn_search_pose_grid_scene_host: the lattice search among tracked objects as ONE synchronous call from host arrays --
        one upload of [rots | trans | depth], the occluders (as scene_fit's `objects`: a ctypes array of _lib.Object, or (mesh |
        HipRenderer, object_width_mm) pairs) rendered at occ_poses ([n_occ,4,4]) and composed into a scene frame that stays on the
        device, the scene-aware grid kernel, the ranking, one read-back.  Returns (idx[top] int32, records[top] of
        _lib.SCENE_POINT_FIT_DTYPE, the occluders' records [n_occ] of _lib.SCENE_FIT_DTYPE); with keep_scene=True a fourth value, a
        cuda int16 [H,W] tensor holding a copy of the composed scene (se3tn_last_search_scene) for score_pose_grid(scene=...)."""
        if not isinstance(points, ModelPoints) or not points._h:
            raise Se3tnError("search_pose_grid_scene: points must be an open ModelPoints handle (Engine.model_points)")
        objs, n_occ = self._scene_objects(occluders)
        op = np.ascontiguousarray(np.asarray(occ_poses, np.float64).reshape(-1, 16))
        if len(op) != n_occ:
            raise ValueError("search_pose_grid_scene: %d poses for %d occluders" % (len(op), n_occ))
        Kp = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9)).ctypes.data_as(C.POINTER(C.c_double))
        r = np.ascontiguousarray(np.asarray(rots, np.float64).reshape(-1, 9))
        t = np.ascontiguousarray(np.asarray(trans, np.float64).reshape(-1, 3))
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise ValueError("search_pose_grid_scene: depth must be [H,W]")
        H, W = int(d.shape[0]), int(d.shape[1])
        k = int(top)
        idx = np.empty(max(k, 0), np.int32)
        fit = np.zeros(max(k, 0), SCENE_POINT_FIT_DTYPE)
        occ = np.zeros(max(n_occ, 1), SCENE_FIT_DTYPE)
        check(self.lib.se3tn_search_pose_grid_scene_host(self._h, points._h, int(r.shape[0]), C.c_void_p(r.ctypes.data), int(t.shape[0]),
                                                         C.c_void_p(t.ctypes.data), C.c_void_p(d.ctypes.data), H, W, Kp, int(tol_mm),
                                                         1 if facing else 0, k, n_occ, objs, C.c_void_p(op.ctypes.data),
                                                         C.c_void_p(idx.ctypes.data), C.c_void_p(fit.ctypes.data), C.c_void_p(occ.ctypes.data),
                                                         _stream_ptr()), "se3tn_search_pose_grid_scene_host")
        if not keep_scene:
            return idx, fit, occ[:n_occ]
        ptr, h, w = C.c_void_p(), C.c_int(), C.c_int()
        check(self.lib.se3tn_last_search_scene(self._h, C.byref(ptr), C.byref(h), C.byref(w)), "se3tn_last_search_scene")
        scene_t = torch.empty((H, W), dtype=torch.int16, device="cuda:%d" % self.device)
        check(self.lib.se3tn_memcpy_d2d(C.c_void_p(scene_t.data_ptr()), ptr, H * W * 2, _stream_ptr()), "se3tn_memcpy_d2d")
        return idx, fit, occ[:n_occ], scene_t

    def _score_pose_grid_device(self, points, rots, trans, depth, Kp, tol_mm, facing, top, scene=None):
        assert rots.is_cuda and rots.dtype == torch.float64 and rots.is_contiguous() and rots.numel() % 9 == 0
        assert trans.is_cuda and trans.dtype == torch.float64 and trans.is_contiguous() and trans.numel() % 3 == 0
        assert depth.is_cuda and depth.element_size() == 2 and depth.dim() == 2 and depth.is_contiguous()
        n_rot, n_trans = rots.numel() // 9, trans.numel() // 3
        n = n_rot * n_trans
        fit = torch.empty((n, 8), dtype=torch.int32, device=rots.device)
        if scene is not None:
            assert scene.is_cuda and scene.element_size() == 2 and scene.is_contiguous() and scene.shape == depth.shape
            check(self.lib.se3tn_score_pose_grid_scene(self._h, points._h, n_rot, C.c_void_p(rots.data_ptr()), n_trans,
                                                       C.c_void_p(trans.data_ptr()), C.c_void_p(depth.data_ptr()), C.c_void_p(scene.data_ptr()),
                                                       int(depth.shape[0]), int(depth.shape[1]), Kp, int(tol_mm), int(facing),
                                                       C.c_void_p(fit.data_ptr()), _stream_ptr()), "se3tn_score_pose_grid_scene")
        else:
            check(self.lib.se3tn_score_pose_grid(self._h, points._h, n_rot, C.c_void_p(rots.data_ptr()), n_trans, C.c_void_p(trans.data_ptr()),
                                                 C.c_void_p(depth.data_ptr()), int(depth.shape[0]), int(depth.shape[1]), Kp, int(tol_mm),
                                                 int(facing), C.c_void_p(fit.data_ptr()), _stream_ptr()), "se3tn_score_pose_grid")
        if top is None:
            return fit
        idx = torch.empty((max(int(top), 0),), dtype=torch.int32, device=rots.device)
        check(self.lib.se3tn_rank_poses(self._h, n, C.c_void_p(fit.data_ptr()), int(top), C.c_void_p(idx.data_ptr()), _stream_ptr()),
              "se3tn_rank_poses")
        return idx, fit[idx.long()]

    # ---- n pose hypotheses aligned to one depth frame ------------------------------------------------
    def align_poses(self, points, poses, depth, K, gate_mm=20, iters=20, min_pairs=12, damping=1e-6, stop=1e-6, sums=False, scene=None,
                    scene_tol_mm=10):
        """se3tn_align_poses: up to `iters` damped point-to-plane steps of the facing points of the model `points` (a ModelPoints
        handle WITH normals) against the depth frame (uint16 mm [H,W]), for each of n poses, in ONE launch -- the rule of
        include/se3tracknet.h: points pair with the pixel they project to when it lies within gate_mm of them, every sum is an
        integer, the rotation is taken about the object's origin.  A pose stops when fewer than min_pairs points pair (status
        _lib.ALIGN_FEW), when the system cannot be solved (ALIGN_SINGULAR, the pose unchanged), when its step falls to `stop`
        (ALIGN_CONVERGED) or after `iters` iterations (ALIGN_ITERS).
        numpy in ([n,4,4] or [n,16] poses, [H,W] depth) -> (poses [n,4,4] float64, records [n] of _lib.ALIGN_REC_DTYPE), ONE synchronous
        call (se3tn_align_poses_host: one upload, one launch, one read-back); cuda tensors in (float64 poses, 16-bit depth) -> (poses
        [n,4,4] float64 tensor, records uint8 tensor [n,40]: ``.cpu().numpy().view(ALIGN_REC_DTYPE)``), stream-ordered on the current
        stream, nothing allocated by the library.  sums=True appends the int64 [n,28] sums of each pose's last evaluated iteration.
        scene (default None: exactly the calls above) is the composed depth of the tracked objects, uint16 mm [H,W], 0 where there is
        none -- what scene_fit(..., scene=True) and search_pose_grid_scene(keep_scene=True) return: se3tn_align_poses_scene, under
        which a facing point with a tracked surface at or in front of it (100 < s < 2000 and s <= m + scene_tol_mm) is hidden: not
        paired, and counted in hidden_pts.  The records then have _lib.SCENE_ALIGN_REC_DTYPE (hidden_pts in the place of _reserved).
        numpy poses and depth with a numpy scene: the host entry, one call; cuda tensors with a cuda 16-bit scene: the device entry on
        the current stream; numpy poses and depth with a cuda scene: poses and depth are uploaded, the device entry runs, numpy out."""
        if not isinstance(points, ModelPoints) or not points._h:
            raise Se3tnError("align_poses: points must be an open ModelPoints handle (Engine.model_points)")
        Kh = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        Kp = Kh.ctypes.data_as(C.POINTER(C.c_double))
        prm = _lib.AlignParams(int(gate_mm), int(iters), int(min_pairs), 0, float(damping), float(stop))
        if scene is not None:
            return self._align_poses_scene(points, poses, depth, Kp, prm, sums, scene, int(scene_tol_mm))
        if torch.is_tensor(poses) or torch.is_tensor(depth):
            if not (torch.is_tensor(poses) and torch.is_tensor(depth)):
                raise Se3tnError("align_poses: poses and depth must both be tensors or both be arrays")
            assert poses.is_cuda and poses.dtype == torch.float64 and poses.is_contiguous() and poses.numel() % 16 == 0
            assert depth.is_cuda and depth.element_size() == 2 and depth.dim() == 2 and depth.is_contiguous()
            n = poses.numel() // 16
            out = torch.empty((n, 4, 4), dtype=torch.float64, device=poses.device)
            rec = torch.empty((n, ALIGN_REC_DTYPE.itemsize), dtype=torch.uint8, device=poses.device)
            sm = torch.empty((n, _lib.POSE_ALIGN_SUMS), dtype=torch.int64, device=poses.device) if sums else None
            check(self.lib.se3tn_align_poses(self._h, points._h, n, C.c_void_p(poses.data_ptr()), C.c_void_p(depth.data_ptr()),
                                             int(depth.shape[0]), int(depth.shape[1]), Kp, C.byref(prm), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(rec.data_ptr()), C.c_void_p(sm.data_ptr()) if sums else None, _stream_ptr()),
                  "se3tn_align_poses")
            return (out, rec, sm) if sums else (out, rec)
        p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise ValueError("align_poses: depth must be [H,W]")
        n = int(p.shape[0])
        out = np.empty((max(n, 0), 4, 4), np.float64)
        rec = np.zeros(max(n, 0), ALIGN_REC_DTYPE)
        sm = np.zeros((max(n, 0), _lib.POSE_ALIGN_SUMS), np.int64) if sums else None
        check(self.lib.se3tn_align_poses_host(self._h, points._h, n, C.c_void_p(p.ctypes.data), C.c_void_p(d.ctypes.data), int(d.shape[0]),
                                              int(d.shape[1]), Kp, C.byref(prm), C.c_void_p(out.ctypes.data), C.c_void_p(rec.ctypes.data),
                                              C.c_void_p(sm.ctypes.data) if sums else None, _stream_ptr()), "se3tn_align_poses_host")
        return (out, rec, sm) if sums else (out, rec)

    def _align_poses_scene(self, points, poses, depth, Kp, prm, sums, scene, scene_tol_mm):
        """align_poses with a scene: tensors in -> tensors out; arrays in -> the host entry, or with a cuda scene uploaded, the device
        entry, numpy out"""
        tensors = [torch.is_tensor(poses), torch.is_tensor(depth)]
        if any(tensors):
            if not (all(tensors) and torch.is_tensor(scene)):
                raise Se3tnError("align_poses: poses, depth and scene must all be tensors or all be arrays")
            return self._align_poses_scene_device(points, poses, depth, Kp, prm, sums, scene, scene_tol_mm)
        p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise ValueError("align_poses: depth must be [H,W]")
        if torch.is_tensor(scene):   # (a scene kept on the device beside host hypotheses: MultiTracker.recover's alignment)
            dev = "cuda:%d" % self.device
            out = self._align_poses_scene_device(points, torch.from_numpy(p).to(dev), torch.from_numpy(d.view(np.int16)).to(dev), Kp, prm,
                                                 sums, scene, scene_tol_mm)
            res = (out[0].cpu().numpy(), out[1].cpu().numpy().view(SCENE_ALIGN_REC_DTYPE).reshape(-1))
            return res + (out[2].cpu().numpy(),) if sums else res
        sc = np.ascontiguousarray(scene, dtype=np.uint16)
        if sc.shape != d.shape:
            raise ValueError("align_poses: scene must have the frame's shape")
        n = int(p.shape[0])
        out = np.empty((max(n, 0), 4, 4), np.float64)
        rec = np.zeros(max(n, 0), SCENE_ALIGN_REC_DTYPE)
        sm = np.zeros((max(n, 0), _lib.POSE_ALIGN_SUMS), np.int64) if sums else None
        check(self.lib.se3tn_align_poses_scene_host(self._h, points._h, n, C.c_void_p(p.ctypes.data), C.c_void_p(d.ctypes.data),
                                                    C.c_void_p(sc.ctypes.data), int(d.shape[0]), int(d.shape[1]), Kp, C.byref(prm),
                                                    scene_tol_mm, C.c_void_p(out.ctypes.data), C.c_void_p(rec.ctypes.data),
                                                    C.c_void_p(sm.ctypes.data) if sums else None, _stream_ptr()),
              "se3tn_align_poses_scene_host")
        return (out, rec, sm) if sums else (out, rec)

    def _align_poses_scene_device(self, points, poses, depth, Kp, prm, sums, scene, scene_tol_mm):
        assert poses.is_cuda and poses.dtype == torch.float64 and poses.is_contiguous() and poses.numel() % 16 == 0
        assert depth.is_cuda and depth.element_size() == 2 and depth.dim() == 2 and depth.is_contiguous()
        assert scene.is_cuda and scene.element_size() == 2 and scene.is_contiguous() and scene.shape == depth.shape
        n = poses.numel() // 16
        out = torch.empty((n, 4, 4), dtype=torch.float64, device=poses.device)
        rec = torch.empty((n, SCENE_ALIGN_REC_DTYPE.itemsize), dtype=torch.uint8, device=poses.device)
        sm = torch.empty((n, _lib.POSE_ALIGN_SUMS), dtype=torch.int64, device=poses.device) if sums else None
        check(self.lib.se3tn_align_poses_scene(self._h, points._h, n, C.c_void_p(poses.data_ptr()), C.c_void_p(depth.data_ptr()),
                                               C.c_void_p(scene.data_ptr()), int(depth.shape[0]), int(depth.shape[1]), Kp, C.byref(prm),
                                               scene_tol_mm, C.c_void_p(out.data_ptr()), C.c_void_p(rec.data_ptr()),
                                               C.c_void_p(sm.data_ptr()) if sums else None, _stream_ptr()), "se3tn_align_poses_scene")
        return (out, rec, sm) if sums else (out, rec)

    def fill_depth(self, depth_mm, max_depth=2.0, extrapolate=False, blur_type="bilateral", return_metres=False):
        """Utils.py:455-514 fill_depth as predict_ros.py:38-41 applies it: uint16 millimetre frame (numpy [H,W] or a
        cuda int16/uint16 tensor) -> hole-filled uint16 millimetres (same container kind); return_metres=True also
        returns the float32 metre image fill_depth itself returns."""
        dev = "cuda:%d" % self.device
        is_np = not torch.is_tensor(depth_mm)
        d = torch.from_numpy(np.ascontiguousarray(depth_mm, dtype=np.uint16).view(np.int16)).to(dev) if is_np else depth_mm
        assert d.is_cuda and d.element_size() == 2 and d.dim() == 2 and d.is_contiguous()
        H, W = int(d.shape[0]), int(d.shape[1])
        out = torch.empty((H, W), dtype=torch.int16, device=dev)
        out_m = torch.empty((H, W), dtype=torch.float32, device=dev) if return_metres else None
        blur = {"bilateral": _lib.BLUR_BILATERAL, "gaussian": _lib.BLUR_GAUSSIAN}.get(blur_type, _lib.BLUR_NONE)
        check(self.lib.se3tn_fill_depth(self._h, C.c_void_p(d.data_ptr()), H, W, float(max_depth), 1 if extrapolate else 0, blur,
                                        C.c_void_p(out.data_ptr()), C.c_void_p(out_m.data_ptr()) if return_metres else None,
                                        _stream_ptr()), "se3tn_fill_depth")
        if is_np:
            mm = out.cpu().numpy().view(np.uint16)
            return (mm, out_m.cpu().numpy()) if return_metres else mm
        return (out, out_m) if return_metres else out

    def fill_depth_rect(self, depth_mm, rect, max_depth=2.0, extrapolate=False, blur_type="bilateral"):
        """fill_depth for the pixels of one rectangle (se3tn_fill_depth_rect): rect = (x0, y0, x1, y1) inside the frame ->
        uint16 millimetres [y1-y0, x1-x0], every value the same pixel of fill_depth's result (same container kind as
        depth_mm: numpy [H,W] or a cuda int16/uint16 tensor)."""
        dev = "cuda:%d" % self.device
        is_np = not torch.is_tensor(depth_mm)
        d = torch.from_numpy(np.ascontiguousarray(depth_mm, dtype=np.uint16).view(np.int16)).to(dev) if is_np else depth_mm
        assert d.is_cuda and d.element_size() == 2 and d.dim() == 2 and d.is_contiguous()
        H, W = int(d.shape[0]), int(d.shape[1])
        r = (C.c_int32 * 4)(*[int(v) for v in rect])
        out = torch.empty((max(r[3] - r[1], 0), max(r[2] - r[0], 0)), dtype=torch.int16, device=dev)
        blur = blur_type if isinstance(blur_type, int) else \
            {"bilateral": _lib.BLUR_BILATERAL, "gaussian": _lib.BLUR_GAUSSIAN}.get(blur_type, _lib.BLUR_NONE)
        check(self.lib.se3tn_fill_depth_rect(self._h, C.c_void_p(d.data_ptr()), H, W, float(max_depth), 1 if extrapolate else 0, blur, r,
                                             C.c_void_p(out.data_ptr()), _stream_ptr()), "se3tn_fill_depth_rect")
        return out.cpu().numpy().view(np.uint16) if is_np else out

    def fill_depth_rects(self, depth_mm, rects, max_depth=2.0, extrapolate=False, blur_type="bilateral"):
        """fill_depth for the pixels of n rectangles of ONE frame in one call (se3tn_fill_depth_rects: the chain up to the median
        once, the last pass for all rectangles in one launch per 64): rects = n x (x0, y0, x1, y1), each inside the frame or empty
        (x1 <= x0 or y1 <= y0: skipped, an array of shape (0, 0) comes back) -> a list of n uint16 millimetre arrays
        [y1-y0, x1-x0], every value the same pixel of fill_depth's result whatever the other rectangles (same container kind as
        depth_mm: numpy [H,W] or a cuda int16/uint16 tensor)."""
        dev = "cuda:%d" % self.device
        is_np = not torch.is_tensor(depth_mm)
        d = torch.from_numpy(np.ascontiguousarray(depth_mm, dtype=np.uint16).view(np.int16)).to(dev) if is_np else depth_mm
        assert d.is_cuda and d.element_size() == 2 and d.dim() == 2 and d.is_contiguous()
        H, W = int(d.shape[0]), int(d.shape[1])
        r = np.ascontiguousarray(np.asarray(rects, np.int64).reshape(-1, 4).astype(np.int32))
        n = int(r.shape[0])
        hw = [(max(int(q[3]) - int(q[1]), 0), max(int(q[2]) - int(q[0]), 0)) for q in r]
        hw = [(h, w) if h and w else (0, 0) for h, w in hw]
        offs = np.zeros(max(n, 1), np.uintp)
        total = 0
        for i, (h, w) in enumerate(hw):
            offs[i] = total
            total += h * w
        out = torch.empty((max(total, 1),), dtype=torch.int16, device=dev)
        blur = blur_type if isinstance(blur_type, int) else \
            {"bilateral": _lib.BLUR_BILATERAL, "gaussian": _lib.BLUR_GAUSSIAN}.get(blur_type, _lib.BLUR_NONE)
        check(self.lib.se3tn_fill_depth_rects(self._h, C.c_void_p(d.data_ptr()), H, W, float(max_depth), 1 if extrapolate else 0, blur, n,
                                              r.ctypes.data_as(C.POINTER(C.c_int32)), offs.ctypes.data_as(C.POINTER(C.c_size_t)),
                                              C.c_void_p(out.data_ptr()), _stream_ptr()), "se3tn_fill_depth_rects")
        parts = [out[int(offs[i]):int(offs[i]) + h * w].view(h, w) for i, (h, w) in enumerate(hw)]
        if is_np:
            flat = out.cpu().numpy().view(np.uint16)
            return [flat[int(offs[i]):int(offs[i]) + h * w].reshape(h, w).copy() for i, (h, w) in enumerate(hw)]
        return parts

    def infer(self, A, B, n, layout=NCHW, trans=None, rot=None, poseA=None, poseB=None):
        def p(x):
            if x is None:
                return None
            return C.c_void_p(x.data_ptr() if torch.is_tensor(x) else int(x))
        check(self.lib.se3tn_infer(self._h, p(A), p(B), int(n), int(layout), p(trans), p(rot), p(poseA), p(poseB),
                                   _stream_ptr()), "se3tn_infer")

    def feature(self, n):
        out = torch.empty((n, 256, 22, 22), dtype=torch.float32, device="cuda:%d" % self.device)
        check(self.lib.se3tn_get_feature(self._h, n, C.c_void_p(out.data_ptr()), _stream_ptr()), "se3tn_get_feature")
        return out

    def logits(self, n):
        out = torch.empty((n, 6), dtype=torch.float32, device="cuda:%d" % self.device)
        check(self.lib.se3tn_memcpy_d2d(C.c_void_p(out.data_ptr()), C.c_void_p(self.lib.se3tn_logits(self._h)),
                                        n * 6 * 4, _stream_ptr()), "se3tn_memcpy_d2d")
        return out

    def debug_buffer(self, name, n):
        """Copy of an internal NHWC activation buffer: float32 cuda tensor [n,H,W,C]."""
        ptr = C.c_void_p()
        dims = (C.c_int32 * 3)()
        check(self.lib.se3tn_debug_buffer(self._h, name.encode(), C.byref(ptr), dims), "se3tn_debug_buffer")
        out = torch.empty((n, dims[0], dims[1], dims[2]), dtype=torch.float32, device="cuda:%d" % self.device)
        check(self.lib.se3tn_memcpy_d2d(C.c_void_p(out.data_ptr()), ptr, out.numel() * 4, _stream_ptr()),
              "se3tn_memcpy_d2d")
        return out

    # ---- profiling -------------------------------------------------------------------------
    def profile_enable(self, slots=1):
        check(self.lib.se3tn_profile_enable(self._h, int(slots)), "se3tn_profile_enable")

    def profile_read(self, slot=0):
        """(ms inside the conv3x3 MFMA family, number of such launches, ms of all launches)"""
        conv = C.c_float(); nl = C.c_int(); tot = C.c_float()
        check(self.lib.se3tn_profile_read(self._h, slot, C.byref(conv), C.byref(nl), C.byref(tot)),
              "se3tn_profile_read")
        return conv.value, nl.value, tot.value

    def profile_launches(self, slot=0):
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        k = self.lib.se3tn_profile_launches(self._h, slot, 32, names, ms)
        if k <= 0:
            raise Se3tnError("se3tn_profile_launches: " + self.lib.se3tn_last_error().decode())
        return [(names[i].decode(), ms[i]) for i in range(k)]


class PipelinedEngine:
    """Throughput mode: `depth` contexts (activation workspaces) that share ONE packed weight blob, each with its own HIP
    stream; successive batches go to successive lanes, so the HBM-bound passes of one batch (crop / normalise, max-pool,
    Winograd transforms, pose) run under the matrix-core-bound kernels of the other.  Measured at batch 64: two lanes
    35.7 k pairs/s vs 33.0 k on one stream; a third lane adds nothing (scripts/two_stream_probe.py).

        pe = PipelinedEngine(0, 64); pe.load_state_dict(sd); pe.set_normalization(mean, std)
        for batch in batches:
            eng, stream = pe.next_lane()
            with torch.cuda.stream(stream):
                eng.preprocess(...); eng.infer(...)          # asynchronous; outputs must be per-lane buffers
        pe.synchronize()
    """

    def __init__(self, device=0, max_batch=64, depth=2):
        assert depth >= 1
        self.device = int(device)
        self.engines = [Engine(device, max_batch) for _ in range(depth)]
        dev = "cuda:%d" % self.device
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(depth)]
        self._i = 0
        self._blob = None

    def load_state_dict(self, state_dict):
        """Fold + pack once, upload once, bind the same device blob to every lane."""
        blob = self.engines[0].pack_state_dict(state_dict).to("cuda:%d" % self.device)
        self.bind_blob(blob)

    def bind_blob(self, blob_cuda):
        self._blob = blob_cuda
        for e in self.engines:
            e.bind_blob(blob_cuda)

    def __getattr__(self, name):
        # configuration calls (set_normalization, set_normalizers, set_precision, set_winograd, ...) go to every lane
        if name.startswith("set_") or name in ("keep_intermediates", "enable_graphs"):
            def fan_out(*a, **k):
                for e in self.engines:
                    getattr(e, name)(*a, **k)
            return fan_out
        raise AttributeError(name)

    def next_lane(self):
        k = self._i % len(self.engines)
        self._i += 1
        return self.engines[k], self.streams[k]

    def synchronize(self):
        for s in self.streams:
            s.synchronize()


# ---- host-side float64 helpers (pure CPU entry points of the C ABI) ---------------------------
def compute_bbox(pose, K, object_width_mm):
    """Utils.py:302-316 with scale=(1000,1000,1000): int32 [4,2] (v,u)."""
    lib = _lib.load()
    p = (C.c_double * 16)(*np.asarray(pose, np.float64).reshape(16))
    k = (C.c_double * 9)(*np.asarray(K, np.float64).reshape(9))
    out = (C.c_int32 * 8)()
    check(lib.se3tn_compute_bbox(p, k, float(object_width_mm), out), "se3tn_compute_bbox")
    return np.array(out[:], dtype=np.int32).reshape(4, 2)


def frame_rect(pose, K, object_width_mm, H, W):
    """The rectangle (x0, y0, x1, y1) of an H x W frame the full-frame (pyrender) route renders for this pose: compute_bbox's crop
    window clipped to the frame (se3tn_frame_rect); None when the window misses the frame."""
    lib = _lib.load()
    p = (C.c_double * 16)(*np.asarray(pose, np.float64).reshape(16))
    k = (C.c_double * 9)(*np.asarray(K, np.float64).reshape(9))
    out = (C.c_int32 * 4)()
    check(lib.se3tn_frame_rect(p, k, float(object_width_mm), int(H), int(W), out), "se3tn_frame_rect")
    r = tuple(int(x) for x in out)
    return r if r[2] > r[0] and r[3] > r[1] else None


def pose_update_host(A_in_cam, trans, rot, trans_normalizer, rot_normalizer):
    """datasets.py:159-175 processPredict (host float64)."""
    lib = _lib.load()
    a = (C.c_double * 16)(*np.asarray(A_in_cam, np.float64).reshape(16))
    t = (C.c_float * 3)(*np.asarray(trans, np.float32).reshape(3))
    r = (C.c_float * 3)(*np.asarray(rot, np.float32).reshape(3))
    out = (C.c_double * 16)()
    check(lib.se3tn_pose_update_host(a, t, r, float(trans_normalizer), float(rot_normalizer), out),
          "se3tn_pose_update_host")
    return np.array(out[:], dtype=np.float64).reshape(4, 4)
