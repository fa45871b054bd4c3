"""ctypes binding of libse3tracknet.so (C ABI: include/se3tracknet.h).

The HIP library IS the product path: there is no CPU / PyTorch fallback.  If the shared object
is missing this module raises ImportError telling how to build it; a compute call on a box
without a gfx950 GPU fails in se3tn_create with SE3TN_E_DEVICE / a hipError.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SE3TN_LIB: developer override used for within-session A/B of kernel variants
LIB_PATH = os.environ.get("SE3TN_LIB") or os.path.join(_HERE, "libse3tracknet.so")

NCHW, NHWC = 0, 1
PREC_F32, PREC_F16X3 = 0, 1
WINOGRAD_TILE_AUTO, WINOGRAD_TILE6_MIN_BATCH = 46, 14   # as include/se3tracknet.h: F(4x4) below 14 pairs, F(6x6) from there
WINOGRAD_TILE_6_4, WINOGRAD_HEADS_TILE6_MAX_ROT = 64, 0.2     # F(6x6) 256-channel block + F(4x4) heads; AUTO's rot_normalizer bound for F(6x6) heads
TRUNK_WINOGRAD_DEFAULT_MIN_BATCH, TRUNK_WINOGRAD_DEFAULT_MIN_FILL = 8, 55   # as include/se3tracknet.h (tests/test_host_abi.py)
OFFSET_RULE_NUMPY1, OFFSET_RULE_NUMPY2 = 0, 1   # as include/se3tracknet.h: rounding of OffsetDepth's float64-scalar subtraction
BLUR_NONE, BLUR_BILATERAL, BLUR_GAUSSIAN = 0, 1, 2
COLOR_RGB, COLOR_BGR = 0, 1        # se3tn_on_track_live's / se3tn_on_track_objects_live's color_order
ROUTE_WINDOW, ROUTE_FRAME = 0, 1   # as include/se3tracknet.h: the renderer se3tn_on_track uses for a mesh's image A
FIT_MAX_PAIRS = 32                 # as include/se3tracknet.h: pairs per launch of se3tn_fit_stats (larger n are chunked)
FIT_SCENE_MAX_PAIRS = 16           # as include/se3tracknet.h: pairs per launch of se3tn_color_stats_scene (three descriptors per pair)
POSE_ERRORS_CHUNK = 256            # as include/se3tracknet.h: pose pairs per launch of se3tn_pose_errors (larger n are chunked)
POSE_ERRORS_MAX_POINTS = 1 << 20   # as include/se3tracknet.h: the largest model se3tn_points_create accepts
POSE_SEARCH_MAX_POSES = 1 << 20   # as include/se3tracknet.h: the most candidate poses one se3tn_score_poses / se3tn_rank_poses call takes
POSE_RANK_MAX = 64                 # as include/se3tracknet.h: the largest k of se3tn_rank_poses
POSE_ALIGN_MAX_POSES = 4096        # as include/se3tracknet.h: the most poses one se3tn_align_poses call takes
POSE_ALIGN_MAX_ITERS = 64          # as include/se3tracknet.h: the most iterations of one se3tn_align_poses call
POSE_ALIGN_SUMS = 28               # as include/se3tracknet.h: int64 sums per pose (21 of S_A | 6 of S_b | S_e)
ALIGN_ITERS, ALIGN_CONVERGED, ALIGN_FEW, ALIGN_SINGULAR = 0, 1, 2, 3   # as include/se3tracknet.h: se3tn_align_rec.status
SCENE_MAX_OBJECTS = 32             # as include/se3tracknet.h: the most layers / objects of one se3tn_scene_stats / se3tn_scene_fit call
SCENE_MAX_PIXELS = 1 << 21         # as include/se3tracknet.h: the largest frame (H * W) of the scene calls
MAX_BATCH_LIMIT = 1982             # as include/se3tracknet.h: the largest max_batch se3tn_create accepts
RES = 176


class Se3tnError(RuntimeError):
    pass


class Crop(C.Structure):
    """se3tn_crop (include/se3tracknet.h)."""
    _fields_ = [("rgb", C.c_void_p), ("depth", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32),
                ("left", C.c_int32), ("top", C.c_int32), ("right", C.c_int32), ("bottom", C.c_int32),
                ("z_offset_mm", C.c_double), ("stats", C.c_int32), ("_pad", C.c_int32)]


class Object(C.Structure):
    """se3tn_object (include/se3tracknet.h): one object of se3tn_on_track_objects."""
    _fields_ = [("model", C.c_void_p), ("mesh", C.c_void_p), ("object_width_mm", C.c_double)]


class Fit(C.Structure):
    """se3tn_fit (include/se3tracknet.h): the fit record of one (model, observed) pair."""
    _fields_ = [(k, C.c_uint32) for k in ("model_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm", "tol_mm",
                                          "_reserved")]


class ColorFit(C.Structure):
    """se3tn_color_fit (include/se3tracknet.h): the colour record of one (model, observed) pair."""
    _fields_ = [("px", C.c_uint32), ("tol_mm", C.c_uint32)] + [(k, C.c_uint32 * 3) for k in ("sum_m", "sum_o", "sum_mm", "sum_oo", "sum_mo",
                                                                                           "sum_abs")]


class AlignParams(C.Structure):
    """se3tn_align_params (include/se3tracknet.h): gate, iteration and stop settings of se3tn_align_poses."""
    _fields_ = [("gate_mm", C.c_int32), ("iters", C.c_int32), ("min_pairs", C.c_int32), ("_reserved", C.c_int32),
                ("damping", C.c_double), ("stop", C.c_double)]


class AlignRec(C.Structure):
    """se3tn_align_rec (include/se3tracknet.h): what became of one pose of se3tn_align_poses."""
    _fields_ = [("iterations", C.c_uint32), ("status", C.c_uint32), ("pairs", C.c_uint32), ("facing_pts", C.c_uint32),
                ("sum_r2", C.c_int64), ("pairs0", C.c_uint32), ("_reserved", C.c_uint32), ("sum_r2_0", C.c_int64)]


class SceneAlignRec(C.Structure):
    """se3tn_scene_align_rec (include/se3tracknet.h): what became of one pose of se3tn_align_poses_scene."""
    _fields_ = [("iterations", C.c_uint32), ("status", C.c_uint32), ("pairs", C.c_uint32), ("facing_pts", C.c_uint32),
                ("sum_r2", C.c_int64), ("pairs0", C.c_uint32), ("hidden_pts", C.c_uint32), ("sum_r2_0", C.c_int64)]


class PointFit(C.Structure):
    """se3tn_point_fit (include/se3tracknet.h): the record of one candidate pose of se3tn_score_poses."""
    _fields_ = [(k, C.c_uint32) for k in ("points", "in_frame_pts", "seen_pts", "inlier_pts", "front_pts", "behind_pts", "tol_mm",
                                          "_reserved")]


class SceneFit(C.Structure):
    """struct se3tn_scene_fit (include/se3tracknet.h): the record of one object of a frame composed with the others."""
    _fields_ = [(k, C.c_uint32) for k in ("model_px", "visible_px", "hidden_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm",
                                          "hidden_by", "tol_mm", "n_objects", "_reserved")]


class SceneLayer(C.Structure):
    """se3tn_scene_layer (include/se3tracknet.h): one depth layer of se3tn_scene_stats: a device sub-image and its rectangle."""
    _fields_ = [("depth", C.c_void_p), ("rect", C.c_int32 * 4)]


# the same record as a numpy dtype, for building many descriptors without a Python loop
import numpy as _np
CROP_DTYPE = _np.dtype([("rgb", "<u8"), ("depth", "<u8"), ("H", "<i4"), ("W", "<i4"), ("left", "<i4"), ("top", "<i4"),
                        ("right", "<i4"), ("bottom", "<i4"), ("z_offset_mm", "<f8"), ("stats", "<i4"), ("_pad", "<i4")])
assert CROP_DTYPE.itemsize == C.sizeof(Crop)
FIT_FIELDS = ("model_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm", "tol_mm")   # the seven that carry data
FIT_DTYPE = _np.dtype([(k, "<u4") for k in FIT_FIELDS + ("_reserved",)])
assert FIT_DTYPE.itemsize == C.sizeof(Fit) == 32
# the depth record of the scene-aware crop rule (se3tn_color_stats_scene): the same 32 bytes with word 7 in use (hidden_px)
SCENE_CROP_FIT_DTYPE = _np.dtype([(k, "<u4") for k in FIT_FIELDS + ("hidden_px",)])
assert SCENE_CROP_FIT_DTYPE.itemsize == 32 and SCENE_CROP_FIT_DTYPE.fields["hidden_px"][1] == 28
COLOR_FIT_SUMS = ("sum_m", "sum_o", "sum_mm", "sum_oo", "sum_mo", "sum_abs")   # three words each: R, G, B
COLOR_FIT_DTYPE = _np.dtype([("px", "<u4"), ("tol_mm", "<u4")] + [(k, "<u4", (3,)) for k in COLOR_FIT_SUMS])
assert COLOR_FIT_DTYPE.itemsize == C.sizeof(ColorFit) == 80
POINT_FIT_FIELDS = ("points", "in_frame_pts", "seen_pts", "inlier_pts", "front_pts", "behind_pts", "tol_mm")   # the seven that carry data
POINT_FIT_DTYPE = _np.dtype([(k, "<u4") for k in POINT_FIT_FIELDS + ("_reserved",)])
assert POINT_FIT_DTYPE.itemsize == C.sizeof(PointFit) == 32
# se3tn_scene_point_fit: the same 32 bytes with word 7 in use (hidden_pts); se3tn_rank_poses and recover.pose_key read both alike
SCENE_POINT_FIT_FIELDS = POINT_FIT_FIELDS + ("hidden_pts",)
SCENE_POINT_FIT_DTYPE = _np.dtype([(k, "<u4") for k in SCENE_POINT_FIT_FIELDS])
assert SCENE_POINT_FIT_DTYPE.itemsize == 32
SCENE_FIT_FIELDS = ("model_px", "visible_px", "hidden_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm", "hidden_by", "tol_mm",
                    "n_objects")   # the eleven that carry data
SCENE_FIT_DTYPE = _np.dtype([(k, "<u4") for k in SCENE_FIT_FIELDS + ("_reserved",)])
assert SCENE_FIT_DTYPE.itemsize == C.sizeof(SceneFit) == 48 and C.sizeof(SceneLayer) == 24
ALIGN_REC_DTYPE = _np.dtype([("iterations", "<u4"), ("status", "<u4"), ("pairs", "<u4"), ("facing_pts", "<u4"), ("sum_r2", "<i8"),
                             ("pairs0", "<u4"), ("_reserved", "<u4"), ("sum_r2_0", "<i8")])
assert ALIGN_REC_DTYPE.itemsize == C.sizeof(AlignRec) == 40 and C.sizeof(AlignParams) == 32
# se3tn_scene_align_rec: the same 40 bytes with the word at offset 28 in use (hidden_pts)
SCENE_ALIGN_REC_DTYPE = _np.dtype([(k if k != "_reserved" else "hidden_pts", ALIGN_REC_DTYPE.fields[k][0]) for k in ALIGN_REC_DTYPE.names])
assert SCENE_ALIGN_REC_DTYPE.itemsize == C.sizeof(SceneAlignRec) == 40 and SCENE_ALIGN_REC_DTYPE.fields["hidden_pts"][1] == 28


_SIGS = {
    "se3tn_version": (C.c_char_p, []),
    "se3tn_last_error": (C.c_char_p, []),
    "se3tn_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "se3tn_destroy": (None, [C.c_void_p]),
    "se3tn_max_batch": (C.c_int, [C.c_void_p]),
    "se3tn_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "se3tn_split_weights_bytes": (C.c_size_t, [C.c_void_p]),
    "se3tn_split_weights_device": (C.c_void_p, [C.c_void_p]),
    "se3tn_split_weights_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "se3tn_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "se3tn_pack_weights": (C.c_int, [C.c_void_p]),
    "se3tn_packed_bytes": (C.c_size_t, [C.c_void_p]),
    "se3tn_packed_host": (C.c_void_p, [C.c_void_p]),
    "se3tn_upload_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "se3tn_bind_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "se3tn_set_normalization": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "se3tn_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_set_offset_rule": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_get_offset_rule": (C.c_int, [C.c_void_p]),
    "se3tn_set_small_kernels": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_get_small_kernels": (C.c_int, [C.c_void_p]),
    "se3tn_set_raster_rule": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_get_raster_rule": (C.c_int, [C.c_void_p]),
    "se3tn_set_winograd": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "se3tn_get_winograd": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "se3tn_set_trunk_winograd": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "se3tn_get_trunk_winograd": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "se3tn_overflow": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "se3tn_keep_intermediates": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_set_normalizers": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "se3tn_preprocess": (C.c_int, [C.c_void_p, C.POINTER(Crop), C.c_int, C.c_void_p, C.c_void_p]),
    "se3tn_crop_raw": (C.c_int, [C.c_void_p, C.POINTER(Crop), C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_input_buffer": (C.c_void_p, [C.c_void_p, C.c_int]),
    "se3tn_infer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_enable_graphs": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_get_feature": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "se3tn_logits": (C.c_void_p, [C.c_void_p]),
    "se3tn_mesh_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                    C.POINTER(C.c_void_p)]),
    "se3tn_mesh_destroy": (None, [C.c_void_p]),
    "se3tn_mesh_set_texture": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "se3tn_render_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_render_frame_rect": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int,
                                          C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_mesh_set_route": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_mesh_get_route": (C.c_int, [C.c_void_p]),
    "se3tn_frame_rect": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "se3tn_on_track": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                 C.POINTER(C.c_int32), C.c_void_p]),
    "se3tn_on_track_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_on_track_objects": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Object), C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_render": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_fill_depth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "se3tn_fill_depth_rect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                        C.c_void_p, C.c_void_p]),
    "se3tn_fill_depth_rects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p]),
    "se3tn_on_track_objects_live": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Object), C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_on_track_live": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p]),
    "se3tn_fit_stats": (C.c_int, [C.c_void_p, C.POINTER(Crop), C.POINTER(Crop), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "se3tn_set_fit_check": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_get_fit_check": (C.c_int, [C.c_void_p]),
    "se3tn_last_fit": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "se3tn_last_fit_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "se3tn_color_stats": (C.c_int, [C.c_void_p, C.POINTER(Crop), C.POINTER(Crop), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_color_stats_scene": (C.c_int, [C.c_void_p, C.POINTER(Crop), C.POINTER(Crop), C.POINTER(Crop), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "se3tn_color_score": (C.c_double, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "se3tn_verify_poses_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_verify_poses_scene_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_scene_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SceneLayer), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "se3tn_scene_fit": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Object), C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_scene_fit_host": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Object), C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_points_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "se3tn_points_destroy": (None, [C.c_void_p]),
    "se3tn_points_count": (C.c_int, [C.c_void_p]),
    "se3tn_pose_errors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_pose_errors_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_score_poses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int,
                                    C.c_void_p, C.c_void_p]),
    "se3tn_rank_poses": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "se3tn_search_poses_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double),
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_points_set_normals": (C.c_int, [C.c_void_p, C.c_void_p]),
    "se3tn_points_has_normals": (C.c_int, [C.c_void_p]),
    "se3tn_score_pose_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.POINTER(C.c_double), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "se3tn_search_pose_grid_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                              C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_score_pose_grid_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "se3tn_search_pose_grid_scene_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                    C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Object), C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_last_search_scene": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "se3tn_align_poses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double),
                                    C.POINTER(AlignParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_align_poses_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double),
                                         C.POINTER(AlignParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_align_poses_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(AlignParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se3tn_align_poses_scene_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.POINTER(C.c_double), C.POINTER(AlignParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "se3tn_compute_bbox": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                     C.POINTER(C.c_int32)]),
    "se3tn_pose_update_host": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "se3tn_debug_buffer": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "se3tn_memcpy_d2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "se3tn_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "se3tn_profile_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int),
                                     C.POINTER(C.c_float)]),
    "se3tn_profile_launches": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_float)]),
}

_lib = None


def load():
    """Load the HIP library (once).  torch is imported first so that the process keeps a single
    HIP runtime: torch's bundled libamdhip64.so.7 has the same SONAME as /opt/rocm's and the
    dynamic loader reuses the already-loaded one for our NEEDED entry."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            "HIP extension %s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C %s/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % (LIB_PATH, _HERE))
    import torch  # noqa: F401  (loads the HIP runtime this library must share)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError = header/library drift: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return sorted(_SIGS)


def check(rc, what=""):
    if rc != 0:
        msg = load().se3tn_last_error().decode()
        raise Se3tnError("%s failed (rc=%d): %s" % (what or "se3tn call", rc, msg))
