"""Seeded synthetic inputs shared by oracle/make_golden.py, tests/ and bench.py
(TEST INFRASTRUCTURE ONLY).  numpy's PCG64 and torch's CPU mt19937 streams are
platform-independent, so the GPU box regenerates exactly what the goldens were made from;
every golden file also stores fingerprints of its inputs to detect generator drift."""
import hashlib

import numpy as np

# dataset_info.yml:4-7
K_YCB = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])
DATASET_INFO = {
    "camera": {"height": 480, "width": 640, "focalX": 1066.778, "focalY": 1067.487,
               "centerX": 312.9869, "centerY": 241.3109},
    "resolution": 176, "boundingbox": 10, "object_width": 250.0,
}


def sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def synthetic_frame(seed, H=480, W=640):
    """rgb u8 [H,W,3], depth u16 [H,W] in mm with holes (0), near (<=100) and far (>=2000)."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = rng.integers(500, 1200, (H, W)).astype(np.uint16)
    sel = rng.random((H, W))
    depth[sel < 0.05] = 0
    depth[(sel >= 0.05) & (sel < 0.07)] = rng.integers(1, 101, int(((sel >= 0.05) & (sel < 0.07)).sum()))
    depth[(sel >= 0.07) & (sel < 0.10)] = rng.integers(2000, 5000, int(((sel >= 0.07) & (sel < 0.10)).sum()))
    return rgb, depth


def structured_frame(seed, H=480, W=640):
    """Camera frame with image structure (low-frequency colour fields, per-frame gain / offset / noise level, a tilted depth
    plane with bumps and holes): unlike synthetic_frame's i.i.d. noise, the network's pooled features -- and so its
    (trans, rot) output -- differ from frame to frame and with the crop window (oracle/closed_loop.py)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rgb = np.zeros((H, W, 3))
    for c in range(3):
        f = np.zeros((H, W))
        for _ in range(4):
            fx, fy = rng.uniform(-0.04, 0.04, 2)
            f += rng.uniform(0.3, 1.0) * np.sin(fx * xx + fy * yy + rng.uniform(0, 2 * np.pi))
        rgb[..., c] = f
    rgb = (rgb - rgb.min()) / (rgb.max() - rgb.min())
    gain = rng.uniform(80, 255)
    rgb = rgb * gain + rng.uniform(0, 255 - gain) + rng.normal(0, rng.uniform(2, 25), (H, W, 3))
    rgb = np.clip(rgb, 0, 255).astype(np.uint8)
    d = rng.uniform(600, 1000) + rng.uniform(-0.4, 0.4) * (xx - W / 2) + rng.uniform(-0.4, 0.4) * (yy - H / 2)
    for _ in range(5):
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(30, 120)
        d -= rng.uniform(50, 250) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))
    d += rng.normal(0, 3, (H, W))
    depth = np.clip(d, 300, 2500).astype(np.uint16)
    depth[rng.random((H, W)) < 0.04] = 0
    return rgb, depth


def synthetic_render(seed, z_m, res=176):
    """Stand-in for Tracker.render_window (predict.py:193-215): rgbA u8 [res,res,3],
    depthA u16 [res,res] mm, background exactly 0, object a disc around depth z."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:res, 0:res]
    obj = (yy - res / 2) ** 2 + (xx - res / 2) ** 2 < (0.38 * res) ** 2
    rgb = rng.integers(0, 256, (res, res, 3), dtype=np.uint8) * obj[..., None].astype(np.uint8)
    depth = (z_m * 1000 + rng.integers(-60, 60, (res, res))).astype(np.uint16) * obj.astype(np.uint16)
    return rgb, depth


def mean_std(seed):
    """mean.npy / std.npy surface: float64 [8] = A(R,G,B,D) then B(R,G,B,D)
    (predict.py:657-658, train.py:114-125)."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(50, 150, 8)
    std = rng.uniform(10, 60, 8)
    return mean, std


def pose(seed, t=(0.05, -0.02, 0.8)):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    P = np.eye(4)
    P[:3, :3] = Rotation.from_rotvec(rng.normal(0, 0.6, 3)).as_matrix()
    P[:3, 3] = t
    return P


def net_inputs(seed, n, scale=1.0, res=176):
    import torch                                   # lazily: the renderer fixtures also run under an interpreter without torch
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((n, 4, res, res), generator=g) * scale
    B = torch.randn((n, 4, res, res), generator=g) * scale
    return A, B


def depth_frame_with_holes(seed, H=120, W=160, hole_frac=0.25):
    """uint16 mm depth with holes: random blobs of zeros, a few near (<100 mm) and far (> 2 m) pixels, a large empty corner
    (fill_depth fixtures: tests/test_fill_depth.py, oracle/pin_opencv.py)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (700 + 150 * np.sin(xx / 17.0) + 100 * np.cos(yy / 11.0) + rng.integers(-8, 9, (H, W))).astype(np.float64)
    holes = rng.random((H, W)) < hole_frac * 0.3
    for _ in range(12):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(2, 9)
        holes |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    d[holes] = 0
    d[rng.random((H, W)) < 0.01] = rng.integers(1, 100)
    d[rng.random((H, W)) < 0.01] = rng.integers(2100, 4000)
    d[: H // 6, : W // 5] = 0                      # a large empty corner (reaches the image border)
    return d.astype(np.uint16)


def depth_frame_with_far_wall(seed):
    """+ a 40 x 60 region at 2.5-3 m (beyond max_depth = 2 m), larger than every structuring element of fill_depth."""
    mm = depth_frame_with_holes(seed, 240, 320)
    rng = np.random.default_rng(seed)
    mm[100:140, 200:260] = rng.integers(2500, 3000, (40, 60))
    return mm


# ---- depth frames built to reach the branches of the fill chain that smooth mid-range surfaces never reach --------------------
# (tests/test_fill_depth_hard_frames_oracle.py proves on the CPU that each family reaches the branch it names;
#  tests/test_gpu_fill_depth_hard_frames.py holds the HIP kernels to the oracle on them)
def _speckle(mm, rng, frac):
    """isolated zero pixels, none within 3 of another (the 7 x 7 fill closes each of them)"""
    H, W = mm.shape
    for _ in range(max(1, int(frac * H * W))):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        if (mm[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] > 0).all():
            mm[y, x] = 0
    return mm


def depth_frame_thresholds(max_depth=2.0, seed=0, H=24):
    """The two `> 0.1` comparisons of fill_depth, before and after the inversion max_depth - d: vertical bands 12 pixels wide of
    holes | 99 | 100 | 101 mm | a mid-range surface | far - 101 | far - 100 | far - 99 (far = max_depth in mm) | 98..102 and
    far - 102..far - 98 per pixel | a surface beyond max_depth (negative once inverted) | the mid-range surface again."""
    rng = np.random.default_rng(seed)
    far = int(round(max_depth * 1000))
    mid = far // 2
    B = 12
    surf = lambda: mid + rng.integers(-40, 41, (H, B))
    bands = [np.zeros((H, B)), np.full((H, B), 99), np.full((H, B), 100), np.full((H, B), 101), surf(),
             np.full((H, B), far - 101), np.full((H, B), far - 100), np.full((H, B), far - 99),
             rng.integers(98, 103, (H, B)), far - rng.integers(98, 103, (H, B)), far + rng.integers(300, 900, (H, B)), surf()]
    return np.concatenate(bands, 1).astype(np.uint16)


def depth_frame_constant(seed=0, H=20, W=30, level=700):
    """one flat surface with isolated holes: constant after the median, the bilateral filter's copy-through branch"""
    return _speckle(np.full((H, W), level, np.uint16), np.random.default_rng(seed), 0.03)


def depth_frame_near_constant(seed=0, H=20, W=30, level=700):
    """two flat halves one millimetre apart: the smallest range above FLT_EPSILON that a uint16 frame can have after the median.
    Every tap across the step indexes the LAST bins of the bilateral table (idx = BIL_BINS)."""
    mm = np.full((H, W), level, np.uint16)
    mm[:, W // 2:] = level + 1
    return _speckle(mm, np.random.default_rng(seed), 0.03)


def depth_frame_huge_range(seed=0, H=40, W=56):
    """a block of 65535 (inverted: about -63.5 m, larger than every structuring element, so its core stays) inside a near surface
    with holes and, against the block, a patch at 101 mm (the largest inverted value there is): the bilateral table's scale_index is about 63 bins per metre, the table underflows to zeros
    and the taps across the block's rim index its last bins"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    d = 600 + 150 * np.sin(xx / 9.0) + 100 * np.cos(yy / 7.0) + rng.integers(-8, 9, (H, W))
    d[rng.random((H, W)) < 0.08] = 0
    d[10:30, 18:40] = 65535
    d[12:22, 40:48] = 101                          # touches the block: the image's max next to its min
    d[32:, :6] = 0
    return d.astype(np.uint16)


def depth_frame_columns(seed=0, H=20, W=257):
    """fd_extrapolate_kernel's columns, in seven segments of W // 7 columns (the last takes the rest, so that at W = 257 the second
    workgroup's only column has a top of its own):
      0 a surface that reaches row 0 | 1 NO valid pixel: 100 mm (exactly 0.1, neither valid nor empty) over zeros |
      2 a surface in the lower half only | 3 NO valid pixel: zeros over a band beyond max_depth |
      4 the only valid pixels in the LAST row | 5, 6 a surface that starts at row 6 + x % 12, with holes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    surf = 700 + 120 * np.sin(xx / 13.0) + 60 * np.cos(yy / 5.0) + rng.integers(-8, 9, (H, W))
    seg = np.minimum(xx // max(W // 7, 1), 6)
    d = np.zeros((H, W))
    d[seg == 0] = surf[seg == 0]
    d[(seg == 1) & (yy < H // 3)] = 100
    m = (seg == 2) & (yy >= H // 2); d[m] = surf[m]
    d[(seg == 3) & (yy >= H // 2) & (yy < H // 2 + 3)] = 2600
    m = (seg == 4) & (yy == H - 1); d[m] = surf[m]
    m = (seg >= 5) & (yy >= 6 + xx % 12) & (rng.random((H, W)) > 0.1); d[m] = surf[m]
    if H > 31:                                     # a hole that only the 31 x 31 fill behind the extrapolation closes
        d[H // 2:H // 2 + 16, W // 6:W // 6 + 16] = 0
    return d.astype(np.uint16)


def depth_frame_geometry(H, W, seed=0):
    """any size from 1 x 1 up: a stepped surface with noise, holes, an empty first pixel (frames of four pixels and more) and a
    valid last one.  A strip (one or two pixels across, six or more long) starts with five holes, then 700 and 640 mm: the 7-wide
    fill closes the holes with 700, 640, 640, the median keeps a step two pixels from the end of the strip, and the taps the blurs
    reflect there read another value than the end pixel (a strip of five or fewer is flat by the time it is blurred)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    d = 600 + 20 * ((xx * 7 + yy * 13) % 11) + rng.integers(-8, 9, (H, W))
    d[rng.random((H, W)) < 0.15] = 0
    if min(H, W) <= 2 and max(H, W) >= 7:
        head = np.array([0, 0, 0, 0, 0, 700, 640])
        if W >= H:
            d[:, :7] = head[None, :]
        else:
            d[:7, :] = head[:, None]
    if H * W >= 4:
        d[0, 0] = 0
    d[H - 1, W - 1] = 640
    return d.astype(np.uint16)


def depth_frame_plateaus(seed=0, H=40, W=60):
    """terraces of three flat levels with curved edges, a hole too large to be filled and small ones: after the fill the 25 taps of
    the median hold two or three distinct values, and along the edges the 13th smallest sits on a step"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ph = rng.random(4) * 6.28
    f = np.sin(xx / 6.0 + ph[0]) + np.sin(yy / 5.0 + ph[1]) + np.sin((xx + yy) / 7.0 + ph[2]) + np.sin((xx - yy) / 9.0 + ph[3])
    d = np.where(f < -0.7, 600, np.where(f < 0.7, 800, 1000)).astype(np.float64)
    d[(yy - H // 2) ** 2 + (xx - W // 3) ** 2 < 81] = 0
    d[rng.random((H, W)) < 0.1] = 0
    return d.astype(np.uint16)


def icosphere(subdiv=2, radius=0.05, seed=0):
    """Test mesh: subdivided icosahedron, outward (CCW) faces, random vertex colours, analytic normals."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = (v[a] + v[b]) / 2
                v.append(m / np.linalg.norm(m)); cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v)
    rng = np.random.default_rng(seed)
    return dict(vertices=(v * radius).astype(np.float32), faces=np.array(f, np.int32),
                colors=rng.integers(40, 256, (len(v), 3)).astype(np.float64), normals=v.copy())


def textured_sphere(subdiv=2, radius=0.05, tex_hw=(64, 128)):
    """icosphere with spherical texture coordinates and a synthetic RGB texture (ramps + checker + white speckles): the mesh of the
    pyrender-route tests (tests/test_renderer.py, tests/test_gl_swiftshader.py).  Returns dict(vertices f64, faces, uv, texture u8, kd)."""
    m = icosphere(subdiv, radius, 3)
    v = m["vertices"].astype(np.float64)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    uv = np.stack([0.5 + np.arctan2(n[:, 1], n[:, 0]) / (2 * np.pi), 0.5 + np.arcsin(np.clip(n[:, 2], -1, 1)) / np.pi], 1)
    rng = np.random.default_rng(9)
    th, tw = tex_hw
    yy, xx = np.mgrid[0:th, 0:tw]
    tex = np.stack([(xx * 255 // (tw - 1)), (yy * 255 // (th - 1)), ((xx // 8 + yy // 8) % 2) * 200 + 30], -1).astype(np.uint8)
    tex[rng.random((th, tw)) < 0.05] = (255, 255, 255)
    return dict(vertices=v, faces=m["faces"], uv=uv, texture=tex, kd=np.array([0.9, 1.0, 0.8]), colors=m["colors"])


# ---- triangle soups: the geometry a closed, convex, well-conditioned sphere never shows the rasteriser ----------------------------
# (tests/test_raster_soups_oracle.py holds the oracle to itself and to the live GL library on them and proves each family reaches
# the path it names; tests/test_gpu_raster_soups.py holds the HIP kernels to the oracle.)  Every triangle has its OWN three
# vertices (faces = arange), so colours and normals differ per triangle and a wrong owner shows in rgb; normals point anywhere,
# so max(ndl, 0) of the window shader takes both branches.  The soups are modelled around the object origin and seen under
# soup_poses(family): a pure translation (the pose the lattice is back-projected for) and a rotated pose at the same place.
SOUP_FAMILIES = ("small", "big", "near", "far", "lattice", "ties")
SOUP_WIDTH = 150.0                       # object_width (mm): the 176 x 176 window spans +-75 mm at the object's depth
SOUP_T = dict(small=(0.02, -0.01, 0.5), big=(0.02, -0.01, 0.5), near=(0.01, 0.005, 0.14), far=(-0.01, 0.02, 1.95),
              lattice=(0.02, -0.01, 0.5), ties=(0.02, -0.01, 0.5))
# |w| (= camera z) of every vertex stays above this under every pose of its family.  The rasteriser gives up on a window
# coordinate at |Xf| >= 1e9 (csrc/raster.hip), oracle/ss_rules.project at 2^30: nothing pins either value to the live library, so
# the soups stay far below both (tests/test_raster_soups_oracle.py asserts |X|, |Y| < 2^24).
SOUP_MIN_W = 4e-3
SOUP_POSE_SEED = dict(small=20, big=21, near=31, far=22, ties=25)       # of the rotated pose


def gl_window(P, K, width):
    """left, top, right, bottom of the render window (predict.py:201-207: compute_bbox in the y-flipped GL image)"""
    x, y, z = P[0, 3] * 1000, P[1, 3] * -1000, P[2, 3] * 1000
    u = np.round(np.array([x - width / 2, x + width / 2]) * K[0, 0] / z + K[0, 2]).astype(np.int32)
    v = np.round(np.array([y - width / 2, y + width / 2]) * K[1, 1] / z + K[1, 2]).astype(np.int32)
    return (int(u.min()), int(v.min()), int(u.max()), int(v.max()))


def soup_poses(family):
    P0 = np.eye(4)
    P0[:3, 3] = SOUP_T[family]
    if family == "lattice":                      # the grid alignment exists under the pose it was back-projected for only
        return [P0]
    return [P0, pose(SOUP_POSE_SEED[family], SOUP_T[family])]


def _window_to_object(g, z, P, K, win, size=176):
    """object coordinates (float64) of the points that the window render under the pure translation P shows at window position g
    [..., 2] (pixels; pixel i's centre is i + 0.5; GL rows, bottom-up) and camera depth z [...]"""
    left, top, right, bottom = win
    u = left + g[..., 0] * (right - left) / float(size)
    vf = top + g[..., 1] * (bottom - top) / float(size)
    cam = np.stack([(u - K[0, 2]) * z / K[0, 0], (K[1, 2] - vf) * z / K[1, 1], z], -1)
    return cam - P[:3, 3]


def _soup_pack(tris, rng, faces=None):
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    n = len(tris)
    nrm = rng.normal(0, 1, (3 * n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(vertices=tris.reshape(-1, 3).astype(np.float32), faces=(np.arange(3 * n).reshape(n, 3) if faces is None else faces).astype(np.int32),
                colors=rng.integers(40, 256, (3 * n, 3)).astype(np.uint8), normals=nrm.astype(np.float32))


def _random_tris(rng, n, spread, size):
    """n triangles: centres uniform in +-spread (x, y, z), vertices uniform in +-size around them (size: scalar, [3] or [n,1,1])"""
    c = rng.uniform(-1, 1, (n, 3)) * np.asarray(spread, np.float64)
    return c[:, None, :] + rng.uniform(-1, 1, (n, 3, 3)) * size


def _off_the_camera_plane(m, poses, rng):
    """moves the (few) vertices whose camera z comes closer to 0 than SOUP_MIN_W under one of the poses"""
    v = m["vertices"]
    for _ in range(50):
        bad = np.zeros(len(v), bool)
        for P in poses:
            bad |= np.abs(v.astype(np.float64) @ P[2, :3] + P[2, 3]) < 1.5 * SOUP_MIN_W
        if not bad.any():
            return m
        v[bad] += rng.normal(0, 0.01, (int(bad.sum()), 3)).astype(np.float32)
    raise AssertionError("soup vertices stay on the camera plane")


def soup(family, seed=0):
    """dict(vertices float32 [3n,3], faces int32 [n,3], colors uint8 [3n,3], normals float32 [3n,3]) of one family:
      small    ~400 triangles with edges of 2-15 window pixels, random winding, heavily overlapping in depth; mixed in: faces that
               repeat a vertex index, collinear vertices, triangles smaller than a pixel laid between the pixel centres, slivers over
               100 pixels long and under 1/16 pixel wide
      big      40 triangles with edges of 50-150 pixels (bounding boxes beyond the rasteriser's RASTER_BIG_PX), some across the window's edges
      near     triangles across the near plane (0.1 m) and the camera plane: one, two and three vertices with w < 0
      far      triangles across the far plane (2 m), and very large ones that the near, the far and two or more side planes cut at once
      lattice  vertices back-projected (float64) from the half-pixel grid of the window at varying depth: after the float32 projection
               they snap onto it exactly, so pixel centres lie ON edges and vertices; fans around one point, pairs on one edge
      ties     exact copies of triangles (own vertices, other colours) later and earlier in draw order, copies with permuted vertex
               order (the same plane through another anchor vertex), overlapping triangles in one plane z = const of the camera (equal
               w on three vertices) and with equal w on two vertices"""
    rng = np.random.default_rng(1000 + 17 * SOUP_FAMILIES.index(family) + seed)
    poses = soup_poses(family)
    P0, T = poses[0], np.asarray(SOUP_T[family])
    win = gl_window(P0, K_YCB, SOUP_WIDTH)
    if family == "small":
        tris = [_random_tris(rng, 380, (0.05, 0.05, 0.05), rng.uniform(0.002, 0.0085, (380, 1, 1)))]
        a, b = _random_tris(rng, 5, (0.05, 0.05, 0.03), 0.01)[:, :2].transpose(1, 0, 2)
        tris.append(np.stack([a, b, a + rng.uniform(0.2, 0.8, (5, 1)) * (b - a)], 1))                 # collinear
        g = rng.integers(20, 156, (6, 1, 2)) + rng.uniform(-0.2, 0.2, (6, 3, 2))                       # around pixel CORNERS: no centre inside
        tris.append(_window_to_object(g, np.repeat(rng.uniform(0.42, 0.5, (6, 1)), 3, 1), P0, K_YCB, win))
        a = _random_tris(rng, 4, (0.02, 0.02, 0.03), 0.0)[:, 0]
        d = rng.normal(0, 1, (4, 3)) * (1, 1, 0.2)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        b = a + 0.1 * d                                                                                # 117 pixels long ...
        c = (a + b) / 2 + 2e-5 * np.stack([-d[:, 1], d[:, 0], 0 * d[:, 0]], 1)                         # ... 0.02 pixel wide
        tris.append(np.stack([a, b, c], 1))
        tris.append(_random_tris(rng, 5, (0.05, 0.05, 0.03), 0.006))                                   # faces (i, i, j) below
        m = _soup_pack(np.concatenate(tris), rng)
        m["faces"][-5:, 1] = m["faces"][-5:, 0]
    elif family == "big":
        m = _soup_pack(np.concatenate([_random_tris(rng, 28, (0.02, 0.02, 0.04), (0.045, 0.045, 0.03)),
                                       _random_tris(rng, 12, (0.07, 0.07, 0.04), (0.05, 0.05, 0.03))]), rng)
    elif family == "near":
        tris = [_random_tris(rng, 90, (0.03, 0.03, 0.1), 0.05)]
        for k in (1, 2, 3):                                                                            # k vertices behind the camera
            t = rng.uniform(-1, 1, (8, 3, 3)) * (0.05, 0.05, 0)
            zc = rng.uniform(0.12, 0.35, (8, 3))
            zc[:, :k] = rng.uniform(-0.2, -0.01, (8, k))
            t[..., 2] = zc - T[2]
            tris.append(t[:, rng.permutation(3)])
        m = _soup_pack(np.concatenate(tris), rng)
    elif family == "far":
        tris = [_random_tris(rng, 50, (0.05, 0.05, 0.1), (0.04, 0.04, 0.15)),
                _random_tris(rng, 20, (0.05, 0.05, 0.004), (0.03, 0.03, 0.012)) + (0, 0, 2.0 - T[2])]     # steep and gentle
        # from before the near plane to beyond the far one, in a plane that all but holds the camera centre, n . (x, y) = a z + b
        # (x, y measured from the ray through the window's centre):
        # the window shows it as a diagonal band between the line where the near plane cuts it and the line where the far plane does,
        # its ends cut off by the window's sides -- near, far and two to four side planes on one triangle
        t = np.zeros((4, 3, 3))
        for i, (deg, a, b) in enumerate([(45, -0.008, 0.002), (135, 0.007, -0.0018), (45, 0.006, -0.0018), (135, -0.009, 0.0022)]):
            n_ = np.array([np.cos(np.radians(deg)), np.sin(np.radians(deg))])
            for k, (z, l) in enumerate([(0.05, rng.uniform(-0.002, 0.002)), (rng.uniform(2.3, 2.6), -0.6), (rng.uniform(2.3, 2.6), 0.6)]):
                t[i, k] = np.r_[(a * z + b) * n_ + l * np.array([-n_[1], n_[0]]) + z * T[:2] / T[2], z]
            if i % 2:
                t[i] = t[i, ::-1]
        tris.append(t - T)
        m = _soup_pack(np.concatenate(tris), rng)
    elif family == "lattice":
        half = lambda lo, hi, shape: rng.integers(2 * lo, 2 * hi + 1, shape) / 2.0                      # the half-pixel grid
        pts, zs = [], []
        g = half(10, 166, (60, 3, 2))                                                                  # large
        pts.append(g); zs.append(rng.uniform(0.35, 0.65, (60, 3)))
        g = half(20, 156, (80, 1, 2)) + half(-8, 8, (80, 3, 2))                                        # small
        pts.append(g); zs.append(rng.uniform(0.35, 0.65, (80, 3)))
        for _ in range(5):                                                                             # fans around a pixel centre
            hub, hz = rng.integers(30, 146, 2) + 0.5, rng.uniform(0.4, 0.6)
            ang = np.sort(rng.uniform(0, 2 * np.pi, 6))
            ring = hub + np.round(2 * rng.uniform(6, 20, (6, 1)) * np.stack([np.cos(ang), np.sin(ang)], 1)) / 2.0
            rz = rng.uniform(0.4, 0.6, 6)
            for i in range(6):
                j = (i + 1) % 6
                pts.append(np.stack([hub, ring[i], ring[j]])[None]); zs.append(np.array([[hz, rz[i], rz[j]]]))
        for _ in range(15):                                                                            # (a, b, c) and (a, b, d): one edge, two windings
            q, qz = half(20, 156, (1, 2)) + half(-15, 15, (4, 2)), rng.uniform(0.4, 0.6, 4)
            pts.append(q[[0, 1, 2]][None]); zs.append(qz[[0, 1, 2]][None])
            pts.append(q[[0, 1, 3]][None]); zs.append(qz[[0, 1, 3]][None])
        g, z = np.concatenate(pts), np.concatenate(zs)
        m = _soup_pack(_window_to_object(g, z, P0, K_YCB, win), rng)
    elif family == "ties":
        base = _random_tris(rng, 60, (0.05, 0.05, 0.04), 0.015)
        flat = _random_tris(rng, 20, (0.03, 0.03, 0.0), (0.03, 0.03, 0.0))
        flat[..., 2] = 0.47 - T[2]                                                                     # one plane of the camera: w equal on all three
        two = _random_tris(rng, 15, (0.05, 0.05, 0.03), 0.02)
        two[:, :2, 2] = 0.45 - T[2]                                                                    # ... on two
        two = np.stack([two[i][rng.permutation(3)] for i in range(15)])
        perms = [[1, 2, 0], [2, 0, 1], [0, 2, 1], [1, 0, 2], [2, 1, 0]]
        permuted = np.stack([base[30 + i][perms[i % 5]] for i in range(15)])
        m = _soup_pack(np.concatenate([base[15:30], base, flat, two, base[0:15], permuted]), rng)      # copies drawn earlier | ... | later
    else:
        raise ValueError(family)
    return _off_the_camera_plane(m, poses, rng)


SOUP_FRAME_HW = (120, 160)
SOUP_FRAME_K = np.array([[266.7, 0, 78.2], [0, 266.9, 60.3], [0, 0, 1.0]])       # the small camera of tests/test_renderer.py


def soup_frame(seed=0):
    """The soup of the full-frame route's tests: 90 triangles spread over the edges of the SOUP_FRAME_HW frame and the near plane under
    soup_frame_pose(), with a planar texture map (affine in the vertex position, reaching outside [0, 1]: REPEAT wraps) and
    textured_sphere's texture.  colors as the window soups'; kd for both the textured and the vertex-colour mesh."""
    rng = np.random.default_rng(2000 + seed)
    m = _off_the_camera_plane(_soup_pack(_random_tris(rng, 90, (0.12, 0.1, 0.25), 0.06), rng), [soup_frame_pose()], rng)
    v = m["vertices"].astype(np.float64)
    m["uv"] = np.stack([0.5 + 3.0 * v[:, 0] + 1.0 * v[:, 1], 0.4 - 1.5 * v[:, 0] + 3.5 * v[:, 1] + 1.0 * v[:, 2]], 1)
    m["texture"] = textured_sphere(0)["texture"]
    m["kd"] = np.array([0.9, 1.0, 0.8])
    return m


def soup_frame_pose():
    return pose(4, (0.01, -0.02, 0.28))


# ---- large frames: where the rasteriser's float32 set-up arithmetic stops being exact --------------------------------------------------
# (tests/test_raster_large_frames_oracle.py proves on the CPU what the two soups reach at these sizes and holds the rules to the live GL
# library on them; tests/test_gpu_raster_large_frames.py holds the HIP kernels to the rules.)  (H, W): the size include/se3tracknet.h
# names; the row limit and the 2^21-pixel limit at once; the row limit in a cheap frame.
LARGE_FRAMES = [(1080, 1920), (2048, 1024), (2048, 96)]
SLIVER_Z = (0.2, 1.8, 1.9)               # camera depth (m) of the nearest and the farthest sliver band, and of the backdrop
SLIVER_LATTICE = 12                      # near-collinear lattice triangles per sliver soup
SLIVER_MARGIN = 2.0                      # pixels between every sliver vertex and the frame's edge


def large_frame_K(hw):
    """SOUP_FRAME_K scaled to an H x W frame: the frame soup keeps its layout across every edge and the near plane under soup_frame_pose()"""
    K = SOUP_FRAME_K.copy()
    K[0] *= hw[1] / float(SOUP_FRAME_HW[1])
    K[1] *= hw[0] / float(SOUP_FRAME_HW[0])
    return K


def float_area(X, Y):
    """the sign-deciding sum of oracle/ss_rules.setup_triangle on snapped coordinates X, Y [n,3], in its float32 operation order"""
    x, y = np.asarray(X).astype(np.float32), np.asarray(Y).astype(np.float32)
    return ((y[:, 2] - y[:, 0]) * x[:, 1] + (y[:, 1] - y[:, 2]) * x[:, 0]) + (y[:, 0] - y[:, 1]) * x[:, 2]


def exact_area(X, Y):
    """the same sum in integers"""
    x, y = np.asarray(X).astype(np.int64), np.asarray(Y).astype(np.int64)
    return (y[:, 2] - y[:, 0]) * x[:, 1] + (y[:, 1] - y[:, 2]) * x[:, 0] + (y[:, 0] - y[:, 1]) * x[:, 2]


def _bezout(p, q):
    """(ex, ey) with p ey - q ex = 1 for coprime p, q"""
    r0, r1, s0, s1, t0, t1 = p, q, 1, 0, 0, 1
    while r1:
        k = r0 // r1
        r0, r1, s0, s1, t0, t1 = r1, r0 - k * r1, s1, s0 - k * s1, t1, t0 - k * t1
    assert abs(r0) == 1                                   # s0 p + t0 q = r0
    return -t0 * r0, s0 * r0


def _near_collinear(rng, hw, n, misjudged):
    """n triangles in snapped coordinates (1/16 pixel), two vertices on one lattice line v0 + k (p, q), the third one lattice step e off
    it with p e_y - q e_x = 1: twice the area is the number of steps between the first two, at most 64 units where the products of the
    float32 sum reach 2^30.  Up to `misjudged` of them are chosen so that the float sum is zero or has the wrong sign."""
    H, W = hw
    lo, hi = int(16 * SLIVER_MARGIN), np.array([16 * (W - SLIVER_MARGIN) - 16, 16 * (H - SLIVER_MARGIN) - 16])
    bad, good = [], []
    for _ in range(6000):
        if len(bad) >= misjudged and len(bad) + len(good) >= n:
            break
        p, q = int(rng.integers(50, 8 * W)) * int(rng.choice([-1, 1])), int(rng.integers(50, 8 * H))
        if np.gcd(p, q) != 1:
            continue
        e = np.array(_bezout(p, q))
        assert p * e[1] - q * e[0] == 1
        v0 = rng.integers(lo, hi + 1)
        reach = min(int(min((hi[0] - v0[0]) // p if p > 0 else (v0[0] - lo) // -p, (hi[1] - v0[1]) // q)), 64)
        if reach < 2:
            continue
        m = int(rng.integers(2, reach + 1))
        k = int(rng.integers(0, m + 1))
        tri = np.stack([v0, v0 + m * np.array([p, q]), v0 + k * np.array([p, q]) + int(rng.choice([-1, 1])) * e])[rng.permutation(3)]
        if (tri < lo).any() or (tri > hi).any():
            continue
        fa, ea = float(float_area(tri[None, :, 0], tri[None, :, 1])[0]), int(exact_area(tri[None, :, 0], tri[None, :, 1])[0])
        assert abs(ea) == m
        (bad if (fa == 0 or (fa < 0) != (ea < 0)) else good).append(tri)
    out = bad[:misjudged] + good
    out = (out + bad[misjudged:])[:n]
    assert len(out) == n, "near-collinear lattice triangles"
    return np.array(out)


def soup_slivers(hw, seed=0):
    """The soup that makes the float32 set-up of a triangle inexact at large frames, for the frame hw = (H, W) under large_frame_K(hw)
    and soup_frame_pose(): 480 thin triangles, both windings, three strongly different vertex colours each -- 456 with a long edge of a
    quarter to the whole of the frame's diagonal and a width of 1 to 20 pixels (bounding boxes far above RASTER_BIG_PX: the wave-per-
    triangle path), 24 upright ones, up to 110 pixels long and 1 to 2 wide, in the corner farthest from the window's origin (the
    thread-per-triangle path); SLIVER_LATTICE near-collinear lattice triangles
    (_near_collinear); behind them one backdrop quad.  Everything lies inside the frustum (the unclipped small and big paths).  Every
    triangle has a band of camera depth of its own (sliver_owner_from_depth reads the owner back from a depth buffer).  All vertices
    are chosen in snapped window coordinates and inverted through the projection in float64; the generator asserts with
    oracle/ss_rules.project that the float32 projection snaps the lattice triangles where targeted.  Dict as soup_frame()'s, no texture,
    plus `target` int64 [n,3,2]: the snapped (X, Y) aimed at, `lattice` / `short`: the indices of the near-collinear and of the short
    triangles, `band`: each triangle's depth band."""
    from . import ss_rules as S
    H, W = hw
    rng = np.random.default_rng(5000 + 7 * H + W + seed)
    n_sl, n_short = 480, 24
    lo, hi = np.array([SLIVER_MARGIN, SLIVER_MARGIN]), np.array([W - SLIVER_MARGIN, H - SLIVER_MARGIN])
    diag = float(np.hypot(H, W))
    tris = []
    while len(tris) < n_sl:
        a, b = rng.uniform(lo, hi), rng.uniform(lo, hi)
        L = np.linalg.norm(b - a)
        if not diag / 4 <= L <= diag:
            continue
        nrm = np.array([-(b - a)[1], (b - a)[0]]) / L
        c = a + rng.uniform(0.1, 0.9) * (b - a) + rng.choice([-1, 1]) * rng.uniform(1, 20) * nrm
        if (c < lo).any() or (c > hi).any():
            continue
        tris.append(np.stack([a, b, c])[rng.permutation(3)])
    for k in range(n_short):                             # the last n_short: along an axis and short, a bounding box of under 256 pixels
        ax = 1                                           # upright (the sum's products are row differences times columns), in the corner
                                                         # farthest from the window's origin
        L, wd, t = rng.uniform(0.55, 1.0) * min(110.0, 0.6 * (hi - lo)[ax]), rng.uniform(1.0, 2.0), rng.uniform(0.1, 0.9)
        tri, ext = np.array([[0, 0], [L, 0], [t * L, wd]]), np.array([L + 1, wd + 1])
        if ax:
            tri, ext = tri[:, ::-1], ext[::-1]
        corner = np.array([hi[0], lo[1]])                # (image coordinates: the largest X, and the largest GL Y = the smallest v)
        base = corner + [-1, 1] * (rng.uniform(0, 0.2, 2) * (hi - lo)) - [ext[0], 0]
        tris[n_sl - n_short + k] = (base + tri)[rng.permutation(3)]
    target = np.rint((np.array(tris) - 0.5) * 16).astype(np.int64)                    # pixel i's centre (i + 0.5) is 16 i
    lattice = _near_collinear(rng, hw, SLIVER_LATTICE, 8)
    m_px = SLIVER_MARGIN + 1.3125
    back = np.rint((np.array([[m_px, m_px], [W - m_px, m_px], [W - m_px, H - m_px], [m_px, H - m_px]]) - 0.5) * 16).astype(np.int64)
    order = rng.permutation(n_sl + SLIVER_LATTICE)                                    # draw order; the depth bands follow the index before it
    target = np.concatenate([np.concatenate([target, lattice])[order], back[[0, 1, 2]][None], back[[0, 2, 3]][None]])
    n = len(target)
    band = (SLIVER_Z[1] - SLIVER_Z[0]) / (n_sl + SLIVER_LATTICE)
    z = SLIVER_Z[0] + band * (order[:, None] + rng.uniform(0.0, 0.3, (len(order), 3)))
    is_lat = order >= n_sl
    z[is_lat] = z[is_lat, :1]                            # (a near-collinear triangle's depth plane means nothing: one depth on all three)
    z = np.concatenate([z, np.full((2, 3), SLIVER_Z[2])])
    # snapped window coordinates -> continuous image coordinates (GL rows count bottom-up) -> camera -> object, in float64
    K, P = large_frame_K(hw), soup_frame_pose()
    u, v = target[..., 0] / 16.0 + 0.5, H - (target[..., 1] / 16.0 + 0.5)
    cam = np.stack([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z], -1)
    obj = (cam - P[:3, 3]) @ P[:3, :3]
    m = _soup_pack(obj, rng)
    base = np.array([[250, 30, 30], [30, 250, 30], [30, 30, 250]])
    m["colors"] = np.concatenate([base[rng.permutation(3)] + rng.integers(-25, 6, (3, 3)) for _ in range(n)]).astype(np.uint8)
    m["kd"] = np.array([0.9, 1.0, 0.8])
    m["target"], m["lattice"] = target, np.nonzero(np.r_[is_lat, False, False])[0]
    m["band"] = np.r_[order, n - 2, n - 2].astype(np.int64)
    m["short"] = np.nonzero(np.r_[(order >= n_sl - n_short) & (order < n_sl), False, False])[0]
    pv = S.project(S.clip_positions(m["vertices"], S.frame_pv(P, K, W, H)), W, H)
    got = np.stack([pv["X"], pv["Y"]], -1).reshape(n, 3, 2)
    assert np.array_equal(got[m["lattice"]], target[m["lattice"]]), "the near-collinear triangles snap where targeted"
    assert not pv["flags"].any(), "the sliver soup stays inside the frustum"
    return m


def sliver_owner_from_depth(zbuf, m):
    """the triangle each pixel of a float32 depth buffer (1.0 = cleared) of the sliver soup m shows, read from the depth alone: every
    triangle lies in a band of camera depth of its own (vertex depths fill the lower 30 % of the band).  int32 [H,W], -1 = none; the two
    triangles of the backdrop share one depth and both read as the first of them, len(faces) - 2."""
    n = len(m["faces"])
    zb = np.asarray(zbuf, np.float64)
    near, far = 0.1, 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        cam = 2.0 * near * far / ((far + near) - (2.0 * zb - 1.0) * (far - near))
    band = (SLIVER_Z[1] - SLIVER_Z[0]) / (n - 2)
    k = np.floor((cam - SLIVER_Z[0]) / band + 0.35)
    k = np.where(np.isfinite(k), np.clip(k, -1, n - 2), -1).astype(np.int64)
    of_band = np.full(n, -1, np.int32)                  # band -> triangle; the last entry serves band n - 2 and beyond: the backdrop
    of_band[m["band"][:n - 2]] = np.arange(n - 2)
    of_band[n - 2] = n - 2
    owner = of_band[k]
    owner[~(zb < 1.0)] = -1
    return owner


def soup_composite_poses():
    """two ordinary views and a close-up that puts much of the model before the near plane and some of it behind the camera"""
    return [pose(32, (0.02, -0.01, 0.5)), pose(33, (-0.03, 0.02, 0.62)), pose(34, (0.01, 0.0, 0.16))]


def soup_composite(seed=0):
    """small + big + near in one model (394 triangles): the model of the batched-launch tests, seen under soup_composite_poses()"""
    parts = [soup("small", seed), soup("big", seed), soup("near", seed)]
    take = [250, 30, 114]
    m = {k: np.concatenate([p[k][:3 * n] for p, n in zip(parts, take)]) for k in ("vertices", "colors", "normals")}
    off = np.cumsum([0] + [3 * n for n in take[:-1]])
    m["faces"] = np.concatenate([p["faces"][:n] + o for p, n, o in zip(parts, take, off)]).astype(np.int32)
    return _off_the_camera_plane(m, soup_composite_poses(), np.random.default_rng(3000 + seed))


# ---- textured cards: the hard cases of the full-frame renderer's texture filter ---------------------------------------------------
# (oracle/texture_oracle.py states the filter in float64 with a per-pixel bound; tests/test_texture_filter_oracle.py holds the float32
# oracle and planted faults to it on the CPU, tests/test_gpu_texture_filter.py the HIP kernel.)  A card is a fronto-parallel rectangle
# of the SOUP_FRAME_HW frame, a 2 x 2 grid of quads (8 triangles, each with its own vertices), seen under a pure translation with a
# texture map that is affine in the image position: w is constant, so the level of detail is the same at every pixel and known in
# closed form from the map's Jacobian J (base-level texels per pixel; rows u, v; columns image x, y):
# rho = max(|J[:, 0]|, |J[:, 1]|), lod = clamp(log2 rho).
CARD_T = (0.01, -0.02, 0.4)
# the 3 x 3 grid's columns and rows in continuous image coordinates (pixel i's centre: i + 0.5), on multiples of 1/16 pixel: the
# rasteriser snaps vertices to that grid, so the map below holds at the pixel centres up to float32 rounding, not up to 1/32 pixel
CARD_GRID_X, CARD_GRID_Y = (49.3125, 81.875, 110.6875), (38.625, 57.75, 81.1875)
CARD_RECT = (CARD_GRID_X[0], CARD_GRID_Y[0], CARD_GRID_X[2], CARD_GRID_Y[2])         # left, top, right, bottom
# the image point where u = v = 0.  Generic, so that the real colour does not sit ON a byte boundary (bilinear weights of exactly 1/2
# on both axes make it a multiple of 1/4: every fourth pixel-channel would admit two bytes by construction); the two "edges" cards
# put one axis on the centre of pixel 80 / 60 and leave the other generic
CARD_ORIGIN = (80.37, 60.21)
CARD_ORIGINS = {"edges_u": (80.5, 60.21), "edges_v": (80.37, 60.5)}
FILTER_TEXTURES = ("noise", "noise40x24", "noise5x3", "row1x7", "col7x1", "one", "corners", "channels")
FILTER_KDS = ((0.9, 1.0, 0.8), (0.0, 1.0, 2.5), None)      # the reference's material; zero and saturation; the default
# name -> J, or a function of the texture's level count L (the top level and the clamp above it), or "uv": a map given in uv units
CARDS = {
    "mag4": np.eye(2) * 0.25,                           # magnification, 1/4 texel per pixel: lod clamped at 0 from below
    "lod0": np.eye(2) * 1.0,                            # rho = 1: lod 0 without the clamp (up to rounding)
    "lod0.5": np.eye(2) * 2.0 ** 0.5,
    "lod1": np.eye(2) * 2.0,                            # fl = 0: a pure level
    "lod2": np.eye(2) * 4.0,
    "lod2.37": np.eye(2) * 2.0 ** 2.37,
    "top": lambda L: np.eye(2) * 2.0 ** (L - 1),        # the top level, reached exactly
    "beyond": lambda L: np.eye(2) * 2.0 ** (L + 2),     # 8 x beyond it: lod clamped from above
    "aniso_x": np.diag([4.0, 0.5]),                     # rho is the larger axis, in both orders
    "aniso_y": np.diag([0.5, 4.0]),
    "sheared": np.array([[1.5, 2.0], [-2.5, 0.5]]),     # |J[:, 0]| = 2.92 > |J[:, 1]| = 2.06
    "edges_u": np.eye(2) * 0.5,                         # pixel centres ON texel edges (x = k - 0.5) and centres (x = k), through u = 0
    "edges_v": np.eye(2) * 0.5,                         # the same in v
    "repeats": "uv",                                    # u and v from -3.25 to 2.5 across the card: negative, above 1, several repeats
}


def filter_texture(name):
    """RGB uint8 [th,tw,3] of FILTER_TEXTURES"""
    rng = np.random.default_rng(4000 + FILTER_TEXTURES.index(name))
    noise = lambda th, tw: rng.integers(0, 256, (th, tw, 3), dtype=np.uint8)
    if name == "noise":
        return noise(64, 128)                           # the largest gradients: a one-texel or one-level slip moves bytes by tens
    if name == "noise40x24":
        return noise(40, 24)                            # 40 x 24 -> ... -> 5 x 3 -> 2 x 1: an odd size drops its last row / column
    if name == "noise5x3":
        return noise(5, 3)
    if name == "row1x7":
        return noise(1, 7)                              # one texel high while the width still halves
    if name == "col7x1":
        return noise(7, 1)
    if name == "one":
        return noise(1, 1)
    if name == "corners":                               # black with one lit texel in each corner: a wrap that clamps shows at once
        t = np.zeros((16, 16, 3), np.uint8)             # (white, red, green, blue: four EQUAL corners would look the same wrapped or clamped)
        t[[0, 0, -1, -1], [0, -1, 0, -1]] = [(255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)]
        return t
    if name == "channels":                              # other noise in every channel, in disjoint ranges: a permutation shows
        return np.stack([rng.integers(lo, lo + 80, (32, 32)) for lo in (0, 88, 176)], -1).astype(np.uint8)
    raise ValueError(name)


def _levels_of(th, tw):
    return int(np.floor(np.log2(max(th, tw)))) + 1


def card_jacobian(card, tex_hw):
    """J (base texels per pixel) of card `card` on a th x tw texture, and the closed-form lod"""
    th, tw = tex_hw
    L = _levels_of(th, tw)
    J = CARDS[card]
    if callable(J):
        J = J(L)
    elif isinstance(J, str):
        l, t, r, b = CARD_RECT
        J = np.diag([(2.5 + 3.25) * tw / (r - l), (2.5 + 3.25) * th / (b - t)])
    rho = max(np.hypot(*J[:, 0]), np.hypot(*J[:, 1]))
    return J, float(min(max(np.log2(rho), 0.0), L - 1))


def _card_texels(card, tex_hw, pts):
    """texel coordinates (u tw, v th) of the image points pts [...,2] under the card's map"""
    th, tw = tex_hw
    J, _ = card_jacobian(card, tex_hw)
    if isinstance(CARDS[card], str):
        l, t, r, b = CARD_RECT
        return np.stack([-3.25 * tw + J[0, 0] * (pts[..., 0] - l), -3.25 * th + J[1, 1] * (pts[..., 1] - t)], -1)
    return (pts - np.asarray(CARD_ORIGINS.get(card, CARD_ORIGIN))) @ J.T


def card_allows(card, tex_hw):
    """the range rule: |u w_l|, |v h_l| < 512 at the sampled level l = floor(lod), where the rounding of x = u w_l - 0.5 (an ulp of
    its magnitude, times the texel differences) still leaves most pixels a single admissible byte"""
    l, t, r, b = CARD_RECT
    tex = np.abs(_card_texels(card, tex_hw, np.array([[l, t], [r, t], [l, b], [r, b]])))
    _, lod = card_jacobian(card, tex_hw)
    return bool(tex.max() / 2.0 ** np.floor(lod) < 512)


def card_pose():
    P = np.eye(4)
    P[:3, 3] = CARD_T
    return P


def _card_pack(pts_obj, uv):
    """3 x 3 grid of points -> 8 triangles with their own vertices (both diagonals occur)"""
    quads = [(0, 1, 4, 3), (1, 2, 5, 4), (3, 4, 7, 6), (4, 5, 8, 7)]
    idx = []
    for k, (a, b, c, d) in enumerate(quads):
        idx += [a, b, c, a, c, d] if k % 2 == 0 else [a, b, d, b, c, d]
    idx = np.array(idx)
    n = len(idx)
    return dict(vertices=pts_obj[idx].astype(np.float32), faces=np.arange(n).reshape(-1, 3).astype(np.int32), uv=uv[idx].astype(np.float64),
                colors=np.full((n, 3), 200, np.uint8), normals=np.tile(np.array([0, 0, -1], np.float32), (n, 1)))


def card(name, tex_hw):
    """mesh dict (vertices, faces, uv, colors, normals) of card `name` for a th x tw texture, seen under card_pose() with SOUP_FRAME_K"""
    th, tw = tex_hw
    K, T = SOUP_FRAME_K, np.asarray(CARD_T)
    gx, gy = np.meshgrid(CARD_GRID_X, CARD_GRID_Y)
    pts = np.stack([gx.ravel(), gy.ravel()], 1)
    obj = np.stack([(pts[:, 0] - K[0, 2]) * T[2] / K[0, 0] - T[0], (pts[:, 1] - K[1, 2]) * T[2] / K[1, 1] - T[1], np.zeros(9)], 1)
    return _card_pack(obj, _card_texels(name, tex_hw, pts) / np.array([tw, th], np.float64))


def filter_cases():
    """(card, texture, kd index) of every card on every texture its map allows, under every Kd"""
    return [(c, t, k) for c in CARDS for t in FILTER_TEXTURES if card_allows(c, filter_texture(t).shape[:2]) for k in range(len(FILTER_KDS))]


def card_tilted():
    """A card rotated about both image axes, z from about 0.2 to 0.5 m: the level of detail varies continuously over several
    floor(lod) transitions.  Returns (mesh dict for the 64 x 128 noise texture, pose)."""
    from scipy.spatial.transform import Rotation
    P = np.eye(4)
    P[:3, :3] = Rotation.from_euler("xy", [35, 50], degrees=True).as_matrix()
    P[:3, 3] = (0.0, 0.005, 0.35)
    gx, gy = np.meshgrid([-0.15, 0.01, 0.15], [-0.035, 0.004, 0.035])
    obj = np.stack([gx.ravel(), gy.ravel(), np.zeros(9)], 1)
    uv = np.stack([obj[:, 0] / 0.15 * 1.9 + 0.13, obj[:, 1] / 0.035 * 0.9 + 0.41], 1)
    return _card_pack(obj, uv), P


def soup_horizon():
    """Three triangles in planes that pass within millimetres of the camera centre, from 0.15 m to beyond the far plane: each shows as
    a wedge that ends at the plane's horizon (1 / w = 0) where the far plane cuts it.  The 1 / w plane falls by more than the far
    plane's 0.5 / m within one pixel there, so covered pixels have a quad corner ACROSS w = 0 (extrapolated uv that mean nothing: the
    level of detail must survive them), and the level of detail runs through every level of the 64 x 128 noise texture on the way.
    (soup_frame() has no such pixel.)  Returns (mesh dict, pose)."""
    P = np.eye(4)
    P[:3, 3] = (0.0, 0.0, 0.5)
    tris = []
    for d, ang in ((0.005, 0.0), (-0.004, 0.5), (0.006, -0.9)):              # the plane n . (x, y) = d of the camera
        n = np.array([np.sin(ang), np.cos(ang)])
        along = np.array([n[1], -n[0]])
        tris.append([np.r_[d * n + l * along, z] - P[:3, 3] for z, l in ((0.15, 0.0), (2.6, -0.5), (2.6, 0.5))])
    m = _soup_pack(np.array(tris), np.random.default_rng(2100))
    v = m["vertices"].astype(np.float64)
    m["uv"] = np.stack([0.5 + 1.5 * v[:, 0] + 0.2 * v[:, 2], 0.3 + 1.2 * v[:, 1] + 0.3 * v[:, 2]], 1)
    return m, P
