"""`object_width` derived from a model file (predict.py:131-142): the product's load_model_points -> voxel_down_sample ->
compute_obj_max_width against a SECOND, independent implementation (a dict of voxels filled point by point; the diameter by brute
force over every pair of down-sampled points) on the reference's own object_models/bunny/1.ply (11,159 vertices; stored gzipped as
tests/golden/bunny.ply.gz) and on a fixture mesh.  trimesh.load / open3d themselves are absent offline: oracle/pin_open3d.py turns this
restated rule into a pinned one on first contact (tests/test_pinned_third_party.py)."""
import os

import numpy as np
import pytest

from oracle import fixtures as Fx

BUNNY_GZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bunny.ply.gz")


@pytest.fixture(scope="module")
def U():
    import importlib
    return importlib.import_module("iros20-6d-pose-tracking_amd.utils")


def _voxels_by_dict(points, voxel=0.005):
    """open3d's documented rule, written the slow way: voxel index = floor((p - (min_bound - voxel / 2)) / voxel), mean per voxel"""
    pts = np.asarray(points, np.float64)
    origin = pts.min(0) - 0.5 * voxel
    cells = {}
    for p in pts:
        key = tuple(int(np.floor(v)) for v in (p - origin) / voxel)
        acc = cells.setdefault(key, [np.zeros(3), 0])
        acc[0] += p
        acc[1] += 1
    return np.array([acc[0] / acc[1] for acc in cells.values()])


def _diameter_brute(points):
    best = 0.0
    p = np.asarray(points, np.float64)
    for i in range(0, len(p), 256):
        d = np.sqrt(((p[i:i + 256, None, :] - p[None, :, :]) ** 2).sum(-1))
        best = max(best, float(d.max()))
    return best


def _check(U, pts):
    ds = U.voxel_down_sample(pts, 0.005)
    want = _voxels_by_dict(pts)
    assert len(ds) == len(want)
    a = ds[np.lexsort((ds[:, 2], ds[:, 1], ds[:, 0]))]
    b = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
    assert np.abs(a - b).max() < 1e-15
    w = U.compute_obj_max_width(ds)
    assert abs(w - _diameter_brute(ds) * 1000) < 1e-9
    return len(ds), w


def test_object_width_of_the_references_bunny(U, tmp_path):
    import gzip
    bunny = tmp_path / "1.ply"                  # the reference's file, byte for byte
    bunny.write_bytes(gzip.decompress(open(BUNNY_GZ, "rb").read()))
    pts = U.load_model_points(str(bunny))
    assert pts.shape == (11159, 3) and pts.dtype == np.float64
    # `property float`: the values are float32 numbers (as trimesh / plyfile return them), held in float64
    assert np.array_equal(pts, pts.astype(np.float32).astype(np.float64))
    n, w = _check(U, pts)
    print("bunny: %d points after 5 mm voxels, diameter %.6f mm" % (n, w))
    assert 300 < n < 2000 and 60.0 < w < 120.0                                   # (a bunny scaled to 8 cm)
    # predict.py:136-142 with the repo's dataset_info.yml (boundingbox: 10)
    assert abs(w * 1.10 - (w + 10 / 100 * w)) < 1e-9


def test_object_width_of_a_fixture_mesh(U, tmp_path):
    m = Fx.icosphere(3, 0.06, 2)
    n, w = _check(U, m["vertices"].astype(np.float64))
    assert abs(w - 120.0) < 0.5 and n > 200                                      # a 60 mm sphere
