"""CPU: the rule of a model point against the depth frame (csrc/pose_point_rule.h, csrc/pose_transform.h) -- the statements
pose_search.hip and pose_grid.hip run per point -- compiled for the host with -ffp-contract=off under AddressSanitizer + UBSan in a
stand-alone program (tests/c_abi/pose_point_rule_check.cpp), gives the records of the numpy oracles (tests/pose_search_oracle.py,
tests/pose_grid_oracle.py) BYTE FOR BYTE.  The inputs are those of tests/test_gpu_pose_search.py and tests/test_gpu_pose_grid.py
(tests/pose_search_cases.py), which hold the device to the same oracles."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_grid_oracle as PGO
import pose_search_cases as PC
import pose_search_oracle as PSO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("pose_point_rule") / "pose_point_rule_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "pose_point_rule_check.cpp"), "-o", out])
    return out


def run(exe, tmp_path, pts, nrm, poses, rots, trans, frames, K, tol, facing):
    """[(records of the poses, records of the candidates)] per frame, from the host program"""
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    PC.write_case(src, pts, nrm, poses, rots, trans, frames, K, tol, facing)
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "case done" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    return PC.read_records(dst, len(frames), len(poses), len(rots) * len(trans))


@pytest.mark.parametrize("hw", [(6, 6), (7, 7), (6, 7), (7, 6)])
@pytest.mark.parametrize("tol", [1, 7, 65535])
def test_exact_boundaries_on_the_host(exe, tmp_path, hw, tol):
    """The frames of test_gpu_pose_search.py::test_exact_boundaries, every shift of the pixel values: the three poses through
    transform() and the same three as the lattice identity x their translations through rotate() + t."""
    pts, poses, vals = PC.boundary_points(hw), PC.boundary_poses(), PC.boundary_values(tol)
    rots, trans = np.eye(3)[None], np.ascontiguousarray(poses[:, :3, 3])
    frames = np.array([PC.boundary_depth(hw, vals, shift) for shift in range(len(vals))])
    got = run(exe, tmp_path, pts, None, poses, rots, trans, frames, PC.BOUNDARY_K, tol, 0)
    n_in = (3 if hw[1] % 2 == 0 else 4) * (3 if hw[0] % 2 == 0 else 4)
    seen_total = 0
    for depth, (by_pose, by_candidate) in zip(frames, got):
        want = PSO.score(pts, poses, depth, PC.BOUNDARY_K, tol)
        assert want["in_frame_pts"][0] == n_in and want["in_frame_pts"][2] == 0       # the case shows what it is meant to show
        assert by_pose.tobytes() == want.tobytes(), (hw, tol, by_pose, want)
        want_grid = PGO.score(pts, None, rots, trans, depth, PC.BOUNDARY_K, tol, 0)
        assert by_candidate.tobytes() == want_grid.tobytes() == want.tobytes(), (hw, tol, by_candidate, want_grid)
        seen_total += int(want["seen_pts"][0])
    assert seen_total == n_in * int(((vals > 100) & (vals < 2000)).sum())             # every hit pixel has taken every value


@pytest.mark.parametrize("facing", [0, 1])
def test_the_blob_on_the_host(exe, tmp_path, facing):
    """65 points (one over a wave) on the 48 x 64 frame with holes and borderline values, 3 rotations x 53 translations, with and
    without the facing rule; the composed poses through transform() give the words of the lattice without it."""
    pts, nrm = PC.blob(65)
    rots, trans = PC.grid_factors()
    depth = PC.grid_depth()
    poses = PGO.compose(rots, trans)
    (by_pose, by_candidate), = run(exe, tmp_path, pts, nrm, poses, rots, trans, depth[None], PC.GRID_K, 5, facing)
    want = PGO.score(pts, nrm, rots, trans, depth, PC.GRID_K, 5, facing)
    plain = PSO.score(pts, poses, depth, PC.GRID_K, 5)
    PGO.check_invariants(want, 65, 5, facing)
    assert want["inlier_pts"].max() > 0 and want["in_frame_pts"][7] == 0 and want["in_frame_pts"][11] == 0
    if facing:
        assert 0.3 * 65 < want["points"][0] < 0.7 * 65 and want["front_pts"].sum() < plain["front_pts"].sum()
    else:
        assert want.tobytes() == plain.tobytes()
    assert by_candidate.tobytes() == want.tobytes(), (by_candidate, want)
    assert by_pose.tobytes() == plain.tobytes(), (by_pose, plain)
