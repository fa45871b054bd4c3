"""GPU: the synchronous _host entry points of the pose family share ONE staging pair on the context (csrc/api.cpp: StagedCall), laid
out anew by every call.  A sequence of calls of all four on one Engine -- layouts of different kinds, a growth in the middle, a
layout smaller than the buffer -- gives, call by call, the bytes the same call gives on a fresh Engine: no call sees another's bytes."""
import numpy as np
import pytest

import pose_grid_oracle as PGO
import pose_search_cases as PC
import pose_search_oracle as PSO

pytestmark = pytest.mark.gpu


def as_bytes(result):
    return [np.ascontiguousarray(x).tobytes() for x in result]


def test_one_staging_pair_serves_every_host_entry_point_in_turn():
    import se3tracknet_amd as se3
    pts, nrm = PC.blob(65)
    rots, trans = PC.grid_factors()
    depth, K = PC.grid_depth(), PC.GRID_K
    poses = PGO.compose(rots, trans)                       # 159 poses around (0, 0, 0.5)
    rng = np.random.default_rng(70)
    gts = poses[rng.permutation(len(poses))[:70]]
    steps = [
        lambda e, mp: e.pose_errors(mp, poses[:3], gts[:3]),
        lambda e, mp: e.score_poses(mp, poses[:37], depth, K, 5, top=8),
        lambda e, mp: e.score_pose_grid(mp, rots, trans[:5], depth, K, 5, facing=True, top=8),
        lambda e, mp: e.align_poses(mp, poses[:5], depth, K, iters=4, sums=True),
        lambda e, mp: e.pose_errors(mp, poses[:70], gts),  # the staging grows under it
        lambda e, mp: e.score_poses(mp, poses[:2], depth, K, 5, top=2),   # a layout smaller than the buffer
        lambda e, mp: e.pose_errors(mp, poses[:3], gts[:3]),
    ]
    shared = se3.Engine(0, 1)
    mp = shared.model_points(pts, nrm)
    got = [as_bytes(step(shared, mp)) for step in steps]
    again = as_bytes(steps[1](shared, mp))                 # after everything else: the first search once more
    mp.close()
    shared.close()
    for k, step in enumerate(steps):
        fresh = se3.Engine(0, 1)
        fp = fresh.model_points(pts, nrm)
        want = step(fresh, fp)
        assert got[k] == as_bytes(want), k
        if k == 1:                                         # and the searches say what the oracles say
            fit = PSO.score(pts, poses[:37], depth, K, 5)
            assert np.array_equal(want[0], PSO.rank(fit, 8)) and want[1].tobytes() == fit[want[0]].tobytes()
        if k == 2:
            fit = PGO.score(pts, nrm, rots, trans[:5], depth, K, 5, 1)
            assert np.array_equal(want[0], PSO.rank(fit, 8)) and want[1].tobytes() == fit[want[0]].tobytes()
        fp.close()
        fresh.close()
    assert got[0] == got[6] and got[1] == again
    assert len(got[4][0]) == 70 * 8 and len(got[3]) == 3   # (add, adds) of 70 pairs; (poses, records, sums)
