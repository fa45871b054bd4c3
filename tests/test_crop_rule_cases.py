"""Preconditions of tests/test_gpu_crop_sizes.py, stated on the oracle alone (no GPU, no library): the decisive set is what the
documents say it is, and every case of the sweep has teeth -- under each alternative evaluation that differs at the case's width or
height, the oracle's own crop of the case's window changes, in the colour image and in the depth image.  So a device copy of the rule
that slid into one of those evaluations cannot pass the GPU file, whichever size it is run at.

No case is excused.  The seeds of tests/crop_rule_cases.py (FRAME_SEED, EDGE_SEED, MODEL_FRAME_SEED) are the first tried; what had
to change for every precondition to hold is the edge placement of the small decisive sizes, whose overhang is bounded so that
their last decisive column / row stays on the frame (crop_rule_cases.place says why)."""
import numpy as np
import pytest

import crop_rule_cases as CR
from oracle import fixtures as Fx
from oracle import se3_oracle as O


def test_counts_of_the_decisive_set():
    d = CR.decisive(2000)
    per_alt = {name: sum(1 for s in d if name in d[s]) for name in CR.ALTERNATIVES}
    print("decisive sizes per alternative:", per_alt, "union:", len(d))
    assert per_alt == {"exact_integers": 156, "one_division": 156, "scale_first": 142, "float32": 207}
    assert len(d) == 239 and sum(1 for s in d if s <= 352) == 46
    assert sum(1 for s in d if s % 2) == 5
    positions = set()
    for s, diff in d.items():
        want = CR.rule(CR.DST, s)
        for name, pos in diff.items():
            got = CR.ALTERNATIVES[name](CR.DST, s)
            assert (np.abs(got[pos] - want[pos]) == 1).all(), (s, name)       # off by exactly one index wherever it differs
            assert ((pos * s) % CR.DST == 0).all(), (s, name)                 # ... and only where x * s / 176 is an integer
            positions.update(int(p) for p in pos)
    assert len(positions) == 25 and sorted(positions)[:6] == [11, 16, 22, 32, 33, 44]
    assert sorted(set(int(p) for pos in d[144].values() for p in pos)) == [33, 66, 77, 121, 132, 143, 154]
    for s in (72, 84, 144, 168, 248, 288, 336) + CR.TRACK_SIZES:
        assert s in d, s


def test_sweep_sizes_and_pairing():
    sizes, cases = CR.SWEEP_SIZES, CR.sweep_cases()
    assert len(sizes) == 352 + 239 - 46 == len(cases) and sizes[0] == 1 and sizes[-1] <= 2000
    assert set(range(1, 353)) <= set(sizes) and set(CR.decisive(2000)) <= set(sizes)
    assert sorted(c.width for c in cases) == list(sizes) == sorted(c.height for c in cases)      # once as a width, once as a height
    assert all(c.width != c.height for c in cases)
    H, W = CR.FRAME_HW
    over = 0
    for c in cases:
        l, t, r, b = c.windows["inside"]
        assert 0 <= l and r <= W and 0 <= t and b <= H and (r - l, b - t) == (c.width, c.height)
        l, t, r, b = c.windows["edge"]
        assert (r - l, b - t) == (c.width, c.height) and -40 <= l <= 0 < r and -40 <= t <= 0 < b
        assert (l < 0 or c.width == 1) and (t < 0 or c.height == 1)                # a 1-pixel window cannot leave the frame and touch it
        over += int(l < 0 and t < 0)
    assert over >= len(cases) - 2
    for k in range(CR.CHUNKS):
        ch = CR.chunk(k)
        assert 2 * len(ch) > 2 * 64 and {c.offset_rule for c in ch} == {("numpy1", "numpy2")[k % 2]}
        assert {c.stats for c in ch} == {0, 1} and len({c.z_offset_mm for c in ch}) == len(CR.Z_OFFSETS_MM)
        assert max(c.width for c in ch) > 1500 and min(c.width for c in ch) < 5
    # float32 holds some of the offsets exactly and not the others: the two offset rules part on the latter
    exact = [z for z in CR.Z_OFFSETS_MM if float(np.float32(z)) == z]
    assert sorted(exact) == [-640.25, 812.5] and len(CR.Z_OFFSETS_MM) - len(exact) == 5
    rgb, depth = CR.frame()
    assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8 and depth.dtype == np.uint16 and depth.max() == 2499
    for v in (0, 100, 101, 1999, 2000):
        assert (depth == v).any()
    assert rgb.min() == 0 and rgb.max() == 255


def test_the_restatement_of_the_precondition_helper_is_crop_bbox_under_the_rule():
    """crop_with_tables under the oracle's own tables IS O.crop_bbox -- so what it shows under other tables is what another
    evaluation would have shown"""
    rgb, depth = CR.frame()
    for c in CR.sweep_cases()[::9]:
        for p in CR.PLACEMENTS:
            want = CR.oracle_crop(rgb, depth, c.windows[p])
            got = CR.alternative_crop(rgb, depth, c.windows[p], "rule")
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (c, p)


@pytest.mark.parametrize("k", range(CR.CHUNKS))
def test_every_sweep_case_has_teeth(k):
    rgb, depth = CR.frame()
    H, W = CR.FRAME_HW
    n_checked = 0
    for c in CR.chunk(k):
        names = CR.differing((c.width, c.height))
        for p in CR.PLACEMENTS:
            win = c.windows[p]
            if p == "inside":        # every decisive column and row of the crop shows a frame pixel
                for size, org, lim in ((c.width, win[0], W), (c.height, win[1], H)):
                    src = org + CR.rule(CR.DST, size)[CR.decisive_positions(size)]
                    assert ((src >= 0) & (src < lim)).all(), (c, p)
            if not names:
                continue
            want = CR.oracle_crop(rgb, depth, win)
            for name in names:
                got = CR.alternative_crop(rgb, depth, win, name)
                assert (got[0] != want[0]).any() and (got[1] != want[1]).any(), (c, p, name)
                n_checked += 1
    print("chunk %d: %d (case, placement, alternative) crops differ from the oracle's" % (k, n_checked))
    assert n_checked > 100


def test_fit_cases_have_teeth():
    import se3tracknet_amd as se3
    model, observed = CR.fit_frames()
    cases = CR.fit_cases()
    assert len(cases) == CR.FIT_PAIRS > se3._lib.FIT_MAX_PAIRS
    d = CR.decisive()
    kinds = set()
    seen = set()
    for name, mw, ow in cases:
        sizes = (mw[2] - mw[0], mw[3] - mw[1], ow[2] - ow[0], ow[3] - ow[1])
        assert len(set(sizes)) == 4 and all(s in d for s in sizes), name       # different decisive sizes, both axes, both descriptors
        kinds.add((mw[0] < 0, ow[0] < 0))
        want = CR.fit_expected(se3, name)
        assert min(int(want[f]) for f in ("model_px", "seen_px", "inlier_px", "front_px", "behind_px", "sum_abs_mm")) > 0, name
        assert int(want["model_px"]) > int(want["seen_px"])
        seen.add(tuple(int(want[f]) for f in se3._lib.FIT_FIELDS))
        for alt in CR.differing(sizes):
            got = se3.utils.fit_stats(CR.alternative_crop(None, model, mw, alt)[1], CR.alternative_crop(None, observed, ow, alt)[1], CR.FIT_TOL)
            assert got != want, (name, alt)
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}          # both placements on both sides
    assert len(seen) == len(cases)


def test_track_poses_have_the_window_sizes_they_name():
    K = Fx.K_YCB
    H, W = Fx.DATASET_INFO["camera"]["height"], Fx.DATASET_INFO["camera"]["width"]
    d = CR.decisive()
    assert len(CR.TRACK_SIZES) >= 6 and {144, 248, 288} <= set(CR.TRACK_SIZES) and all(s in d and s <= 352 for s in CR.TRACK_SIZES)
    kinds = {}
    for name, size, centre in CR.track_cases():
        P = CR.find_pose(size, K, centre)
        bb = O.compute_bbox(P, K, CR.TRACK_WIDTH_MM, (1000, 1000, 1000))
        l, t, r, b = int(bb[:, 1].min()), int(bb[:, 0].min()), int(bb[:, 1].max()), int(bb[:, 0].max())
        assert (r - l, b - t) == (size, size), (name, l, t, r, b)
        kinds[name] = ("L" if l < 0 else "") + ("T" if t < 0 else "") + ("R" if r > W else "") + ("B" if b > H else "") or "inside"
        assert r > 0 and b > 0 and l < W and t < H
    assert "LT" in kinds.values() and "RB" in kinds.values() and list(kinds.values()).count("inside") >= 5
