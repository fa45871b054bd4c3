"""CPU: the cases of tests/f16x3_range_cases.py are what they claim, in float64.

Per over-range case: the target stage exceeds OVER_MIN = 1.2 x 65504 somewhere (its f16 hi half really is inf), and every other
split-stored quantity of the routes it runs on -- the F(4x4) planes included where the heads run fused -- stays at or below
OTHERS_MAX = 32000, so float32-against-float64 rounding decides no flag.  Per in-range case: the largest stored value of its routes
lies in IN_RANGE = (16000, 60000].  The generator's own forward pass and its numpy statement of the F(4x4) in-transform are held to
oracle/se3_oracle.py and to the 3 x 3 correlation the transform stands for."""
import numpy as np
import pytest
import torch

import f16x3_range_cases as R
from oracle import se3_oracle as O


def test_generator_forward_is_the_oracle_forward():
    b = R.base()
    sd64 = R._f64(b["sd"])
    o = O.forward(sd64, b["A"].double(), b["B"].double(), intermediates=True)
    assert torch.equal(torch.cat([o["trans_logit"], o["rot_logit"]], 1), b["lg"])
    same = {"poolA": o["poolA"], "poolB": o["poolB"], "A2_t": o["A2_t"], "B3_t": o["B3_t"], "ab1": o["ab1"], "ab_t": o["ab_t"], "ab": o["feature"],
            "head": torch.cat([o["trans_c1"], o["rot_c1"]], 1), "head_t": torch.cat([o["trans_t"], o["rot_t"]], 1),
            "A2": o["cat"][:, :64], "B3": o["cat"][:, 64:]}
    for k, v in same.items():
        assert torch.equal(b["maps"][k], v), k
    # the two the oracle does not hand out: B2 is what B3's block reads, B2_t what B2's second conv reads
    sd = sd64
    t = torch.relu(O._bn(sd, "convB2.bn1", torch.nn.functional.conv2d(o["poolB"], sd["convB2.conv1.weight"], sd["convB2.conv1.bias"], padding=1)))
    assert torch.equal(b["maps"]["B2_t"], t)
    assert torch.equal(O._basic_block(sd, "convB3", b["maps"]["B2"]), o["cat"][:, 64:])


def test_in_transform_restatement_against_the_correlation_it_stands_for():
    """A^T [(G g G^T) (.) V] A with V from wino4_in_planes equals the padded 3 x 3 correlation of the map (all three tables are the ones
    compiled into wino_mfma.hip); the tile grid covers an 11 x 11 map with 3 x 3 tiles, the last ones reading zeros past the border"""
    from test_winograd_matrices import SRC, _matrix
    src = open(SRC).read()
    BT, G, AT = (_matrix(src, f, "t4") for f in ("wino_bt", "wino_g", "wino_at"))
    assert np.array_equal(BT, R.base()["BT"])
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.normal(size=(2, 3, 11, 11)))
    g = rng.normal(size=(3, 3))
    V = R.wino4_in_planes(x, BT).numpy()
    assert V.shape == (2, 3, 3, 3, 6, 6)
    Y = np.einsum("pi,nctuij,qj->nctupq", AT, (G @ g @ G.T) * V, AT)          # [n,c,ty,tx,4,4]
    got = Y.transpose(0, 1, 2, 4, 3, 5).reshape(2, 3, 12, 12)[:, :, :11, :11]
    want = torch.nn.functional.conv2d(x.reshape(6, 1, 11, 11), torch.from_numpy(g).reshape(1, 1, 3, 3), padding=1).reshape(2, 3, 11, 11).numpy()
    assert np.abs(got - want).max() < 1e-11


@pytest.mark.parametrize("cid", R.OVER_IDS)
def test_over_range_case_is_over_at_its_stage_only(cid):
    c = R.build(cid)
    mx = c["maxima"]
    assert mx[c["stage"]] > R.OVER_MIN, (cid, mx[c["stage"]])
    assert c["routes"], cid
    for route in c["routes"]:
        st = R.stored(route == "fused")
        assert c["stage"] in st, (cid, route)
        for s in st:
            if s == c["stage"] or s in c["follows"]:
                continue
            assert mx[s] <= R.OTHERS_MAX, "%s on the %s route: %s reaches %.4g" % (cid, route, s, mx[s])
    # the hot channel is dead downstream: the logits are those of an ordinary network
    assert np.isfinite(c["lg64"]).all() and np.abs(c["lg64"]).max() < 10


def test_the_one_case_that_is_not_isolated_says_so():
    """"head" on the fused route: the in-transform reads the hot channel, so V_in leaves the range after it (first violation at head)"""
    assert [cid for cid in R.OVER_IDS if R.build(cid)["follows"]] == ["over:head"]
    c = R.build("over:head")
    assert c["maxima"]["V_in"] > R.OVER_MIN and "fused" in c["routes"]


@pytest.mark.parametrize("cid", R.IN_IDS)
def test_in_range_case_is_in_range_on_its_routes(cid):
    c = R.build(cid)
    assert c["routes"], cid
    assert R.IN_RANGE[0] < c["maxima"][c["stage"]] <= R.IN_RANGE[1]
    for route in c["routes"]:
        top = max(c["maxima"][s] for s in R.stored(route == "fused"))
        assert R.IN_RANGE[0] < top <= R.IN_RANGE[1], (cid, route, top)
    if c["kind"] == "whole":     # positively homogeneous: the logits are the unscaled network's
        assert np.abs(c["lg64"] - R.base()["lg"].numpy()).max() < 1e-12


def test_batch_sizes_follow_from_the_plan_rule():
    """every conv is split-K at 6 pairs and on the big tiles from 53 on (csrc/infer_plan.h pick_slices, restated in f16x3_family)"""
    assert all(R.f16x3_family(k, n) == "split-K" for k in R.GEOM for n in (1, 5, 6))
    n = R.smallest_all_big_tile()
    assert n == 53 and any(R.f16x3_family(k, n - 1) == "split-K" for k in R.GEOM)
    assert {R.f16x3_family(k, n) for k in ("ab1", "h1")} == {"gather"} and R.f16x3_family("h2.1", n) == "slab"
