"""Cases for the range guard of SE3TN_PREC_F16X3 (tests/test_f16x3_range_cases.py without a GPU, tests/test_gpu_f16x3_range.py on it).

f16x3 stores every activation as split rows (f16 hi + f16 lo); a stored value above 65000 must raise the flag se3tn_overflow reads.
The split stores of one forward pass, in order (STAGES): the two inputs, the pooled stems, the 64-channel trunk (A2_t, B2_t, B2, B3_t,
A2, B3), ab1, ab_t, ab, the heads' stride-2 conv ("head"), and then either head_t (conv by conv) or -- where the heads run as the fused
F(4x4) block -- the transformed planes of "head" (V_in) and of head_t (V_mid; head_t itself then stays in LDS as float32).  The last
head map is float32 and no target.

Every case starts from O.make_state_dict(SEED_SD) and the two pairs Fx.net_inputs(SEED_IN, 2):

  hot channel   one output channel c of the layer that produces the stage gets its BN gamma and beta multiplied by a power of two k,
                every conv that reads the stage gets input channel c zeroed, and where a residual carries the stage into a block output
                that block's bn2.bias[c] is set to -2^30 (the block output in c is exactly 0).  In exact arithmetic nothing but channel
                c of that stage changes, so a flag raised by the case was raised at that stage.  k: the smallest power of two that lifts
                the stage above OVER_MIN ("over"), or the largest that keeps it at or below IN_RANGE_HI / 2 ("in").
                Not isolated: "head" where the heads run fused (V_in transforms the same channel and follows), noted in `follows`.
  whole stage   (the ReLU mids, positively homogeneous) the layer's BN gamma and beta times 2^k and the weights of the conv that reads
                it times 2^-k: the logits are unchanged in exact arithmetic, every stored value of the stage moves by 2^k.
  scaled SELU   (head conv1: SELU is not homogeneous, so this is another network, evaluated in float64 like every case)
                gamma and beta times 2^k, the reading conv's weights times 2^-k; see WHOLE for the block's residual.

`build(...)` returns the state dict, the inputs, the float64 maxima of every split-stored quantity and the float64 logits."""
import math

import numpy as np
import torch

from oracle import fixtures as Fx
from oracle import se3_oracle as O

F16_MAX = 65504.0
GUARD = 65000.0                   # the kernels' test: !(|x| <= 65000) raises the flag
OVER_MIN = 1.2 * F16_MAX          # an over-range case exceeds this (hi really becomes inf; float32 rounding cannot decide it)
OTHERS_MAX = 32000.0              # ... and every other split-stored quantity stays below this
IN_RANGE = (16000.0, 60000.0)     # the maximum of an in-range case: (lo, hi]
SEED_SD, SEED_IN = 31, 3100
DEAD_BIAS = -float(2 ** 30)

STAGES = ("inA", "inB", "poolA", "poolB", "A2_t", "B2_t", "B2", "B3_t", "A2", "B3", "ab1", "ab_t", "ab", "head", "head_t", "V_in", "V_mid")
# stage -> (BN of the producing layer, [(conv weight that reads it, first input channel of the stage in that conv)], bn2.bias of the block
#           whose residual carries it on | None, the conv of tests/route_model.py LAYERS that stores it)
PRODUCER = {
    "poolA": ("convA1.1", [("convA2.conv1.weight", 0)], "convA2.bn2.bias", None),
    "poolB": ("convB1.1", [("convB2.conv1.weight", 0)], "convB2.bn2.bias", None),
    "A2_t": ("convA2.bn1", [("convA2.conv2.weight", 0)], None, "trunk1"),
    "B2_t": ("convB2.bn1", [("convB2.conv2.weight", 0)], None, "trunk1"),
    "B2": ("convB2.bn2", [("convB3.conv1.weight", 0)], "convB3.bn2.bias", "trunk2"),
    "B3_t": ("convB3.bn1", [("convB3.conv2.weight", 0)], None, "trunk3"),
    "A2": ("convA2.bn2", [("convAB1.0.weight", 0)], None, "trunk2"),
    "B3": ("convB3.bn2", [("convAB1.0.weight", 64)], None, "trunk4"),
    "ab1": ("convAB1.1", [("convAB2.conv1.weight", 0)], "convAB2.bn2.bias", "ab1"),
    "ab_t": ("convAB2.bn1", [("convAB2.conv2.weight", 0)], None, "ab2.1"),
    "ab": ("convAB2.bn2", [("trans_conv1.0.weight", 0), ("rot_conv1.0.weight", 0)], None, "ab2.2"),
    "head": ("trans_conv1.1", [("trans_conv2.conv1.weight", 0)], "trans_conv2.bn2.bias", "h1"),
    "head_t": ("trans_conv2.bn1", [("trans_conv2.conv2.weight", 0)], None, "h2.1"),
}
PRODUCER["V_in"] = PRODUCER["head"]        # the planes are transforms of these two maps (the trans head's half)
PRODUCER["V_mid"] = PRODUCER["head_t"]
HOMOGENEOUS = ("A2_t", "B2_t", "B3_t", "ab_t", "head_t")   # ReLU(BN(conv)): scaling gamma and beta scales the stage exactly


# ---- which quantities a route stores, and which kernel family stores them ----------------------------------------------------------
def stored(fused_heads):
    """the split-stored quantities of a forward pass whose heads run conv by conv | as the fused F(4x4) block"""
    return tuple(s for s in STAGES if (s not in ("V_in", "V_mid") if not fused_heads else s != "head_t"))


# output map side, stride, couts per group, groups of the ten convs (csrc/infer_plan.h: conv_specs, conv_table)
GEOM = {"trunk1": (44, 1, 64, 2), "trunk2": (44, 1, 64, 2), "trunk3": (44, 1, 64, 1), "trunk4": (44, 1, 64, 1), "ab1": (22, 2, 256, 1),
        "ab2.1": (22, 1, 256, 1), "ab2.2": (22, 1, 256, 1), "h1": (11, 2, 1024, 1), "h2.1": (11, 1, 512, 2), "h2.2": (11, 1, 512, 2)}
BIG_TILE_MIN_BLOCKS = 200          # csrc/infer_plan.h pick_slices: below this many big-tile workgroups a conv runs split-K


def f16x3_family(layer, n):
    """the f16x3 kernel family of a conv outside a fused block at n pairs: "split-K" (partial sums + the reduce epilogue) or the
    big-tile kernels, "slab" at stride 1 and "gather" at stride 2.  The rule of pick_slices, restated; the GPU test reads the family
    that ran from the profile names and holds this to it."""
    ho, stride, cout, groups = GEOM[layer]
    rows, bn = (256 if stride == 1 else 128), (128 if cout >= 128 else 64)
    blocks = -(-(n * ho * ho) // rows) * (cout // bn) * groups
    return "split-K" if blocks < BIG_TILE_MIN_BLOCKS else ("slab" if stride == 1 else "gather")


def smallest_all_big_tile(n_max=64):
    """the smallest batch at which every conv runs a big-tile kernel (with the Winograd blocks off)"""
    for n in range(1, n_max + 1):
        if all(f16x3_family(k, n) != "split-K" for k in GEOM):
            return n
    raise AssertionError("no batch up to %d runs every conv on the big tiles" % n_max)


# ---- float64 evaluation with every split-stored map ----------------------------------------------------------------------------------
def _mats():
    from test_winograd_matrices import SRC, _matrix      # the tables compiled into wino_mfma.hip, parsed from the source
    src = open(SRC).read()
    return _matrix(src, "wino_bt", "t4")


def wino4_in_planes(x, BT):
    """B^T d B of every 6 x 6 tile (stride 4) of the zero-bordered map x [N,C,H,W], as wino_input_kernel<4> forms it: tiles
    ceil(H / 4) a side over the padded map, rows and columns past it read as 0.  -> [N,C,th,tw,6,6] float64"""
    x = x.double()
    N, C, H, W = x.shape
    th, tw = -(-H // 4), -(-W // 4)
    p = torch.zeros((N, C, 4 * th + 2, 4 * tw + 2), dtype=torch.float64)
    p[:, :, 1:H + 1, 1:W + 1] = x
    d = p.unfold(2, 6, 4).unfold(3, 6, 4)                 # [N,C,th,tw,6,6]
    B = torch.from_numpy(np.asarray(BT, np.float64))
    return torch.einsum("ir,ncturs,js->nctuij", B, d, B)


def stage_maps(sd64, A, B, BT=None):
    """Se3TrackNet.forward in float64 (the layers of oracle/se3_oracle.py), keeping every split-stored map; -> (maps, logits [N,6])"""
    m = {"inA": A, "inB": B}
    a = torch.nn.functional.max_pool2d(O._conv_bn_selu(sd64, "convA1", A, 2), 3, 2, 1)
    b = torch.nn.functional.max_pool2d(O._conv_bn_selu(sd64, "convB1", B, 2), 3, 2, 1)
    m["poolA"], m["poolB"] = a, b
    mid = []
    m["A2"] = O._basic_block(sd64, "convA2", a, mid)
    m["B2"] = O._basic_block(sd64, "convB2", b, mid)
    m["B3"] = O._basic_block(sd64, "convB3", m["B2"], mid)
    m["A2_t"], m["B2_t"], m["B3_t"] = mid
    m["ab1"] = O._conv_bn_selu(sd64, "convAB1", torch.cat((m["A2"], m["B3"]), 1), 2)
    mid = []
    m["ab"] = O._basic_block(sd64, "convAB2", m["ab1"], mid)
    m["ab_t"] = mid[0]
    c1, t, lg = [], [], []
    for head in ("trans", "rot"):
        h = O._conv_bn_selu(sd64, head + "_conv1", m["ab"], 2)
        c1.append(h)
        h = O._basic_block(sd64, head + "_conv2", h, t)
        h = torch.nn.functional.adaptive_avg_pool2d(h, 1).reshape(A.shape[0], -1)
        lg.append(torch.nn.functional.linear(h, sd64[head + "_out.0.weight"], sd64[head + "_out.0.bias"]))
    m["head"], m["head_t"] = torch.cat(c1, 1), torch.cat(t, 1)
    if BT is not None:
        m["V_in"], m["V_mid"] = wino4_in_planes(m["head"], BT), wino4_in_planes(m["head_t"], BT)
    return m, torch.cat(lg, 1)


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _chan_max(t):
    """largest |value| per channel of a map [N,C,...]"""
    return t.abs().transpose(0, 1).reshape(t.shape[1], -1).max(1).values


_BASE = {}


def base():
    """the seeded state dict, the two pairs, the float64 maps of the unmodified network (computed once)"""
    if not _BASE:
        sd = O.make_state_dict(SEED_SD)
        A, B = Fx.net_inputs(SEED_IN, 2)
        BT = _mats()
        maps, lg = stage_maps(_f64(sd), A.double(), B.double(), BT)
        _BASE.update(sd=sd, A=A, B=B, BT=BT, maps=maps, lg=lg, cmax={s: _chan_max(maps[s]) for s in STAGES})
    return _BASE


# ---- the constructions ---------------------------------------------------------------------------------------------------------------
def _pow2_over(m):
    return 2.0 ** math.ceil(math.log2(1.25 * OVER_MIN / m))          # k m > 1.25 OVER_MIN (the margin is checked, not assumed)


def _pow2_in(m):
    return 2.0 ** math.floor(math.log2(OTHERS_MAX / m))              # OTHERS_MAX / 2 < k m <= OTHERS_MAX: inside IN_RANGE


def hot_input(which, kind):
    """input case: depth channel of image A | B times k, the stem's weights on that channel zeroed"""
    b = base()
    sd = {k: v.clone() for k, v in b["sd"].items()}
    A, B = b["A"].clone(), b["B"].clone()
    x, conv = (A, "convA1.0.weight") if which == "inA" else (B, "convB1.0.weight")
    m = float(x[:, 3].abs().max())
    k = _pow2_over(m) if kind == "over" else _pow2_in(m)
    x[:, 3] *= k
    sd[conv][:, 3] = 0
    return sd, A, B, dict(channel=3, k=k)


def hot_channel(stage, kind, shift=0):
    """-> (sd, note): the hot-channel state dict of a stage; kind "over" | "in"; shift: extra powers of two on k"""
    b = base()
    bn, readers, res_bias, _ = PRODUCER[stage]
    cm = b["cmax"][stage]
    pick = _pow2_over if kind == "over" else _pow2_in
    if stage in ("V_in", "V_mid"):
        # the channel (of the trans head) whose map stays lowest where its planes reach the target
        src = b["cmax"]["head" if stage == "V_in" else "head_t"][:512]
        live = cm[:512] > 0.5       # (a dead channel has no planes to lift)
        ks = torch.tensor([pick(float(v)) if ok else 1.0 for v, ok in zip(cm[:512], live)], dtype=torch.float64)
        c = int(torch.where(live, ks * src, torch.full_like(src, float("inf"))).argmin())
    else:
        c = int(cm[:512 if stage.startswith("head") else cm.shape[0]].argmax())
    k = pick(float(cm[c])) * 2.0 ** shift
    sd = {key: v.clone() for key, v in b["sd"].items()}
    sd[bn + ".weight"][c] *= k
    sd[bn + ".bias"][c] *= k
    for w, c0 in readers:
        sd[w][:, c0 + c] = 0
    if res_bias:
        sd[res_bias][c] = DEAD_BIAS
    return sd, dict(channel=c, k=k)


# whole-stage scaling: (the BNs whose gamma and beta take 2^k, the weights that take 2^-k -- each of those convs reads nothing else).
# "head": its block adds the stage back as the residual, so bn2 takes 2^k as well (relu(k y + k x) = k relu(y + x): the last head map,
# float32 and not split-stored, is k times larger) and the fully connected layer takes 2^-k
WHOLE = {"A2_t": (["convA2.bn1"], ["convA2.conv2.weight"]), "ab_t": (["convAB2.bn1"], ["convAB2.conv2.weight"]),
         "head_t": (["trans_conv2.bn1", "rot_conv2.bn1"], ["trans_conv2.conv2.weight", "rot_conv2.conv2.weight"]),
         "head": (["trans_conv1.1", "rot_conv1.1", "trans_conv2.bn2", "rot_conv2.bn2"],
                  ["trans_conv2.conv1.weight", "rot_conv2.conv1.weight", "trans_out.0.weight", "rot_out.0.weight"])}


def scaled_stage(stage, log2k):
    """whole-stage scaling: gamma and beta of the producing BN times 2^log2k, the weights of the convs that read the stage times
    2^-log2k.  Exact (unchanged logits) for the HOMOGENEOUS stages; "head" (SELU(k y) is not k SELU(y)) is another network with
    logits of the same size."""
    b = base()
    bns, ws = WHOLE[stage]
    k = 2.0 ** log2k
    sd = {key: v.clone() for key, v in b["sd"].items()}
    for p in bns:
        sd[p + ".weight"] *= k
        sd[p + ".bias"] *= k
    for w in ws:
        sd[w] *= 1.0 / k
    return sd, dict(channel=None, k=k)


_CASES = {}


def _target_max(case):
    return case["maxima"][case["stage"]]


def build(cid):
    """case id -> dict(id, stage, kind, sd, A, B, maxima {quantity: float64 max |value|}, lg64 [2,6], channel, k, follows).
    ids: "over:<stage>" / "in:<stage>" (hot channel), "whole:<stage>" (a homogeneous stage scaled into range),
    "scaled:<stage>:<log2 k>" (whole-stage scaling by a given power of two)"""
    if cid in _CASES:
        return _CASES[cid]
    kind, stage = cid.split(":")[:2]
    b = base()
    for shift in (0, 1, -1, 2, -2):      # (a residual adds to a hot block output: the first k can miss its window by a power of two)
        A, B = b["A"], b["B"]
        if kind == "scaled":
            sd, note = scaled_stage(stage, int(cid.split(":")[2]))
        elif kind == "whole":
            sd, note = scaled_stage(stage, int(math.log2(_pow2_in(float(b["cmax"][stage].max())))) + shift)
        elif stage in ("inA", "inB"):
            sd, A, B, note = hot_input(stage, kind)
        else:
            sd, note = hot_channel(stage, kind, shift)
        maps, lg = stage_maps(_f64(sd), A.double(), B.double(), b["BT"])
        case = dict(id=cid, stage=stage, kind=kind, sd=sd, A=A, B=B, maxima={s: float(maps[s].abs().max()) for s in STAGES},
                    lg64=lg.numpy(), follows=("V_in",) if (stage == "head" and kind == "over") else (), **note)
        t = _target_max(case)
        if kind == "scaled" or (t > OVER_MIN if kind == "over" else IN_RANGE[0] < t <= IN_RANGE[1]):
            break
    else:
        raise AssertionError("%s: no power of two puts the target where the case needs it (last maximum %.4g)" % (cid, t))
    case["routes"] = case_routes(case)
    _CASES[cid] = case
    return case


def case_routes(case):
    """the head routes a case runs on.  over: where the target is stored.  in / whole: where the target is stored and nothing stored
    leaves IN_RANGE (a map in range can have F(4x4) planes that are not: the fused route is left out then)"""
    kinds = ("plain",) if case["stage"] == "head_t" else ("fused",) if case["stage"] in ("V_in", "V_mid") else ("plain", "fused")
    if case["kind"] == "over":
        return kinds
    return tuple(r for r in kinds if max(case["maxima"][s] for s in stored(r == "fused")) <= IN_RANGE[1])


HOT_STAGES = ("inA", "inB", "poolA", "poolB", "A2_t", "B2_t", "B2", "B3_t", "A2", "B3", "ab1", "ab_t", "ab", "head", "head_t", "V_in", "V_mid")
OVER_IDS = ["over:" + s for s in HOT_STAGES]
IN_IDS = ["in:" + s for s in HOT_STAGES] + ["whole:" + s for s in ("A2_t", "ab_t", "head_t")]
