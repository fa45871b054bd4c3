"""CPU: the C-ABI library loads without a GPU, exports every symbol include/se3tracknet.h declares,
and its host-side (float64 / packing / error-path) logic matches the oracle bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import fixtures as Fx
from oracle import se3_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    return se3tracknet_amd


def test_library_exports_every_declared_symbol(se3):
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    declared = sorted(set(re.findall(r"\b(se3tn_[a-z0-9_]+)\s*\(", hdr)))
    lib = C.CDLL(se3._lib.LIB_PATH)
    assert len(declared) >= 24
    for name in declared:
        assert hasattr(lib, name), "header declares %s but the library does not export it" % name
    assert sorted(se3._lib.exported_symbols()) == declared  # ctypes table == header
    assert b"gfx950" in se3._lib.load().se3tn_version()


def test_compute_bbox_bit_exact_vs_oracle(se3):
    rng = np.random.default_rng(0)
    for i in range(300):
        P = Fx.pose(i, (rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(0.25, 2.0)))
        w = float(rng.uniform(80, 400))
        got = se3.compute_bbox(P, Fx.K_YCB, w)
        want = O.compute_bbox(P, Fx.K_YCB, w, (1000, 1000, 1000))
        assert got.dtype == np.int32 and (got == want).all(), (i, got, want)
    # half-to-even rounding, as np.round: K chosen so that u lands exactly on .5
    P = np.eye(4); P[2, 3] = 1.0
    K = np.array([[1.0, 0, 0.5], [0, 1.0, 1.5], [0, 0, 1.0]])
    assert (se3.compute_bbox(P, K, 0.0) == O.compute_bbox(P, K, 0.0, (1000, 1000, 1000))).all()
    assert se3.compute_bbox(P, K, 0.0)[0].tolist() == [2, 0]  # 1.5 -> 2, 0.5 -> 0


def test_renderer_window_variant_matches_oracle(se3):
    P = Fx.pose(5)
    got = se3.compute_bbox(P, Fx.K_YCB, 250.0, scale=(1000, -1000, 1000))
    assert (got == O.compute_bbox(P, Fx.K_YCB, 250.0, (1000, -1000, 1000))).all()


def test_pose_update_host_bit_exact_vs_reference_golden(se3, golden_dir):
    g = np.load(os.path.join(golden_dir, "pose_update.npz"))
    for i in range(len(g["A"])):
        B = se3.pose_update_host(g["A"][i], g["trans"][i], g["rot"][i], float(g["norm"][i][0]), float(g["norm"][i][1]))
        assert np.abs(B - g["B"][i]).max() <= 2.3e-16, (i, np.abs(B - g["B"][i]).max())  # libm sin/cos ulp
        assert (B[3] == [0, 0, 0, 1]).all()
    assert (se3.pose_update_host(g["A"][0], g["trans"][0], np.zeros(3, np.float32), 0.03, 0.1)[:3, :3] == g["A"][0][:3, :3]).all()


def _numpy_pack(sd):
    """Independent restatement of the blob layout (float32 panels) and of the f16x3 split layout documented in
    csrc/se3tn_internal.h (BlobLayout / SplitLayout).  Returns (blob, split) as float32 word arrays."""
    def fold(conv, bn):
        w = sd[conv + ".weight"].double().numpy(); b = sd[conv + ".bias"].double().numpy()
        s = sd[bn + ".weight"].double().numpy() / np.sqrt(sd[bn + ".running_var"].double().numpy() + 1e-5)
        return (w * s[:, None, None, None]).astype(np.float32), ((b - sd[bn + ".running_mean"].double().numpy()) * s + sd[bn + ".bias"].double().numpy()).astype(np.float32)

    def pack3(w):  # OIHW -> [chunk][tap][cout][32]
        co, ci = w.shape[:2]
        return w.reshape(co, ci // 32, 32, 9).transpose(1, 3, 0, 2).reshape(-1)

    parts = [np.zeros(64, np.float32)]
    stems = [fold(n + ".0", n + ".1") for n in ("convA1", "convB1")]
    pairs = [((r, 2 * sp), (r, 2 * sp + 1)) for r in range(7) for sp in range(3)]
    pairs += [((2 * j, 6), (2 * j + 1, 6)) for j in range(3)] + [((6, 6), None)]
    stem_plain = []
    for w, _ in stems:  # [o][pair*8 + half*4 + c], row padded to 204
        t = np.zeros((64, 204), np.float32)
        for pi, pr in enumerate(pairs):
            for h, tap in enumerate(pr):
                if tap is not None:
                    t[:, pi * 8 + h * 4: pi * 8 + h * 4 + 4] = w[:, :, tap[0], tap[1]]
        parts.append(t.reshape(-1))
        stem_plain.append(t)
    parts += [b for _, b in stems]
    split = []
    inv = []
    for t in stem_plain:  # f16x3 stem: per 16-byte entry 4 f16 hi | 4 f16 lo of w * 2^k(cout)
        mx = np.abs(t[:, :200]).max(1).astype(np.float64)
        k = np.where(mx > 0, np.floor(10.0 - np.log2(np.where(mx > 0, mx, 1.0))), 0.0)
        ws = t[:, :200] * np.exp2(k).astype(np.float32)[:, None]
        hi = ws.astype(np.float16); lo = (ws - hi.astype(np.float32)).astype(np.float16)
        e = np.concatenate([hi.reshape(64, 50, 4), lo.reshape(64, 50, 4)], axis=2).reshape(64, 400)
        row = np.zeros((64, 408), np.float16); row[:, :400] = e
        split.append(np.ascontiguousarray(row).view(np.float32).reshape(-1))
        inv.append(np.exp2(-k).astype(np.float32))
    split += inv
    groups = [[("convA2.conv1", "convA2.bn1"), ("convB2.conv1", "convB2.bn1")],
              [("convA2.conv2", "convA2.bn2"), ("convB2.conv2", "convB2.bn2")],
              [("convB3.conv1", "convB3.bn1")], [("convB3.conv2", "convB3.bn2")],
              [("convAB1.0", "convAB1.1")], [("convAB2.conv1", "convAB2.bn1")], [("convAB2.conv2", "convAB2.bn2")],
              "H1",
              [("trans_conv2.conv1", "trans_conv2.bn1"), ("rot_conv2.conv1", "rot_conv2.bn1")],
              [("trans_conv2.conv2", "trans_conv2.bn2"), ("rot_conv2.conv2", "rot_conv2.bn2")]]
    for g in groups:
        if g == "H1":  # trans|rot fused along Cout
            (wt, bt), (wr, br) = fold("trans_conv1.0", "trans_conv1.1"), fold("rot_conv1.0", "rot_conv1.1")
            parts += [pack3(np.concatenate([wt, wr], 0)), bt, br]
        else:
            f = [fold(c, b) for c, b in g]
            parts += [pack3(w) for w, _ in f] + [b for _, b in f]
    # f16x3 sections: the deep layers again as split rows [chunk][tap][cout][32 f16 hi | 32 f16 lo] of
    # w * 2^k(cout) plus the per-cout 2^-k
    def pack3_split(w):
        co, ci = w.shape[:2]
        mx = np.abs(w).reshape(co, -1).max(1).astype(np.float64)
        k = np.where(mx > 0, np.floor(10.0 - np.log2(np.where(mx > 0, mx, 1.0))), 0.0)
        ws = (w.astype(np.float32) * np.exp2(k).astype(np.float32)[:, None, None, None])
        hi = ws.astype(np.float16)
        lo = (ws - hi.astype(np.float32)).astype(np.float16)
        def rows(x):  # OIHW -> [chunk][tap][cout][32]
            return x.reshape(co, ci // 32, 32, 9).transpose(1, 3, 0, 2)
        both = np.concatenate([rows(hi), rows(lo)], axis=3)  # [..][64] halfs = 128 bytes
        return np.ascontiguousarray(both).view(np.float32).reshape(-1), np.exp2(-k).astype(np.float32)
    for g in groups:
        if g == "H1":
            (wt, _), (wr, _) = fold("trans_conv1.0", "trans_conv1.1"), fold("rot_conv1.0", "rot_conv1.1")
            ws, sc = pack3_split(np.concatenate([wt, wr], 0))
            split += [ws, sc]
        else:
            f = [pack3_split(fold(c, b)[0]) for c, b in g]
            split += [x[0] for x in f] + [x[1] for x in f]
    for h in ("trans_out", "rot_out"):
        parts.append(sd[h + ".0.weight"].numpy().reshape(-1))
    for h in ("trans_out", "rot_out"):
        parts.append(np.concatenate([sd[h + ".0.bias"].numpy(), np.zeros(1, np.float32)]))
    blob = np.concatenate(parts)
    split = np.concatenate(split)
    pad = lambda x: np.concatenate([x, np.zeros((-len(x)) % 64, np.float32)])   # noqa: E731
    return pad(blob), pad(split)


def test_weight_folding_and_packing_host_only(se3):
    eng = se3.Engine(device=-1, max_batch=1)  # host-only context: no GPU needed
    sd = O.make_state_dict(3)
    blob_t = eng.pack_state_dict(sd)
    blob = blob_t.numpy().view(np.float32)
    want, want_split = _numpy_pack(sd)
    assert blob.size == want.size == eng.packed_bytes() // 4
    assert 54.0e6 < eng.packed_bytes() < 54.3e6      # float32 panels only: what the RCCL broadcast carries (blob v7)
    hdr = blob[:4].view(np.uint32)
    assert hdr[0] == 0x53453354 and hdr[1] == 7 and hdr[2] == blob.size
    assert (blob[64:].view(np.uint32) == want[64:].view(np.uint32)).all()  # bit-exact
    # the f16x3 split panels are no longer in the blob: derived from it (on the device in the product; the library's host
    # statement of the same arithmetic here) -- bit-exact against the independent numpy restatement from the OIHW weights
    split = eng.split_weights_host(blob_t).numpy().view(np.float32)
    assert split.size == want_split.size
    assert (split.view(np.uint32) == want_split.view(np.uint32)).all()


def test_split_exponent_rule_at_powers_of_two(se3):
    """k = floor(10 - log2(max|w|)) is evaluated on the float's exponent: exact at powers of two and their neighbours."""
    eng = se3.Engine(device=-1, max_batch=1)
    sd = O.make_state_dict(5)
    w = sd["convAB2.conv1.weight"].clone()
    for i, mx in enumerate([1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(0)),
                            2.0 ** -12, 3.0, 1024.0, 2047.9, 2048.0]):
        w[i] = w[i] * 1e-3
        w[i, 0, 0, 0] = float(mx)
    sd["convAB2.conv1.weight"] = w
    # fold with identity BN so that the row maxima survive exactly
    for k in ("weight", "bias", "running_mean", "running_var"):
        sd["convAB2.bn1." + k] = torch.ones(256) if k in ("weight",) else torch.zeros(256)
    sd["convAB2.bn1.running_var"] = torch.ones(256) - 1e-5
    blob_t = eng.pack_state_dict(sd)
    _, want_split = _numpy_pack(sd)
    split = eng.split_weights_host(blob_t).numpy().view(np.float32)
    assert (split.view(np.uint32) == want_split.view(np.uint32)).all()


def test_error_paths(se3):
    lib = se3._lib.load()
    eng = se3.Engine(device=-1, max_batch=1)
    t = torch.zeros(3, 3)
    sh = (C.c_int64 * 2)(3, 3)
    assert lib.se3tn_set_tensor(eng._h, b"not.a.key", C.c_void_p(t.data_ptr()), sh, 2) == -4  # SE3TN_E_KEY
    assert b"not.a.key" in lib.se3tn_last_error()
    assert lib.se3tn_set_tensor(eng._h, b"trans_out.0.weight", C.c_void_p(t.data_ptr()), sh, 2) == -3  # SE3TN_E_SHAPE
    assert lib.se3tn_pack_weights(eng._h) == -4 and b"missing" in lib.se3tn_last_error()
    with pytest.raises(se3._lib.Se3tnError):  # int64 / float64 tensors are refused, not silently cast
        eng.pack_state_dict({"trans_out.0.bias": torch.zeros(3, dtype=torch.float64)})
    h = C.c_void_p()
    assert lib.se3tn_create(0, 0, C.byref(h)) == -1  # bad max_batch
    if not torch.cuda.is_available():
        assert lib.se3tn_create(0, 1, C.byref(h)) != 0  # no device: loud failure, no fallback
        with pytest.raises(se3._lib.Se3tnError):
            se3.Engine(0, 1)
    # compute entry points refuse a host-only context
    assert lib.se3tn_infer(eng._h, C.c_void_p(8), C.c_void_p(8), 1, 0, None, None, None, None, None) == -1


def test_trunk_winograd_switch_defaults_and_argument_checks(se3):
    """se3tn_set/get_trunk_winograd on a host-only context: the defaults are the header's, the ctypes mirror carries the same
    numbers, bad arguments are refused."""
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "se3tracknet.h")).read()
    mb = int(re.search(r"#define SE3TN_TRUNK_WINOGRAD_DEFAULT_MIN_BATCH (\d+)", hdr).group(1))
    mf = int(re.search(r"#define SE3TN_TRUNK_WINOGRAD_DEFAULT_MIN_FILL (\d+)", hdr).group(1))
    assert (mb, mf) == (se3._lib.TRUNK_WINOGRAD_DEFAULT_MIN_BATCH, se3._lib.TRUNK_WINOGRAD_DEFAULT_MIN_FILL)
    eng = se3.Engine(device=-1, max_batch=1)
    assert eng.get_trunk_winograd() == (mb, mf)
    eng.set_trunk_winograd(0)
    assert eng.get_trunk_winograd() == (0, mf)
    eng.set_trunk_winograd(16, 0)
    assert eng.get_trunk_winograd() == (16, 0)
    lib = se3._lib.load()
    assert lib.se3tn_set_trunk_winograd(eng._h, -1, 80) == -1 and lib.se3tn_set_trunk_winograd(eng._h, 8, 101) == -1
    assert eng.get_trunk_winograd() == (16, 0)


def test_model_points_and_object_width(se3, tmp_path):
    rng = np.random.default_rng(1)
    pts = rng.uniform(-0.05, 0.05, (500, 3))
    ply = tmp_path / "m.ply"
    with open(ply, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 500\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        for p in pts:
            f.write("%.9f %.9f %.9f\n" % tuple(p))
    U = se3.utils
    got = U.load_model_points(str(ply))
    assert np.abs(got - pts).max() < 1e-8
    ds = U.voxel_down_sample(got, 0.005)
    # (`property float` columns are float32, as plyfile / trimesh return them: 4e-9 at this magnitude)
    assert len(ds) <= 500 and np.all(ds.min(0) >= pts.min(0) - 1e-8) and np.all(ds.max(0) <= pts.max(0) + 1e-8)
    w = U.compute_obj_max_width(ds)
    from scipy.spatial.distance import pdist
    assert abs(w - pdist(ds).max() * 1000) < 1e-6
    assert U.crop_window(np.array([[48, 213], [381, 213], [48, 546], [381, 546]])) == (213, 48, 546, 381)


def test_winograd_tile_codes_offset_rule_and_the_ctypes_mirror(se3):
    """The constants the Python mirror repeats are the header's; se3tn_set_winograd / se3tn_set_offset_rule accept exactly the
    documented codes (host-only context: no device work)."""
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "se3tracknet.h")).read()

    def h(name, conv=int):
        return conv(re.search(r"#define %s ([0-9.]+)" % name, hdr).group(1))
    L = se3._lib
    assert (h("SE3TN_WINOGRAD_TILE_AUTO"), h("SE3TN_WINOGRAD_TILE_6_4"), h("SE3TN_WINOGRAD_TILE6_MIN_BATCH")) == \
        (L.WINOGRAD_TILE_AUTO, L.WINOGRAD_TILE_6_4, L.WINOGRAD_TILE6_MIN_BATCH)
    assert h("SE3TN_WINOGRAD_HEADS_TILE6_MAX_ROT", float) == L.WINOGRAD_HEADS_TILE6_MAX_ROT
    assert (h("SE3TN_OFFSET_RULE_NUMPY1"), h("SE3TN_OFFSET_RULE_NUMPY2")) == (L.OFFSET_RULE_NUMPY1, L.OFFSET_RULE_NUMPY2)
    eng = se3.Engine(device=-1, max_batch=1)
    lib = L.load()
    assert eng.get_winograd() == (h("SE3TN_WINOGRAD_DEFAULT_MIN_BATCH"), L.WINOGRAD_TILE_AUTO)
    for tile in (2, 4, 6, L.WINOGRAD_TILE_6_4, L.WINOGRAD_TILE_AUTO):
        eng.set_winograd(9, tile)
        assert eng.get_winograd() == (9, tile)
    eng.set_winograd(3)                                  # tile 0 keeps the tile
    assert eng.get_winograd() == (3, L.WINOGRAD_TILE_AUTO)
    for bad in (1, 3, 5, 8, 46 + 1, 63):
        assert lib.se3tn_set_winograd(eng._h, 6, bad) == -1
    assert eng.get_offset_rule() == "numpy1"             # the reference's pinned NumPy generation is the default
    eng.set_offset_rule("numpy2")
    assert eng.get_offset_rule() == "numpy2" and lib.se3tn_get_offset_rule(eng._h) == L.OFFSET_RULE_NUMPY2
    eng.set_offset_rule(L.OFFSET_RULE_NUMPY1)
    assert eng.get_offset_rule() == "numpy1"
    assert lib.se3tn_set_offset_rule(eng._h, 2) == -1 and lib.se3tn_get_offset_rule(None) == -1


def test_track_plan_host_arithmetic_under_sanitizers(tmp_path):
    """csrc/track_plan.h (the windows, staging offsets, row gather and crop descriptors all three on_track bodies share) in a
    stand-alone host program built with AddressSanitizer + UBSan: the staging buffer is malloc'ed with exactly the planned bytes, so an
    overrun of the gather is a report; every window pixel read through the descriptors equals the frame with zero outside."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "track_plan_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "track_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "track_plan_check: ok" in out.stdout


def test_infer_plan_routes_under_sanitizers(tmp_path):
    """csrc/infer_plan.h (which kernel runs for which conv of a forward pass, decided on the host before anything is enqueued) in a
    stand-alone host program built with AddressSanitizer + UBSan.  The program walks every configuration recorded in
    tests/golden/infer_routes.json for n = 1 .. 72, and the default one up to SE3TN_MAX_BATCH_LIMIT, and asserts the plan's invariants
    itself (tests/c_abi/infer_plan_check.cpp: workspace bounds, split-K divisibility, fused blocks only with their planes, fallbacks with
    a readiness bit cleared, the mixed-model call's explicit family = the default plan of 1 .. 5 pairs and an error at 6).  It prints
    the launch names and written stages of every cell; here they are held against
      * the record of what the library launched on the device at the commit named in the file (scripts/record_infer_routes.py), exactly;
      * the Python route model (tests/route_model.py `expected`), for every cell."""
    import json
    import shutil
    import subprocess
    from route_model import actual, expected
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "infer_routes.json")))
    cases = rec["cases"]
    assert cases[0]["id"] == "default" and rec["n_max"] == 72 and len({c["id"] for c in cases}) == len(cases)
    cfgs = tmp_path / "configs.txt"
    with open(cfgs, "w") as f:
        for c in cases:
            g = c["cfg"]
            ch = 32 if c["env"].get("SE3TN_TAIL_PARTS") == "2" else 16
            f.write("%s %d %d %d %d %d %d %d %.17g %d %d %d %d %d\n" % (c["id"], g["wmin"], g["tile"], g["tmin"], g["tfill"], g["small"], g["keep"],
                                                                      g["f16"], g["rn"], g["fuse"], g["tail_parts"], ch, g["ovr"][0], g["ovr"][1]))
    exe = str(tmp_path / "infer_plan_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "infer_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe, str(cfgs)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "infer_plan_check: ok" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        if line.startswith("R\t"):
            _, cid, n, names, stages = line.split("\t")
            got[(cid, int(n))] = (names.split(";"), stages.split(",") if stages else [])
    assert len(got) == 72 * len(cases)
    for c in cases:
        seen = 0
        for first, last, names, stages in c["rows"]:
            for n in range(first, last + 1):
                seen += 1
                assert got[(c["id"], n)] == (names, stages), (c["id"], n, got[(c["id"], n)], names, stages)
                want_r, written = expected(c["cfg"], n)
                assert actual(got[(c["id"], n)][0]) == want_r, (c["id"], n)
                assert {s: s in got[(c["id"], n)][1] for s in written} == written, (c["id"], n)
        assert seen == 72, c["id"]


def test_hip_buffers_ownership_under_sanitizers(tmp_path):
    """csrc/hip_buffers.h (the owners of every device and pinned buffer of a context and a mesh) in a stand-alone host program built
    with AddressSanitizer + UBSan.  The program defines the six HIP runtime functions the header calls over malloc / free with a count
    of live blocks and a switch that fails the k-th allocation, so it links no HIP library and touches no device: destruction frees
    everything, alloc over a held block frees it, a failed alloc leaves the object empty, the rasteriser's group of four survives a
    failure of each of its allocations (grown again, destroyed: no leak, no double free), a move leaves the source empty, a mapped
    pinned block reports its device alias."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime_api.h")):
        pytest.skip("no ROCm headers")
    exe = str(tmp_path / "hip_buffers_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc, "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "hip_buffers_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "hip_buffers_check: ok" in out.stdout


def test_create_refuses_a_max_batch_above_the_limit(se3):
    """se3tn_create: SE3TN_E_ARG with a message above SE3TN_MAX_BATCH_LIMIT (the bound of the kernels' 32-bit byte offsets, derived by
    reading them: tests/test_largest_batch_plan.py; run up to it by tests/test_gpu_largest_batch.py), before a context exists; a normal create works afterwards.  The constant is the
    header's, mirrored in _lib, and is where the stride-2 gather's `int` offsets into the 46 x 46 x 128 map would pass 2^31."""
    L = se3._lib
    hdr = open(os.path.join(ROOT, "include", "se3tracknet.h")).read()
    assert int(re.search(r"#define SE3TN_MAX_BATCH_LIMIT (\d+)", hdr).group(1)) == L.MAX_BATCH_LIMIT
    per_pair = 46 * 46 * 128 * 4
    assert L.MAX_BATCH_LIMIT * per_pair <= 2 ** 31 < (L.MAX_BATCH_LIMIT + 1) * per_pair
    with pytest.raises(L.Se3tnError, match="SE3TN_MAX_BATCH_LIMIT"):
        se3.Engine(-1, L.MAX_BATCH_LIMIT + 1)
    h = C.c_void_p()
    assert L.load().se3tn_create(-1, L.MAX_BATCH_LIMIT + 1, C.byref(h)) != 0 and not h.value
    eng = se3.Engine(-1, 4)
    assert eng.lib.se3tn_max_batch(eng._h) == 4
    eng.close()
