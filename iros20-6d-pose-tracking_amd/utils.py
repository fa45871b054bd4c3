"""Host-side helpers of the hot path that the reference keeps in Utils.py, plus dependency-free
stand-ins for the trimesh / open3d calls of Tracker.__init__ (predict.py:131-142)."""
import numpy as np

from .engine import compute_bbox as _compute_bbox_c


def compute_bbox(pose, K, scale_size=230, scale=(1000, 1000, 1000)):
    """Utils.py:302-316.  The path only ever calls it with scale (1000,1000,1000)
    (predict.py:232) or (1000,-1000,1000) for the GL renderer window (predict.py:201)."""
    if tuple(scale) == (1000, 1000, 1000):
        return _compute_bbox_c(pose, K, scale_size)
    # generic float64 numpy path for the renderer's flipped-y window
    obj = [pose[i, 3] * scale[i] for i in range(3)]
    off = scale_size / 2
    pts = np.array([[obj[0] - off, obj[1] - off, obj[2]], [obj[0] - off, obj[1] + off, obj[2]],
                    [obj[0] + off, obj[1] - off, obj[2]], [obj[0] + off, obj[1] + off, obj[2]]], np.float64)
    vus = np.zeros((4, 2))
    vus[:, 1] = pts[:, 0] * K[0, 0] / pts[:, 2] + K[0, 2]
    vus[:, 0] = pts[:, 1] * K[1, 1] / pts[:, 2] + K[1, 2]
    return np.round(vus).astype(np.int32)


def crop_window(bbox):
    """left, top, right, bottom as crop_bbox derives them (Utils.py:321-324)."""
    return (int(np.min(bbox[:, 1])), int(np.min(bbox[:, 0])), int(np.max(bbox[:, 1])), int(np.max(bbox[:, 0])))


class PointCloud:
    """Minimal stand-in for the open3d cloud kept in Tracker.object_cloud (callers read
    np.asarray(tracker.object_cloud.points), predict.py:424,549)."""
    def __init__(self, points):
        self.points = np.asarray(points, np.float64)


_PLY_TYPES = {"float": "f4", "float32": "f4", "double": "f8", "float64": "f8", "uchar": "u1", "uint8": "u1", "char": "i1",
              "int8": "i1", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2"}


def _read_ply(path):
    """All elements of a .ply (ascii / binary_little_endian / binary_big_endian): {element: {property: array}}; a list
    property (the faces' vertex_indices) comes back as an [count, k] array when every row has the same length k, else as
    a list of lists.  Vectorised: scalar elements are one np.frombuffer with a structured dtype, uniform list elements a
    structured view [(count, idx[k], ...)] -- a YCB scan (260 k vertices, 520 k faces) loads in milliseconds, not the tens
    of seconds a per-vertex struct.unpack takes."""
    with open(path, "rb") as f:
        assert f.readline().strip() == b"ply", "%s: not a PLY file" % path
        fmt, elems, cur = None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: PLY header without end_header" % path)
            tok = line.strip().decode().split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                cur = dict(name=tok[1], count=int(tok[2]), props=[])
                elems.append(cur)
            elif tok[0] == "property":
                cur["props"].append(tok[1:])
            elif tok[0] == "end_header":
                break
        bo = ">" if fmt == "binary_big_endian" else "<"
        data = {}
        for el in elems:
            n, props = el["count"], el["props"]
            has_list = any(p_[0] == "list" for p_ in props)
            names = [p_[-1] for p_ in props]
            if not has_list:
                if fmt == "ascii":
                    arr = np.loadtxt(f, max_rows=n, ndmin=2) if n else np.zeros((0, len(props)))
                    # every property in its DECLARED type, as plyfile returns it (the reference normalises `float` normals in float32)
                    data[el["name"]] = {nm: arr[:, i].astype(_PLY_TYPES[p_[0]]) for i, (nm, p_) in enumerate(zip(names, props))}
                else:
                    dt = np.dtype([(nm, bo + _PLY_TYPES[p_[0]]) for nm, p_ in zip(names, props)])
                    rec = np.frombuffer(f.read(dt.itemsize * n), dtype=dt, count=n)
                    data[el["name"]] = {nm: rec[nm] for nm in names}
                continue
            if fmt == "ascii":
                rows = [f.readline().split() for _ in range(n)]
                out, col = {}, [0] * n
                for p_ in props:
                    if p_[0] == "list":
                        vals = []
                        for i, r in enumerate(rows):
                            k = int(r[col[i]])
                            vals.append([int(float(x)) for x in r[col[i] + 1:col[i] + 1 + k]])
                            col[i] += 1 + k
                        ks = {len(v) for v in vals}
                        out[p_[-1]] = np.asarray(vals, np.int64).reshape(n, -1) if len(ks) == 1 else vals
                    else:
                        out[p_[-1]] = np.array([float(r[col[i]]) for i, r in enumerate(rows)]).astype(_PLY_TYPES[p_[0]])
                        col = [c + 1 for c in col]
                data[el["name"]] = out
                continue
            # binary element with list properties: try "every list has the length of the first row's" as ONE structured view
            start = f.tell()
            fields, ok = [], True
            for j, p_ in enumerate(props):
                if p_[0] == "list":
                    cnt_t, idx_t = bo + _PLY_TYPES[p_[1]], bo + _PLY_TYPES[p_[2]]
                    here = start + int(np.dtype(fields).itemsize if fields else 0)
                    f.seek(here)
                    kraw = f.read(np.dtype(cnt_t).itemsize)
                    if len(kraw) < np.dtype(cnt_t).itemsize:
                        ok = n == 0
                        break
                    k = int(np.frombuffer(kraw, dtype=cnt_t)[0])
                    fields += [("_n%d" % j, cnt_t), (p_[-1], idx_t, (k,))]
                else:
                    fields.append((p_[-1], bo + _PLY_TYPES[p_[0]]))
            f.seek(start)
            if ok and n:
                dt = np.dtype(fields)
                raw = f.read(dt.itemsize * n)
                if len(raw) == dt.itemsize * n:
                    rec = np.frombuffer(raw, dtype=dt, count=n)
                    for j, p_ in enumerate(props):
                        if p_[0] == "list" and not (rec["_n%d" % j] == dt[p_[-1]].shape[0]).all():
                            ok = False
                    if ok:
                        data[el["name"]] = {p_[-1]: (rec[p_[-1]].astype(np.int64) if p_[0] == "list" else rec[p_[-1]]) for p_ in props}
                        continue
                f.seek(start)
            # ragged lists: row by row
            out = {p_[-1]: [] for p_ in props}
            for _ in range(n):
                for p_ in props:
                    if p_[0] == "list":
                        cnt_t, idx_t = np.dtype(bo + _PLY_TYPES[p_[1]]), np.dtype(bo + _PLY_TYPES[p_[2]])
                        k = int(np.frombuffer(f.read(cnt_t.itemsize), dtype=cnt_t)[0])
                        out[p_[-1]].append(np.frombuffer(f.read(idx_t.itemsize * k), dtype=idx_t).astype(np.int64).tolist())
                    else:
                        t = np.dtype(bo + _PLY_TYPES[p_[0]])
                        out[p_[-1]].append(float(np.frombuffer(f.read(t.itemsize), dtype=t)[0]))
            data[el["name"]] = out
    return data


def load_model_points(path):
    """Vertices of a .ply (ascii / binary) or .obj model: float64 [V,3] (predict.py:131-133 reads them through open3d)."""
    if path.endswith(".obj"):
        with open(path) as f:
            vl = [l for l in f if l.startswith("v ")]
        if not vl:
            return np.zeros((0, 3))
        ntok = len(vl[0].split()) - 1
        flat = np.array(" ".join(l[2:] for l in vl).split(), dtype=np.float64)
        if flat.size == ntok * len(vl):
            return np.ascontiguousarray(flat.reshape(len(vl), ntok)[:, :3])
        return np.asarray([list(map(float, l.split()[1:4])) for l in vl], np.float64)
    v = _read_ply(path)["vertex"]
    return np.stack([np.asarray(v[k], np.float64) for k in ("x", "y", "z")], 1)


def load_ply_mesh(path):
    """Vertices, faces, vertex colours and normals of a .ply (ascii or binary), the
    fields VispyRenderer reads (vispy_renderer.py:113-127).  Non-triangular faces are dropped."""
    data = _read_ply(path)
    v = {k: np.asarray(a, np.float64) for k, a in data["vertex"].items()}
    out = dict(vertices=np.stack([v["x"], v["y"], v["z"]], 1))
    tri = np.zeros((0, 3), np.int32)
    if "face" in data:
        fl = next((a for k, a in data["face"].items() if k in ("vertex_indices", "vertex_index")), None)
        if fl is None:
            fl = next(iter(data["face"].values()))
        if isinstance(fl, np.ndarray):
            tri = fl.astype(np.int32) if fl.ndim == 2 and fl.shape[1] == 3 else tri
        else:
            tri = np.asarray([t for t in fl if len(t) == 3], np.int32).reshape(-1, 3)
    out["faces"] = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    if "red" in v:
        out["colors"] = np.stack([v["red"], v["green"], v["blue"]], 1)
    else:
        out["colors"] = np.full((len(out["vertices"]), 3), 255.0)
    # normals in the file's declared type: vispy_renderer.py:126 normalises them in whatever dtype plyfile returned (float32 for
    # `property float`), and that arithmetic reaches image A
    raw = data["vertex"]
    out["normals"] = np.stack([np.asarray(raw[k]) for k in ("nx", "ny", "nz")], 1) if "nx" in v else None
    if out["normals"] is not None and not np.all(np.linalg.norm(out["normals"].astype(np.float64), axis=1) > 0):
        out["normals"] = None
    return out


def _obj_geometry_fast(lines):
    """Vectorised parse of the v / vt / f records of an .obj whose faces are all triangles written in ONE corner format
    (v, v/vt, v/vt/vn or v//vn) -- what scanners and Blender export.  Returns (pos [P,3], col [P,3], tex [T,2] | None,
    corner index pairs [F,3,2] (vi, ti; ti = -1 without texcoords)) or None when the file needs the general parser."""
    # records are selected as the general parser selects them (first whitespace-separated token), so tab-separated or indented
    # records cannot be seen by one parser and missed by the other
    vl, tl, fl = [], [], []
    for l in lines:
        t = l.split(None, 1)
        if len(t) < 2:
            if t and t[0] in ("v", "vt", "f"):
                return None                           # a record without fields: let the general parser report it
            continue
        if t[0] == "v":
            vl.append(t[1])
        elif t[0] == "vt":
            tl.append(t[1])
        elif t[0] == "f":
            fl.append(t[1])
    if not vl or not fl:
        return None

    def uniform_tokens(recs):
        """token count shared by EVERY record, or -1"""
        cnt = np.fromiter((len(r.split()) for r in recs), dtype=np.int64, count=len(recs))
        return int(cnt[0]) if (cnt == cnt[0]).all() else -1

    nv_tok = uniform_tokens(vl)
    if nv_tok not in (3, 4, 6):
        return None
    try:
        flat = np.array(" ".join(vl).split(), dtype=np.float64)
    except ValueError:
        return None
    vv = flat.reshape(len(vl), nv_tok)
    pos = vv[:, :3]
    col = vv[:, -3:] * 255.0 if nv_tok >= 6 else np.full((len(vl), 3), 255.0)
    tex = None
    if tl:
        nt_tok = uniform_tokens(tl)
        if nt_tok < 1:
            return None
        try:
            tflat = np.array(" ".join(tl).split(), dtype=np.float64)
        except ValueError:
            return None
        tt = tflat.reshape(len(tl), nt_tok)
        tex = np.stack([tt[:, 0], tt[:, 1] if nt_tok > 1 else np.zeros(len(tl))], 1)
    # every face a triangle, every corner in the SAME format: per-line token and '/' counts (a file that mixes "1/1 2/2 3/3" with
    # "1 2 3 4 5 6" has matching flattened counts and must not be accepted: ADVICE r3)
    if uniform_tokens(fl) != 3:
        return None
    first = fl[0].split()
    nslash = first[0].count("/")
    double = "//" in first[0]
    nsl = np.fromiter((r.count("/") for r in fl), dtype=np.int64, count=len(fl))
    ndb = np.fromiter((r.count("//") for r in fl), dtype=np.int64, count=len(fl))
    if not (nsl == 3 * nslash).all() or not (ndb == (3 if double else 0)).all():
        return None
    # ... and per TOKEN: "1/4 2/3/1 4" has 3 tokens and 3 slashes like "1/4 2/3 4/1" (ADVICE r4); only when a line's count
    # matches are its tokens looked at one by one
    if nslash and any(t.count("/") != nslash or ("//" in t) != double for r in fl for t in r.split()):
        return None
    joined = " ".join(fl)
    if double:
        joined = joined.replace("//", "/0/")
    ncomp = nslash + 1
    try:
        ints = np.array(joined.replace("/", " ").split(), dtype=np.int64)
    except ValueError:
        return None
    if ints.size != len(fl) * 3 * ncomp:
        return None                                   # an empty slot ("1/ 2/ 3/"): general parser
    c = ints.reshape(len(fl), 3, ncomp)
    if (c[..., 0] <= 0).any() or (ncomp >= 2 and not double and (c[..., 1] < 0).any()):
        return None                                   # relative (negative) indices depend on the line order
    vi = c[..., 0] - 1
    if ncomp >= 2 and not double and tex is not None:
        ti = c[..., 1] - 1                            # "v/" with an empty vt slot never parses as an int: general path
    else:
        ti = np.full_like(vi, -1)
    if vi.min() < 0 or vi.max() >= len(vl) or (tex is not None and (ti.max() >= len(tl))):
        return None
    return pos, col, tex, np.stack([vi, ti], -1)


def load_obj_mesh(path):
    """Wavefront .obj as the reference's pyrender route reads it through trimesh (offscreen_renderer.py:60-63):
    vertices, triangles (polygons fan-triangulated), texture coordinates, the material's diffuse texture (map_Kd)
    and Kd.  Vertices are split per distinct (position, texcoord) pair so that every vertex carries one uv, numbered in
    order of first use.  Triangle meshes in one corner format take a vectorised parser (a 260 k-vertex YCB `textured.obj`
    in about a second); anything else the general line-by-line one.  Both give identical results.
    Returns dict(vertices [V,3], faces [F,3] int32, uv [V,2] | None, colors [V,3] 0..255, texture uint8 [h,w,3] | None,
    kd [3], normals None)."""
    import os
    with open(path) as f:
        lines = f.read().splitlines()
    mtllib = next((l.split(None, 1)[1].strip() for l in lines if l.startswith("mtllib ") and len(l.split(None, 1)) > 1), None)
    fast = _obj_geometry_fast(lines)
    if fast is not None:
        pos, col, tex, corners = fast
        flat = corners.reshape(-1, 2)
        # distinct (vi, ti) pairs numbered by first occurrence (the general parser's dict order)
        key = flat[:, 0] * (int(flat[:, 1].max()) + 2) + (flat[:, 1] + 1)
        uniq, first_idx, inv = np.unique(key, return_index=True, return_inverse=True)
        order = np.argsort(first_idx, kind="stable")
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        sel = flat[first_idx[order]]
        out = dict(vertices=np.ascontiguousarray(pos[sel[:, 0]], np.float64), faces=rank[inv.reshape(-1)].astype(np.int32).reshape(-1, 3),
                   uv=(np.where(sel[:, 1:2] >= 0, tex[np.maximum(sel[:, 1], 0)], 0.0) if tex is not None else None),
                   colors=np.ascontiguousarray(col[sel[:, 0]], np.float64), texture=None, kd=np.ones(3), normals=None)
    else:
        out = _load_obj_geometry_general(lines)
    if mtllib:
        mpath = os.path.join(os.path.dirname(path), mtllib)
        if os.path.isfile(mpath):
            for line in open(mpath):
                t = line.split()
                if not t:
                    continue
                if t[0] == "Kd" and len(t) >= 4:
                    out["kd"] = np.array([float(x) for x in t[1:4]])
                elif t[0] == "map_Kd":
                    tpath = os.path.join(os.path.dirname(mpath), line.split(None, 1)[1].strip())
                    if os.path.isfile(tpath):
                        from PIL import Image
                        out["texture"] = np.ascontiguousarray(np.array(Image.open(tpath).convert("RGB")), dtype=np.uint8)
    if out["texture"] is not None and np.all(out["kd"] == 0):
        out["kd"] = np.ones(3)   # exporters write Kd 0 0 0 next to a map_Kd; trimesh then takes the texture as the colour
    return out


def _load_obj_geometry_general(lines):
    """Line-by-line .obj geometry: polygons (fan triangulation), mixed corner formats, negative indices."""
    pos, tex, col, corners, faces = [], [], [], {}, []
    out_v, out_uv, out_c = [], [], []

    def corner(tok):
        parts = tok.split("/")
        vi = int(parts[0]); vi = vi - 1 if vi > 0 else len(pos) + vi
        ti = -1
        if len(parts) > 1 and parts[1]:
            ti = int(parts[1]); ti = ti - 1 if ti > 0 else len(tex) + ti
        key = (vi, ti)
        if key not in corners:
            corners[key] = len(out_v)
            out_v.append(pos[vi]); out_c.append(col[vi])
            out_uv.append(tex[ti] if ti >= 0 else (0.0, 0.0))
        return corners[key]

    for line in lines:
        t = line.split()
        if not t:
            continue
        if t[0] == "v":
            pos.append(tuple(float(x) for x in t[1:4]))
            col.append(tuple(float(x) * 255.0 for x in t[4:7]) if len(t) >= 7 else (255.0, 255.0, 255.0))
        elif t[0] == "vt":
            tex.append((float(t[1]), float(t[2]) if len(t) > 2 else 0.0))
        elif t[0] == "f":
            idx = [corner(tok) for tok in t[1:]]
            for k in range(1, len(idx) - 1):
                faces.append((idx[0], idx[k], idx[k + 1]))
    return dict(vertices=np.asarray(out_v, np.float64).reshape(-1, 3), faces=np.asarray(faces, np.int32).reshape(-1, 3),
                uv=np.asarray(out_uv, np.float64).reshape(-1, 2) if tex else None,
                colors=np.asarray(out_c, np.float64).reshape(-1, 3), texture=None, kd=np.ones(3), normals=None)


def vertex_normals(vertices, faces):
    """Area-weighted vertex normals for meshes that store none."""
    v = np.asarray(vertices, np.float64)
    n = np.zeros_like(v)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    ln = np.linalg.norm(n, axis=1)
    n[ln > 0] /= ln[ln > 0, None]
    n[ln == 0] = (0, 0, 1)
    return n


def voxel_down_sample(points, voxel_size=0.005):
    """open3d PointCloud.voxel_down_sample restated: grid origin = min_bound - voxel/2, one
    averaged point per occupied voxel (predict.py:133)."""
    pts = np.asarray(points, np.float64)
    origin = pts.min(0) - voxel_size * 0.5
    idx = np.floor((pts - origin) / voxel_size).astype(np.int64)
    _, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    out = np.zeros((inv.max() + 1, 3))
    np.add.at(out, inv, pts)
    return out / np.bincount(inv)[:, None]


def voxel_down_sample_normals(points, normals, voxel_size=0.005):
    """voxel_down_sample for a cloud with one normal per point -> (points, normals): the points are voxel_down_sample's, bit for
    bit (the same statements on the same arrays), the normal of a voxel is the mean of its points' normals -- not of unit length, and
    zero where opposite faces of a thin wall share a voxel (such a point never faces the camera: only the sign of a dot product is used)."""
    pts = np.asarray(points, np.float64)
    nrm = np.asarray(normals, np.float64)
    if nrm.shape != pts.shape:
        raise ValueError("voxel_down_sample_normals: %s normals for %s points" % (nrm.shape, pts.shape))
    origin = pts.min(0) - voxel_size * 0.5
    idx = np.floor((pts - origin) / voxel_size).astype(np.int64)
    _, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    out = np.zeros((inv.max() + 1, 3))
    np.add.at(out, inv, pts)
    cnt = np.bincount(inv)[:, None]
    mean = np.zeros((inv.max() + 1, 3))
    np.add.at(mean, inv, nrm)
    return out / cnt, mean / cnt


def load_model_normals(path, points):
    """One normal per vertex of load_model_points(path) (`points`), float64 [V,3], or None when the file gives none: the normals a
    .ply stores, else vertex_normals of the model's triangles.  An .obj is read through load_obj_mesh, which splits a vertex per
    texture corner: the copies' normals are summed per position and scaled to unit length."""
    mesh = load_obj_mesh(path) if path.endswith(".obj") else load_ply_mesh(path)
    v = np.asarray(mesh["vertices"], np.float64)
    nrm = mesh.get("normals")
    if nrm is None:
        if len(mesh["faces"]) == 0:
            return None
        nrm = vertex_normals(v, mesh["faces"])
    nrm = np.asarray(nrm, np.float64)
    pts = np.asarray(points, np.float64)
    if v.shape == pts.shape and np.array_equal(v, pts):
        return nrm
    _, inv = np.unique(np.concatenate([pts, v]), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    acc = np.zeros((inv.max() + 1, 3))
    np.add.at(acc, inv[len(pts):], nrm)
    out = acc[inv[:len(pts)]]
    ln = np.linalg.norm(out, axis=1)
    out[ln > 0] /= ln[ln > 0, None]
    return out


def compute_obj_max_width(points):
    """Utils.py:101-105,450-451: convex-hull diameter in millimetres."""
    from scipy.spatial import ConvexHull, distance_matrix
    hull = ConvexHull(points)
    hp = points[hull.vertices]
    return float(np.max(distance_matrix(hp, hp))) * 1000


def quaternion_matrix(quaternion):
    """transformations.quaternion_matrix (C. Gohlke's transformations.py, which predict.py:118,372,389 call as T.quaternion_matrix):
    homogeneous rotation matrix of the quaternion (w, x, y, z); |q|^2 below 4 eps gives the identity.  Third-party rule, restated
    from the published algorithm (the package is not installable offline: parity unpinned, like cv2.Rodrigues)."""
    q = np.array(quaternion, dtype=np.float64, copy=True)
    n = np.dot(q, q)
    if n < np.finfo(float).eps * 4.0:
        return np.identity(4)
    q *= np.sqrt(2.0 / n)
    q = np.outer(q, q)
    return np.array([[1.0 - q[2, 2] - q[3, 3], q[1, 2] - q[3, 0], q[1, 3] + q[2, 0], 0.0],
                     [q[1, 2] + q[3, 0], 1.0 - q[1, 1] - q[3, 3], q[2, 3] - q[1, 0], 0.0],
                     [q[1, 3] - q[2, 0], q[2, 3] + q[1, 0], 1.0 - q[1, 1] - q[2, 2], 0.0],
                     [0.0, 0.0, 0.0, 1.0]])


def _hidden_mask(model_depth, scene_depth, tol):
    """the hidden verdict of the scene-aware crop rule (csrc/fit_rule.h: fit_hidden): valid(m) && valid(s) && s <= m + tol"""
    m = np.asarray(model_depth).astype(np.int64)
    s = np.asarray(scene_depth).astype(np.int64)
    return (m > 100) & (m < 2000) & (s > 100) & (s < 2000) & (s <= m + tol)


def fit_stats(model_depth_u16, observed_depth_u16, tol_mm, scene=None):
    """The fit record of se3tn_fit_stats (include/se3tracknet.h) in NumPy, for callers without a device image: model / observed
    depth crops in millimetres, [..., 176, 176] (any shape whose last two axes are the image) -> a structured array of shape [...]
    with the fields of se3tn_fit.  valid(d) = 100 < d < 2000; seen_px == inlier_px + front_px + behind_px.
    scene: the crop of the composed depth of the tracked objects at the same pixels, [..., 176, 176] -- the scene-aware rule of
    se3tn_color_stats_scene: a pixel with valid(m) && valid(s) && s <= m + tol_mm is hidden; it enters model_px and hidden_px and
    nothing else, every other pixel is classified as without a scene.  The record is then _lib.SCENE_CROP_FIT_DTYPE (hidden_px in
    the place of _reserved); model_px == hidden_px + (the pixels classified as before)."""
    from ._lib import FIT_DTYPE, SCENE_CROP_FIT_DTYPE
    m = np.asarray(model_depth_u16).astype(np.int64)
    o = np.asarray(observed_depth_u16).astype(np.int64)
    d, tol = o - m, int(tol_mm)
    model = (m > 100) & (m < 2000)
    shown = model if scene is None else model & ~_hidden_mask(m, scene, tol)
    seen = shown & (o > 100) & (o < 2000)
    inlier = seen & (np.abs(d) <= tol)
    rec = np.zeros(m.shape[:-2], FIT_DTYPE if scene is None else SCENE_CROP_FIT_DTYPE)
    for key, mask in (("model_px", model), ("seen_px", seen), ("inlier_px", inlier), ("front_px", seen & (d < -tol)),
                      ("behind_px", seen & (d > tol))):
        rec[key] = mask.sum(axis=(-2, -1))
    rec["sum_abs_mm"] = (np.abs(d) * inlier).sum(axis=(-2, -1))
    rec["tol_mm"] = tol
    if scene is not None:
        rec["hidden_px"] = (model & ~shown).sum(axis=(-2, -1))
    return rec


def color_stats(model_rgb, model_depth, observed_rgb, observed_depth, tol_mm, scene=None):
    """The colour record of se3tn_color_stats (include/se3tracknet.h) in NumPy: model / observed crops, rgb uint8 [..., 176, 176, 3]
    and depth uint16 mm [..., 176, 176] -> a structured array of shape [...] with the fields of se3tn_color_fit.  A pixel is compared
    exactly when it is an inlier of fit_stats: both depths valid (100 < d < 2000) and |o - m| <= tol_mm.
    scene: as fit_stats' -- the pixels hidden by a tracked surface are not compared (se3tn_color_stats_scene)."""
    from ._lib import COLOR_FIT_DTYPE
    m = np.asarray(model_depth).astype(np.int64)
    o = np.asarray(observed_depth).astype(np.int64)
    tol = int(tol_mm)
    cmp_ = (m > 100) & (m < 2000) & (o > 100) & (o < 2000) & (np.abs(o - m) <= tol)
    if scene is not None:
        cmp_ = cmp_ & ~_hidden_mask(m, scene, tol)
    cmp_ = cmp_[..., None]
    mc = np.asarray(model_rgb).astype(np.int64) * cmp_
    oc = np.asarray(observed_rgb).astype(np.int64) * cmp_
    rec = np.zeros(m.shape[:-2], COLOR_FIT_DTYPE)
    rec["px"] = cmp_.sum(axis=(-3, -2, -1))
    rec["tol_mm"] = tol
    for key, img in (("sum_m", mc), ("sum_o", oc), ("sum_mm", mc * mc), ("sum_oo", oc * oc), ("sum_mo", mc * oc), ("sum_abs", np.abs(oc - mc))):
        rec[key] = img.sum(axis=(-3, -2))
    return rec


def color_score(rec, min_px=64, per_channel=False):
    """se3tn_color_score (include/se3tracknet.h) in NumPy, the same double: the mean over R, G, B of the zero-mean normalised
    cross-correlation of the compared pixels; 0 below min_px compared pixels, a flat channel counts 0.  float for one record, float64
    array otherwise; per_channel=True: (score, z[..., 3])."""
    rec = np.asarray(rec)
    n = rec["px"].astype(np.int64)[..., None]
    sm, so = rec["sum_m"].astype(np.int64), rec["sum_o"].astype(np.int64)
    cov = n * rec["sum_mo"].astype(np.int64) - sm * so
    vm = n * rec["sum_mm"].astype(np.int64) - sm * sm
    vo = n * rec["sum_oo"].astype(np.int64) - so * so
    ok = (vm > 0) & (vo > 0) & (n >= int(min_px))
    den = np.sqrt(np.where(ok, vm, 1).astype(np.float64)) * np.sqrt(np.where(ok, vo, 1).astype(np.float64))
    z = np.where(ok, cov.astype(np.float64) / den, 0.0)
    s = ((z[..., 0] + z[..., 1]) + z[..., 2]) / 3.0
    if s.ndim == 0:
        s = float(s)
    return (s, z) if per_channel else s


def fit_ratio(rec):
    """inlier_px / model_px of fit records (0.0 where model_px == 0): float for one record, float64 array otherwise."""
    rec = np.asarray(rec)
    r = np.where(rec["model_px"] > 0, rec["inlier_px"] / np.maximum(rec["model_px"], 1), 0.0)
    return float(r) if r.ndim == 0 else r


def scene_stats(layers, rects, observed, tol_mm):
    """The rule of se3tn_scene_stats (include/se3tracknet.h, csrc/scene_fit_rule.h) in NumPy: n depth layers of one frame composed
    through a shared depth test.  layers: n uint16 millimetre sub-images, layer i of shape [y1-y0, x1-x0] of rects[i] = (x0, y0, x1,
    y1) (None or anything for an empty rectangle, x1 <= x0 or y1 <= y0); observed: uint16 [H,W].  Returns (records [n] of
    _lib.SCENE_FIT_DTYPE, ids uint8 [H,W], scene uint16 [H,W]): owner(p) = the layer with the smallest valid depth at p, ties to the
    lowest index; ids = owner + 1 or 0; every count of layer i over the frame, inlier .. behind over the pixels it owns."""
    from ._lib import SCENE_FIT_DTYPE, SCENE_MAX_OBJECTS, SCENE_MAX_PIXELS
    o = np.asarray(observed).astype(np.int64)
    if o.ndim != 2 or o.size < 1 or o.size > SCENE_MAX_PIXELS:
        raise ValueError("scene_stats: observed must be [H,W] with 1 <= H * W <= 2^21")
    H, W = o.shape
    rects = np.asarray(rects, np.int64).reshape(-1, 4)
    n, tol = len(rects), int(tol_mm)
    if not 1 <= n <= SCENE_MAX_OBJECTS or len(layers) != n or not 1 <= tol <= 65535:
        raise ValueError("scene_stats: 1 .. %d layers with one rectangle each, tol_mm in [1, 65535]" % SCENE_MAX_OBJECTS)
    M = np.zeros((n, H, W), np.int64)
    for i, (x0, y0, x1, y1) in enumerate(rects):
        if x1 <= x0 or y1 <= y0:
            continue
        if x0 < 0 or y0 < 0 or x1 > W or y1 > H:
            raise ValueError("scene_stats: rectangle %d is not empty and not inside the frame" % i)
        M[i, y0:y1, x0:x1] = np.asarray(layers[i]).astype(np.int64).reshape(y1 - y0, x1 - x0)
    valid = (M > 100) & (M < 2000)
    key = np.where(valid, M, 1 << 30)
    owner = key.argmin(0)                       # the first minimum: ties go to the lowest index
    owned = valid.any(0)
    ids = np.where(owned, owner + 1, 0).astype(np.uint8)
    scene = np.where(owned, key.min(0), 0).astype(np.uint16)
    valid_o = (o > 100) & (o < 2000)
    rec = np.zeros(n, SCENE_FIT_DTYPE)
    for i in range(n):
        visible = valid[i] & (owner == i)
        hidden = valid[i] & ~visible
        seen = visible & valid_o
        d = o - M[i]
        inlier = seen & (np.abs(d) <= tol)
        for k, mask in (("model_px", valid[i]), ("visible_px", visible), ("hidden_px", hidden), ("seen_px", seen), ("inlier_px", inlier),
                        ("front_px", seen & (d < -tol)), ("behind_px", seen & (d > tol))):
            rec[k][i] = mask.sum()
        rec["sum_abs_mm"][i] = np.abs(d)[inlier].sum()
        rec["hidden_by"][i] = np.bitwise_or.reduce(np.left_shift(1, np.unique(owner[hidden])), initial=0)
    rec["tol_mm"] = tol
    rec["n_objects"] = n
    return rec, ids, scene


def scene_ratio(rec):
    """inlier_px / visible_px of scene records, NaN where visible_px == 0 (float64 array)."""
    rec = np.asarray(rec)
    v = rec["visible_px"].astype(np.float64)
    return np.where(v > 0, rec["inlier_px"] / np.maximum(v, 1.0), np.nan)


def visible_share(rec):
    """visible_px / model_px of scene records, NaN where model_px == 0 (float64 array)."""
    rec = np.asarray(rec)
    m = rec["model_px"].astype(np.float64)
    return np.where(m > 0, rec["visible_px"] / np.maximum(m, 1.0), np.nan)


def scene_status(records, lost_below, min_visible):
    """What scene records say about each object, pure host: "occluded" when visible_px < min_visible * model_px or model_px == 0 (too
    little of it is the nearest tracked surface to judge; nothing visible at all counts as occluded whatever min_visible is), else
    "lost" when inlier_px / visible_px < lost_below, else "tracked".  A list of n strings."""
    out = []
    for r in np.atleast_1d(np.asarray(records)):
        model, visible, inlier = int(r["model_px"]), int(r["visible_px"]), int(r["inlier_px"])
        if model == 0 or visible == 0 or visible < float(min_visible) * model:
            out.append("occluded")
        elif inlier / visible < float(lost_below):
            out.append("lost")
        else:
            out.append("tracked")
    return out
