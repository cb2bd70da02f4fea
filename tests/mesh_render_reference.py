"""K35 restated in numpy: the mesh-shading rule of include/gens_hip.h, step by step.  Arithmetic is float64 from the stored inputs, every
operation rounded on its own in the order written (numpy never contracts), results rounded once -- so gens_mesh_shade
(csrc/k35_mesh_shade.hip) equals shade() bit for bit.  Shared by tests/test_mesh_render_cpu.py and tests/test_hip_mesh_render.py."""
import numpy as np

from . import mesh_texture_reference as TR
from . import surface_trace_reference as ST

F = np.float32
OUTPUTS = ("hit", "bary", "depth", "normal", "normal_img", "img", "seen")


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def unit_normals(n):
    """K30's rule on float64 components: n / sqrt((nx^2 + ny^2) + nz^2) rounded once; zero rows where a component is not finite or the
    norm is 0."""
    with np.errstate(all="ignore"):
        norm = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = np.isfinite(n).all(axis=1) & (norm > 0)
        return np.where(ok[:, None], n / np.where(ok, norm, 1.0)[:, None], 0.0).astype(F)


def round8(x):
    """floor(x + 0.5) clamped to 0 .. 255."""
    return np.minimum(np.maximum(np.floor(x + 0.5), 0.0), 255.0).astype(np.uint8)


def hits(vertices, triangles, face, t):
    """-> (hit (n,) bool, idx (n, 3) int64: the face's indices, 0 where the ray is not a hit, so that nothing is read through a bad one)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    face, t = np.asarray(face, dtype=np.int32).reshape(-1), np.asarray(t, dtype=F).reshape(-1)
    with np.errstate(all="ignore"):
        hit = (face >= 0) & (face < tri.shape[0]) & np.isfinite(t) & (t > 0)
    idx = np.zeros((len(face), 3), dtype=np.int64)
    idx[hit] = tri[face[hit]]
    hit &= ((idx >= 0) & (idx < v.shape[0])).all(axis=1)
    idx[~hit] = 0
    if v.shape[0]:
        hit &= np.isfinite(v[idx].reshape(len(face), 9)).all(axis=1)
    idx[~hit] = 0
    return hit, idx


def barycentrics(a3, b3, c3, rays_o, rays_d, t):
    """Step 3 for rows that are hits -> (a, b, c) float64 (n,) each."""
    o, d = np.asarray(rays_o, dtype=F).astype(np.float64), np.asarray(rays_d, dtype=F).astype(np.float64)
    t = np.asarray(t, dtype=F).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        p = o + t * d
        e1, e2, w = b3 - a3, c3 - a3, p - a3
        d11, d12, d22, w1, w2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(w, e1), _dot(w, e2)
        den = d11 * d22 - d12 * d12
        b, c = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
        ok = (den > 0.0) & np.isfinite(b) & np.isfinite(c)
        b, c = np.where(b > 0.0, b, 0.0), np.where(c > 0.0, c, 0.0)
        s = b + c
        over = s > 1.0
        b, c = np.where(over, b / s, b), np.where(over, c / s, c)
        a = (1.0 - b) - c
        a = np.where(a > 0.0, a, 0.0)
    return np.where(ok, a, 1.0), np.where(ok, b, 0.0), np.where(ok, c, 0.0)


def atlas_taps(b, c, texels):
    """Step 6 -> (ip (n, 4), jp (n, 4) int64 local texels, w (n, 4) float64 weights) in the order (i0, j0), (i0 + 1, j0), (i0, j0 + 1),
    (i0 + 1, j0 + 1).  A tap whose weight is not > 0 is not read."""
    scale = np.float64(int(texels) - 2)
    x, y = b * scale, c * scale
    fi, fj = np.floor(x), np.floor(y)
    fx, fy = x - fi, y - fj
    gx, gy = 1.0 - fx, 1.0 - fy
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    ip = np.stack([i0, i0 + 1, i0, i0 + 1], axis=1)
    jp = np.stack([j0, j0, j0 + 1, j0 + 1], axis=1)
    w = np.stack([gx * gy, fx * gy, gx * fy, fx * fy], axis=1)
    return ip, jp, w


def atlas_color(face, n_faces, b, c, texels, atlas=None, atlas_seen=None):
    """-> (x (n, 3) float64 before rounding or None, seen (n,) bool or None) from the taps of atlas_taps."""
    ip, jp, w = atlas_taps(b, c, texels)
    read = w > 0.0
    px, py = TR.pixel(n_faces, texels, np.asarray(face, dtype=np.int64)[:, None], np.where(read, ip, 0), np.where(read, jp, 0))
    x = seen = None
    if atlas is not None:
        term = np.where(read[:, :, None], w[:, :, None] * np.asarray(atlas)[py, px].astype(np.float64), 0.0)
        x = ((term[:, 0] + term[:, 1]) + term[:, 2]) + term[:, 3]
    if atlas_seen is not None:
        seen = (~read | (np.asarray(atlas_seen)[py, px] != 0)).all(axis=1)
    return x, seen


def shade(vertices, triangles, rays_o, rays_d, face, t, rot, normals=None, colors=None, seen=None, texture=None, texture_seen=None, texels=None,
          shading="flat", orient=0):
    """gens_mesh_shade -> dict of every output the inputs allow: hit (bool), bary, depth, normal, normal_img, img, seen (bool); and
    "bary64", the barycentrics before their rounding."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    o, d = np.asarray(rays_o, dtype=F).reshape(-1, 3), np.asarray(rays_d, dtype=F).reshape(-1, 3)
    face, t = np.asarray(face, dtype=np.int32).reshape(-1), np.asarray(t, dtype=F).reshape(-1)
    n = len(face)
    hit, idx = hits(v, tri, face, t)
    vv = v if v.shape[0] else np.zeros((1, 3))
    a3, b3, c3 = (np.where(hit[:, None], vv[idx[:, k]], 0.0) for k in range(3))
    out = {"hit": hit}
    with np.errstate(all="ignore"):
        out["depth"] = np.where(hit, (t * ST.rot_times(rot, d)[:, 2]).astype(F), F(0)).astype(F) if n else np.zeros(0, F)
        wa, wb, wc = barycentrics(a3, b3, c3, o, d, t)
        wa, wb, wc = (np.where(hit, x, 0.0) for x in (wa, wb, wc))
        out["bary64"] = np.stack([wa, wb, wc], axis=1)
        out["bary"] = out["bary64"].astype(F)
        if shading == "smooth":
            nn = np.asarray(normals, dtype=F).reshape(-1, 3).astype(np.float64)
            nn = nn if nn.shape[0] else np.zeros((1, 3))
            g = (wa[:, None] * nn[idx[:, 0]] + wb[:, None] * nn[idx[:, 1]]) + wc[:, None] * nn[idx[:, 2]]
        else:
            e1, e2 = b3 - a3, c3 - a3
            g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            g = -g if orient else g
        nrm = np.where(hit[:, None], unit_normals(g), F(0)).astype(F)
        out["normal"] = nrm
        img = ((ST.rot_times(rot, nrm) * F(128)).astype(F) + F(128)).astype(F) if n else np.zeros((0, 3), F)
        out["normal_img"] = np.where(hit[:, None], np.minimum(np.maximum(img, F(0)), F(255)), F(0)).astype(F)
        x = s = None
        if texture is not None:
            x, s = atlas_color(np.where(hit, face, 0), tri.shape[0], wb, wc, texels, texture, texture_seen)
        elif colors is not None:
            cc = np.asarray(colors, dtype=np.uint8).reshape(-1, 3).astype(np.float64)
            cc = cc if cc.shape[0] else np.zeros((1, 3))
            x = (wa[:, None] * cc[idx[:, 0]] + wb[:, None] * cc[idx[:, 1]]) + wc[:, None] * cc[idx[:, 2]]
            if seen is not None:
                sv = np.asarray(seen).reshape(-1) != 0
                sv = sv if sv.shape[0] else np.zeros(1, bool)
                s = (~(wa > 0) | sv[idx[:, 0]]) & (~(wb > 0) | sv[idx[:, 1]]) & (~(wc > 0) | sv[idx[:, 2]])
        if x is not None:
            out["img"] = np.where(hit[:, None], round8(x), 0).astype(np.uint8)
        if s is not None:
            out["seen"] = hit & s
    return out


# ---------------------------------------------------------------------------------------------------------------- shared test inputs
ROT = np.array([0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6], dtype=F)          # a rotation with exactly representable-ish entries


def planted_mesh(n_faces, seed=0):
    """A mesh of n_faces triangles with small-integer float64 coordinates: a fan-like strip over a jittered integer grid (so faces are
    non-degenerate and differ), then planted specials in the LAST faces where n_faces allows: a repeated face, a face with a repeated
    vertex (zero area), a face with an index out of range, a face with a NaN vertex, vertices with signed zeros and subnormals.
    -> (vertices (V, 3) float64, triangles (T, 3) int32, special: dict name -> face index)."""
    rng = np.random.default_rng(seed + 1000 * n_faces)
    nv = n_faces + 2
    v = np.stack([np.arange(nv) // 2 * 3.0, (np.arange(nv) % 2) * 4.0, np.zeros(nv)], axis=1)
    v += rng.integers(-1, 2, v.shape)
    v[:, 2] += rng.integers(-2, 3, nv)
    t = np.stack([np.arange(n_faces), np.arange(n_faces) + 1, np.arange(n_faces) + 2], axis=1).astype(np.int32)
    t[1::2] = t[1::2][:, [1, 0, 2]]
    special = {}
    v = np.concatenate([v, [[np.nan, 1.0, 2.0], [-0.0, 0.0, 5e-324], [3.0, -0.0, 1e-310], [1e-320, 4.0, -0.0]]])
    if n_faces >= 9:
        k = n_faces - 5
        t[k] = t[0]
        t[k + 1] = [t[1, 0], t[1, 0], t[1, 2]]
        t[k + 2] = [0, nv + 4, 1]
        t[k + 3] = [0, nv, 1]
        t[k + 4] = [nv + 1, nv + 2, nv + 3]
        special = {"repeated_face": k, "repeated_vertex": k + 1, "bad_index": k + 2, "nan_vertex": k + 3, "tiny": k + 4}
    return v.astype(np.float64), t, special


def planted_rays(vertices, triangles, n, seed=0):
    """n rays aimed at the mesh: ray r takes face r % T (in a shuffled order) at seeded barycentrics -- corners, edge points and interior
    points in rotation -- with o = p - d and t = 1 for small-integer float32 d (so p = o + t d up to the rounding of o), then planted bad
    rays in the LAST rows where n allows: face -1, face T, face 2^31 - 1, t = +inf, NaN, 0, -1, -0.0.
    -> (rays_o, rays_d (n, 3) float32, face (n) int32, t (n) float32)."""
    rng = np.random.default_rng(seed + 7 * n)
    v, tri = np.asarray(vertices), np.asarray(triangles)
    n_f, n_v = len(tri), len(v)
    face = rng.permutation(max(n_f, 1))[np.arange(n) % max(n_f, 1)].astype(np.int32) if n else np.zeros(0, np.int32)
    w = rng.dirichlet(np.ones(3), size=n)
    kind = np.arange(n) % 5
    w[kind == 0] = np.eye(3)[rng.integers(0, 3, int((kind == 0).sum()))]
    edge = kind == 1
    w[edge, 2] = 0.0
    w[edge, 0] = 1.0 - w[edge, 1]
    w[kind == 2] = np.eye(3)[[1]]
    idx = np.clip(tri[face].astype(np.int64), 0, n_v - 1) if n_f else np.zeros((n, 3), np.int64)
    corners = np.nan_to_num(v[idx]) if n_v else np.zeros((n, 3, 3))
    p = (w[:, :, None] * corners).sum(axis=1)
    d = rng.integers(-3, 4, (n, 3)).astype(F)
    d[(d == 0).all(axis=1)] = [0, 0, 1]
    t = np.ones(n, dtype=F)
    o = (p - d).astype(F)
    bad = [(-1, 1.0), (n_f, 1.0), (2 ** 31 - 1, 1.0), (0, np.inf), (0, np.nan), (0, 0.0), (0, -1.0), (0, -0.0)]
    if n >= 2 * len(bad):
        for k, (f, tt) in enumerate(bad):
            face[n - 1 - k], t[n - 1 - k] = f, tt
    return o, d, face, t


def planted_attributes(n_vertices, n_faces, texels, seed=0):
    """Seeded vertex normals (with a zero and a NaN row), colours, seen flags, and an atlas + seen plane of K34's layout."""
    rng = np.random.default_rng(seed + n_vertices + 31 * n_faces + texels)
    normals = rng.standard_normal((n_vertices, 3)).astype(F)
    if n_vertices > 3:
        normals[1], normals[2, 0] = 0.0, np.nan
    colors = rng.integers(0, 256, (n_vertices, 3)).astype(np.uint8)
    seen = (rng.uniform(size=n_vertices) < 0.8).astype(np.uint8)
    h, w = TR.layout(n_faces, texels)[:2]
    atlas = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    atlas_seen = (rng.uniform(size=(h, w)) < 0.8).astype(np.uint8)
    return normals, colors, seen, atlas, atlas_seen
