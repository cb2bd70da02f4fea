"""A float64 restatement of the reference's DTU scoring (evaluation/dtu_eval.py), for the K24 tests -- numpy and torch only, neither
sklearn nor open3d -- and the seeded synthetic scans that the golden generator (tests/golden/make_golden_dtu_eval.py) and the tests share.

    make_scan               one of the 15 synthetic scans: a jittered lat-long sphere mesh, a noisy partial scan of it, ObsMask / BB / Res
                            and a ground plane; regenerated from seeds, never stored
    sample_mesh_points      dtu_eval.py:11-20, 55-78, operation for operation in numpy (the builtin `max`, as the script intends)
    greedy_downsample       the sequential loop of :94-102 over brute-force neighbour lists (d^2 <= r^2, sklearn's reduced distance)
    nearest                 brute-force nearest neighbour in chunks: distance, smallest index of the minimum, whether the minimum is unique
    dtu_chamfer             the loop body of :49-165 on these pieces, with every intermediate

Conditions the exact comparisons rest on are asserted here, not measured: no triangle has l / thr within 1e-9 of an integer
(sample_mesh_points), no pair of points has |d^2 - r^2| <= 1e-9 r^2 (greedy_downsample)."""
import numpy as np
import torch

SCAN_IDS = (24, 37, 40, 55, 63, 65, 69, 83, 97, 105, 106, 110, 114, 118, 122)
SHUFFLE_SEED = 20260                 # scan k is shuffled by numpy.random.default_rng(SHUFFLE_SEED + k)
DENSITY, PATCH, MAX_DIST = 0.2, 2.0, 3.0         # the generator's --downsample_density, --patch_size, --max_dist
OBS_N = 40


def f32(x):
    """Round to float32 and widen again: what a PLY file with float coordinates holds."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def sphere_mesh(radius, centre, n_lat=24, n_lon=32, jitter=0.0, rng=None):
    """A lat-long sphere (vertices (n_lat + 1) * n_lon float64, triangles int32).  The two polar rings are n_lon coincident vertices
    each, and one triangle of every polar quad has zero area."""
    th = np.linspace(0.0, np.pi, n_lat + 1)
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    t, p = np.meshgrid(th, ph, indexing="ij")
    v = np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], -1).reshape(-1, 3) * radius
    if jitter:
        ring = np.ones((n_lat + 1, n_lon, 1))
        ring[0] = ring[-1] = 0.0                                   # the poles stay coincident
        v = v + jitter * rng.standard_normal(v.shape) * ring.reshape(-1, 1)
    tri = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            c, d = a + n_lon, b + n_lon
            tri += [(a, c, b), (b, c, d)]
    return v + np.asarray(centre, dtype=np.float64), np.asarray(tri, dtype=np.int32)


def make_scan(k, radius=None, n_stl=None):
    """Synthetic scan k (0 .. 14) -> dict(vertices, triangles, stl, ObsMask, BB, Res, P), coordinates float32-representable (they survive a
    PLY file).  DTU-like coordinates: hundreds of mm from the origin.  The scans differ in radius, centre, noise and mask, and:
        k = 3    a zero-area triangle with three distinct, collinear vertices and one with a repeated index
        k = 5    duplicate vertices: a copy of forty vertices, used by copies of their triangles
        k = 7    the mesh is pushed out of BB on one side: part of it fails `inbound`, part of it lies outside the ObsMask array
        k = 9    a cluster of scan points farther than max_dist from the mesh (and a part of the mesh farther than that from the scan)
    radius / n_stl override the scan's size (the generator's timing run)."""
    rng = np.random.default_rng(9100 + k)
    r = float(radius) if radius is not None else (6.0 if k == 14 else 5.0 + 0.25 * (k % 9))
    centre = np.array([40.0 + 7.0 * k, -150.0 + 11.0 * k, 620.0 + 3.0 * k])
    v, t = sphere_mesh(r, centre, jitter=0.02, rng=rng)
    v = f32(v)
    if k == 3:
        a, d = v[40], np.array([0.25, 0.5, -0.25])                 # a, a + 2 d, a + 4 d: exactly collinear, also in float32
        v = np.concatenate([v, [a + 2.0 * d, a + 4.0 * d]], 0)
        t = np.concatenate([t, [[40, len(v) - 2, len(v) - 1], [50, 50, 51]]], 0).astype(np.int32)
    if k == 5:
        dup = np.arange(100, 140)
        remap = np.arange(len(v))
        remap[dup] = len(v) + np.arange(len(dup))
        v = np.concatenate([v, v[dup]], 0)
        use = np.isin(t, dup).any(-1)
        t = np.concatenate([t, remap[t[use]]], 0).astype(np.int32)
    half = r + 2.0
    bb = np.stack([centre - half, centre + half])
    if k == 7:
        v = v + np.array([0.0, 0.0, 0.55 * r + 4.0])
    res = 2 * half / OBS_N
    obs = np.ones((OBS_N, OBS_N, OBS_N), dtype=np.uint8)
    obs[:, :, :6] = 0
    obs[(3 * k) % OBS_N:(3 * k) % OBS_N + 4, :, :] = 0             # an empty slab, elsewhere in every scan
    n = int(n_stl) if n_stl is not None else 6000 + 300 * k
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d[d[:, 0] > -0.3]                                           # a partial scan: the back of the sphere has no scan points
    stl = centre + d * (r + 0.05 * (1 + k % 3) * rng.standard_normal((len(d), 1)))
    if k == 7:
        stl = stl + np.array([0.0, 0.0, 0.55 * r + 4.0])
    if k == 9:
        far = centre + np.array([r + 6.0, 0.0, 0.0]) + 0.3 * rng.standard_normal((200, 3))
        stl = np.concatenate([stl, far], 0)
    plane = np.array([0.0, 0.0, 1.0, -(centre[2] - 0.4 * r)]) if k != 7 else np.array([0.0, 0.0, 1.0, -(centre[2] + 0.1 * r)])
    return {"vertices": f32(v), "triangles": t, "stl": f32(stl), "ObsMask": obs, "BB": f32(bb), "Res": np.array([[res]]), "P": plane.reshape(4, 1)}


# ------------------------------------------------------------------------------------------------------------------ the chain
def sample_single_tri(n1, n2, v1, v2, tri_vert):
    """dtu_eval.py:11-20."""
    c = np.mgrid[:n1 + 1, :n2 + 1]
    c += 0.5
    c[0] /= max(n1, 1e-7)
    c[1] /= max(n2, 1e-7)
    c = np.transpose(c, (1, 2, 0))
    k = c[c.sum(axis=-1) < 1]
    return v1 * k[:, :1] + v2 * k[:, 1:] + tri_vert


def sample_mesh_points(vertices, triangles, density, check=True):
    """dtu_eval.py:55-78 -> data_pcd (V + S,3) float64: the vertices, then every triangle's lattice points."""
    vertices = np.asarray(vertices, dtype=np.float64)
    tri_vert = vertices[np.asarray(triangles).astype(np.int64)]
    v1 = tri_vert[:, 1] - tri_vert[:, 0]
    v2 = tri_vert[:, 2] - tri_vert[:, 0]
    l1 = np.linalg.norm(v1, axis=-1, keepdims=True)
    l2 = np.linalg.norm(v2, axis=-1, keepdims=True)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
    non_zero_area = (area2 > 0)[:, 0]
    l1, l2, area2, v1, v2, tri_vert = [arr[non_zero_area] for arr in [l1, l2, area2, v1, v2, tri_vert]]
    thr = density * np.sqrt(l1 * l2 / area2)
    q1, q2 = l1 / thr, l2 / thr
    if check:
        for q in (q1, q2):
            q = q[np.isfinite(q) & (q < 1e6)]
            assert (np.abs(q - np.rint(q)) > 1e-9).all(), "a triangle has l / thr within 1e-9 of an integer: pick another seed"
    n1, n2 = np.floor(q1), np.floor(q2)
    new_pts = [sample_single_tri(n1[i, 0], n2[i, 0], v1[i:i + 1], v2[i:i + 1], tri_vert[i:i + 1, 0]) for i in range(len(n1))]
    return np.concatenate([vertices] + new_pts, axis=0)


def _d2(a, b):
    d = a[:, None, :] - b[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbour_pairs(points, radius, device=None, chunk=2048, check=True):
    """All ordered pairs (i, j), i != j, with d^2 <= radius^2, by brute force -> (P,2) int64 numpy, sorted by i."""
    device = device or torch.device("cpu")
    p = torch.as_tensor(np.asarray(points, dtype=np.float64), device=device)
    r2 = radius * radius
    out = []
    for s in range(0, len(p), chunk):
        d2 = _d2(p[s:s + chunk], p)
        if check:
            assert not bool(((d2 - r2).abs() <= 1e-9 * r2).any()), "a pair of points has |d^2 - r^2| <= 1e-9 r^2: pick another seed"
        ij = torch.nonzero(d2 <= r2)
        ij[:, 0] += s
        out.append(ij[ij[:, 0] != ij[:, 1]].cpu())
    return torch.cat(out).numpy() if out else np.zeros((0, 2), dtype=np.int64)


def greedy_downsample(points, radius, order=None, device=None, check=True):
    """dtu_eval.py:94-102 -> mask (n,) bool over `points`, visited in `order` (None: index order)."""
    n = len(points)
    pairs = neighbour_pairs(points, radius, device, check=check)
    start = np.searchsorted(pairs[:, 0], np.arange(n + 1))
    nbr = pairs[:, 1]
    mask = np.ones(n, dtype=np.bool_)
    for curr in (range(n) if order is None else np.asarray(order).tolist()):
        if mask[curr]:
            mask[nbr[start[curr]:start[curr + 1]]] = 0
            mask[curr] = 1
    return mask


def nearest(queries, targets, max_dist=np.inf, device=None, chunk=2048):
    """Brute force in float64 -> (dist (Q,), index (Q,) int64, unique (Q,) bool): the nearest target's distance, the smallest index that
    attains it, and whether no other target does; +inf / -1 / True where nothing is closer than max_dist."""
    device = device or torch.device("cpu")
    q = torch.as_tensor(np.asarray(queries, dtype=np.float64), device=device).reshape(-1, 3)
    t = torch.as_tensor(np.asarray(targets, dtype=np.float64), device=device).reshape(-1, 3)
    dist, idx, uniq = [], [], []
    for s in range(0, len(q), chunk):
        d2 = _d2(q[s:s + chunk], t)
        m, i = d2.min(dim=1)
        hit = d2 == m[:, None]
        first = hit.to(torch.uint8).argmax(dim=1)                  # the first index of the minimum
        dist.append(m.sqrt().cpu())
        idx.append(first.cpu())
        uniq.append((hit.sum(dim=1) == 1).cpu())
    if not dist:
        return np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    dist, idx, uniq = torch.cat(dist).numpy(), torch.cat(idx).numpy(), torch.cat(uniq).numpy()
    far = ~(dist < max_dist)
    dist[far], idx[far], uniq[far] = np.inf, -1, True
    return dist, idx, uniq


def dtu_chamfer(scan, density=DENSITY, patch=PATCH, max_dist=MAX_DIST, rng=None, points=None, device=None, check=True):
    """dtu_eval.py:49-165 for one scan dict (make_scan's) -> dict with the three means, the counts and every intermediate."""
    data_pcd = sample_mesh_points(scan["vertices"], scan["triangles"], density, check) if points is None else np.array(points, dtype=np.float64)
    n_sampled = len(data_pcd)
    rng.shuffle(data_pcd, axis=0)
    data_down = data_pcd[greedy_downsample(data_pcd, density, device=device, check=check)]
    ObsMask, BB, Res = scan["ObsMask"], scan["BB"].astype(np.float32), scan["Res"]
    inbound = ((data_down >= BB[:1] - patch) & (data_down < BB[1:] + patch * 2)).sum(axis=-1) == 3
    data_in = data_down[inbound]
    data_grid = np.around((data_in - BB[:1]) / Res).astype(np.int32)
    grid_inbound = ((data_grid >= 0) & (data_grid < np.expand_dims(ObsMask.shape, 0))).sum(axis=-1) == 3
    data_grid_in = data_grid[grid_inbound]
    in_obs = ObsMask[data_grid_in[:, 0], data_grid_in[:, 1], data_grid_in[:, 2]].astype(np.bool_)
    data_in_obs = data_in[grid_inbound][in_obs]
    stl = np.asarray(scan["stl"], dtype=np.float64)
    dist_d2s, _, _ = nearest(data_in_obs, stl, device=device)
    with np.errstate(invalid="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore")
        mean_d2s = dist_d2s[dist_d2s < max_dist].mean()
        stl_hom = np.concatenate([stl, np.ones_like(stl[:, :1])], -1)
        above = (scan["P"].reshape((1, 4)) * stl_hom).sum(-1) > 0
        stl_above = stl[above]
        dist_s2d, _, _ = nearest(stl_above, data_in, device=device)
        mean_s2d = dist_s2d[dist_s2d < max_dist].mean()
    in_obs_of_down = np.zeros(len(data_down), dtype=bool)
    in_obs_of_down[np.where(inbound)[0][grid_inbound][in_obs]] = True
    return {"d2s": float(mean_d2s), "s2d": float(mean_s2d), "overall": float((mean_d2s + mean_s2d) / 2), "n_sampled": n_sampled,
            "n_down": len(data_down), "n_in": len(data_in), "n_in_obs": len(data_in_obs), "n_stl_above": len(stl_above),
            "data_pcd": data_pcd, "data_down": data_down, "inbound": inbound, "in_obs": in_obs_of_down, "above": above,
            "data_in": data_in, "data_in_obs": data_in_obs, "stl_above": stl_above, "dist_d2s": dist_d2s, "dist_s2d": dist_s2d}
