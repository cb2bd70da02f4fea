"""A float64 / numpy / torch-CPU restatement of the reference's DTU mesh finalising script (evaluation/clean_meshes.py), for the K25 tests.

    ellipse_footprint       cv.getStructuringElement(cv.MORPH_ELLIPSE, (kw, kh)) as a boolean array
    dilate                  cv.dilate with the default border: the maximum over the footprint, pixels outside the image taking no part
    vertex_votes            clean_points_by_mask's loop (:118-139) -> votes and the vertices whose projection lies within 1e-9 of a
                            half-integer in some view (numpy's matmul may or may not fuse: those are left out of exact comparisons)
    view_rays               gen_rays_from_single_image + the mask test of :235 + the 425 mm advance of :239, built with torch on the CPU
    hit_lists / values      :212-260: per-view unique first hits (-1: miss), Counter >= 2, sort; values[1:] is kept
    clean_mesh_faces_by_mask / clean_mesh_faces_outside_frustum / finalize      the chains of :144-162, :189-295, :318-344

first_hits, face_adjacency, large_components_keep and remove_unreferenced are tests/mesh_clean_reference.py's, unchanged.  Where no component
survives the reference raises: these return an empty mesh, as the product does.  make_scene builds the seeded synthetic DTU scans the
tests share: cameras 600 - 700 mm from a 100 mm object, masks from disk parameters, a mesh with a floater, an inner shell, a piece nearer
than 425 mm to one camera and regions only one view sees."""
import os
from collections import Counter

import numpy as np
import torch

import mesh_clean_reference as M

NEAR_HALF = 1e-9
VIEW_LISTS = ([23, 24, 33, 22, 15, 34, 14, 32, 16, 35, 25], [43, 33, 44, 42, 34, 32, 45, 23, 41, 24, 31])


def round_half_even(x):
    f = np.floor(x)
    d = x - f
    return int(f + (1 if d > 0.5 or (d == 0.5 and int(f) % 2 == 1) else 0))


def ellipse_footprint(kw, kh):
    r, c = kh // 2, kw // 2
    fp = np.zeros((kh, kw), dtype=bool)
    for i in range(kh):
        dy = i - r
        dx = round_half_even(c * np.sqrt((r * r - dy * dy) / (r * r))) if r else 0
        fp[i, max(c - dx, 0):min(c + dx + 1, kw)] = True
    return fp


def dilate(img, footprint):
    """img (h,w[,c]) uint8 -> the same shape: max over the footprint anchored at its centre, a border of 0."""
    img = np.asarray(img)
    kh, kw = footprint.shape
    ry, rx = kh // 2, kw // 2
    h, w = img.shape[:2]
    pad = np.zeros((h + 2 * ry, w + 2 * rx) + img.shape[2:], dtype=img.dtype)
    pad[ry:ry + h, rx:rx + w] = img
    out = np.zeros_like(img)
    for i in range(kh):
        for k in range(kw):
            if footprint[i, k]:
                np.maximum(out, pad[i:i + h, k:k + w], out=out)
    return out


def vertex_votes(points, P, masks):
    """points (V,3) float64, P (nv,4,4) float32, masks (nv,H,W) uint8 dilated channel 0 -> (votes (V,) int64, near_half (V,) bool)."""
    points = np.asarray(points, dtype=np.float64)
    nv, H, W = masks.shape
    votes = np.zeros(len(points), dtype=np.int64)
    near = np.zeros(len(points), dtype=bool)
    for i in range(nv):
        Pi = np.asarray(P[i], dtype=np.float32).astype(np.float64)
        q = points @ Pi[:3, :3].T + Pi[:3, 3]
        with np.errstate(all="ignore"):
            q = q / q[:, 2:]
            frac = np.abs(q[:, :2] - np.floor(q[:, :2]) - 0.5)
            near |= (frac < NEAR_HALF).any(1)
            r = np.rint(q[:, :2])
        ok = np.isfinite(r).all(1) & (np.abs(r) < 2147483000.0).all(1)      # (the kernel's rule: far outside any image either way)
        uv = np.where(ok[:, None], r, -10).astype(np.int64) + 1
        inside = ok & (uv[:, 0] >= 0) & (uv[:, 0] <= W) & (uv[:, 1] >= 0) & (uv[:, 1] <= H)
        framed = np.ones((H + 2, W + 2), dtype=bool)
        framed[1:-1, 1:-1] = masks[i] > 128
        votes += framed[uv[:, 1].clip(0, H + 1), uv[:, 0].clip(0, W + 1)] & inside
    return votes, near


def load_K_Rt(P34):
    """:77-98 with cv.decomposeProjectionMatrix restated by gens_amd.datasets.camera (pinned against OpenCV's results by golden g12)."""
    from gens_amd.datasets.camera import load_K_Rt_from_P
    return load_K_Rt_from_P(None, np.asarray(P34, dtype=np.float32))


def view_rays(P, mask, H, W, dep_min=425):
    """:218-239 for one view: P (4,4) float32, mask (H,W) uint8 dilated channel 0 -> the cast rays' (rays_o advanced, rays_d) float32 and
    the flat pixel indices that cast."""
    intrinsic, pose = load_K_Rt(np.asarray(P)[:3, :])
    intrinsic, c2w = torch.from_numpy(intrinsic)[:3, :3].float(), torch.from_numpy(pose).float()
    ys, xs = torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), indexing="ij")
    p = torch.stack([xs, ys, torch.ones_like(ys)], dim=-1).view(-1, 3).float()
    p = torch.matmul(torch.inverse(intrinsic)[None, :3, :3], p[:, :, None]).squeeze()
    rays_v = p / torch.linalg.norm(p, ord=2, dim=-1, keepdim=True)
    rays_v = torch.matmul(c2w[None, :3, :3], rays_v[:, :, None]).squeeze()
    rays_o = c2w[None, :3, 3].expand(rays_v.shape)
    cast = torch.from_numpy(np.asarray(mask)).reshape(-1).float() > 128
    rays_o, rays_v = rays_o[cast], rays_v[cast]
    return (rays_o + rays_v * dep_min).contiguous(), rays_v.contiguous(), torch.nonzero(cast).reshape(-1)


def hit_lists(vertices, triangles, P, masks, H, W, dep_min=425, device=None):
    """-> per view (np.unique of the first hits, -1 for a miss), and per view a (F,) bool array: the face's hit status in that view rests
    only on ambiguous rays (it is hit by ambiguous rays only, or not hit while an ambiguous ray is about)."""
    lists, shaky = [], []
    F = len(triangles)
    for i in range(len(P)):
        ro, rd, _ = view_rays(P[i], masks[i], H, W, dep_min)
        face, _, amb = M.first_hits(vertices, triangles, ro, rd, device=device)
        face, amb = face.numpy(), amb.numpy()
        lists.append(np.unique(face))
        sure = np.zeros(F, dtype=bool)
        sure[face[(face >= 0) & ~amb]] = True
        # a face is shaky in this view if no unambiguous ray hits it and some ambiguous ray exists that could (any ambiguous ray: cheap bound)
        shaky.append(~sure & bool(amb.any()) & _near_ambiguous(vertices, triangles, ro[amb], rd[amb], device))
    return lists, shaky


def _near_ambiguous(vertices, triangles, ro, rd, device):
    """(F,) bool: faces some ambiguous ray hits with the barycentric test loosened (the faces whose status such a ray can change)."""
    F = len(triangles)
    out = np.zeros(F, dtype=bool)
    if len(ro) == 0:
        return out
    V = torch.as_tensor(np.asarray(vertices), dtype=torch.float64)
    T = torch.as_tensor(np.asarray(triangles).astype(np.int64))
    v0, v1, v2 = (V[T[:, k]][None] for k in range(3))
    for s in range(0, len(ro), 256):
        u, w, t, ok = M._mt(ro[s:s + 256, None].double(), rd[s:s + 256, None].double(), v0, v1, v2)
        bary = torch.minimum(torch.minimum(u, w), 1 - u - w)
        out |= (ok & (bary >= -10 * M.AMBIGUOUS_BARY) & (t > 0)).any(0).numpy()
    return out


def values_of(lists, num_com_vis=2):
    """:248-256: the sorted entries (faces and the -1 of the misses) that at least num_com_vis views list."""
    count = Counter(np.concatenate(lists).tolist()) if len(lists) else Counter()
    return sorted(int(e) for e, c in count.items() if c >= num_com_vis)


def clean_mesh_faces_by_mask(vertices, triangles, P, masks, minimal_vis=0, mask_dilated_size=11):
    """masks (nv,H,W) uint8 channel 0 as read -> (vertices, triangles), kept vertex mask."""
    fp = ellipse_footprint(mask_dilated_size, mask_dilated_size)
    dil = np.stack([dilate(m, fp) for m in masks])
    votes, _ = vertex_votes(vertices, P, dil)
    keep = votes > minimal_vis
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    index = np.cumsum(keep) - 1
    tri = tri[keep[tri].all(1)]
    return np.asarray(vertices)[keep], index[tri], keep


def clean_mesh_faces_outside_frustum(vertices, triangles, P, masks, H=1200, W=1600, mask_dilated_size=11, dep_min=425, num_com_vis=2,
                                     min_faces=500, device=None, stats=None):
    fp = ellipse_footprint(mask_dilated_size, mask_dilated_size)
    dil = np.stack([dilate(m, fp) for m in masks])
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    lists, _ = hit_lists(np.asarray(vertices, dtype=np.float64), tri, P, dil, H, W, dep_min, device)
    values = values_of(lists, num_com_vis)
    if stats is not None:
        stats.update(n_faces=len(tri), n_values=len(values))
    keep = np.zeros(len(tri), dtype=bool)
    keep[np.asarray(values[1:], dtype=np.int64)] = True        # (a -1 can only be values[0])
    tri = tri[keep]
    tri = tri[M.large_components_keep(M.face_adjacency(tri), len(tri), min_faces)]
    return M.remove_unreferenced(vertices, tri)


# ------------------------------------------------------------------------------------------------------------------ synthetic scans
def uv_sphere(centre, radius, n_lat, n_lon):
    """A closed, manifold UV sphere: 2 + (n_lat - 1) * n_lon vertices, 2 * (n_lat - 1) * n_lon faces."""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None]], -1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radius + np.asarray(centre, dtype=np.float64)
    idx = lambda a, b: 1 + a * n_lon + (b % n_lon)  # noqa: E731
    f = []
    for b in range(n_lon):
        f.append([0, idx(0, b), idx(0, b + 1)])
        f.append([len(v) - 1, idx(n_lat - 2, b + 1), idx(n_lat - 2, b)])
    for a in range(n_lat - 2):
        for b in range(n_lon):
            f.append([idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)])
            f.append([idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)])
    return v, np.asarray(f, dtype=np.int64)


def look_at(centre, target=(0.0, 0.0, 0.0)):
    """world-to-camera (4,4) float64 of a camera at `centre` looking at `target` (z forward, y down)."""
    c, t = np.asarray(centre, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (t - c) / np.linalg.norm(t - c)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ c
    return E


def make_scene(seed, H=1200, W=1600, misses=True, n_lat=40, n_lon=60, focal_scale=1.8):
    """One synthetic scan -> dict(vertices float32 (V,3), triangles (F,3) int64, K (3,3), E (3, 4,4), disks: per view a list of
    (cx, cy, r) mask disks in pixels).  misses=True: every view's mask reaches past the object's silhouette, so at least two views have a
    masked ray that misses; False: the masks stay inside the silhouette of the big sphere, so no view has one."""
    rng = np.random.default_rng(seed)
    parts = [uv_sphere((0, 0, 0), 50.0, n_lat, n_lon),                       # the main component
             uv_sphere((0, 0, 0), 25.0, 12, 16),                             # an inner shell no ray reaches
             uv_sphere((10, 70, 5), 6.0, 8, 12)]                             # a floater below 500 faces
    centres = [np.array([650.0, 0.0, 60.0]), np.array([600.0, 260.0, 40.0]), np.array([610.0, -250.0, -30.0])]
    cam_rng = np.random.default_rng(25)                                      # (the cameras are the data set's: the same for every scan)
    centres = [c + cam_rng.uniform(-5, 5, 3) for c in centres]
    parts.append(uv_sphere(centres[0] * 0.55, 4.0, 8, 12))                   # nearer than 425 mm to camera 0, on its axis
    v, f, off = [], [], 0
    for pv, pf in parts:
        v.append(pv + rng.uniform(-1e-3, 1e-3, pv.shape))
        f.append(pf + off)
        off += len(pv)
    v, f = np.concatenate(v).astype(np.float32), np.concatenate(f)
    focal = focal_scale * W
    K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1.0]])
    E = np.stack([look_at(c) for c in centres])
    disks = []
    for i in range(3):
        r_px = focal * 50.0 / np.linalg.norm(centres[i])
        cx, cy = W / 2 - 0.5, H / 2 - 0.5
        if misses:
            d = [(cx + (0.35 if i == 0 else -0.3) * r_px, cy + 0.1 * r_px * (i - 1), (0.9 if i < 2 else 0.8) * r_px)]
            d.append((cx, cy - focal * 70.0 / 650.0 * (1 if i == 0 else 0.9), 0.2 * r_px))       # over the floater, past the silhouette
        else:
            d = [(cx + (0.2 if i == 0 else -0.15) * r_px, cy, 0.6 * r_px)]
        disks.append(d)
    return dict(vertices=v, triangles=f, K=K, E=E, disks=disks, H=H, W=W)


def disk_mask(disks, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), dtype=bool)
    for cx, cy, r in disks:
        m |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
    return (m * 255).astype(np.uint8)


def scene_P(scene):
    """The float32 K4 @ E products the script's read_cam_file returns for the scene's cameras."""
    K4 = np.float32(np.diag([1, 1, 1, 1]))
    K4[:3, :3] = scene["K"].astype(np.float32)
    return np.stack([K4 @ e.astype(np.float32) for e in scene["E"]])


def write_tree(root_dir, out_dir, scenes, view_ids, colour=False):
    """The script's file layout for {scan: scene}: cameras/{vid:0>8}_cam.txt, scan{n}/mask/{vid:0>3}.png, {out_dir}/x_scan{n}_epoch0.ply."""
    from PIL import Image
    from gens_amd import io
    os.makedirs(os.path.join(root_dir, "cameras"), exist_ok=True)
    os.makedirs(out_dir, exist_ok=True)
    first = True
    for scan, sc in scenes.items():
        os.makedirs(os.path.join(root_dir, f"scan{scan}", "mask"), exist_ok=True)
        for k, vid in enumerate(view_ids):
            if first:                                   # (the cameras are shared by the scans, as in DTU)
                with open(os.path.join(root_dir, "cameras", f"{vid:0>8}_cam.txt"), "w") as fh:
                    fh.write("extrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in sc["E"][k]) + "\n\nintrinsic\n" +
                             "\n".join(" ".join(repr(float(x)) for x in row) for row in sc["K"]) + "\n\n425.0 2.5\n")
            m = disk_mask(sc["disks"][k], sc["H"], sc["W"])
            img = np.stack([np.zeros_like(m), np.zeros_like(m), m], -1) if colour else m        # (RGB with the mask in blue: cv's channel 0)
            Image.fromarray(img).save(os.path.join(root_dir, f"scan{scan}", "mask", f"{vid:0>3}.png"))
        io.write_ply(os.path.join(out_dir, f"dtu_scan{scan}_epoch0.ply"), sc["vertices"], sc["triangles"])
        first = False


G21_SCANS = {24: dict(seed=21, misses=True, n_lat=40, n_lon=60), 37: dict(seed=22, misses=False, n_lat=80, n_lon=120)}
G21_FOCAL_SCALE = 0.9           # (masks of about 1.6 % of the image: the generator's brute-force ray stub stays within minutes on a CPU)
G21_SUBSAMPLE = 16              # every 16th cast ray of a view is stored with its first hit, for the CPU test of the ray stage


def golden_scenes():
    """The two full-size scans of golden g21 (tests/golden/make_golden_dtu_clean.py), regenerated from their seeds."""
    return {scan: make_scene(p["seed"], misses=p["misses"], n_lat=p["n_lat"], n_lon=p["n_lon"], focal_scale=G21_FOCAL_SCALE) for scan, p in G21_SCANS.items()}


def load_g21():
    """Golden g21 (the reference's own run, see tests/golden/make_golden_dtu_clean.py) -> {scan: dict(scene, P, masks (3,H,W) as read,
    near_half, keep_vertices, clean_vertices / clean_faces, runs: {"chain" | "raw": dict(vertices, triangles: the ray step's input,
    hits: per view the listed entries, listed / shaky (3,F) bool, miss (3,), printed (n_faces, n_values), keep_values (F,),
    keep_components, final_vertices, final_faces, sub_face / sub_amb / n_cast per view)})}.  The scenes are regenerated from the seeds and
    checked against the stored inputs."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_dtu_clean.npz"))
    assert float(g["focal_scale"]) == G21_FOCAL_SCALE and int(g["subsample"]) == G21_SUBSAMPLE and g["scan_ids"].tolist() == list(G21_SCANS)
    out = {}
    for scan, sc in golden_scenes().items():
        p = f"s{scan}"
        assert np.array_equal(sc["vertices"], g[f"{p}_vertices"]) and np.array_equal(sc["triangles"], g[f"{p}_triangles"])
        assert np.array_equal(scene_P(sc), g[f"{p}_P"])
        keep = g[f"{p}_keep_vertices"]
        d = dict(scene=sc, P=g[f"{p}_P"], masks=np.stack([disk_mask(k, sc["H"], sc["W"]) for k in sc["disks"]]), near_half=g[f"{p}_near_half"],
                 keep_vertices=keep, clean_vertices=sc["vertices"][keep], clean_faces=g[f"{p}_clean_faces"].astype(np.int64), runs={})
        for name in ("chain", "raw"):
            q = f"{p}_{name}"
            if f"{q}_printed" not in g:
                continue
            v, t = (d["clean_vertices"], d["clean_faces"]) if name == "chain" else (sc["vertices"], sc["triangles"])
            F = len(t)
            hits = [g[f"{q}_hits_{i}"].astype(np.int64) for i in range(3)]
            listed = np.zeros((3, F), dtype=bool)
            for i, h in enumerate(hits):
                listed[i, h[h >= 0]] = True
            kv = np.unpackbits(g[f"{q}_keep_values"])[:F].astype(bool)
            d["runs"][name] = dict(vertices=v, triangles=t, hits=hits, listed=listed, miss=g[f"{q}_miss"], printed=g[f"{q}_printed"].tolist(),
                                   shaky=np.unpackbits(g[f"{q}_shaky"], axis=1)[:, :F].astype(bool), keep_values=kv,
                                   keep_components=np.unpackbits(g[f"{q}_keep_components"])[:int(kv.sum())].astype(bool),
                                   final_vertices=g[f"{q}_final_vertices"], final_faces=g[f"{q}_final_faces"].astype(np.int64),
                                   sub_face=[g[f"{q}_sub_face_{i}"].astype(np.int64) for i in range(3)],
                                   sub_amb=[g[f"{q}_sub_amb_{i}"] for i in range(3)], n_cast=[int(g[f"{q}_n_cast_{i}"]) for i in range(3)])
        out[scan] = d
    return out
