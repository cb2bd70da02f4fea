"""A float64 restatement of the reference's validation-mesh cleaning (utils/clean_mesh.py), for the K23 tests.

    view_rays               the rays and the active mask of one view, built with torch exactly as clean_mesh.py:50-66 does
    first_hits              brute-force first hit (Moller-Trumbore in float64 over all faces; the smallest (t, face) wins), with the
                            rays whose answer a last-bit difference could change marked ambiguous
    values_after_quirk      the faces clean_mesh.py:79-92 keeps from the per-view hit lists: Counter, sort, `values[1:]`
    face_adjacency          trimesh's: pairs of faces sharing an edge used by exactly two faces (group_rows(require_count=2))
    large_components_keep   trimesh.graph.connected_components(adjacency, min_len) as a keep mask (nodes = the faces in the adjacency)
    clean_mesh_outside_frustum / clean_mesh   the chains of clean_mesh.py:38-106 and :109-130 on these pieces; the mask half is
                            gens_amd.io's (pinned by golden g14).  Where no component survives, the reference raises: these return an
                            empty mesh, as the product does.
"""
from collections import Counter

import numpy as np
import torch
import torch.nn.functional as F

AMBIGUOUS_BARY = 1e-6
AMBIGUOUS_T = 1e-5


def view_rays(intr, c2w, mask, upscale):
    """clean_mesh.py:50-66 (+ the mask of :68-69): -> rays_o (N,3), rays_d (N,3) float32, active (N,) bool on the CPU."""
    intr, c2w, mask = intr.cpu().float(), c2w.cpu().float(), mask.cpu()
    h, w = mask.shape
    ys, xs = torch.meshgrid(torch.linspace(0, h - 1, int(h * upscale)), torch.linspace(0, w - 1, int(w * upscale)), indexing="ij")
    p = torch.stack([xs, ys, torch.ones_like(ys)], dim=-1)
    p = p.view(-1, 3).float()
    p = torch.matmul(intr.inverse()[None, :3, :3], p[:, :, None]).squeeze()
    rays_d = p / torch.linalg.norm(p, ord=2, dim=-1, keepdim=True)
    rays_d = torch.matmul(c2w[None, :3, :3], rays_d[:, :, None]).squeeze()
    rays_o = c2w[None, :3, 3].expand(rays_d.shape)
    up = F.interpolate(mask.float().unsqueeze(0).unsqueeze(0), scale_factor=upscale, mode="nearest").squeeze(0).squeeze(0)
    return rays_o.contiguous(), rays_d.contiguous(), (up > 0).view(-1)


def _mt(o, d, v0, v1, v2):
    e1, e2 = v1 - v0, v2 - v0
    pv = torch.cross(d.expand(-1, e2.shape[1], -1), e2.expand(d.shape[0], -1, -1), dim=-1)
    det = (e1 * pv).sum(-1)
    ok = det != 0
    inv = 1.0 / torch.where(ok, det, torch.ones_like(det))
    tv = o - v0
    u = (tv * pv).sum(-1) * inv
    qv = torch.cross(tv, e1.expand(tv.shape[0], -1, -1), dim=-1)
    w = (d * qv).sum(-1) * inv
    t = (e2 * qv).sum(-1) * inv
    return u, w, t, ok


def first_hits(vertices, triangles, rays_o, rays_d, device=None, chunk_elems=1 << 22):
    """Brute force over every face in float64 (rays widened from their float32 values): -> face (N,) int64 (-1: miss), t (N,) float64
    (+inf: miss), ambiguous (N,) bool: the best hit lies within 1e-6 of an edge in barycentrics, or another face is hit (with the
    barycentric test loosened by 1e-6) within 1e-5 t of the best, or the ray misses but grazes a face within that tolerance."""
    device = device or torch.device("cpu")
    V = torch.as_tensor(np.asarray(vertices), dtype=torch.float64, device=device)
    T = torch.as_tensor(np.asarray(triangles).astype(np.int64), device=device)
    ro = torch.as_tensor(rays_o, device=device).double().reshape(-1, 3)
    rd = torch.as_tensor(rays_d, device=device).double().reshape(-1, 3)
    n, nf = ro.shape[0], T.shape[0]
    face = torch.full((n,), -1, dtype=torch.int64, device=device)
    tt = torch.full((n,), float("inf"), dtype=torch.float64, device=device)
    amb = torch.zeros(n, dtype=torch.bool, device=device)
    if nf == 0 or n == 0:
        return face.cpu(), tt.cpu(), amb.cpu()
    v0, v1, v2 = (V[T[:, k]][None] for k in range(3))
    step = max(1, chunk_elems // nf)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=device)
    idx = torch.arange(nf, device=device)
    for s in range(0, n, step):
        o, d = ro[s:s + step, None], rd[s:s + step, None]
        u, w, t, ok = _mt(o, d, v0, v1, v2)
        bary = torch.minimum(torch.minimum(u, w), 1 - u - w)
        strict = ok & (bary >= 0) & (t > 0)
        loose = ok & (bary >= -AMBIGUOUS_BARY) & (t > 0)
        ts = torch.where(strict, t, inf)
        best = ts.min(1)
        f = torch.argmin(ts, 1)                   # (the first of equal minima: the smallest face index)
        hit = torch.isfinite(best.values)
        face[s:s + step] = torch.where(hit, f, torch.full_like(f, -1))
        tt[s:s + step] = best.values
        tl = torch.where(loose & (idx[None] != f[:, None]), t, inf).min(1).values
        near_edge = bary.gather(1, f[:, None])[:, 0] < AMBIGUOUS_BARY
        rival = tl <= torch.where(hit, best.values, torch.full_like(tl, float("inf"))) * (1 + AMBIGUOUS_T)
        amb[s:s + step] = (hit & (near_edge | rival)) | (~hit & loose.any(1))
    return face.cpu(), tt.cpu(), amb.cpu()


def values_after_quirk(hit_lists, num_com_vis=1):
    """clean_mesh.py:79-92: per-view arrays of first-hit face indices (-1 for a miss) -> the kept face indices (sorted, `values[1:]`)."""
    all_indices = np.concatenate([np.unique(np.asarray(h, dtype=np.int64)) for h in hit_lists]) if len(hit_lists) else np.zeros(0, np.int64)
    values = sorted(int(e) for e, c in Counter(all_indices.tolist()).items() if c >= num_com_vis)
    return np.asarray(values[1:], dtype=np.int64)


def face_adjacency(triangles):
    """trimesh's face_adjacency: (P,2) face pairs across edges used by exactly two faces, pairs of a face with itself dropped."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(tri) == 0:
        return np.zeros((0, 2), np.int64)
    edges = np.sort(np.stack([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]], 1).reshape(-1, 2), axis=1)
    face_of = np.repeat(np.arange(len(tri)), 3)
    _, inv, cnt = np.unique(edges, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    two = cnt[inv] == 2
    order = np.argsort(inv[two], kind="stable")
    pairs = face_of[two][order].reshape(-1, 2)
    return pairs[pairs[:, 0] != pairs[:, 1]]                # (trimesh drops a degenerate face's pair with itself)


def large_components_keep(pairs, n_faces, min_len):
    """trimesh.graph.connected_components(pairs, min_len=min_len) as a keep mask over n_faces faces (nodes: the faces in `pairs`)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    keep = np.zeros(n_faces, dtype=bool)
    if len(pairs) == 0:
        return keep
    _, label = connected_components(coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n_faces, n_faces)),
                                    directed=False)
    nodes = np.zeros(n_faces, dtype=bool)
    nodes[pairs.reshape(-1)] = True
    size = np.bincount(label[nodes], minlength=n_faces)
    return nodes & (size[label] >= min_len)


def remove_unreferenced(vertices, triangles):
    v = np.asarray(vertices)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    used = np.zeros(len(v), dtype=bool)
    used[t.reshape(-1)] = True
    return v[used], (np.cumsum(used) - 1)[t]


def frustum_hit_lists(vertices, triangles, masks, intrs, c2ws, upscale, device=None):
    """clean_mesh.py:45-78: per view, the first-hit faces of the masked rays (-1 for a miss) -> (lists, any ambiguous masked ray)."""
    lists, amb_any = [], False
    for i in range(masks.shape[0]):
        ro, rd, act = view_rays(intrs[i], c2ws[i], masks[i], upscale)
        face, _, amb = first_hits(vertices, triangles, ro[act], rd[act], device=device)
        lists.append(np.unique(face.numpy()))
        amb_any = amb_any or bool(amb.any())
    return lists, amb_any


def clean_mesh_outside_frustum(vertices, triangles, masks, intrs, c2ws, upscale=4, min_faces=500, device=None):
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    lists, _ = frustum_hit_lists(vertices, tri, masks, intrs, c2ws, upscale, device)
    hull = np.zeros(len(tri), dtype=bool)
    hull[values_after_quirk(lists)] = True
    tri = tri[hull]
    tri = tri[large_components_keep(face_adjacency(tri), len(tri), min_faces)]
    return remove_unreferenced(vertices, tri)


def clean_mesh(vertices, triangles, masks, intrs, c2ws, dilation_radius=11, min_nb_visible=1, upscale=2, min_faces=500, device=None):
    from gens_amd import io
    masks = masks.cpu()
    if masks.dim() > 3:
        masks = masks.mean(dim=-1)
    kept = io.clean_mesh_by_mask(vertices, triangles, io.dilate_masks(masks, dilation_radius), intrs, c2ws, min_nb_visible)
    return clean_mesh_outside_frustum(vertices, kept, masks, intrs, c2ws, upscale=upscale, min_faces=min_faces, device=device)
