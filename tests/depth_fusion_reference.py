"""K32 restated with numpy, straight from its definition (include/gens_hip.h, K32): the camera table, the per-pixel fusion rule and the
points of the kept pixels.  The GPU tests compare the device against these, the CPU tests pin the restatement itself on an analytic scene
and planted pixels.  Nothing here imports the library.

Every float64 operation is a numpy float64 operation of its own: numpy never contracts, so each is rounded once, in the order written.
Sums are spelled out element by element -- no `@`, einsum or hypot, which BLAS and libm may fuse or reorder."""
import numpy as np

D = np.float64


def cams_table(intrs, c2ws):
    """(nv, 24) float64: per view P = K[:3,:3] w2c[:3,:4] (12), B = inverse(K[:3,:3] w2c[:3,:3]) (9), the camera centre (3).  The kernels and
    the restatement read the same table, so how it is inverted here does not enter a comparison (ops.fusion_cams builds the shipped one)."""
    intrs, c2ws = np.asarray(intrs, dtype=D), np.asarray(c2ws, dtype=D)
    out = np.zeros((len(c2ws), 24), D)
    for v in range(len(c2ws)):
        k, w2c = intrs[v][:3, :3], np.linalg.inv(c2ws[v])
        out[v, :12] = np.dot(k, w2c[:3, :4]).reshape(-1)
        out[v, 12:21] = np.linalg.inv(np.dot(k, w2c[:3, :3])).reshape(-1)
        out[v, 21:] = c2ws[v][:3, 3]
    return out


def usable(d):
    with np.errstate(all="ignore"):
        return np.isfinite(d) & (d > 0)


def ray_row(b, i, x, y):
    """row i of B [x, y, 1] = (B[i][0] x + B[i][1] y) + B[i][2]; b: the 9 values."""
    return (b[3 * i] * x + b[3 * i + 1] * y) + b[3 * i + 2]


def proj_row(p, i, x0, x1, x2):
    """row i of P [X, 1] = ((P[i][0] X0 + P[i][1] X1) + P[i][2] X2) + P[i][3]; p: the 12 values."""
    return ((p[4 * i] * x0 + p[4 * i + 1] * x1) + p[4 * i + 2] * x2) + p[4 * i + 3]


def default_pairs(nv):
    """Every other view votes: (nv, nv - 1) int32."""
    return np.array([[s for s in range(nv) if s != r] for r in range(nv)], dtype=np.int32).reshape(nv, max(nv - 1, 0))


def check_pairs(pairs, nv):
    pairs = np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[0] != nv:
        raise ValueError(f"pairs is (nv, k), not {pairs.shape}")
    for r in range(nv):
        for s in pairs[r]:
            if s != -1 and (s < 0 or s >= nv or s == r):
                raise ValueError(f"pairs[{r}] lists view {s}")
    return pairs.astype(np.int32)


def fuse(depth, cams, pairs=None, pix_tol=1.0, rel_tol=0.01, min_views=3, normal=None, normal_cos=None):
    """The definition on host arrays -> (votes (nv, H, W) uint8, keep (nv, H, W) bool, fused (nv, H, W) float64)."""
    depth = np.asarray(depth, dtype=np.float32)
    nv, h, w = depth.shape
    cams = np.asarray(cams, dtype=D).reshape(nv, 24)
    pairs = default_pairs(nv) if pairs is None else check_pairs(pairs, nv)
    use_normal = normal is not None and normal_cos is not None
    if use_normal:
        normal = np.asarray(normal, dtype=np.float32).reshape(nv, h, w, 3)
    pix_tol2 = D(pix_tol) * D(pix_tol)
    votes, fused = np.zeros((nv, h, w), np.int64), np.zeros((nv, h, w), D)
    ys_, xs_ = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x, y = xs_.reshape(-1).astype(D), ys_.reshape(-1).astype(D)
    with np.errstate(all="ignore"):
        for r in range(nv):
            pr, br, cr = cams[r, :12], cams[r, 12:21], cams[r, 21:]
            d = depth[r].reshape(-1).astype(D)
            ok = usable(depth[r].reshape(-1))
            X = [cr[i] + d * ray_row(br, i, x, y) for i in range(3)]
            n, dsum = np.zeros(h * w, np.int64), np.zeros(h * w, D)
            for s in pairs[r]:
                if s < 0:
                    continue
                ps, bs, cs = cams[s, :12], cams[s, 12:21], cams[s, 21:]
                qz = proj_row(ps, 2, *X)
                vote = ok & (qz > 0)
                xs, ys = proj_row(ps, 0, *X) / qz, proj_row(ps, 1, *X) / qz
                x0, y0 = np.floor(xs), np.floor(ys)
                vote &= (0 <= x0) & (x0 + 1 <= w - 1) & (0 <= y0) & (y0 + 1 <= h - 1)
                xi, yi = np.where(vote, x0, 0).astype(np.int64), np.where(vote, y0, 0).astype(np.int64)
                xi1, yi1 = np.minimum(xi + 1, w - 1), np.minimum(yi + 1, h - 1)      # (only clamps pixels that do not vote)
                t00, t01, t10, t11 = depth[s, yi, xi], depth[s, yi, xi1], depth[s, yi1, xi], depth[s, yi1, xi1]
                vote &= usable(t00) & usable(t01) & usable(t10) & usable(t11)
                fx, fy = xs - x0, ys - y0
                gx, gy = 1.0 - fx, 1.0 - fy
                ds = (t00.astype(D) * gx + t01.astype(D) * fx) * gy + (t10.astype(D) * gx + t11.astype(D) * fx) * fy
                Xs = [cs[i] + ds * ray_row(bs, i, xs, ys) for i in range(3)]
                bz = proj_row(pr, 2, *Xs)
                vote &= bz > 0
                ex, ey = proj_row(pr, 0, *Xs) / bz - x, proj_row(pr, 1, *Xs) / bz - y
                vote &= (ex * ex + ey * ey) < pix_tol2
                vote &= (np.abs(bz - d) / d) < D(rel_tol)
                if use_normal:
                    xn, yn = np.where(vote, np.floor(xs + 0.5), 0).astype(np.int64), np.where(vote, np.floor(ys + 0.5), 0).astype(np.int64)
                    na, nb = normal[r].reshape(-1, 3).astype(D), normal[s, yn, xn].astype(D)
                    dot = (na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1]) + na[:, 2] * nb[:, 2]
                    vote &= dot >= D(normal_cos)
                n = n + vote
                dsum = np.where(vote, dsum + bz, dsum)
            kept = n >= int(min_views)
            votes[r] = n.reshape(h, w)
            fused[r] = np.where(kept, (d + dsum) / (n + 1).astype(D), 0.0).reshape(h, w)
    keep = votes >= int(min_views)
    return np.minimum(votes, 255).astype(np.uint8), keep, fused


def points(fused, cams, pixel):
    """point = c_r + fused (B_r [x, y, 1]) for the flat pixel indices `pixel` -> (N, 3) float64."""
    fused = np.asarray(fused, dtype=D)
    nv, h, w = fused.shape
    cams = np.asarray(cams, dtype=D).reshape(nv, 24)
    pixel = np.asarray(pixel, dtype=np.int64).reshape(-1)
    r, rem = pixel // (h * w), pixel % (h * w)
    y, x = (rem // w).astype(D), (rem % w).astype(D)
    f = fused.reshape(-1)[pixel]
    out = np.zeros((len(pixel), 3), D)
    for i in range(3):
        out[:, i] = cams[r, 21 + i] + f * ((cams[r, 12 + 3 * i] * x + cams[r, 12 + 3 * i + 1] * y) + cams[r, 12 + 3 * i + 2])
    return out


def cloud(depth, cams, normal=None, img=None, **kw):
    """fuse + points of the kept pixels in index order -> dict: votes, keep, fused, pixel, points, and normals / colors where maps are given."""
    votes, keep, fused = fuse(depth, cams, normal=normal, **kw)
    pixel = np.nonzero(keep.reshape(-1))[0].astype(np.int64)
    out = {"votes": votes, "keep": keep, "fused": fused, "pixel": pixel, "points": points(fused, cams, pixel)}
    if normal is not None:
        out["normals"] = np.asarray(normal, dtype=np.float32).reshape(-1, 3)[pixel]
    if img is not None:
        out["colors"] = np.asarray(img, dtype=np.uint8).reshape(-1, 3)[pixel]
    return out


# ---------------------------------------------------------------------------------------------------------------- shared test inputs
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """c2w (4, 4) float64 of a camera at `eye` looking at `target`: +z forward, +x right, +y down (the pinhole convention of the rays)."""
    eye, target, up = (np.asarray(v, dtype=D) for v in (eye, target, up))
    f = target - eye
    f = f / np.sqrt((f * f).sum())
    rgt = np.cross(f, up)
    rgt = rgt / np.sqrt((rgt * rgt).sum())
    dwn = np.cross(f, rgt)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = rgt, dwn, f, eye
    return m


def intrinsics(h, w, f):
    k = np.eye(4)
    k[0, 0] = k[1, 1] = f
    k[0, 2], k[1, 2] = w / 2 - 0.5, h / 2 - 0.5
    return k


def sphere_scene(nv=6, h=48, w=64, f=60.0, dist=2.0, radius=0.5, step=0.35):
    """A sphere of `radius` at the origin seen by nv look-at cameras at distance `dist`, azimuth step * i, height 0.4 sin(3 a), up +z ->
    (depth (nv, h, w) float32 analytic z-depth, 0 where the ray misses; normal (nv, h, w, 3) float32 outward unit normals; intrs, c2ws)."""
    intrs = np.stack([intrinsics(h, w, f)] * nv)
    c2ws = []
    for i in range(nv):
        a = step * i
        z = 0.4 * np.sin(3 * a)
        rho = np.sqrt(dist * dist - z * z)
        c2ws.append(look_at((rho * np.cos(a), rho * np.sin(a), z)))
    c2ws = np.stack(c2ws)
    depth, normal = np.zeros((nv, h, w), np.float32), np.zeros((nv, h, w, 3), np.float32)
    ys, xs = np.meshgrid(np.arange(h, dtype=D), np.arange(w, dtype=D), indexing="ij")
    for v in range(nv):
        kinv = np.linalg.inv(intrs[v][:3, :3])
        dc = np.stack([kinv[i, 0] * xs + kinv[i, 1] * ys + kinv[i, 2] for i in range(3)], axis=-1)      # camera-frame ray, z = 1
        dw = np.stack([c2ws[v][i, 0] * dc[..., 0] + c2ws[v][i, 1] * dc[..., 1] + c2ws[v][i, 2] * dc[..., 2] for i in range(3)], axis=-1)
        o = c2ws[v][:3, 3]
        aa, bb, cc = (dw * dw).sum(-1), (dw * o).sum(-1), (o * o).sum() - radius * radius
        disc = bb * bb - aa * cc
        hit = disc > 0
        t = np.where(hit, (-bb - np.sqrt(np.where(hit, disc, 0.0))) / aa, 0.0)                # z-depth: the ray has z = 1 in the camera
        hit &= t > 0
        depth[v] = np.where(hit, t, 0.0)
        p = o + t[..., None] * dw
        normal[v] = np.where(hit[..., None], p / radius, 0.0)
    return depth, normal, intrs, c2ws


def planted_scene():
    """Pixels for every branch of the rule.  Three cameras, 6 x 8 pixels, f = 4, principal point (3.5, 2.5):
    views 0 and 1 face each other's scene: view 1 is view 0 moved 0.5 to the right (+x), both look down +z at a fronto-parallel plane
    z = 2 (depth 2 everywhere: a pixel x of view 0 lands on x - 1 of view 1); view 2 looks the opposite way from far off and sees
    neither (every point of theirs is behind it, and its own points are behind them).
    -> (depth (3, 6, 8) float32, normal (3, 6, 8, 3) float32, cams (3, 24), cases), cases: name -> (r, y, x) of the planted pixel."""
    h, w, f = 6, 8, 4.0
    intrs = np.stack([intrinsics(h, w, f)] * 3)
    c2ws = np.stack([np.eye(4), np.eye(4), look_at((0.0, 0.0, -50.0), (0.0, 0.0, -60.0), up=(0.0, 1.0, 0.0))])
    c2ws[1, 0, 3] = 0.5                                        # disparity f * 0.5 / 2 = 1 pixel, exactly
    depth = np.full((3, h, w), 2.0, np.float32)
    normal = np.zeros((3, h, w, 3), np.float32)
    normal[..., 2] = -1.0
    cases = {}
    # unusable reference depths (row 0 of view 0)
    for x, (name, v) in enumerate((("zero", 0.0), ("negative", -2.0), ("nan", np.nan), ("inf", np.inf))):
        depth[0, 0, x] = v
        cases["unusable " + name] = (0, 0, x)
    # view 0, x = 0 projects to x = -1 in view 1: outside; view 1, x = 7 projects to x = 8 in view 0: outside
    cases["x0 < 0"] = (0, 2, 0)
    # view 1 -> view 0: xs = x + 1.  x = 6: x0 + 1 = 8 = W (refused); x = 5: x0 + 1 = 7 = W - 1 (taken)
    cases["x0 + 1 == W"] = (1, 2, 6)
    cases["x0 + 1 == W - 1"] = (1, 2, 5)
    # one unusable tap of four: view 0 pixel (4, 5) reads view 1 taps (4..5, 4..5); break (5, 5) of view 1 only
    depth[1, 5, 5] = np.nan
    cases["one unusable tap"] = (0, 4, 5)
    cases["all taps usable"] = (0, 3, 3)
    # a point behind a source and q'_z <= 0: view 2 against views 0 / 1
    cases["behind the source"] = (2, 3, 3)
    # the normal test: one pixel of view 0 whose normal is tilted by 60 degrees against view 1's (cos = 0.5)
    normal[0, 3, 2] = (np.float32(np.sqrt(0.75)), 0.0, -0.5)
    cases["normal tilted"] = (0, 3, 2)
    return depth, normal, cams_table(intrs, c2ws), cases


def back_facing_scene():
    """q'_z <= 0 in isolation.  A positive depth along a forward ray of a parallel camera never lands behind the reference, so the source
    looks back at it: view 0 at the origin looks down +z, view 1 sits at z = 4 and looks down -z; both see the plane z = 2 between them
    from opposite sides.  A pixel of view 0 projects into view 1 with q_z = 2 > 0; view 1's depth is planted as 30, which lifts to
    z = 4 - 30 = -26, behind view 0.  (With 2 in its place the views confirm each other.)  -> (depth (2, 6, 8), cams (2, 24))."""
    h, w, f = 6, 8, 4.0
    intrs = np.stack([intrinsics(h, w, f)] * 2)
    c2ws = np.stack([np.eye(4), look_at((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))])
    depth = np.full((2, h, w), 2.0, np.float32)
    depth[1] = 30.0
    return depth, cams_table(intrs, c2ws)
