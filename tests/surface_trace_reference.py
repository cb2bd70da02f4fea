"""K31 restated with numpy, straight from its definition (include/gens_hip.h, K31): the begin rule, one march round, one refine round, the
whole loop around a callable evaluator, and the pack.  The GPU tests compare the device against these, the CPU tests pin the restatement
itself on analytic fields and planted rays.  Nothing here imports the library.

Every float32 operation is a numpy float32 operation of its own: numpy never contracts, so each is rounded once, in the order written."""
import numpy as np

from . import vertex_attrs_reference as VR

LIVE, HIT, MISS, INSIDE, EXHAUSTED, BAD, BRACKET = range(7)
NAMES = {LIVE: "live", HIT: "hit", MISS: "miss", INSIDE: "inside", EXHAUSTED: "exhausted", BAD: "bad", BRACKET: "bracket"}
F = np.float32
STATE = ("t", "t_lo", "t_hi", "g_lo", "g_hi", "t_end", "dlen", "status", "steps", "points", "live")


def _f(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F))


def points_at(rays_o, rays_d, t):
    """o + t * d, un-fused float32."""
    return (rays_o + (t[:, None] * rays_d).astype(F)).astype(F)


def begin(rays_o, rays_d, near, far, lo, hi):
    """-> the state dict of every ray after the begin rule (numpy arrays; rays_o / rays_d ride along)."""
    o, d = _f(rays_o).reshape(-1, 3), _f(rays_d).reshape(-1, 3)
    n = o.shape[0]
    lo, hi = _f(lo), _f(hi)
    near = np.broadcast_to(_f(near).reshape(-1), (n,))
    far = np.broadcast_to(_f(far).reshape(-1), (n,))
    d64 = d.astype(np.float64)
    with np.errstate(all="ignore"):
        dlen = np.sqrt((d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2]).astype(F)
        finite = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
        t0, t1 = near.copy(), far.copy()
        miss = np.zeros(n, bool)
        for a in range(3):
            flat = d[:, a] == 0
            miss |= flat & ~((lo[a] <= o[:, a]) & (o[:, a] <= hi[a]))
            ta, tb = ((lo[a] - o[:, a]) / d[:, a]).astype(F), ((hi[a] - o[:, a]) / d[:, a]).astype(F)
            enter, leave = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            t0 = np.where(~flat & (enter > t0), enter, t0)
            t1 = np.where(~flat & (leave < t1), leave, t1)
        status = np.full(n, LIVE, np.uint8)
        status[miss | ~(dlen > 0) | ~(t0 < t1)] = MISS
        status[~finite] = BAD
    live = status == LIVE
    t = np.where(live, t0, F(0)).astype(F)
    s = {"rays_o": o, "rays_d": d, "t": t, "t_lo": t.copy(), "t_hi": t.copy(), "g_lo": np.zeros(n, F), "g_hi": np.zeros(n, F),
         "t_end": np.where(live, t1, F(0)).astype(F), "dlen": dlen, "status": status, "steps": np.zeros(n, np.int32),
         "points": np.zeros((n, 3), F), "live": live.astype(np.uint8)}
    with np.errstate(all="ignore"):
        s["points"][live] = points_at(o[live], d[live], t[live])
    return s


def march(s, sdf, idx, threshold, lipschitz, min_step, max_steps):
    """One march round in place: sdf (m) are the evaluator's values at the points of the rays idx (None: rays 0 .. m - 1)."""
    sdf = _f(sdf).reshape(-1)
    idx = np.arange(len(sdf)) if idx is None else np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < len(s["t"]))
    idx, sdf = idx[ok], sdf[ok]
    keep = s["status"][idx] == LIVE
    r, sdf = idx[keep], sdf[keep]
    with np.errstate(all="ignore"):
        g = (sdf + F(threshold)).astype(F)
        t = s["t"][r]
        k = s["steps"][r] + 1
        s["steps"][r] = k
        bad = ~np.isfinite(g)
        below = ~bad & (g <= 0)
        inside, bracket = below & (k == 1), below & (k != 1)
        above = ~bad & ~below
        miss = above & (t == s["t_end"][r])
        exhausted = above & ~miss & (k == max_steps)
        go = above & ~miss & ~exhausted
        st = np.full(len(r), LIVE, np.uint8)
        st[bad], st[inside], st[bracket], st[miss], st[exhausted] = BAD, INSIDE, BRACKET, MISS, EXHAUSTED
        # BRACKET
        rb = r[bracket]
        s["t_hi"][rb], s["g_hi"][rb] = t[bracket], g[bracket]
        tm = (F(0.5) * (s["t_lo"][rb] + t[bracket]).astype(F)).astype(F)
        s["t"][rb] = tm
        s["points"][rb] = points_at(s["rays_o"][rb], s["rays_d"][rb], tm)
        # LIVE
        rg = r[go]
        s["t_lo"][rg], s["g_lo"][rg] = t[go], g[go]
        q = (g[go] / F(lipschitz)).astype(F)
        step = (np.where(q > F(min_step), q, F(min_step)).astype(F) / s["dlen"][rg]).astype(F)
        tn = (t[go] + step).astype(F)
        te = s["t_end"][rg]
        t_next = np.where(tn < te, tn, te).astype(F)
        s["t"][rg] = t_next
        s["points"][rg] = points_at(s["rays_o"][rg], s["rays_d"][rg], t_next)
    s["status"][r] = st
    s["live"][r] = (st == LIVE).astype(np.uint8)
    return s


def refine(s, sdf, idx, threshold, final):
    """One refine round in place on the BRACKET rays of idx (None: rays 0 .. m - 1); sdf None: no bisection (final only)."""
    m = len(idx) if sdf is None else np.size(sdf)
    idx = np.arange(m) if idx is None else np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < len(s["t"]))
    keep = ok.copy()
    keep[ok] = s["status"][idx[ok]] == BRACKET
    r = idx[keep]
    with np.errstate(all="ignore"):
        if sdf is not None:
            g = (_f(sdf).reshape(-1)[keep] + F(threshold)).astype(F)
            tm = s["t"][r]
            below = g <= 0
            s["t_hi"][r[below]], s["g_hi"][r[below]] = tm[below], g[below]
            s["t_lo"][r[~below]], s["g_lo"][r[~below]] = tm[~below], g[~below]
        t_lo, t_hi, g_lo, g_hi = (s[k][r] for k in ("t_lo", "t_hi", "g_lo", "g_hi"))
        if final:
            w = (g_lo / (g_lo - g_hi).astype(F)).astype(F)
            t = (t_lo + ((t_hi - t_lo).astype(F) * w).astype(F)).astype(F)
            s["status"][r] = HIT
        else:
            t = (F(0.5) * (t_lo + t_hi).astype(F)).astype(F)
        s["t"][r] = t
        s["points"][r] = points_at(s["rays_o"][r], s["rays_d"][r], t)
    return s


def trace(evaluate, rays_o, rays_d, near, far, lo, hi, lipschitz, min_step, max_steps=256, refine_rounds=2, threshold=0.0, keep_first_bracket=False):
    """The whole definition.  evaluate: (m, 3) float32 points -> m signed distances.  -> (state, stats); stats as ops.sphere_trace's.
    keep_first_bracket: also return the (t_lo, t_hi) every BRACKET ray had before the refine rounds (state["first_lo"], ["first_hi"])."""
    s = begin(rays_o, rays_d, near, far, lo, hi)
    rounds = evaluated = 0
    while rounds < max_steps:
        idx = np.nonzero(s["live"])[0]
        if len(idx) == 0:
            break
        sdf = np.asarray(evaluate(s["points"][idx]), dtype=F).reshape(-1)
        evaluated += len(idx)
        rounds += 1
        march(s, sdf, idx, threshold, lipschitz, min_step, max_steps)
    assert not s["live"].any()               # (evaluation number max_steps ends every ray that is still LIVE)
    idx = np.nonzero(s["status"] == BRACKET)[0]
    if keep_first_bracket:
        s["first_lo"], s["first_hi"] = s["t_lo"].copy(), s["t_hi"].copy()
    for k in range(refine_rounds):
        sdf = np.asarray(evaluate(s["points"][idx]), dtype=F).reshape(-1)
        evaluated += len(idx)
        refine(s, sdf, idx, threshold, final=(k == refine_rounds - 1))
    if refine_rounds == 0:
        refine(s, None, idx, threshold, final=True)
    stats = {NAMES[c]: int((s["status"] == c).sum()) for c in (HIT, MISS, INSIDE, EXHAUSTED, BAD)}
    stats.update(rounds=rounds, evaluated_points=evaluated, rays=len(s["t"]))
    return s, stats


def rot_times(rot, v):
    """rot @ v per row of v as validate forms it in float32: (v0 rot[k][0] + v1 rot[k][1]) + v2 rot[k][2]."""
    rot, v = _f(rot).reshape(3, 3), _f(v)
    with np.errstate(all="ignore"):
        return np.stack([(((v[:, 0] * rot[k, 0]).astype(F) + (v[:, 1] * rot[k, 1]).astype(F)).astype(F) + (v[:, 2] * rot[k, 2]).astype(F)).astype(F)
                         for k in range(3)], axis=1)


def pack(status, t, rays_d, rot, grad=None, color=None, vis=None, normal=None):
    """Per-ray outputs of gens_surface_pack; grad / color / vis are per RAY here (rows of rays that are not hits are ignored).
    normal: the float32 unit normals to form normal_img from (default: the restatement's own, VR.normals(grad)).
    -> dict: hit, depth, and with grad: normal64 (float64, not yet rounded), normal, normal_img; with color: img, seen."""
    status = np.asarray(status, dtype=np.uint8)
    hit = status == HIT
    out = {"hit": hit}
    with np.errstate(all="ignore"):
        out["depth"] = np.where(hit, (_f(t) * rot_times(rot, rays_d)[:, 2]).astype(F), F(0)).astype(F)
        if grad is not None:
            out["normal64"] = np.where(hit[:, None], VR.normals64(grad), 0.0)
            nrm = np.where(hit[:, None], VR.normals(grad) if normal is None else _f(normal), F(0)).astype(F)
            out["normal"] = nrm
            img = ((rot_times(rot, nrm) * F(128)).astype(F) + F(128)).astype(F)
            out["normal_img"] = np.where(hit[:, None], np.minimum(np.maximum(img, F(0)), F(255)), F(0)).astype(F)
        if color is not None:
            out["img"] = np.where(hit[:, None], VR.colors(color), 0).astype(np.uint8)
            out["seen"] = hit & (VR.seen(vis) if len(hit) else np.zeros(0, bool))
    return out


# ---------------------------------------------------------------------------------------------------------------- shared test inputs
def pinhole_rays(h=48, w=64, dist=2.2, focal=3.75):
    """h x w unit rays of a pinhole camera at (0, 0, -dist) looking at the origin -> (rays_o, rays_d) float32."""
    ys, xs = np.meshgrid((np.arange(h) + 0.5) / h - 0.5, (np.arange(w) + 0.5) / w - 0.5, indexing="ij")
    d = np.stack([xs * (w / h), ys, np.full_like(xs, focal / 2)], axis=-1).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.array([0.0, 0.0, -dist]), d.shape)
    return _f(o), _f(d)


def sphere_field(p, r=0.5):
    p = np.asarray(p, dtype=np.float64)
    return (np.sqrt((p * p).sum(axis=1)) - r).astype(F)


def two_sphere_field(p):
    """min of two exact sphere distances (1-Lipschitz): r = 0.4 at (-0.3, 0, 0) and r = 0.3 at (0.35, 0.1, 0.2)."""
    p = np.asarray(p, dtype=np.float64)
    a = np.sqrt(((p - np.array([-0.3, 0.0, 0.0])) ** 2).sum(axis=1)) - 0.4
    b = np.sqrt(((p - np.array([0.35, 0.1, 0.2])) ** 2).sum(axis=1)) - 0.3
    return np.minimum(a, b).astype(F)


def poly_field(p):
    """x^2 + y^2 + z^2 - 0.25 in separate float32 multiplications and additions (|grad| = 2 |p| <= 2 sqrt(3) < 3.5 in the +-1 box)."""
    p = _f(p)
    return ((((p[:, 0] * p[:, 0]).astype(F) + (p[:, 1] * p[:, 1]).astype(F)).astype(F) + (p[:, 2] * p[:, 2]).astype(F)).astype(F) - F(0.25)).astype(F)


PLANE = (0.25, -0.5, -0.75, 0.1)


def plane_field(p):
    """a x + b y + c z + e in separate float32 operations; |grad| = |(a, b, c)| < 1."""
    p, (a, b, c, e) = _f(p), (F(v) for v in PLANE)
    return ((((p[:, 0] * a).astype(F) + (p[:, 1] * b).astype(F)).astype(F) + (p[:, 2] * c).astype(F)).astype(F) + e).astype(F)


def planted_rays():
    """Rays for every branch of the begin rule on the box +-1 with near = 0.5, far = 5 -> (rays_o, rays_d, near (n), far (n), expected status
    after begin (LIVE / MISS / BAD), names)."""
    inf, nan = np.inf, np.nan
    rows = [
        ("through the box", (0, 0, -2.2), (0, 0, 1), 0.5, 5.0, LIVE),
        ("d_x = 0 inside the slab", (0.5, 0.1, -2.2), (0, 0.01, 1), 0.5, 5.0, LIVE),
        ("d_x = 0 outside the slab", (1.5, 0, -2.2), (0, 0, 1), 0.5, 5.0, MISS),
        ("d_x = -0.0 on the slab's face", (1.0, 0, -2.2), (-0.0, 0, 1), 0.5, 5.0, LIVE),
        ("origin inside the box", (0.1, 0.2, 0.3), (0.3, -0.2, 0.9), 0.0, 5.0, LIVE),
        ("origin inside the box, near inside too", (0.1, 0.2, 0.3), (0.3, -0.2, 0.9), 0.25, 5.0, LIVE),
        ("near beyond the exit", (0, 0, -2.2), (0, 0, 1), 3.5, 5.0, MISS),
        ("far before the entry", (0, 0, -2.2), (0, 0, 1), 0.5, 1.0, MISS),
        ("far inside the box", (0, 0, -2.2), (0, 0, 1), 0.5, 2.0, LIVE),
        ("d = 0", (0, 0, 0), (0, 0, 0), 0.5, 5.0, MISS),
        ("d = 0 outside", (0, 0, -2.2), (0, 0, 0), 0.5, 5.0, MISS),
        ("|d| = 3", (0, 0, -2.2), (0, 0, 3), 0.1, 5.0, LIVE),
        ("|d| = 0.25, oblique", (0.2, -0.1, -2.2), (0.05, 0.05, 0.24), 0.5, 50.0, LIVE),
        ("pointing away", (0, 0, -2.2), (0, 0, -1), 0.5, 5.0, MISS),
        ("beside the box", (0, 3, -2.2), (0, 0, 1), 0.5, 5.0, MISS),
        ("o not finite (nan)", (nan, 0, -2.2), (0, 0, 1), 0.5, 5.0, BAD),
        ("o not finite (inf)", (0, inf, -2.2), (0, 0, 1), 0.5, 5.0, BAD),
        ("d not finite", (0, 0, -2.2), (0, -inf, 1), 0.5, 5.0, BAD),
        ("near is nan", (0, 0, -2.2), (0, 0, 1), nan, 5.0, MISS),
        ("far is inf", (0, 0, -2.2), (0, 0, 1), 0.5, inf, LIVE),
    ]
    names = [r[0] for r in rows]
    return (_f([r[1] for r in rows]), _f([r[2] for r in rows]), _f([r[3] for r in rows]), _f([r[4] for r in rows]),
            np.array([r[5] for r in rows], np.uint8), names)
