"""K31 without a GPU: the numpy restatement of the sphere trace (tests/surface_trace_reference.py) on analytic fields and planted rays, and the
argument checks of the C entry points through ctypes with made-up pointers."""
import ctypes as C

import numpy as np
import pytest

from . import surface_trace_reference as SR

F = np.float32
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
NEAR, FAR = F(0.95 * 1.2), F(1.05 * 3.2)           # gens_amd.synthetic.make_cameras' range for a camera 2.2 units away


def _spacing(r):
    return 2.0 / (r - 1)


FIELDS = {"sphere": (SR.sphere_field, (1.0, 2.0)), "two_spheres": (SR.two_sphere_field, (1.0, 2.0)), "poly": (SR.poly_field, (3.5,))}
CASES = [(name, lip, r) for name, (_, lips) in FIELDS.items() for lip in lips for r in (64, 512)]


@pytest.mark.parametrize("name,lipschitz,r", CASES)
def test_every_ray_ends_as_a_hit_or_a_miss_and_every_crossing_is_bracketed(name, lipschitz, r):
    """48 x 64 pinhole rays from 2.2 units into the +-1 box, max_steps = 256: no ray is EXHAUSTED, INSIDE or BAD; the bracket the march
    leaves is at most min_step / |d| wide (plus the rounding of one float32 addition at t ~ 2); after two refine rounds a quarter of it."""
    o, d = SR.pinhole_rays()
    h = _spacing(r)
    s, stats = SR.trace(FIELDS[name][0], o, d, NEAR, FAR, LO, HI, lipschitz, h, max_steps=256, refine_rounds=2, keep_first_bracket=True)
    evals = stats["evaluated_points"] / len(o)
    print(f"{name} L={lipschitz} R={r}: {stats}, {evals:.2f} evaluations per ray, {s['steps'].max()} steps at most")
    assert stats["hit"] + stats["miss"] == len(o) == 3072 and stats["hit"] > 0 and stats["miss"] > 0
    assert stats["exhausted"] == stats["inside"] == stats["bad"] == 0
    hit = s["status"] == SR.HIT
    if name == "sphere":                          # every ray whose chord through the sphere is longer than min_step hits; no other ray does
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        b, c, a = (o64 * d64).sum(axis=1), (o64 * o64).sum(axis=1) - 0.25, (d64 * d64).sum(axis=1)
        disc = b * b - a * c
        chord = 2 * np.sqrt(np.maximum(disc, 0)) / np.sqrt(a)
        print(f"    analytic: {int((disc > 0).sum())} rays cross the sphere, {int(((disc > 0) & (chord <= h)).sum())} of them on a chord <= min_step")
        assert not (hit & ~(disc > 0)).any() and hit[chord > h].all()
    ulp = np.spacing(s["first_hi"][hit])
    first = (s["first_hi"][hit].astype(np.float64) - s["first_lo"][hit]) * s["dlen"][hit]
    assert (first > 0).all() and (first <= h + ulp).all()
    last = (s["t_hi"][hit].astype(np.float64) - s["t_lo"][hit]) * s["dlen"][hit]
    assert (last <= h / 4 + 4 * ulp).all()
    assert ((s["t"][hit] >= s["t_lo"][hit]) & (s["t"][hit] <= s["t_hi"][hit])).all()
    if name == "sphere":                          # an exact distance: the analytic hit lies in the final bracket
        o64, d64 = o[hit].astype(np.float64), d[hit].astype(np.float64)
        b, c = (o64 * d64).sum(axis=1), (o64 * o64).sum(axis=1) - 0.25
        a = (d64 * d64).sum(axis=1)
        t_true = (-b - np.sqrt(b * b - a * c)) / a
        width = s["t_hi"][hit].astype(np.float64) - s["t_lo"][hit]
        assert (np.abs(s["t"][hit] - t_true) <= width + 4 * ulp).all()


def test_exhausted_is_reachable():
    """max_steps = 64 at R = 512 and L = 2: grazing rays run out of steps, and are reported as such."""
    o, d = SR.pinhole_rays()
    s, stats = SR.trace(SR.sphere_field, o, d, NEAR, FAR, LO, HI, 2.0, _spacing(512), max_steps=64)
    print(stats)
    assert stats["exhausted"] > 0 and stats["rounds"] == 64
    assert (s["steps"][s["status"] == SR.EXHAUSTED] == 64).all()
    assert stats["hit"] + stats["miss"] + stats["exhausted"] == len(o)


def test_planted_rays_reach_every_branch_of_the_begin_rule_and_every_status():
    o, d, near, far, want, names = SR.planted_rays()
    s = SR.begin(o, d, near, far, LO, HI)
    for k, name in enumerate(names):
        assert s["status"][k] == want[k], name
    live = s["status"] == SR.LIVE
    assert (s["t"][live] < s["t_end"][live]).all() and (s["t"][~live] == 0).all() and (s["t_end"][~live] == 0).all()
    k = names.index("through the box")
    assert s["t"][k] == F(1.2) and s["t_end"][k] == F(3.2) and s["dlen"][k] == 1
    k = names.index("origin inside the box")
    assert s["t"][k] == 0 and 0 < s["t_end"][k] < 1
    k = names.index("far inside the box")
    assert s["t_end"][k] == 2
    k = names.index("|d| = 3")
    assert s["dlen"][k] == 3 and s["t"][k] == F(F(1.2) / F(3)) and s["t_end"][k] == F(F(3.2) / F(3))
    k = names.index("d_x = -0.0 on the slab's face")
    assert s["status"][k] == SR.LIVE
    # the whole trace on them: a sphere of radius 0.5 -> every status but EXHAUSTED (test_exhausted_is_reachable) occurs
    s, stats = SR.trace(SR.sphere_field, o, d, near, far, LO, HI, 1.0, _spacing(64))
    print(stats, dict(zip(names, (SR.NAMES[c] for c in s["status"]))))
    assert stats["hit"] > 0 and stats["miss"] > 0 and stats["inside"] > 0 and stats["bad"] > 0 and stats["exhausted"] == 0
    assert s["status"][names.index("origin inside the box")] == SR.INSIDE          # |(0.1, 0.2, 0.3)| < 0.5: the first evaluation is below
    k3, k1 = names.index("|d| = 3"), names.index("through the box")
    assert s["status"][k3] == SR.HIT and abs(s["t"][k3] * 3 - s["t"][k1]) < 1e-5    # t counts in units of d
    # a field that turns non-finite on the way: BAD from the march
    nan_field = lambda p: np.where(p[:, 2] > -0.8, np.nan, SR.sphere_field(p)).astype(F)  # noqa: E731
    s2, stats2 = SR.trace(nan_field, o[:1], d[:1], near[:1], far[:1], LO, HI, 1.0, _spacing(64))
    assert s2["status"][0] == SR.BAD and stats2["bad"] == 1


def test_march_and_refine_rules_on_planted_values():
    """One round each on a hand-made state: every row of the march table, -0.0 counted as 0, the refine ends and the interpolation."""
    n = 10
    o, d = np.zeros((n, 3), F), np.tile(F([0, 0, 2]), (n, 1))
    s = SR.begin(o - F([0, 0, 4]), d, F(0.0), F(10.0), LO, HI)
    assert (s["status"] == SR.LIVE).all() and (s["t"] == 1.5).all() and (s["t_end"] == 2.5).all() and (s["dlen"] == 2).all()
    s["steps"][:] = [0, 0, 3, 3, 3, 3, 254, 255, 3, 3]
    s["t"][5] = s["t_end"][5]
    s["t_lo"][:], s["g_lo"][:] = 1.25, 0.5
    g = F([np.nan, -1.0, -0.0, 0.0, np.inf, 0.25, 0.25, 0.25, np.finfo(F).tiny, 1.0])
    SR.march(s, g, None, 0.0, 2.0, 0.125, 256)
    assert s["status"].tolist() == [SR.BAD, SR.INSIDE, SR.BRACKET, SR.BRACKET, SR.BAD, SR.MISS, SR.LIVE, SR.EXHAUSTED, SR.LIVE, SR.LIVE]
    assert s["live"].tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 1, 1]
    assert s["t"][6] == F(1.5 + 0.125 / 2) and s["t"][9] == F(1.5 + 0.5 / 2) and s["t"][8] == F(1.5 + 0.125 / 2)       # max(g / L, min_step) / |d|
    assert s["t_hi"][2] == 1.5 and s["t"][2] == F(0.5 * (1.25 + 1.5)) and s["t_lo"][2] == 1.25
    SR.refine(s, F([0.0] * 2 + [0.1, -0.1] + [0.0] * 6), None, 0.0, final=True)
    assert s["status"][2] == s["status"][3] == SR.HIT
    assert s["t_lo"][2] == F(1.375) and s["t_hi"][2] == 1.5 and s["t_hi"][3] == F(1.375) and s["t_lo"][3] == 1.25
    assert s["t"][2] == F(1.375) + F(0.125) * (F(0.1) / (F(0.1) - F(-0.0)))       # g_hi = -0.0: the crossing is the hi end
    assert s["t"][3] == F(1.25) + F(0.125) * (F(0.5) / (F(0.5) - F(-0.1)))


def test_pack_rules():
    rot = np.eye(3, dtype=F)[[1, 2, 0]]             # a permutation: (rot v) = (v1, v2, v0)
    status = np.array([SR.HIT, SR.MISS, SR.HIT, SR.INSIDE], np.uint8)
    t, d = F([2.0, 3.0, 0.5, 1.0]), F([[1, 2, 3], [1, 2, 3], [-4, 0, 0], [1, 1, 1]])
    grad = F([[0, 0, 2], [1, 0, 0], [np.nan, 0, 0], [0, 1, 0]])
    color = F([[0.5, 1.5, -1], [0.5, 0.5, 0.5], [np.nan, 0.25, 1.0], [1, 1, 1]])
    vis = np.array([[0, 1], [1, 1], [0, 0], [1, 0]], np.uint8)
    out = SR.pack(status, t, d, rot, grad, color, vis)
    assert out["hit"].tolist() == [True, False, True, False]
    assert out["depth"].tolist() == [2.0, 0.0, -2.0, 0.0]                          # t * (rot d)_z = t * d_x under this rot
    assert out["normal"].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert out["normal_img"].tolist() == [[128, 255, 128], [0, 0, 0], [128, 128, 128], [0, 0, 0]]      # (a hit with a zero normal is mid-grey)
    assert out["img"].tolist() == [[128, 255, 0], [0, 0, 0], [0, 64, 255], [0, 0, 0]]
    assert out["seen"].tolist() == [True, False, False, False]


def test_entry_points_report_bad_arguments_without_a_gpu():
    """Arguments are checked before any launch: -1 with a message for null pointers, negative counts and bad parameters, -2 for the size
    limit; n == 0 / m == 0 succeed."""
    from gens_amd import lib as L
    lib = L.load()
    p = lambda k: 0x7e0000000000 + 4096 * k  # noqa: E731  (made-up addresses: never dereferenced by the host code)
    box = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)

    def state(n, **null):
        fields = [f for f, _ in L.TraceState._fields_ if f != "n"]
        return L.TraceState(*[None if f in null else p(k) for k, f in enumerate(fields)], n)

    def refused(rc, *words):
        msg = lib.gens_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)

    ok = state(5)
    refused(lib.gens_trace_begin(None, p(20), p(21), 0, *box, None), "gens_trace_begin", "null")
    refused(lib.gens_trace_begin(C.byref(state(5, t_hi=1)), p(20), p(21), 0, *box, None), "gens_trace_begin", "null")
    refused(lib.gens_trace_begin(C.byref(ok), None, p(21), 0, *box, None), "gens_trace_begin", "null")
    refused(lib.gens_trace_begin(C.byref(ok), p(20), p(21), 0, None, box[1], None), "gens_trace_begin", "null")
    refused(lib.gens_trace_begin(C.byref(state(-2)), p(20), p(21), 0, *box, None), "gens_trace_begin", "-2 rays")
    assert lib.gens_trace_begin(C.byref(state((1 << 31) + 5)), p(20), p(21), 0, *box, None) == -2
    assert lib.gens_trace_begin(C.byref(state(0)), None, None, 0, *box, None) == 0

    march = lambda st, sdf, idx, m, thr=0.0, lip=2.0, step=0.01, k=256: lib.gens_trace_march(C.byref(st), sdf, idx, m, thr, lip, step, k, None)  # noqa: E731
    refused(march(ok, None, None, 5), "gens_trace_march", "null")
    refused(march(state(5, live=1), p(20), None, 5), "gens_trace_march", "null")
    refused(march(ok, p(20), None, -1), "gens_trace_march", "-1 rays")
    refused(march(ok, p(20), None, 6), "gens_trace_march", "without a list")
    refused(march(ok, p(20), p(21), 5, lip=0.0), "gens_trace_march", "lipschitz")
    refused(march(ok, p(20), p(21), 5, lip=float("inf")), "gens_trace_march", "lipschitz")
    refused(march(ok, p(20), p(21), 5, step=0.0), "gens_trace_march", "min_step")
    refused(march(ok, p(20), p(21), 5, step=-1.0), "gens_trace_march", "min_step")
    refused(march(ok, p(20), p(21), 5, k=0), "gens_trace_march", "max_steps = 0")
    refused(march(ok, p(20), p(21), 5, thr=float("nan")), "gens_trace_march", "threshold")
    assert march(ok, p(20), p(21), (1 << 31) + 5) == -2
    assert march(ok, None, None, 0) == 0

    refine = lambda st, sdf, idx, m, final=0: lib.gens_trace_refine(C.byref(st), sdf, idx, m, 0.0, final, None)  # noqa: E731
    refused(refine(ok, None, p(21), 5), "gens_trace_refine", "null")
    refused(refine(state(5, points=1), p(20), p(21), 5), "gens_trace_refine", "null")
    refused(refine(ok, p(20), None, 6), "gens_trace_refine", "without a list")
    refused(refine(ok, p(20), p(21), -3), "gens_trace_refine", "-3 rays")
    assert refine(ok, p(20), p(21), (1 << 31) + 5) == -2
    assert refine(ok, p(20), p(21), 0) == 0 and refine(ok, None, None, 0, final=1) == 0

    refused(lib.gens_trace_gather(None, p(1), 5, 9, p(2), None), "gens_trace_gather", "null")
    refused(lib.gens_trace_gather(p(0), None, 5, 9, p(2), None), "gens_trace_gather", "null")
    refused(lib.gens_trace_gather(p(0), p(1), 5, 9, None, None), "gens_trace_gather", "null")
    refused(lib.gens_trace_gather(p(0), p(1), -5, 9, p(2), None), "gens_trace_gather", "-5 of 9")
    assert lib.gens_trace_gather(p(0), p(1), 1 << 30, 9, p(2), None) == -2
    assert lib.gens_trace_gather(None, None, 0, 9, None, None) == 0

    def pack(**kw):
        fields = {"grad": p(0), "color": p(1), "vis": p(2), "n_src": 2, "idx": p(3), "m": 5, "n": 9, "status": p(4), "t": p(5), "rays_d": p(6), "rot": p(7),
                  "depth": p(8), "normal": p(9), "normal_img": p(10), "img": p(11), "seen": p(12), "hit": p(13)}
        fields.update(kw)
        return lib.gens_surface_pack(C.byref(L.SurfacePackArgs(**fields)), None)

    refused(lib.gens_surface_pack(None, None), "gens_surface_pack", "null")
    refused(pack(status=None), "gens_surface_pack", "null")
    refused(pack(t=None), "gens_surface_pack", "null")
    refused(pack(rot=None), "gens_surface_pack", "null")
    refused(pack(normal=None, normal_img=None), "gens_surface_pack", "null")
    refused(pack(grad=None), "gens_surface_pack", "normals without a gradient")
    refused(pack(vis=None), "gens_surface_pack", "null")
    refused(pack(seen=None), "gens_surface_pack", "null")
    refused(pack(n_src=0), "gens_surface_pack", "0 source views")
    refused(pack(m=-1), "gens_surface_pack", "-1 of 9")
    refused(pack(idx=None, m=10), "gens_surface_pack", "without a list")
    refused(pack(grad=None, color=None, depth=None, normal=None, normal_img=None, hit=None), "gens_surface_pack", "nothing to write")
    assert pack(n=(1 << 31) + 5) == -2
    assert pack(m=0) == 0
    assert lib.gens_abi_version() == 12
