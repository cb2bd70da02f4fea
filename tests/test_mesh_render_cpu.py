"""CPU tests of the mesh render (K35): the numpy restatement (tests/mesh_render_reference.py) held to what the rule promises -- exact
barycentrics, colours and flags at planted vertices and edge points, the atlas look-up against a viewer's bilinear sample of the written
texture coordinates, zero outputs for degenerate and bad input, the orientation of marching-cubes meshes, K31's depth -- and compare_maps,
the writers, the command line's readers and the argument checks of the entry point through ctypes (these need the built library, not a GPU)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from . import mesh_render_reference as MR
from . import mesh_simplify_reference as SR
from . import mesh_texture_reference as TR
from . import surface_trace_reference as ST

F = np.float32


def _planted_triangle():
    """Two triangles with small-integer corners sharing an edge; colours and flags that tell the vertices apart."""
    v = np.array([[2.0, 0.0, 1.0], [6.0, 2.0, 1.0], [0.0, 4.0, 3.0], [8.0, 8.0, -1.0]])
    t = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    colors = np.array([[10, 20, 30], [200, 100, 50], [7, 77, 177], [255, 0, 128]], dtype=np.uint8)
    return v, t, colors


def _aim(points, dirs):
    """Rays with o = p - d and t = 1, exact for small integers -> (o, d, t)."""
    d = np.asarray(dirs, dtype=F)
    return (np.asarray(points) - d).astype(F), d, np.ones(len(d), dtype=F)


def test_a_vertex_gets_its_own_colour_and_flag_bit_for_bit():
    v, t, colors = _planted_triangle()
    dirs = [[1, 0, 2], [0, -1, 1], [-2, 1, 1]]
    for face in (0, 1):
        for corner in range(3):
            vid = t[face, corner]
            for seen_at in (0, 1):
                seen = np.full(4, 1 - seen_at, dtype=np.uint8)
                seen[vid] = seen_at
                o, d, tt = _aim(np.repeat(v[vid][None], 3, 0), dirs)
                out = MR.shade(v, t, o, d, np.full(3, face), tt, MR.ROT, colors=colors, seen=seen)
                assert out["hit"].all()
                assert np.array_equal(out["bary64"], np.repeat(np.eye(3)[corner][None], 3, 0))
                assert np.array_equal(out["img"], np.repeat(colors[vid][None], 3, 0))
                assert np.array_equal(out["seen"], np.full(3, bool(seen_at)))


def test_on_an_edge_the_third_vertex_does_not_show():
    v, t, colors = _planted_triangle()
    for face in (0, 1):
        for k in range(3):                                          # the edge opposite corner k, at its midpoint (integer coordinates)
            i, j = t[face, (k + 1) % 3], t[face, (k + 2) % 3]
            mid = (v[i] + v[j]) / 2
            assert np.array_equal(mid, np.round(mid))
            planted = colors.copy()
            planted[t[face, k]] = [255, 255, 255]
            seen = np.ones(4, dtype=np.uint8)
            seen[t[face, k]] = 0
            o, d, tt = _aim([mid, mid], [[1, 1, 0], [0, 2, -1]])
            out = MR.shade(v, t, o, d, np.full(2, face), tt, MR.ROT, colors=planted, seen=seen)
            want = np.zeros(3)
            want[(k + 1) % 3] = want[(k + 2) % 3] = 0.5
            assert np.array_equal(out["bary64"], np.repeat(want[None], 2, 0))
            x = 0.5 * colors[i].astype(np.float64) + 0.5 * colors[j].astype(np.float64)
            assert np.array_equal(out["img"], np.repeat(np.floor(x + 0.5).astype(np.uint8)[None], 2, 0))
            assert out["seen"].all()
            seen[:] = 1
            seen[i] = 0
            assert not MR.shade(v, t, o, d, np.full(2, face), tt, MR.ROT, colors=planted, seen=seen)["seen"].any()


@pytest.mark.parametrize("n_faces", (1, 2, 65, 257))
def test_barycentrics_are_weights(n_faces):
    v, t, special = MR.planted_mesh(n_faces)
    o, d, face, tt = MR.planted_rays(v, t, 600)
    o += (np.random.default_rng(3).integers(-1, 2, o.shape) * 0.25).astype(F)      # off the face too: the clamp must bring them back
    out = MR.shade(v, t, o, d, face, tt, MR.ROT)
    b = out["bary64"][out["hit"]]
    assert out["hit"].sum() > 300
    assert (b >= 0).all() and (b <= 1).all() and (np.abs(b.sum(axis=1) - 1.0) <= 2.0 ** -52).all()
    assert (out["bary64"][~out["hit"]] == 0).all()


def _atlas_samples(n_faces, n, seed):
    """Random barycentrics plus planted corners, edge points and near-edge points -> (face (m,), a, b, c (m,) float64) as step 3 leaves them."""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.ones(3), size=n)
    k = n // 10
    w[:k] = np.eye(3)[rng.integers(0, 3, k)]
    w[k:2 * k, rng.integers(0, 3)] = 0.0
    w[2 * k:3 * k, 0] = rng.uniform(0, 1e-12, k)
    w[3 * k:4 * k, 1] = 0.0
    w[4 * k:5 * k, 2] = 0.0
    b, c = w[:, 1] / w.sum(axis=1), w[:, 2] / w.sum(axis=1)
    s = b + c
    with np.errstate(invalid="ignore"):
        b, c = np.where(s > 1.0, b / s, b), np.where(s > 1.0, c / s, c)
    a = np.maximum((1.0 - b) - c, 0.0)
    return rng.integers(0, n_faces, n), a, b, c


@pytest.mark.parametrize("texels", (3, 4, 8, 64))
@pytest.mark.parametrize("n_faces", (1, 2, 7, 65))
def test_the_atlas_look_up_is_what_a_viewer_samples(n_faces, texels):
    """The taps stay inside the hit face's texels, and the colour is a viewer's bilinear sample at the interpolated float32 corner coordinates
    up to 1 unit in at most 0.1 % of the samples (the issue's own measurement of the reference: 0.03 %)."""
    h, w = TR.layout(n_faces, texels)[:2]
    rng = np.random.default_rng(n_faces * 100 + texels)
    atlas = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    face, a, b, c = _atlas_samples(n_faces, 20000, n_faces + texels)
    ip, jp, wt = MR.atlas_taps(b, c, texels)
    read = wt > 0
    assert (ip[read] >= 0).all() and (jp[read] >= 0).all() and ((ip + jp)[read] <= texels - 1).all()
    assert (np.abs(wt.sum(axis=1) - 1.0) < 1e-12).all()
    x, _ = MR.atlas_color(face, n_faces, b, c, texels, atlas)
    uv = TR.texture_uv(n_faces, texels).astype(np.float64)[face]
    at = a[:, None] * uv[:, 0] + b[:, None] * uv[:, 1] + c[:, None] * uv[:, 2]
    ref = TR.bilinear_sample(atlas.astype(np.float64), at)
    print(f"T={n_faces} S={texels}: unrounded max |diff| = {np.abs(x - ref).max():.3g}")
    diff = np.abs(MR.round8(x).astype(np.int64) - MR.round8(ref).astype(np.int64))
    assert diff.max() <= 1
    assert (diff.max(axis=1) > 0).mean() <= 1e-3
    for corner, (ci, cj) in enumerate(((0, 0), (texels - 2, 0), (0, texels - 2))):
        f = np.arange(n_faces)
        e = np.repeat(np.eye(3)[corner][None], n_faces, 0)
        xc, _ = MR.atlas_color(f, n_faces, e[:, 1], e[:, 2], texels, atlas)
        px, py = TR.pixel(n_faces, texels, f, ci, cj)
        assert np.array_equal(MR.round8(xc), atlas[py, px]) and np.array_equal(xc, atlas[py, px].astype(np.float64))


def test_the_atlas_seen_flag_is_every_weighted_tap():
    n_faces, texels = 7, 4
    h, w = TR.layout(n_faces, texels)[:2]
    face = np.array([3, 5, 4])
    b, c = np.array([0.25, 0.5, 0.0]), np.array([0.25, 0.0, 1.0])          # x = y = 0.5: four taps; x = 1: one tap; corner C: one tap
    seen = np.ones((h, w), dtype=np.uint8)
    assert MR.atlas_color(face, n_faces, b, c, texels, None, seen)[1].all()
    for ray, taps in ((0, ((0, 0), (1, 0), (0, 1), (1, 1))), (1, ((1, 0),)), (2, ((0, 2),))):
        for ip, jp in taps:
            px, py = TR.pixel(n_faces, texels, face[ray], ip, jp)
            one = seen.copy()
            one[py, px] = 0
            got = MR.atlas_color(face, n_faces, b, c, texels, None, one)[1]
            assert not got[ray] and got[np.arange(3) != ray].all()
    px, py = TR.pixel(n_faces, texels, 5, 2, 0)                             # a neighbour of ray 1's single tap, with weight 0
    one = seen.copy()
    one[py, px] = 0
    assert MR.atlas_color(face, n_faces, b, c, texels, None, one)[1].all()


def test_degenerate_and_bad_input_gives_zeros_and_is_not_read_through():
    v, t, special = MR.planted_mesh(65)
    normals, colors, seen, atlas, atlas_seen = MR.planted_attributes(len(v), len(t), 4)
    o, d, face, tt = MR.planted_rays(v, t, 257)
    face[:4] = [special["repeated_vertex"], special["bad_index"], special["nan_vertex"], special["tiny"]]
    tt[:4] = 1.0
    for kw in ({"colors": colors, "seen": seen}, {"texture": atlas, "texture_seen": atlas_seen, "texels": 4},
               {"normals": normals, "shading": "smooth"}, {"orient": 1}):
        out = MR.shade(v, t, o, d, face, tt, MR.ROT, **kw)
        hit, idx = MR.hits(v, t, face, tt)
        bad = np.r_[1, 2, np.arange(257 - 8, 257)]                # the two planted faces and the eight planted rays
        assert not hit[bad].any() and hit[0] and hit[3] and (idx[bad] == 0).all()
        for k in MR.OUTPUTS:
            if k in out:
                assert not np.asarray(out[k])[bad].any(), k
        assert np.array_equal(out["bary"][0], [1, 0, 0])             # the zero-area face; the face of signed zeros and subnormals is a plain one
        if kw.get("shading") != "smooth":
            assert not out["normal"][0].any() and np.array_equal(np.abs(out["normal"][3]), [0, 0, 1])
        assert np.isfinite(out["normal"]).all() and np.isfinite(out["bary"]).all()


@pytest.mark.parametrize("orient", (0, 1))
def test_marching_cubes_meshes_wind_along_the_gradient(orient):
    from gens_amd import ops
    v, t = SR.lattice_mesh(SR.sphere_field)
    cen = v[t].mean(axis=1)
    o, d, tt = _aim(cen, np.repeat([[0, 0, 1]], len(t), 0))
    out = MR.shade(v, t, o, d, np.arange(len(t)), tt, MR.ROT, orient=orient)
    dots = (out["normal"].astype(np.float64) * (cen - SR.CENTRE)).sum(axis=1)
    solid = np.linalg.norm(out["normal"], axis=1) > 0
    assert solid.sum() > 0.99 * len(t)
    assert ops.MESH_ORIENT == 0
    assert (dots[solid] > 0).all() if orient == ops.MESH_ORIENT else (dots[solid] < 0).all()


def test_the_depth_is_the_surface_maps_depth():
    v, t, _ = MR.planted_mesh(65)
    o, d, face, tt = MR.planted_rays(v, t, 257)
    tt = (tt * np.random.default_rng(0).uniform(0.5, 2.0, len(tt))).astype(F)
    out = MR.shade(v, t, o, d, face, tt, MR.ROT)
    ref = ST.pack(np.where(out["hit"], ST.HIT, ST.MISS), tt, d, MR.ROT)
    assert np.array_equal(out["depth"].view(np.uint32), ref["depth"].view(np.uint32)) and out["hit"].sum() > 200


def test_compare_maps_counts_and_sums():
    from gens_amd import ops
    hit_a = np.array([[1, 1, 1, 0], [0, 1, 0, 0]], dtype=bool)
    hit_b = np.array([[1, 0, 1, 1], [0, 1, 1, 0]], dtype=np.uint8)
    a = {"hit": hit_a, "depth": np.array([[1.0, 2.0, 3.0, 0.0], [0.0, 5.0, 0.0, 0.0]], dtype=F), "img": np.full((2, 4, 3), 10, np.uint8)}
    b = {"hit": hit_b, "depth": np.array([[1.5, 0.0, 3.0, 9.0], [0.0, 4.0, 7.0, 0.0]], dtype=F), "img": np.full((2, 4, 3), 10, np.uint8)}
    b["img"][0, 0] = [0, 255, 11]
    b["img"][0, 1] = [99, 99, 99]                                   # only a hits this pixel: not counted
    got = ops.compare_maps(a, b)
    assert (got["both"], got["only_a"], got["only_b"], got["neither"]) == (3, 1, 2, 2)
    assert got["color_sum"] == 10 + 245 + 1 and got["color_max"] == 245 and got["color_mean"] == 256 / 9
    assert got["depth_mean"] == 0.5 and got["depth_median"] == 0.5 and got["depth_max"] == 1.0
    same = ops.compare_maps({k: torch.as_tensor(x) for k, x in a.items()}, b)
    assert same == got
    none = ops.compare_maps(a, {**b, "hit": ~hit_a})
    assert none["both"] == 0 and none["color_sum"] == 0 and none["neither"] == 0
    assert all(none[k] is None for k in ("color_mean", "color_max", "depth_mean", "depth_median", "depth_max"))
    assert ops.compare_maps({"hit": hit_a, "depth": a["depth"]}, b)["color_sum"] is None
    with pytest.raises(ValueError):
        ops.compare_maps(a, {"hit": hit_b[:1], "depth": b["depth"][:1]})


def _validation_outputs(h=6, w=8):
    rng = np.random.default_rng(0)
    outputs = {"vertices": np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), "triangles": np.array([[0, 1, 2]], dtype=np.int32),
               "img_fine": rng.uniform(0, 255, (h, w, 3)).astype(F), "normal_img": rng.uniform(0, 255, (h, w, 3)).astype(F),
               "render_depth": rng.uniform(0, 2, (h, w)).astype(F), "sdf_depth": rng.uniform(0, 2, (h, w)).astype(F)}
    inputs = {"scene": "scan1", "file_name": "0007", "scale_mat": torch.eye(4)}
    return outputs, inputs


def test_the_writer_stores_the_mesh_maps_where_present(tmp_path):
    from PIL import Image

    from gens_amd import io
    outputs, inputs = _validation_outputs()
    plain = io.save_validation_outputs(str(tmp_path / "plain"), outputs, inputs, "step5")
    assert not any(k.startswith("mesh_") for k in plain) and not (tmp_path / "plain" / "val_mesh_img").exists()
    hit = np.zeros((6, 8), dtype=bool)
    hit[2:5, 1:7] = True
    outputs.update(mesh_depth=np.where(hit, 1.25, 0).astype(F), mesh_normal_img=np.full((6, 8, 3), 200.7, F),
                   mesh_img=np.full((6, 8, 3), 90, np.uint8), mesh_hit=hit)
    paths = io.save_validation_outputs(str(tmp_path / "full"), outputs, inputs, "step5")
    for name, sub in (("mesh_depth", "val_mesh_depth"), ("mesh_normal", "val_mesh_normal"), ("mesh_img", "val_mesh_img")):
        assert paths[name] == str(tmp_path / "full" / sub / "0007_step5.png")
        rgb = np.asarray(Image.open(paths[name]))
        assert rgb.shape == (6, 8, 3) and not rgb[~hit].any() and rgb[hit].any()
    assert (np.asarray(Image.open(paths["mesh_img"]))[hit] == 90).all() and (np.asarray(Image.open(paths["mesh_normal"]))[hit] == 200).all()
    del outputs["mesh_img"]                                          # a mesh without colours: depth and normals only
    assert "mesh_img" not in io.save_validation_outputs(str(tmp_path / "bare"), outputs, inputs, "step5")


def test_the_command_line_reads_its_files_and_refuses_before_the_device(tmp_path):
    from gens_amd import io, render_mesh
    v, t, colors = _planted_triangle()
    normals = np.repeat([[0.0, 0.6, 0.8]], 4, 0).astype(F)
    io.write_ply(str(tmp_path / "m.ply"), v, t, normals=normals, colors=colors)
    mesh = render_mesh.load_mesh(str(tmp_path / "m.ply"))
    assert np.array_equal(mesh["vertices"], v.astype(mesh["vertices"].dtype)) and np.array_equal(mesh["triangles"], t)
    assert np.array_equal(mesh["colors"], colors) and mesh["colors"].dtype == np.uint8 and np.array_equal(mesh["normals"], normals)
    io.write_ply(str(tmp_path / "bare.ply"), v, t)
    assert sorted(render_mesh.load_mesh(str(tmp_path / "bare.ply"))) == ["triangles", "vertices"]
    h, w = TR.layout(2, 4)[:2]
    atlas = np.random.default_rng(0).integers(0, 256, (h, w, 3)).astype(np.uint8)
    io.write_obj(str(tmp_path / "m.obj"), v, t, TR.texture_uv(2, 4), atlas)
    obj = render_mesh.load_mesh(str(tmp_path / "m.obj"))
    assert np.array_equal(obj["texture"], atlas) and np.array_equal(obj["triangles"], t) and "normals" not in obj
    with pytest.raises(ValueError, match="ply or .obj"):
        render_mesh.load_mesh(str(tmp_path / "m.stl"))
    cams = {"intrs": np.repeat(np.eye(4, dtype=F)[None], 3, 0), "c2ws": np.repeat(np.eye(4, dtype=F)[None], 3, 0), "hw": np.array([6, 8])}
    np.savez(str(tmp_path / "cams.npz"), **cams)
    intrs, c2ws, hw, views = render_mesh.load_cams(str(tmp_path / "cams.npz"))
    assert intrs.shape == (3, 4, 4) and hw == (6, 8) and views == [0, 1, 2]
    assert render_mesh.load_cams(str(tmp_path / "cams.npz"), [2, 0])[3] == [2, 0]
    with pytest.raises(ValueError, match="outside the 3 cameras"):
        render_mesh.load_cams(str(tmp_path / "cams.npz"), [3])
    np.savez(str(tmp_path / "nohw.npz"), intrs=cams["intrs"], c2ws=cams["c2ws"])
    with pytest.raises(ValueError, match="hw"):
        render_mesh.load_cams(str(tmp_path / "nohw.npz"))
    argv = [str(tmp_path / "bare.ply"), "--cams", str(tmp_path / "cams.npz"), "--out", str(tmp_path / "out")]
    with pytest.raises(SystemExit):                                  # refused while parsing: nothing is rendered or written
        render_mesh.main(argv + ["--shading", "smooth"])
    with pytest.raises(ValueError, match="outside"):
        render_mesh.main(argv + ["--view", "7"])
    assert not (tmp_path / "out").exists()


def test_the_python_layers_refuse_bad_arguments_before_any_launch():
    from gens_amd import ops
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    opt = ImplicitSurface._mesh_render_option
    holder = type("Holder", (), {"mesh_render": None, "_MESH_RENDER_KEYS": ImplicitSurface._MESH_RENDER_KEYS})()
    assert opt(holder, None) is None and opt(holder, False) is None and opt(holder, True) == {} and opt(holder, {"shading": "smooth"}) == {"shading": "smooth"}
    holder.mesh_render = True
    assert opt(holder, None) == {} and opt(holder, False) is None
    for bad in (3, {"texels": 8}, {"shading": "phong"}):
        with pytest.raises(ValueError):
            opt(holder, bad)
    cpu = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="device"):
        ops.render_mesh(cpu.double(), torch.zeros(1, 3, dtype=torch.int32), cpu, cpu, torch.eye(3).reshape(-1))
    with pytest.raises(ValueError, match="shading"):
        ops.render_mesh(None, None, cpu, cpu, None, shading="phong")
    with pytest.raises(ValueError, match="normals"):
        ops.render_mesh(None, None, cpu, cpu, None, shading="smooth")
    with pytest.raises(ValueError, match="chunk"):
        ops.render_mesh(None, None, cpu, cpu, None, chunk=0)
    with pytest.raises(ValueError, match="MeshGrid"):
        ops.shade_mesh_hits(None, cpu, cpu, None, None, None)


def test_the_entry_point_reports_bad_arguments_without_a_gpu():
    """Arguments are checked before any launch: -1 with a message, -2 for the size limits; no rays and no outputs succeed whatever the
    pointers."""
    from gens_amd import lib as L
    lib = L.load()
    assert lib.gens_abi_version() == 12
    p = lambda k: 0x7e0000000000 + 4096 * k  # noqa: E731  (made-up addresses: never dereferenced by the host code)
    h, w = TR.layout(4, 8)[:2]
    base = dict(vertices=p(1), triangles=p(2), n_vertices=9, n_faces=4, rays_o=p(3), rays_d=p(4), face=p(5), t=p(6), n=5, rot=p(7),
                vertex_normals=p(8), vertex_colors=p(9), vertex_seen=p(10), atlas=None, atlas_seen=None, atlas_h=0, atlas_w=0, texels=0, shading=0,
                orient=0, hit=p(11), bary=p(12), depth=p(13), normal=p(14), normal_img=p(15), img=p(16), seen=p(17))
    outs = ("hit", "bary", "depth", "normal", "normal_img", "img", "seen")

    def call(**kw):
        return lib.gens_mesh_shade(C.byref(L.MeshShadeArgs(**{**base, **kw})), None)

    def refused(rc, *words):
        msg = lib.gens_last_error().decode()
        assert rc == -1 and "gens_mesh_shade" in msg and all(x in msg for x in words), (rc, msg)

    refused(lib.gens_mesh_shade(None, None), "null")
    refused(call(n=-1), "-1 rays")
    refused(call(n_vertices=-2), "-2 vertices")
    refused(call(n_faces=-3), "-3 triangles")
    for k in ("n", "n_vertices", "n_faces"):
        assert call(**{k: 1 << 31}) == -2
    for bad in (-1, 2):
        refused(call(shading=bad), "shading")
        refused(call(orient=bad), "orient")
    atlas = dict(atlas=p(20), atlas_seen=p(21), atlas_h=h, atlas_w=w, texels=8)
    for s in (2, 65, 0, -1):
        refused(call(**{**atlas, "texels": s}), "texels")
    refused(call(**{**atlas, "atlas_h": h + 1}), "atlas")
    refused(call(**{**atlas, "atlas_w": w - 1}), "atlas")
    refused(call(**{**atlas, "n_faces": 40}), "atlas")
    refused(call(**{**atlas, "atlas": None}), "atlas_seen without")
    refused(call(shading=1, vertex_normals=None), "smooth")
    refused(call(shading=1, vertex_normals=None, normal=None, normal_img=None), "smooth")
    refused(call(vertex_colors=None), "img or seen")
    refused(call(vertex_colors=None, img=None), "img or seen")
    refused(call(vertex_seen=None), "seen")
    refused(call(**{**atlas, "atlas_seen": None}), "seen")
    for k in ("face", "t", "triangles", "vertices", "rays_d", "rays_o", "rot"):
        refused(call(**{k: None}), "null")
    refused(call(rays_d=None, bary=None, normal=None, normal_img=None, img=None, seen=None), "null", "rays_d")       # the depth alone needs it
    refused(call(rot=None, depth=None), "null", "rot")                                                               # ... the normal image the rotation
    # what a requested output does not need may be NULL
    assert lib.gens_last_error() is not None
    nothing = {k: None for k in outs}
    assert call(**nothing, face=None, t=None, triangles=None, vertices=None, rays_o=None, rays_d=None, rot=None) == 0
    assert call(n=0, face=None, t=None, triangles=None, vertices=None, rays_o=None, rays_d=None, rot=None) == 0
    refused(call(**{**nothing, "shading": 3}), "shading")            # the checks of the parameters do not depend on the outputs
