"""GPU tests of the mesh render (K35): gens_mesh_shade against the numpy restatement (tests/mesh_render_reference.py), bit for bit, on planted
meshes and rays in every mode; empty cases launch nothing; ops.render_mesh and ImplicitSurface.render_mesh on the g23 model's cell-2
simplified R = 64 mesh against the restatement driven by the device's own first hits, for every chunking and input kind; the mesh maps
beside K31's surface maps of the same view; validate, the conf key, the written files and the command line; nothing changes when the option
is unset; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import mesh_render_reference as MR
from .test_hip_mesh_texture import _same, _same_dict, _same_floats

gpu = pytest.mark.gpu
F = np.float32
K35 = {"gens_mesh_shade"}
CAST = {"gens_ray_first_hit", "gens_mesh_grid_count", "gens_mesh_grid_fill"}


def _grid(vertices, triangles):
    """An ops.MeshGrid that holds the mesh only (the shade reads no cells): build_mesh_grid refuses the planted bad indices and NaN vertices."""
    from gens_amd import ops
    z = torch.zeros(2, device="cuda", dtype=torch.int32)
    return ops.MeshGrid(torch.from_numpy(np.ascontiguousarray(vertices, np.float64)).cuda(),
                        torch.from_numpy(np.ascontiguousarray(triangles, np.int32)).cuda().reshape(-1, 3), z, z[:1], (0.0, 0.0, 0.0, 1.0), (1, 1, 1))


def _check(got, want, names=None):
    names = [k for k in MR.OUTPUTS if k in got] if names is None else names
    assert sorted(got) == sorted(names)
    for k in names:
        g, w = got[k].cpu().numpy(), want[k]
        if g.dtype == np.float32:
            assert _same_floats(g, w), k
        else:
            assert _same(g, w.astype(np.uint8)), k


@gpu
@pytest.mark.parametrize("s", [3, 4, 8])
@pytest.mark.parametrize("t", [1, 2, 3, 65, 257])
def test_the_kernel_equals_the_restatement(t, s):
    from gens_amd import ops
    v, tri, special = MR.planted_mesh(t)
    normals, colors, seen, atlas, atlas_seen = MR.planted_attributes(len(v), t, s)
    grid = _grid(v, tri)
    cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    rot = cu(MR.ROT)
    dn, dc, ds, da, das = cu(normals), cu(colors), cu(seen), cu(atlas), cu(atlas_seen)
    modes = (
        ({}, {}, ("hit", "bary", "depth")),
        ({"colors": colors, "seen": seen}, {"colors": dc, "seen": ds}, None),
        ({"colors": colors, "orient": 1}, {"colors": dc, "orient": 1}, None),
        ({"texture": atlas, "texture_seen": atlas_seen, "texels": s, "orient": 1}, {"texture": da, "texture_seen": das, "texels": s, "orient": 1}, None),
        ({"texture": atlas, "texels": s, "colors": colors, "normals": normals, "shading": "smooth"},
         {"texture": da, "texels": s, "colors": dc, "normals": dn, "shading": "smooth"}, None),
        ({"normals": normals, "shading": "smooth", "colors": colors, "seen": seen}, {"normals": dn, "shading": "smooth", "colors": dc, "seen": ds},
         ("normal", "normal_img", "img", "seen")),
    )
    for n in (0, 1, 63, 64, 65, 257):
        o, d, face, tt = MR.planted_rays(v, tri, n, seed=s)
        if n >= 65 and special:                                     # every planted face is aimed at
            face[:5] = [special[k] for k in ("repeated_face", "repeated_vertex", "bad_index", "nan_vertex", "tiny")]
        rays = (cu(o), cu(d), cu(face), cu(tt), rot)
        for host_kw, dev_kw, names in modes:
            want = MR.shade(v, tri, o, d, face, tt, MR.ROT, **host_kw)
            got = ops.shade_mesh_hits(grid, *rays, **dev_kw, outputs=names)
            _check(got, want, names)
            again = ops.shade_mesh_hits(grid, *rays, **dev_kw, outputs=names)
            assert all(_same(got[k].cpu().numpy(), again[k].cpu().numpy()) for k in got)
        if n == 257:
            assert 100 < want["hit"].sum() < n and not want["hit"][-8:].any()


@gpu
def test_no_rays_and_no_outputs_launch_nothing():
    from gens_amd import lib as L, ops
    v, tri, _ = MR.planted_mesh(3)
    grid = _grid(v, tri)
    rot = torch.from_numpy(MR.ROT).cuda()
    z3, zi, zf = torch.zeros(0, 3, device="cuda"), torch.zeros(0, device="cuda", dtype=torch.int32), torch.zeros(0, device="cuda")
    o, d, face, tt = (torch.from_numpy(a).cuda() for a in MR.planted_rays(v, tri, 5))
    L.profile_begin(only=K35)
    out = ops.shade_mesh_hits(grid, z3, z3, zi, zf, rot)
    assert sorted(out) == ["bary", "depth", "hit", "normal", "normal_img"] and out["bary"].shape == (0, 3) and out["hit"].dtype == torch.uint8
    assert ops.shade_mesh_hits(grid, o, d, face, tt, rot, outputs=()) == {}
    empty = ops.render_mesh(None, None, z3, z3, rot, grid=grid, colors=torch.zeros(len(v), 3, device="cuda", dtype=torch.uint8))
    assert sorted(empty) == ["bary", "depth", "face", "hit", "img", "normal", "normal_img", "t"] and empty["img"].shape == (0, 3)
    assert not L.profile_end(raw=True)
    lib = L.load()
    args = L.MeshShadeArgs(n=0, hit=1)
    assert lib.gens_mesh_shade(C.byref(args), None) == 0
    assert lib.gens_mesh_shade(C.byref(L.MeshShadeArgs(n=5, n_vertices=3, n_faces=1)), None) == 0
    L.profile_begin(only=K35)
    ops.shade_mesh_hits(grid, o, d, face, tt, rot, outputs=("hit",))
    assert [k for k, *_ in L.profile_end(raw=True)] == ["gens_mesh_shade"]


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface, its synthetic views and its cell-2 simplified R = 64 mesh (tests/test_hip_mesh_texture.py), view 0 at 48 x 64
# ------------------------------------------------------------------------------------------------------------------------------------
_CASE = {}


def _case():
    """Once: the model, the 48 x 64 rays of view 0, the mesh's vertex attributes and its texels = 8 atlas, the device's first hits."""
    from gens_amd import ops, synthetic
    from .test_hip_mesh_texture import _model
    from .test_hip_vertex_attrs import _scene
    if not _CASE:
        m = _model("f32")
        sc, _ = _scene(m["surf"], 3)
        o, d = synthetic.make_rays(sc["intrs"].cpu(), sc["c2ws"].cpu(), 48, 64)
        attrs = m["surf"].vertex_attributes(m["points"], m["vols"], m["views"])
        tex = m["surf"].texture_mesh(m["points"], m["tri"], m["vols"], m["views"], texels=8)
        grid = ops.build_mesh_grid(m["points"], m["tri"])
        face, t = ops.ray_mesh_first_hit(o.cuda(), d.cuda(), grid)
        rot = ops.SceneCams(torch.eye(4, device="cuda").expand(3, 4, 4).contiguous(), sc["c2ws"]).rot_inv
        _CASE.update(m=m, sc=sc, o=o.cuda(), d=d.cuda(), attrs=attrs, tex=tex, grid=grid, face=face.cpu().numpy(), t=t.cpu().numpy(),
                     rot=rot, rot_np=rot.cpu().numpy())
    return _CASE


def _configs(c):
    a, x = c["attrs"], c["tex"]
    vertex = {"normals": a["normals"], "colors": a["colors"], "seen": a["seen"]}
    atlas = {"texture": x["texture"], "texture_seen": x["texture_seen"], "texels": 8}
    return (("attributes", {**vertex, "shading": "smooth"}), ("atlas", atlas), ("both", {**vertex, **atlas, "shading": "smooth"}))


def _restated(c, kw):
    m = c["m"]
    want = MR.shade(m["points_np"].astype(np.float64), m["tri_np"], c["o"].cpu().numpy(), c["d"].cpu().numpy(), c["face"], c["t"], c["rot_np"], **kw)
    want.pop("bary64")
    return {"face": c["face"], "t": c["t"], **want}


@gpu
def test_render_mesh_equals_the_restatement_on_the_models_mesh():
    from gens_amd import lib as L, ops
    c = _case()
    m, surf = c["m"], c["m"]["surf"]
    assert len(m["tri_np"]) > 500
    dev = lambda kw: {k: torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v for k, v in kw.items()}  # noqa: E731
    for name, kw in _configs(c):
        want = _restated(c, kw)
        assert 500 < want["hit"].sum() < 3072, name
        L.profile_begin(only=K35 | CAST)
        got = ops.render_mesh(m["points"], m["tri"], c["o"], c["d"], c["rot"], **dev(kw))
        assert {k for k, *_ in L.profile_end(raw=True)} == K35 | CAST
        assert sorted(got) == sorted(want), name
        for k in want:
            g = got[k].cpu().numpy()
            assert _same_floats(g, want[k]) if g.dtype == np.float32 else _same(g, want[k].astype(g.dtype)), (name, k)
        for chunk in (1000, 64):                                    # no dependence on the chunk, with a grid handed in
            part = ops.render_mesh(None, None, c["o"], c["d"], c["rot"], grid=c["grid"], chunk=chunk, **dev(kw))
            assert all(torch.equal(part[k].view(torch.uint8), got[k].view(torch.uint8)) for k in got), (name, chunk)
        # the model's method: host arrays shaped like the image, from device inputs and from numpy inputs
        shaped = surf.render_mesh(m["points"], m["tri"], c["o"].view(48, 64, 3), c["d"].view(48, 64, 3), c["sc"]["c2ws"], **dev(kw))
        assert shaped["hit"].dtype == bool and shaped["depth"].shape == (48, 64) and shaped["normal_img"].shape == (48, 64, 3)
        for k in want:
            w = want[k].astype(bool) if k in ("hit", "seen") else want[k]
            flat = shaped[k].reshape(w.shape)
            assert _same_floats(flat, w) if flat.dtype == np.float32 else _same(flat, w), (name, k)
        stats = surf.last_mesh_render_stats
        assert stats["rays"] == 3072 and stats["hits"] == int(want["hit"].sum()) and stats["faces"] == len(m["tri_np"]) and stats["cells"] >= 1
        host = surf.render_mesh(m["points_np"].astype(np.float64), m["tri_np"].astype(np.int64), c["o"].cpu().numpy(), c["d"].cpu().numpy(),
                                c["sc"]["c2ws"].cpu().numpy(), hw=(48, 64), chunk=500, **{k: v for k, v in kw.items() if k != "texels"})
        assert _same_dict(host, shaped), name
    bare = ops.render_mesh(m["points"], m["tri"], c["o"], c["d"], c["rot"])
    assert sorted(bare) == ["bary", "depth", "face", "hit", "normal", "normal_img", "t"]
    # flat normals of the extracted mesh point along + grad sdf: against the smooth ones of the same rays
    flat, smooth = bare["normal"].cpu().numpy(), _restated(c, {"normals": c["attrs"]["normals"], "shading": "smooth"})["normal"]
    hit = bare["hit"].cpu().numpy() != 0
    dots = (flat * smooth).sum(axis=1)[hit]
    print(f"flat . smooth normals over {hit.sum()} hits: min {dots.min():.3f}, mean {dots.mean():.3f}, share > 0 {np.mean(dots > 0):.4f}")
    assert np.mean(dots > 0) > 0.99


@gpu
def test_the_mesh_maps_beside_the_surface_maps_of_the_same_view():
    """The unsimplified R = 64 mesh against K31's trace of the same rays.  Both surfaces lie in the lattice cells the zero set crosses, so
    the median depth difference over the pixels both hit is below one lattice spacing: a sanity condition, not a tolerance."""
    from gens_amd import ops
    c = _case()
    m, surf, sc = c["m"], c["m"]["surf"], c["sc"]
    v, t, attrs = surf.extract_geometry(m["vols"], m["lo"], m["hi"], 64, 0.0, attributes=("normals", "colors"), views=m["views"])
    mesh = surf.render_mesh(v, t, c["o"], c["d"], sc["c2ws"], hw=(48, 64), **attrs)
    surface = surf.render_surface(c["o"], c["d"], sc["near"], sc["far"], m["vols"], m["lo"], m["hi"], sc["c2ws"], views=m["views"], resolution=64,
                                  hw=(48, 64))
    fig = ops.compare_maps(mesh, surface)
    print(f"R = 64 mesh ({len(t)} faces) beside the traced surface: {fig}")
    spacing = float((m["hi"] - m["lo"]).min()) / 63
    assert fig["both"] > 500 and fig["depth_median"] < spacing
    assert fig == ops.compare_maps({k: torch.as_tensor(x).cuda() for k, x in mesh.items()}, surface)


@gpu
def test_validate_the_conf_key_the_written_files_and_the_command_line(tmp_path):
    from gens_amd import io as gio, ops, render_mesh as cli
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_vertex_attrs import TODAYS_KEYS, _validate_args
    c = _case()
    m, surf, sc = c["m"], c["m"]["surf"], c["sc"]
    args = _validate_args(surf, m["vols"])
    maps = {"mesh_depth", "mesh_normal_img", "mesh_hit"}
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=64, mesh_simplify=2)
    torch.manual_seed(3)
    out = surf.validate(*args, extract_geometry=True, mesh_resolution=64, mesh_simplify=2, mesh_render=True)
    assert set(out) == TODAYS_KEYS | maps and out["mesh_hit"].dtype == bool and out["mesh_depth"].shape == (24, 32)
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])), k
    want = surf.render_mesh(out["vertices"], out["triangles"], args[0], args[1], sc["c2ws"], hw=(24, 32))
    assert _same(out["mesh_depth"], want["depth"]) and _same(out["mesh_normal_img"], want["normal_img"]) and _same(out["mesh_hit"], want["hit"])
    assert 100 < out["mesh_hit"].sum() < 24 * 32
    torch.manual_seed(3)
    full = surf.validate(*args, extract_geometry=True, mesh_resolution=64, mesh_simplify=2, mesh_attributes=("normals", "colors"), mesh_texture=8,
                         surface_render=True, mesh_render={"shading": "smooth", "chunk": 300})
    assert maps | {"mesh_img", "mesh_fidelity", "texture", "vertex_colors", "surface_img"} <= set(full)
    want = surf.render_mesh(full["vertices"], full["triangles"], args[0], args[1], sc["c2ws"], hw=(24, 32), normals=full["vertex_normals"],
                            colors=full["vertex_colors"], seen=full["vertex_seen"], texture=full["texture"], texture_seen=full["texture_seen"],
                            shading="smooth")
    assert _same(full["mesh_img"], want["img"]) and _same(full["mesh_normal_img"], want["normal_img"]) and _same(full["mesh_depth"], want["depth"])
    surface = {"hit": full["surface_hit"], "depth": full["surface_depth"], "img": full["surface_img"]}
    assert full["mesh_fidelity"] == ops.compare_maps(want, surface) and full["mesh_fidelity"]["both"] > 100
    print(f"validate: cell-2 mesh with the texels = 8 atlas beside the traced surface: {full['mesh_fidelity']}")
    torch.manual_seed(3)
    vertex = surf.validate(*args, extract_geometry=True, mesh_resolution=64, mesh_simplify=2, mesh_attributes=("colors",), mesh_render=True)
    want = surf.render_mesh(vertex["vertices"], vertex["triangles"], args[0], args[1], sc["c2ws"], hw=(24, 32), colors=vertex["vertex_colors"],
                            seen=vertex["vertex_seen"])
    assert _same(vertex["mesh_img"], want["img"]) and "mesh_fidelity" not in vertex
    surf.mesh_render = True
    try:
        torch.manual_seed(3)
        again = surf.validate(*args, extract_geometry=True, mesh_resolution=64, mesh_simplify=2)
        assert _same_dict({k: again[k] for k in maps}, {k: out[k] for k in maps})
    finally:
        del surf.mesh_render
    # the conf key reaches the attribute (and its absence leaves the class default)
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert ImplicitSurface.mesh_render is None and "mesh_render" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "mesh_render": True})).implicit_surface.mesh_render is True
    assert GenS(Conf({**conf, "mesh_render": {"shading": "smooth"}})).implicit_surface.mesh_render == {"shading": "smooth"}
    # the writer
    inputs = {"scene": "scan1", "file_name": "scan1_view0", "scale_mat": torch.eye(4)}
    paths = gio.save_validation_outputs(str(tmp_path), full, inputs, "epoch0")
    from PIL import Image
    img = np.asarray(Image.open(paths["mesh_img"]))
    assert _same(img, np.where(full["mesh_hit"][:, :, None], full["mesh_img"], np.uint8(0)))
    assert paths["mesh_depth"].endswith("val_mesh_depth/scan1_view0_epoch0.png") and paths["mesh_normal"].endswith("val_mesh_normal/scan1_view0_epoch0.png")
    # the command line, on the written OBJ (atlas) and PLY (vertex colours), view 0 of the scene's cameras at 48 x 64
    np.savez(str(tmp_path / "cams.npz"), intrs=sc["intrs"].cpu().numpy(), c2ws=sc["c2ws"].cpu().numpy(), hw=np.array([48, 64]))
    o, d = ImplicitSurface.view_rays(sc["intrs"], sc["c2ws"], 0, (48, 64))
    for mesh_path, kw in ((paths["obj"], {"texture": full["texture"] if full["texture_seen"].all() else np.where(
            full["texture_seen"][:, :, None], full["texture"], np.uint8(128))}), (paths["mesh"], {"colors": np.where(
                np.asarray(full["vertex_seen"], bool)[:, None], full["vertex_colors"], np.uint8(128))})):
        written = cli.main([mesh_path, "--cams", str(tmp_path / "cams.npz"), "--out", str(tmp_path / "views"), "--view", "0"])
        want = surf.render_mesh(full["vertices"].astype(F), full["triangles"], o, d, sc["c2ws"], hw=(48, 64), **kw)
        assert sorted(written) == [0] and sorted(written[0]) == ["depth", "img", "normal"]
        assert _same(np.load(written[0]["depth"]), want["depth"])
        assert _same(np.asarray(Image.open(written[0]["img"])), np.where(want["hit"][:, :, None], want["img"], np.uint8(0)))
        assert _same(np.asarray(Image.open(written[0]["normal"])), np.where(want["hit"][:, :, None], want["normal_img"].astype(np.uint8), np.uint8(0)))


@gpu
def test_nothing_changes_when_the_option_is_unset_and_the_refusals_come_before_any_launch():
    from gens_amd import lib as L, ops
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_vertex_attrs import NETWORK, TODAYS_KEYS, _validate_args
    assert ImplicitSurface.mesh_render is None and ImplicitSurface.last_mesh_render_stats is None
    c = _case()
    m, surf, sc = c["m"], c["m"]["surf"], c["sc"]
    assert "mesh_render" not in vars(surf)
    args = _validate_args(surf, m["vols"])
    L.profile_begin(only=K35 | CAST)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33)
    for off in (None, False):
        torch.manual_seed(3)
        got = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_render=off)
        assert set(got) == set(ref) == TODAYS_KEYS
        for k in TODAYS_KEYS:
            assert torch.equal(torch.as_tensor(got[k]), torch.as_tensor(ref[k])), k
    plain = surf.extract_geometry(m["vols"], m["lo"], m["hi"], 33, 0.0)
    assert len(plain) == 2 and _same(plain[0], ref["vertices"]) and _same(plain[1], ref["triangles"])
    assert not L.profile_end(raw=True)
    L.profile_begin(only=K35 | CAST | NETWORK | {"gens_compact_valid", "gens_mc_emit", "gens_vertex_points"})
    with pytest.raises(ValueError, match="shard"):
        surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_render=True, shard=object())
    with pytest.raises(ValueError, match="extract_geometry=False"):
        surf.validate(*args, extract_geometry=False, mesh_render=True)
    for bad in (3, {"texels": 8}, {"shading": "phong"}):
        with pytest.raises(ValueError, match="mesh_render"):
            surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_render=bad)
    with pytest.raises(ValueError, match="smooth shading needs mesh_attributes"):
        surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_render={"shading": "smooth"}, mesh_attributes=("colors",))
    pts, tri, o, d, w = m["points"], m["tri"], c["o"], c["d"], sc["c2ws"]
    with pytest.raises(ValueError, match="smooth"):
        surf.render_mesh(pts, tri, o, d, w, shading="smooth")
    with pytest.raises(ValueError, match="shading"):
        surf.render_mesh(pts, tri, o, d, w, shading="phong")
    with pytest.raises(ValueError, match="expected \\(T, 3\\)"):
        surf.render_mesh(pts, tri.reshape(-1), o, d, w)
    with pytest.raises(ValueError, match="not the atlas"):
        surf.render_mesh(pts, tri, o, d, w, texture=np.zeros((8, 9, 3), np.uint8))
    with pytest.raises(ValueError, match="texels = 5"):
        surf.render_mesh(pts, tri, o, d, w, texture=c["tex"]["texture"], texels=5)
    with pytest.raises(ValueError, match="seen flags"):
        surf.render_mesh(pts, tri, o, d, w, seen=c["attrs"]["seen"])
    with pytest.raises(ValueError, match="texture_seen without"):
        surf.render_mesh(pts, tri, o, d, w, texture_seen=c["tex"]["texture_seen"])
    face, t = torch.from_numpy(c["face"]).cuda(), torch.from_numpy(c["t"]).cuda()
    for kw, match in (({"normals": torch.zeros(5, 3, device="cuda")}, "normals"), ({"colors": torch.zeros(len(pts), 3, device="cuda")}, "colors"),
                      ({"texture": torch.zeros(8, 9, 3, device="cuda", dtype=torch.uint8), "texels": 8}, "texture"),
                      ({"texture": torch.from_numpy(c["tex"]["texture"]).cuda()}, "texels"), ({"outputs": ("img",)}, "not available"),
                      ({"orient": 2}, "orient")):
        with pytest.raises(ValueError, match=match):
            ops.shade_mesh_hits(c["grid"], o, d, face, t, c["rot"], **kw)
    with pytest.raises(ValueError, match="face"):
        ops.shade_mesh_hits(c["grid"], o, d, face[:-1], t, c["rot"])
    assert not L.profile_end(raw=True)
