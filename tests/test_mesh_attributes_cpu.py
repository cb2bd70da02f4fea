"""Per-vertex mesh attributes, host side: the PLY writer / reader with normals and colours, transform_normals, the vertex index of the
component step, and the restatement of K30's two kernels (tests/vertex_attrs_reference.py) on edge rows.  No GPU."""
import numpy as np
import pytest

from gens_amd import io as gio

from . import vertex_attrs_reference as VR


def _mesh(n_v=7, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n_v, 3))
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], dtype=np.int32)
    n = rng.standard_normal((n_v, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    c = rng.integers(0, 256, (n_v, 3)).astype(np.uint8)
    return v, t, n, c


def _bare_bytes(v, t):
    """Today's layout, assembled by hand."""
    header = ("ply\nformat binary_little_endian 1.0\ncomment gens_amd\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    body = np.asarray(v, dtype="<f4").tobytes()
    for tri in np.asarray(t, dtype="<i4"):
        body += b"\x03" + tri.tobytes()
    return header + body


def test_write_ply_without_attributes_is_todays_file(tmp_path):
    v, t, _, _ = _mesh()
    for name, kw in (("a.ply", {}), ("b.ply", {"normals": None, "colors": None})):
        gio.write_ply(tmp_path / name, v, t, **kw)
        assert (tmp_path / name).read_bytes() == _bare_bytes(v, t)
    got = gio.read_ply(tmp_path / "a.ply")
    assert len(got) == 2 and np.array_equal(got[0], v.astype(np.float32)) and np.array_equal(got[1], t)
    v2, t2, attrs = gio.read_ply(tmp_path / "a.ply", attributes=True)
    assert attrs == {} and np.array_equal(v2, got[0]) and np.array_equal(t2, t)


@pytest.mark.parametrize("with_normals,with_colors", [(True, True), (True, False), (False, True)])
def test_attributes_round_trip_in_the_stated_order(tmp_path, with_normals, with_colors):
    v, t, n, c = _mesh()
    path = tmp_path / "m.ply"
    gio.write_ply(path, v, t, normals=n if with_normals else None, colors=c if with_colors else None)
    header = path.read_bytes().split(b"end_header\n")[0].decode("ascii").splitlines()
    props = [line for line in header if line.startswith("property") and "list" not in line]
    want = ["property float x", "property float y", "property float z"]
    want += ["property float nx", "property float ny", "property float nz"] if with_normals else []
    want += ["property uchar red", "property uchar green", "property uchar blue"] if with_colors else []
    assert props == want
    v2, t2, attrs = gio.read_ply(path, attributes=True)
    assert np.array_equal(v2, v.astype(np.float32)) and np.array_equal(t2, t)
    assert sorted(attrs) == sorted((["normals"] if with_normals else []) + (["colors"] if with_colors else []))
    if with_normals:
        assert attrs["normals"].dtype == np.float32 and np.array_equal(attrs["normals"], n)
    if with_colors:
        assert attrs["colors"].dtype == np.uint8 and np.array_equal(attrs["colors"], c)
    plain = gio.read_ply(path)                               # without the flag: the same 2-tuple as before on the same file
    assert len(plain) == 2 and np.array_equal(plain[0], v2) and np.array_equal(plain[1], t2)


def test_attribute_length_mismatches_raise(tmp_path):
    v, t, n, c = _mesh()
    with pytest.raises(ValueError, match="normals"):
        gio.write_ply(tmp_path / "m.ply", v, t, normals=n[:-1])
    with pytest.raises(ValueError, match="colors"):
        gio.write_ply(tmp_path / "m.ply", v, t, colors=c[:-1])
    with pytest.raises(ValueError, match="colors"):
        gio.write_ply(tmp_path / "m.ply", v, t, normals=n, colors=np.concatenate([c, c]))


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_transform_normals_keeps_normals_perpendicular_to_transformed_tangents():
    rng = np.random.default_rng(3)
    m = np.eye(4)
    m[:3, :3] = _rotation(4) @ np.diag([0.5, 2.0, 7.0])       # a rotation times a non-uniform scale
    m[:3, 3] = [3.0, -1.0, 0.25]
    n = rng.standard_normal((200, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    tangent = np.cross(n, rng.standard_normal((200, 3)))     # tangent directions at p: n . t = 0
    p = rng.standard_normal((200, 3))
    moved = gio.transform_vertices(p + tangent, m) - gio.transform_vertices(p, m)
    n[17] = 0.0
    out = gio.transform_normals(n, m)
    assert out.shape == (200, 3) and out.dtype == np.float64
    rest = np.arange(200) != 17
    dots = np.abs((out * moved).sum(axis=1) / np.linalg.norm(moved, axis=1))
    assert dots[rest].max() < 1e-12, dots[rest].max()
    assert np.abs(np.linalg.norm(out[rest], axis=1) - 1.0).max() < 1e-14
    assert np.array_equal(out[17], [0.0, 0.0, 0.0])
    assert np.abs((out * (n @ m[:3, :3].T)).sum(axis=1)[rest]).min() > 0          # and they keep their side of the surface


def test_transform_normals_under_a_uniform_scale_changes_nothing():
    n = np.random.default_rng(5).standard_normal((50, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    m = np.diag([2.5, 2.5, 2.5, 1.0])
    m[:3, 3] = [1.0, 2.0, 3.0]
    assert np.abs(gio.transform_normals(n, m) - n).max() < 1e-15
    assert gio.transform_normals(np.zeros((0, 3)), m).shape == (0, 3)


def _two_components():
    """An octahedron (8 faces) and a lone tetrahedron (4 faces) sharing no vertex, with one unreferenced vertex in front."""
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    of = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    tet = np.array([[5, 5, 5], [6, 5, 5], [5, 6, 5], [5, 5, 6]], dtype=np.float64)
    tf = [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]
    v = np.concatenate([[[9.0, 9, 9]], tet, octa])
    t = np.array([[a + 1 for a in f] for f in tf] + [[a + 5 for a in f] for f in of], dtype=np.int32)
    return v, t


def test_drop_small_components_returns_the_kept_vertices_index():
    v, t = _two_components()
    plain = gio.drop_small_components(v, t, min_faces=5)
    assert len(plain) == 2
    v1, t1, index = gio.drop_small_components(v, t, min_faces=5, return_index=True)
    assert np.array_equal(v1, plain[0]) and np.array_equal(t1, plain[1]) and t1.dtype == plain[1].dtype
    assert index.dtype == np.int64 and np.array_equal(index, np.arange(5, 11))
    assert np.array_equal(v[index], v1) and len(t1) == 8
    assert np.array_equal(v1[t1], v[t[4:]])                  # the kept faces are the octahedron's, corner for corner
    v0, t0, i0 = gio.drop_small_components(v, t[:0], return_index=True)
    assert len(v0) == 0 and len(t0) == 0 and i0.dtype == np.int64 and len(i0) == 0


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_restated_normals_on_edge_rows():
    n64, n = VR.normals64(VR.EDGE_GRADS), VR.normals(VR.EDGE_GRADS)
    assert n.dtype == np.float32
    for row in (0, 1, 2, 3):                                 # zero gradient, NaN, +inf, -inf
        assert np.array_equal(n[row], np.zeros(3, np.float32)), row
    assert np.array_equal(n[4], [1, 0, 0])                   # 1e-30: its float32 square underflows, the float64 one does not
    assert abs(np.linalg.norm(n64[5]) - 1.0) < 1e-15 and np.allclose(n64[5], np.array([1, -2, 2]) / 3.0, rtol=1e-7)
    assert np.array_equal(n[6], np.array([0.6, 0.8, 0.0], dtype=np.float32))
    assert np.array_equal(n[7], [0, 0, -1])
    assert np.allclose(n64[8], 3 ** -0.5, rtol=1e-15)        # 1e38: the float32 sum of squares would overflow
    assert np.allclose(n64[9], np.array([1, 2, 2]) / 3.0, rtol=1e-15)
    live = np.linalg.norm(n64, axis=1) > 0
    assert np.abs(np.linalg.norm(n64[live], axis=1) - 1.0).max() < 1e-15


def test_restated_colours_on_edge_values():
    c = np.zeros((len(VR.EDGE_COLORS), 3), dtype=np.float32)
    c[:, 0] = VR.EDGE_COLORS
    q = VR.colors(c)
    assert q.dtype == np.uint8
    #           0   1/256-e  1/256  255/256  1.0  1.5  -0.1  nan  +inf  -inf  0.5  255.999/256
    assert q[:, 0].tolist() == [0, 0, 1, 255, 255, 255, 0, 0, 0, 0, 128, 255]
    assert np.array_equal(q[:, 1:], np.zeros_like(q[:, 1:]))
    assert np.float32(1 / 256) - VR.EDGE_COLORS[1] > 0      # the value below 1/256 really is below it in float32


@pytest.mark.parametrize("s", [1, 2, 4])
def test_restated_seen_on_zero_and_one_hot_rows(s):
    flags = VR.flag_rows(s)
    assert VR.seen(flags).tolist() == [False] + [True] * s
    grad, color, vis = VR.random_rows(100, s, seed=s)
    n, q, sn = VR.pack(grad, color, vis)
    assert n.shape == (100, 3) and q.shape == (100, 3) and sn.shape == (100,) and sn.dtype == bool
    assert np.array_equal(sn, vis.sum(axis=1) > 0) and not sn.all() and sn.any()


def test_restated_points_are_the_host_expression():
    lo, hi = np.array([-1, -0.5, -0.25], np.float32), np.array([1, 0.75, 0.5], np.float32)
    v = np.array([[0, 0, 0], [32, 32, 32], [1.5, 7.25, 31.999]], dtype=np.float64)
    want = v / (33 - 1.0) * (hi - lo)[None, :] + lo[None, :]
    got = VR.points(v, 33, lo, hi)
    assert want.dtype == np.float64 and got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(got[0], lo) and np.array_equal(got[1], hi)
