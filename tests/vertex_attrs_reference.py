"""K30's two kernels restated with numpy, straight from their definitions (include/gens_hip.h): the GPU tests compare the device against
these, the CPU tests pin the restatement itself on edge rows.  Nothing here imports the library."""
import numpy as np


def points(vertices, resolution, b_min, b_max):
    """gens_vertex_points: float32 of the float64 vertices extract_geometry returns, its host expression term for term.  b_min / b_max: the
    float32 bounds as numpy arrays; their difference is formed in float32, as extract_geometry forms it."""
    b_min, b_max = np.asarray(b_min, dtype=np.float32), np.asarray(b_max, dtype=np.float32)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    return (v / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]).astype(np.float32)


def normals64(grad):
    """The unit normals in float64 (not yet rounded): g / sqrt((gx^2 + gy^2) + gz^2); zero rows where a component is not finite or the
    norm is 0."""
    g = np.asarray(grad, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = np.isfinite(g).all(axis=1) & (norm > 0)
        return np.where(ok[:, None], g / np.where(ok, norm, 1.0)[:, None], 0.0)


def normals(grad):
    return normals64(grad).astype(np.float32)


def colors(color):
    """uint8(trunc(min(max(c * 256, 0), 255))) on float32 (validate's img_fine convention); 0 where c is not finite."""
    c = np.asarray(color, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.minimum(np.maximum(c * np.float32(256), np.float32(0)), np.float32(255))
    return np.where(np.isfinite(c), np.trunc(np.where(np.isfinite(q), q, 0)), 0).astype(np.uint8)


def seen(vis):
    v = np.asarray(vis)
    return (v.reshape(v.shape[0], -1) != 0).any(axis=1)


def pack(grad, color, vis):
    return normals(grad), colors(color), seen(vis)


# ---------------------------------------------------------------------------------------------------------------- shared test inputs
EPS = float(np.finfo(np.float32).eps)
EDGE_GRADS = np.array([[0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, 1, -np.inf], [1e-30, 0, 0], [1e-30, -2e-30, 2e-30], [3, 4, 0], [-0.0, 0.0, -1.0],
                       [1e38, 1e38, 1e38], [1, 2, 2]], dtype=np.float32)
EDGE_COLORS = np.array([0.0, 1 / 256 - EPS / 256, 1 / 256, 255 / 256, 1.0, 1.5, -0.1, np.nan, np.inf, -np.inf, 0.5, 255.999 / 256], dtype=np.float32)


def edge_rows():
    """-> (grad (n,3), color (n,3)) float32: every edge gradient beside edge colours in the three channels, in rotation."""
    n = max(len(EDGE_GRADS), len(EDGE_COLORS))
    grad = EDGE_GRADS[np.arange(n) % len(EDGE_GRADS)]
    color = np.stack([EDGE_COLORS[(np.arange(n) + k) % len(EDGE_COLORS)] for k in range(3)], axis=1)
    return grad.copy(), color.copy()


def random_rows(n, s, seed):
    """Seeded rows: gradients over forty decades, colours around [0, 1] with excursions, sparse in-frustum flags with all-zero rows."""
    rng = np.random.default_rng(seed)
    grad = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-30, 10, (n, 1))).astype(np.float32)
    color = rng.uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
    vis = (rng.uniform(size=(n, s)) < 0.3).astype(np.uint8)
    return grad, color, vis


def flag_rows(s):
    """All-zero and one-hot flag rows for S source views -> (s + 1, s) uint8."""
    return np.concatenate([np.zeros((1, s), np.uint8), np.eye(s, dtype=np.uint8)])
