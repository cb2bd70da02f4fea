"""Autograd-aware operators of the GenS hot path, each a thin shim over one C-ABI entry point of libgens_hip.so.

The shims allocate outputs with torch (device memory + current stream only) and wire first / second order
derivatives the way the reference's Function pair does (models/modules/grid_sample_cuda/cuda_gridsample.py:71-123):
twice differentiable, outputs of the second backward are constants.  Citations are relative to /root/reference.

The operators live in submodules by kernel family; this package re-exports every name (private helpers included), so `gens_amd.ops.X`
is what it was when ops was one module:
    ops.base      Shared pieces of the operator shims: kernel selection, layout helpers, the texel copies of maps, VolumeSet, SceneCams.
    ops.volume    K1: Volume.agg_mean_var (volume.py:13-63), forward and backward, one level or a scene's pyramid.
    ops.lookup    K2 / K2'' (lookup_volume with first and second derivatives), K3 (nearest masks, ray points), K4 (lookup_feature).
    ops.rays      K5-K7 (hierarchical sampling), K8 (compositing and the step-boundary kernels around it), K9 (patch reads, surface patch warp), K10 (TV).
    ops.geometry  K11 (lattice points), K12 (iso-surface extraction on the device), K23 / K25's view rays, face components and culling tail.
    ops.sdf_pack  The weight streams of K6 and K7: slot tables, the gather, the four SDF stream orders (host code, no launch).
    ops.sdf       K6 (the fused SDF network in inference) and K17 (the SDF network of a training step).
    ops.gemm      K14: a^T b for tall operands, the weight-gradient product of the training step.
    ops.conv3d    K15 / K16: the 3 x 3 x 3 convolutions and the instance norm + ReLU of the cost-volume U-Net.
    ops.blend     K7 (fused source-view look-up + BlendingNetwork in inference) and K18 (the same for a training step).
    ops.conv2d    K21: the depth-wise 2-D convolutions of the MnasNet trunk.
    ops.points    K24: mesh sampling, radius down-sampling and capped nearest neighbours of the DTU scoring (evaluation/dtu_eval.py).
    ops.finalize  K25: elliptical dilation and vertex mask votes of the DTU mesh finalising (evaluation/clean_meshes.py).
    ops.filter    K26: the mask pyramid restricted to the dilated SDF band (GenS.filter_volume, models/gens.py:87-122);
                  K27: the largest connected region of a mask volume (clean_volume, utils/tools.py:34-50).
    ops.lattice   K28: the two-level SDF lattice of extract_geometry, evaluated near the iso-surface only (sparse_lattice), and what K29
                  shares with it: dimensions, point and classify launches under either set of limits, the front end of both.
    ops.brick_mcubes  K29: marching cubes on that lattice's bricks, without the dense lattice (brick_marching_cubes).
    ops.vertex_attrs  K30: per-vertex attributes of an extracted mesh: lattice vertices to points, gradient / colour to normals / 8-bit colours.
    ops.trace     K31: sphere tracing of the surface along rays (sphere_trace) and the per-ray depth / normal / colour pack (surface_pack).
    ops.fusion    K32: per-view depth maps fused into a consistency-filtered point cloud (fusion_cams, fuse_depth_maps, fused_points).
    ops.simplify  K33: mesh simplification by vertex clustering with quadric-optimal representatives (simplify_mesh).
    ops.texture   K34: texture atlases for triangle meshes: atlas samples to points, the guarded Newton snap, colours to pixels, corner coordinates.
    ops.mesh_render  K35: a mesh as rays see it: shading at K23's first hits (shade_mesh_hits), grid -> first hit -> shade (render_mesh), compare_maps.
    ops.mesh_distance  K36: exact point-to-mesh distance over K23's grid (closest_point_on_mesh) and the two-sided comparison of two meshes (mesh_distance).
    ops.mesh_topology  K37: the edge table of a mesh, its topology report, pseudonormals (mesh_topology) and the signed distance (signed_distance_to_mesh).
    ops.mesh_repair  K38: mesh repair: duplicate faces, pinches and non-manifold edges split, small components, orientation, small holes (repair_mesh).
    ops.mesh_fairing  K39: mesh fairing: Laplacian / Taubin smoothing with uniform or cotangent weights (smooth_mesh), mesh_laplacian, mesh_roughness.
    ops.winding   K40: generalised winding numbers, exact or with a bounded far field (build_winding_plan, winding_number), and the inside test (mesh_inside).
    ops.mesh_intersect  K41: self-intersections: which pairs of faces intersect, decided exactly or reported undecided (mesh_self_intersections).
"""
from .base import *  # noqa: F401,F403
from .volume import *  # noqa: F401,F403
from .lookup import *  # noqa: F401,F403
from .rays import *  # noqa: F401,F403
from .geometry import *  # noqa: F401,F403
from .sdf import *  # noqa: F401,F403
from .gemm import *  # noqa: F401,F403
from .conv3d import *  # noqa: F401,F403
from .blend import *  # noqa: F401,F403
from .conv2d import *  # noqa: F401,F403
from .points import *  # noqa: F401,F403
from .finalize import *  # noqa: F401,F403
from .filter import *  # noqa: F401,F403
from .lattice import *  # noqa: F401,F403
from .brick_mcubes import *  # noqa: F401,F403
from .vertex_attrs import *  # noqa: F401,F403
from .trace import *  # noqa: F401,F403
from .fusion import *  # noqa: F401,F403
from .simplify import *  # noqa: F401,F403
from .texture import *  # noqa: F401,F403
from .mesh_render import *  # noqa: F401,F403
from .winding import *  # noqa: F401,F403
from .mesh_distance import *  # noqa: F401,F403
from .mesh_topology import *  # noqa: F401,F403
from .mesh_repair import *  # noqa: F401,F403
from .mesh_fairing import *  # noqa: F401,F403
from .mesh_intersect import *  # noqa: F401,F403
