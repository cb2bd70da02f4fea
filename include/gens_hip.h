/*
 * gens_hip.h -- C ABI of libgens_hip.so: the GenS hot path as hand-written HIP kernels for gfx950 (MI355X).
 *
 * Drop-in boundary.  The reference's only native ABI is the pybind pair
 *     grad2_2d / grad2_3d                (models/modules/grid_sample_cuda/gridsample_cuda.cpp:26-56)
 * reached through cuda_gridsample.grid_sample_3d (cuda_gridsample.py:12-14, 71-123); everything else on the
 * path is PyTorch tensor code.  Each entry point below names the reference code it replaces.  All citations are
 * relative to /root/reference.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous float32 unless its comment says otherwise (host arrays of
 *     device pointers are spelled `const float* const*` and documented as host);
 *   - inputs are borrowed and never written; outputs are caller-allocated; outputs documented "accumulates" must
 *     be zero-filled by the caller (they are atomically added to);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work, they never
 *     synchronise;
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative GENS_E* argument error.
 *     gens_last_error() returns a static description of the last failure on the calling thread;
 *   - volumes are (C, X, Y, Z) with world x <-> X ("planar", the reference's (1,C,D,D,D) tensor, Q1) or
 *     (X, Y, Z, 4) ("packed": one 16-byte texel per voxel, built by gens_pack_volume);
 *   - feature maps / images consumed by the samplers are NHWC with the channel count padded to a multiple of 4
 *     ("texel" layout, built by gens_pack_nchw); C_pad below always means 4*ceil(C/4);
 *   - only C = 4 channels per volume level are supported (every shipped config: confs/gens.conf:63-67).
 */
#ifndef GENS_HIP_H
#define GENS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GENS_MAX_LEVELS 8
#define GENS_MAX_VIEWS 16  /* the reference's fine-tune sets hold up to 11 views (dtu_finetune.py: ref + 10 sources); K1's culled fast path serves <= 8, more views take its generic kernel */

#define GENS_EINVAL (-1)   /* bad argument (null pointer, size out of range)          */
#define GENS_ELIMIT (-2)   /* more levels / views / channels than the build supports */

#define GENS_LAYOUT_PLANAR 0
#define GENS_LAYOUT_PACKED 1

const char* gens_last_error(void);
/* 12.  History: 7 = 6 + gens_sdf_grad_f16 (the split-half value + gradient kernel).
 *   8 = round 4's additions, which shipped under the stale number 7: gens_grid_sample_{fwd,bwd,bwd2} (K20), gens_depthwise_conv2d_{fwd,dgrad,wgrad}
 *       + gens_depthwise_conv2d_wgrad_parts (K21), gens_batchnorm2d_train_{fwd,bwd} + gens_batchnorm2d_scratch_doubles (K22),
 *       gens_blend_train_bwd_acc + gens_blend_train_acc_{parts,floats}, gens_merge_upsample, gens_conv3d_wgrad_parts_strided, gens_instnorm_finish,
 *       gens_sdf_grad_stash_reset, gens_sdf_grad_f16_stash_reset, and gens_ray_points' `mid` / `sample_dist` arguments.
 *   9 = round 5: gens_composite_in gained `cos_anneal_dev` (the annealing ratio read from the device, so that a captured step can be replayed
 *       with another ratio) -- a struct-layout change: callers built against 8 must be rebuilt.
 *   10 = round 5: gens_sdf_train_bwd's w6_part has a row per SIXTEEN points (npad / 16 rows, was npad / 32): its workgroups own 16 points
 *       now, two of them to a compute unit.
 *   11 = round 6: gens_blend_train_bwd_t + gens_blend_train_t_parts + gens_blend_train_bwd_t_dump (the colour branch's backward transposed: one
 *       wave per 16 rows, nothing shared between waves but the weights in LDS).
 *   12 = round 6: gens_upsample2d_cat (the warp features in one launch), gens_volume_build_levels_bits (the volume build leaves the masks as bits
 *       too), gens_select_views (the views of a fine-tune step out of the frozen maps and their layouts in one launch),
 *       gens_lookup_volume_bwd_bricks / _bwd2_bricks + gens_lookup_scatter_bricks_scratch_bytes (K2's volume-gradient scatter brick by brick).
 *       Later additions that change no existing entry keep 12: gens_sdf_{value,grad}_bf16x3 + gens_sdf_bf16x3_pieces (+ gens_sdf_bf16x3_residency, gens_sdf_bf16x3_layout;
 *       NOTE: with gens_sdf_bf16x3_layout the STREAM of gens_sdf_{value,grad}_bf16x3 changed at three levels -- forward layer 3 has seven hidden K blocks,
 *       gens_sdf_bf16x3_pieces(3) went from 1520 to 1512 -- without a new number, because the suite pins 12: a caller that packs the stream itself must
 *       ask gens_sdf_bf16x3_layout and pack what it says; a stream packed for the earlier layout gives wrong numbers and no error),
 *       gens_blend_bf16x3_residency, and K23's
 *       gens_mesh_grid_{count,fill}, gens_ray_first_hit, gens_view_rays_hit_faces, gens_face_cc_{hook,compress}, and K24's
 *       gens_mesh_sample_{count,emit}, gens_point_grid_{count,fill}, gens_radius_downsample_round, gens_nearest_point, and K25's
 *       gens_dilate_u8, gens_vertex_mask_votes, gens_view_rays_hit_counts, and K26's gens_filter_masks, gens_filter_band, gens_filter_levels,
 *       and K27's gens_largest_component, gens_components_scratch_bytes, gens_unpack_mask_bits, and K28's gens_sparse_coarse_points,
 *       gens_sparse_classify, gens_sparse_brick_points, gens_sparse_fill, gens_sparse_scatter, gens_sparse_leaks, and K29's
 *       gens_brick_coarse_points, gens_brick_points, gens_brick_active, gens_brick_emit_flags, gens_brick_mc_classify, gens_brick_mc_emit,
 *       and K30's gens_vertex_points, gens_vertex_pack, and K31's gens_trace_begin, gens_trace_march, gens_trace_refine, gens_trace_gather,
 *       gens_surface_pack, and K32's gens_fuse_depth_maps, gens_fused_points, and K33's gens_cluster_keys, gens_cluster_triangles,
 *       gens_cluster_solve, and K34's gens_texture_points, gens_texture_snap, gens_texture_keep_better,
 *       gens_texture_pack, gens_texture_uv, and K35's gens_mesh_shade, and K36's gens_mesh_closest_point, and K37's gens_mesh_edge_keys,
 *       gens_mesh_edge_classify, gens_mesh_fan_pairs, gens_mesh_vertex_classify, gens_mesh_pseudonormals, gens_mesh_distance_sign, and K38's
 *       gens_mesh_face_keys, gens_mesh_split_corners, gens_mesh_orient_pairs, gens_mesh_apply_flips, gens_mesh_loop_centroids,
 *       gens_mesh_fill_emit, and K39's gens_mesh_corner_cot, gens_mesh_edge_weights, gens_mesh_laplacian_step, gens_mesh_dihedral, and K40's
 *       gens_mesh_winding_moments, gens_mesh_winding_number, and K41's gens_mesh_isect_faces, gens_mesh_isect_count, gens_mesh_isect_emit. */
int gens_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Layout helpers (no reference counterpart: the reference keeps NCHW / NCDHW everywhere).
 * ---------------------------------------------------------------------------------------------------------- */

/* src (n, C, H, W) -> dst (n, H, W, C_pad), pad channels are zero. */
int gens_pack_nchw(const float* src, float* dst, int n, int c, int h, int w, void* stream);
/* adjoint: dst (n, C, H, W) = channels 0..C-1 of src (n, H, W, C_pad)   (overwrites dst). */
int gens_unpack_nhwc(const float* src, float* dst, int n, int c, int h, int w, void* stream);
/* src (4, X, Y, Z) -> dst (X, Y, Z, 4). */
int gens_pack_volume(const float* src, float* dst, int x, int y, int z, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K1  Volume.agg_mean_var, one level per call          (models/modules/volume.py:21-61)
 *   feat    (nv, H, W, 4) texels of features[level]
 *   w2c     (nv, 4, 4) = inverse(c2ws)                   (volume.py:34)
 *   intr    (nv, 4, 4) level-0 intrinsics; rows 0-1 are multiplied by intr_scale = 0.5^level in-kernel (:24-25)
 *   volume  (8, D, D, D) = [mean(4) | var(4)], mask (D, D, D) float 0/1 = (count > min_vis_view)   (:53-58)
 * bwd: g_volume (8, D, D, D) -> g_feat (nv, H, W, 4), accumulates (gradient w.r.t. features only, :27-44).
 * ---------------------------------------------------------------------------------------------------------- */
int gens_volume_build_fwd(const float* feat, const float* w2c, const float* intr, float intr_scale, int nv, int h,
                          int w, int d, int min_vis_view, float* volume, float* mask, void* stream);
int gens_volume_build_bwd(const float* feat, const float* w2c, const float* intr, float intr_scale, int nv, int h,
                          int w, int d, const float* g_volume, float* g_feat, void* stream);
/* All levels of one scene in a single launch (volume.py:21-61 is a loop over the levels): feat[l] (nv, H_l, W_l, 4) texels,
 * hw = {H_0, W_0, H_1, W_1, ...}, intr[l] (nv, 4, 4) with rows 0-1 already multiplied by 0.5^l, volumes[l] (8, D_l^3), masks[l] (D_l^3).
 * Same results as n_levels calls of gens_volume_build_fwd with intr_scale = 1 (which it falls back to for sizes the fused kernel
 * does not cover).  counts: NULL, or a HOST array of device pointers (an entry may be NULL) to (D_l^3) uint8 planes, 16-byte aligned,
 * that receive the number of views each voxel is visible in (volume.py:50 `count`) -- what gens_volume_build_bwd_levels reads back. */
int gens_volume_build_levels(const float* const* feat, const int* hw, const int* dims, int n_levels, const float* w2c,
                             const float* const* intr, int nv, int min_vis_view, float* const* volumes, float* const* masks,
                             uint8_t* const* counts, void* stream);
/* The same launch, leaving the masks as BITS too (ABI 12): mask_bits: NULL, or a HOST array of device pointers (an entry may be NULL) to
 * ceil(D_l^3 / 32) uint32 words, bit (i & 31) of word (i >> 5) = masks[l][i] > 0 -- what gens_pack_mask_bits makes of the float plane and the
 * ray-point / nearest look-up kernels read with mask_bits = 1; a training step then has no packing pass over the masks. */
int gens_volume_build_levels_bits(const float* const* feat, const int* hw, const int* dims, int n_levels, const float* w2c,
                                  const float* const* intr, int nv, int min_vis_view, float* const* volumes, float* const* masks,
                                  uint8_t* const* counts, uint32_t* const* mask_bits, void* stream);
/* d(volumes)/d(texels) of ALL levels in one launch set (five launches whatever n_levels is) with the sum owned by the IMAGE: the (64-voxel tile,
 * view) pairs are sorted by the 64 x 60-texel image tile they project into, a workgroup per tile keeps that tile's gradient in LDS (double
 * sums) and writes every touched texel once (gens_volume_build_bwd, the wave-window kernel, is bound by its ~0.3 G global atomics at 256^3).
 * It reads what the forward pass left: the means (volumes[l], planes 0-3) and the visible-view counts (counts[l]) of gens_volume_build_levels
 * on the same inputs; nothing is re-derived per voxel except the projection into the one view a work item serves.  g_volumes[l] (8, D_l^3)
 * or NULL (no gradient for that level), g_feat[l] (nv, H_l, W_l, 4) accumulates.  Every D_l must be a multiple of 16; intrinsics pre-scaled
 * per level as for gens_volume_build_levels.  scratch: gens_volume_build_bwd_levels_scratch_bytes bytes of device memory (20 bytes per
 * (64-voxel tile, view) pair + the bins; 0 = sizes not covered: use gens_volume_build_bwd level by level), contents irrelevant before and
 * after.  Results equal gens_volume_build_bwd's up to the order of the float32 sums. */
int64_t gens_volume_build_bwd_levels_scratch_bytes(const int* hw, const int* dims, int n_levels, int nv);
int gens_volume_build_bwd_levels(const float* const* feat, const int* hw, const int* dims, int n_levels, const float* w2c,
                                 const float* const* intr, int nv, const float* const* volumes, const uint8_t* const* counts,
                                 const float* const* g_volumes, float* const* g_feat, void* scratch, int64_t scratch_bytes, void* stream);
/* Self-test of K1's exact-division shortcuts (RN(1/b) from v_rcp_f32 + one FMA refinement; a/b from that reciprocal + FMA
 * correction) against the IEEE division over all 2^32 float32 bit patterns: counts[0] += reciprocal mismatches,
 * counts[1] += quotient mismatches (device array of 2, zeroed by the caller).  Both stay 0. */
int gens_selftest_division(unsigned long long* counts, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K2  lookup_volume(pts, volumes, "grad"): all levels in one launch
 *     forward            projector.py:217-245 -> cuda_gridsample._GridSample3dForward (cuda_gridsample.py:71-84)
 *     backward           aten::grid_sampler_3d_backward via _GridSample3dBackward.forward (:94-108)
 *     backward-backward  gridsample_grad2.grad2_3d (gridsample_cuda.cpp:42-56, gridsample_cuda.cu:212-533, 601-666)
 *   vols     HOST array of n_levels device pointers; dims HOST int[3*n_levels] = (X,Y,Z) per level
 *   pts      (N, 3) world points in [-1,1] (no flip: x indexes X)
 *   out / g_out / gg_out   (N, 4*n_levels), level-major like torch.cat(feats, -1)
 *   g_vols / g_vols2       HOST arrays of device pointers (same layout as vols), accumulate; NULL = not wanted
 *   gg_vols                HOST array or NULL (the reference's `grad2_grad_input is None`, cuda_gridsample.py:113)
 *   g_pts / gg_pts / g_pts2  (N, 3); g_pts, g_pts2 are overwritten
 * ---------------------------------------------------------------------------------------------------------- */
int gens_lookup_volume_fwd(const float* const* vols, const int* dims, int n_levels, int layout, const float* pts,
                           int64_t n, float* out, void* stream);
int gens_lookup_volume_bwd(const float* const* vols, const int* dims, int n_levels, int layout, const float* pts,
                           const float* g_out, int64_t n, float* const* g_vols, float* g_pts, void* stream);
int gens_lookup_volume_bwd2(const float* const* vols, const int* dims, int n_levels, int layout, const float* pts,
                            const float* g_out, const float* gg_pts, const float* const* gg_vols, int64_t n,
                            float* gg_out, float* const* g_vols2, float* g_pts2, void* stream);
/* The same two with the scatter into the volume gradients done BRICK BY BRICK (ABI 12): the points are counted into bricks of 8^3 cells of the finest
 * level, a workgroup per brick sums its points' corner contributions in LDS (double sums) and sends every touched voxel to memory once -- for large
 * point sets whatever their order (the direct scatter of the entries above sends 32 atomics per point and level).  scratch:
 * gens_lookup_scatter_bricks_scratch_bytes(n) bytes of device memory, 16-byte aligned.  Same results up to the order of the float sums.  Volumes
 * wider than 256 cells per axis fall back to the direct scatter. */
int64_t gens_lookup_scatter_bricks_scratch_bytes(int64_t n);
int gens_lookup_volume_bwd_bricks(const float* const* vols, const int* dims, int n_levels, int layout, const float* pts,
                                  const float* g_out, int64_t n, float* const* g_vols, float* g_pts, void* scratch,
                                  int64_t scratch_bytes, void* stream);
int gens_lookup_volume_bwd2_bricks(const float* const* vols, const int* dims, int n_levels, int layout, const float* pts,
                                   const float* g_out, const float* gg_pts, const float* const* gg_vols, int64_t n,
                                   float* gg_out, float* const* g_vols2, float* g_pts2, void* scratch, int64_t scratch_bytes,
                                   void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K3  lookup_volume(pts, mask_volumes, "nearest").any(-1)        (projector.py:231,240; Q6, Q7)
 *   masks  HOST array of device pointers to (X,Y,Z) float masks; valid (N) uint8; vals (N, n_levels) or NULL.
 * gens_ray_points fuses the point generation of render / render_core (implicit_surface.py:160-174, 367-371):
 *   z (B, n); mid != 0 -> samples at z + 0.5*dist with the last dist = sample_dist (Q10)
 *   pts (B*n, 3), valid (B*n) uint8.
 * gens_pack_mask_bits: (n) float mask -> ceil(n/32) uint32 words, bit i%32 of word i/32 = (mask[i] > 0) -- the 256^3
 *   level becomes 2 MB and stays in L2.  gens_ray_points / gens_upsample read such words when mask_bits != 0
 *   (masks[] then point to the words); the decisions are identical to the float masks.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_lookup_mask_nearest(const float* const* masks, const int* dims, int n_levels, const float* pts, int64_t n,
                             uint8_t* valid, float* vals, void* stream);
int gens_ray_points(const float* rays_o, const float* rays_d, const float* z, int64_t n_rays, int n_samples, int mid,
                    float sample_dist, const float* const* masks, const int* dims, int n_levels, int mask_bits,
                    float* pts, uint8_t* valid, void* stream);
int gens_pack_mask_bits(const float* mask, int64_t n, uint32_t* bits, void* stream);

/* Order-preserving compaction of the valid flags written by gens_ray_points / gens_upsample: idx[0..count) = positions of
 * the non-zero flags in increasing order; if no flag is set, count = min(10, n) and idx = 0..count-1 (Q7,
 * implicit_surface.py:123-124,176-177,372-373).  idx (n) int64, count (1) int32, scratch (ceil(n/1024)+1) int32: DEVICE. */
int gens_compact_valid(const uint8_t* valid, int64_t n, int64_t* idx, int32_t* count, int32_t* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K4  lookup_feature + compute_angle                              (projector.py:278-349)
 *   feats   HOST array of n_levels device pointers to (nv, H_l, W_l, 4) texels, hw HOST int[2*n_levels]
 *   imgs    (nv, H_0, W_0, 4) texels of the RGB images (channel 3 = pad)
 *   w2c, intr, c2w  (nv, 4, 4); view 0 is the reference view, sources are views 1..nv-1
 *   out (N, S, 3 + 4*n_levels), ray_diff (N, S, 4), vis (N, S) uint8       S = nv - 1
 * bwd: g_out -> g_feats[l] (nv, H_l, W_l, 4), g_imgs (nv, H_0, W_0, 4); accumulate; either may be NULL.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_lookup_feature_fwd(const float* const* feats, const int* hw, int n_levels, const float* imgs,
                            const float* w2c, const float* intr, const float* c2w, int nv, const float* pts,
                            int64_t n, float* out, float* ray_diff, uint8_t* vis, void* stream);
int gens_lookup_feature_bwd(const int* hw, int n_levels, const float* w2c, const float* intr, int nv,
                            const float* pts, const float* g_out, int64_t n, float* const* g_feats, float* g_imgs,
                            void* stream);
/* ... with g_out COMPACT (row i = the i-th selected point, as gens_blend_train_bwd writes it) while the point itself is pts[index[i]];
 * only min(n, *n_device) rows exist. */
int gens_lookup_feature_bwd_idx(const int* hw, int n_levels, const float* w2c, const float* intr, int nv,
                                const float* pts, const float* g_out, const int64_t* index, int64_t n, const int32_t* n_device,
                                float* const* g_feats, float* g_imgs, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K5 + K6  ImplicitSurface.up_sample + sample_pdf(det=True)      (implicit_surface.py:14-44, 60-109)
 *   one wavefront per ray; z, sdf (B, n) with n <= 128; inv_s = 64 * 2^round; n_new <= 64
 *   z_new (B, n_new); pts_new (B*n_new, 3) and valid_new (B*n_new) uint8 feed the next SDF evaluation (:117-121).
 *   valid_in (B, n) uint8 or NULL: the mask decisions of the existing samples as written by gens_ray_points /
 *   gens_upsample and carried through gens_merge_samples (the reference looks all n of them up again every round, :66-67;
 *   the values are the same because the samples are); NULL = look them up here.
 * K7  cat_z_vals: sorted merge of (z, sdf) with (z_new, sdf_new)  (:111-133); sdf / sdf_new / sdf_out may be NULL
 *   together (the `last` round); valid / valid_new / valid_out (uint8) likewise.  n + n_new <= 128.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_upsample(const float* rays_o, const float* rays_d, const float* z, const float* sdf, int64_t n_rays, int n,
                  int n_new, float inv_s, const float* const* masks, const int* dims, int n_levels, int mask_bits,
                  const uint8_t* valid_in, float* z_new, float* pts_new, uint8_t* valid_new, void* stream);
int gens_merge_samples(const float* z, const float* sdf, const float* z_new, const float* sdf_new, const uint8_t* valid,
                       const uint8_t* valid_new, int64_t n_rays, int n, int n_new, float* z_out, float* sdf_out,
                       uint8_t* valid_out, void* stream);
/* One launch per sampling round: cat_z_vals of round i (implicit_surface.py:111-133) fused with up_sample + sample_pdf of round i + 1 (:60-109,
 * mode 0) or, after the last round, with render_core's section mid-points and their mask decisions (:163-173, mode 1 = gens_ray_points(mid)).
 * (z, sdf, valid) (n_rays, n) + (z_add, sdf_add, valid_add) (n_rays, n_add) -> merged (n_rays, n + n_add) in z_out / sdf_out / valid_out;
 * mode 0: z_new (n_rays, n_new), pts_out (n_rays n_new, 3), valid_new (n_rays n_new);  mode 1: pts_out (n_rays (n + n_add), 3), valid_new likewise
 * (sdf, valid, sdf_add, valid_add, sdf_out, valid_out, z_new may be NULL).  Results equal gens_merge_samples followed by gens_upsample (mode 0,
 * with the merged mask decisions as valid_in) / by gens_ray_points with mid = 1 (mode 1), bit for bit. */
int gens_merge_upsample(const float* rays_o, const float* rays_d, const float* z, const float* sdf, const uint8_t* valid,
                        const float* z_add, const float* sdf_add, const uint8_t* valid_add, int64_t n_rays, int n, int n_add, int n_new,
                        float inv_s, float sample_dist, const float* const* masks, const int* dims, int n_levels, int mask_bits, int mode,
                        float* z_out, float* sdf_out, uint8_t* valid_out, float* z_new, float* pts_out, uint8_t* valid_new, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K8  render_core compositing                                     (implicit_surface.py:160-168, 202-303)
 *   per-sample inputs (B, n[, 3]); n <= 128; voxel_mask (B*n) uint8; src_vis (B*n, S) uint8 or NULL
 *   smooth may be NULL (inference).  rot = inverse(c2ws[0,:3,:3]) (3,3) HOST floats passed by value as 9 floats, or rot_dev: the same
 *   nine floats in DEVICE memory (gens_scene_setup's rot_inv; NULL = use rot) -- no device-to-host read per scene
 *   inv_s: DEVICE pointer to one float (already clipped, :206); z_max: DEVICE pointer to max(z) (:301)
 *   per-ray outputs: color (B,3) normal (B,3) depth (B) wsum (B) wmax (B) valid (B) uint8 mid_in (B)
 *                    sdf_depth (B) z_cross (B) [clamped, :300-302] cross_idx (B) int32
 *                    eik_num (B) eik_den (B) smooth_vec (B,3)
 *   per-sample outputs: weights (B,n) inside (B,n)
 * bwd: cotangents (NULL = zero) g_color (B,3) g_normal (B,3) g_depth (B) g_weights (B,n) g_wsum (B) g_eik_num (B)
 *      g_smooth_vec (B,3) g_z_cross (B)  ->  g_sdf (B,n) g_grad (B,n,3) g_col (B,n,3) g_smooth (B,n,3 or NULL)
 *      g_inv_s (B) per-ray partials (sum them).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const float *rays_o, *rays_d, *z, *sdf, *grad, *color, *smooth;
    const uint8_t *voxel_mask, *src_vis;
    const float *inv_s, *z_max;
    int64_t n_rays;
    int n, n_src;
    float sample_dist, cos_anneal;
    float rot[9];
    const float* rot_dev;
    const float* cos_anneal_dev;   /* NULL, or a device float that REPLACES cos_anneal (read at launch: a HIP graph of the step can be replayed
                                    * with this step's ratio, runner.py:156-157,394-398) */
} gens_composite_in;

typedef struct {
    float *color, *normal, *depth, *wsum, *wmax, *mid_in, *sdf_depth, *z_cross, *eik_num, *eik_den, *smooth_vec;
    uint8_t* valid;
    int32_t* cross_idx;
    float *weights, *inside;
    float* pts_cross;          /* (B, 3) or NULL: rays_o + rays_d * z_cross, the surface point pts_sdf0 (implicit_surface.py:304) */
} gens_composite_out;

typedef struct {
    const float *g_color, *g_normal, *g_depth, *g_weights, *g_wsum, *g_eik_num, *g_smooth_vec, *g_z_cross;
    const float* weights;      /* forward output */
    const int32_t* cross_idx;  /* forward output */
    const float* smooth_vec;   /* forward output */
    float *g_sdf, *g_grad, *g_col, *g_smooth, *g_inv_s;
    /* cotangents of the per-batch scalars of gens_composite_finish_fwd (DEVICE scalars or NULL) and its `finish` output */
    const float *g_gradient_error, *g_smooth_error, *finish;
} gens_composite_grad;

int gens_composite_fwd(const gens_composite_in* in, const gens_composite_out* out, void* stream);
int gens_composite_bwd(const gens_composite_in* in, const gens_composite_grad* g, void* stream);
/* The per-batch reductions around the compositing of a training step, one workgroup each (implicit_surface.py:248-253, 206):
 *   finish_fwd: finish (4) = {sum eik_num, sum eik_den, gradient_error = sum eik_num / (sum eik_den + 1e-5), smooth_error = mean |smooth_vec|}
 *     (smooth_vec may be NULL).  Their cotangents go into gens_composite_grad.g_gradient_error / g_smooth_error.
 *   finish_bwd: g_variance (1) = 10 inv_s [inside the clip range] sum_r g_inv_s[r] with scalars = gens_compact_points' {z_max, inv_s,
 *     1 / inv_s, in range}; rows [n_ray_pts, n_all) of the dense gradient arrays g_sdf (n_all), g_grad / g_smooth (n_all, 3) are zeroed
 *     (any of the four outputs may be NULL). */
int gens_composite_finish_fwd(const float* eik_num, const float* eik_den, const float* smooth_vec, int64_t n_rays, float* finish, void* stream);
int gens_composite_finish_bwd(const float* g_inv_s, int64_t n_rays, const float* scalars, float* g_variance, float* g_sdf, float* g_grad,
                              float* g_smooth, int64_t n_ray_pts, int64_t n_all, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K6  SDFNetwork.forward(...)[:, :1] and its first derivative, inference only   (sdf_network.py:98-146)
 *   One launch = volume look-up (K2, packed volumes) + both positional encodings + 7 layers on the fp32 matrix
 *   cores (+ reverse-mode d sdf/d x when grad_out != NULL).  Architecture: d_hidden 128, n_layers 6, skip_in [3],
 *   multires 4, feat_multires 2, Softplus(beta=100); n_levels must be 3 or 5 (feat_channels 12 / 20).
 *   wf / wb: HOST arrays of 6 device pointers: forward / transposed weights as grouped MFMA B streams
 *   [n_tile][ceil(K/8)][64 lanes][4] (lane l of group g holds W[32 n_tile + (l & 31)][8 g + 4 (l >> 5) + 0..3]), built by
 *   gens_amd.ops.SdfMlpPlan.  The bias of layer l is row K_l of the forward stream (K_0 = 27, else 128 + 20 n_levels):
 *   the kernel feeds a constant-1 input in that (padding) column.  w_last (128 + 5*4*n_levels) = row 0 of lin6.
 *   index: optional (N) int64 gather/scatter map: point i is pts[index[i]] and results go to sdf_out[index[i]],
 *   grad_out[3*index[i]..] (the masked evaluation of implicit_surface.py:125,179-191); NULL = identity.
 *   n_device: optional DEVICE int32: the number of points actually evaluated is min(n, *n_device) (written by
 *   gens_compact_valid), so the masked evaluation needs no host synchronisation; NULL = n.
 *   w_last_scaled: NULL, or the PRE-SCALED convention of the forward streams (saves the two multiplications of every softplus):
 *   with c = 100 / ln 2, wf[l] then holds W_l with the columns fed by unscaled inputs (point encoding incl. layer 3's 27 skip columns,
 *   volume-feature columns) and the bias row multiplied by c, the columns fed by hidden units as they are; w_last_scaled = w_last with
 *   its first 128 entries divided by c.  wb / w_last (reverse pass) are always the plain weights.  gens_amd.ops.SdfMlpPlan builds both.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_sdf_mlp(const float* const* vols_packed, const int* dims, int n_levels, const float* const* wf,
                 const float* const* wb, const float* w_last, const float* w_last_scaled, float b_last, float scale,
                 const float* pts, const int64_t* index, int64_t n, const int32_t* n_device, float* sdf_out, float* grad_out,
                 void* stream);

/* gens_sdf_mlp with the output bias read from DEVICE memory (training: the weights change every step and the streams come from
 * gens_sdf_train_pack; a by-value bias would cost a device-to-host read per step). */
int gens_sdf_mlp_dev(const float* const* vols_packed, const int* dims, int n_levels, const float* const* wf,
                     const float* const* wb, const float* w_last, const float* b_last_dev, float scale,
                     const float* pts, const int64_t* index, int64_t n, const int32_t* n_device, float* sdf_out, float* grad_out,
                     void* stream);

/* The VALUE of the same network (grad_out == NULL of gens_sdf_mlp), same exact float32 MFMA arithmetic, laid out for the value-only
 * passes (k6t_sdf_value.hip): the hierarchical sampling of implicit_surface.py:125,329-352 and the lattice of :407-427.  A wavefront owns
 * 32 points and all 128 hidden units; the activated accumulators are the next layer's matrix operands (the weights are packed in the
 * order the accumulators come out in), so nothing goes through LDS and there are no barriers.
 *   wstream: DEVICE, 16-byte aligned, (gens_sdf_value_groups(n_levels) + 1) x 4 KB: per group of four feature pairs
 *   [4 output tiles][64 lanes][4 floats] in the pair order of gens_amd.ops._value_pairs, pre-scaled as gens_sdf_mlp's w_last_scaled
 *   convention; the trailing group is zero (read ahead, never used).
 *   w_out: DEVICE (2, 64 + 4 * GC) float32: row 0 of lin6 in the accumulator / slot order of each lane half (hidden part / (100/ln 2)). */
int gens_sdf_value(const float* const* vols_packed, const int* dims, int n_levels, const float* wstream, const float* w_out,
                   float b_last, float scale, const float* pts, const int64_t* index, int64_t n, const int32_t* n_device,
                   float* sdf_out, void* stream);
/* number of 4 KB groups in the weight stream of gens_sdf_value, without the trailing zero group (125 for 3 levels, 0 = unsupported) */
int gens_sdf_value_groups(int n_levels);

/* Value and gradient (gens_sdf_mlp with grad_out) in the transposed dataflow of gens_sdf_value (k6g_sdf_grad.hip): one wavefront per 32
 * points runs the forward chain and the reverse chain G_{l-1} = (W_l^T G_l) * softplus' entirely in registers (softplus' of layers 0 and 1
 * waits in LDS); the gradients of the volume features and of the point encoding accumulate in tiles whose rows are ordered per lane, so
 * the chain rule to x is lane-local.  Three or five volume levels.
 *   wstream: DEVICE, 16-byte aligned, (gens_sdf_grad_groups(n_levels) + 2) x 4 KB in the order of gens_amd.ops._pack_grad_stream: the
 *   forward groups of gens_sdf_value, then the reverse pass on the plain transposed matrices; the two trailing groups are zero
 *   (the kernel requests weights two groups ahead).
 *   w_out: DEVICE (2, 64 + 16 * TC) float32: row 0 of lin6 per lane half (hidden part / (100 / ln 2), then the conditioning slots).
 *   stash: DEVICE, 16-byte aligned, gens_sdf_grad_stash_bytes() bytes, ZEROED ONCE by the caller and then left alone (it may be shared by all
 *   calls on a device, concurrent ones included): a 16 KB slot + lock word per SIMD where softplus' of layer 2 waits for the reverse pass. */
int gens_sdf_grad(const float* const* vols_packed, const int* dims, int n_levels, const float* wstream, const float* w_out,
                  float b_last, float scale, const float* pts, const int64_t* index, int64_t n, const int32_t* n_device,
                  float* sdf_out, float* grad_out, void* stash, void* stream);
int64_t gens_sdf_grad_stash_bytes(void);
/* Re-zero the stash (its lock words) on `stream`: after a launch that died holding a slot -- a wave that finds its slot taken waits a
 * bounded time (seconds) and then traps, so that the host sees a failed launch instead of a hang. */
int gens_sdf_grad_stash_reset(void* stash, void* stream);
/* number of 4 KB groups in the weight stream of gens_sdf_grad, without the trailing zero groups (0 = unsupported level count) */
int gens_sdf_grad_groups(int n_levels);

/* The VALUE of the same network (no gradient) on the f16 matrix cores with SPLIT operands -- every float32 operand an (hi, lo) pair of halfs,
 * every product hi*hi + hi*lo + lo*hi with float32 accumulation (~1e-6 relative error); overflow_flag: DEVICE int, OR-ed with 1 when an
 * activation or volume feature leaves the half range (the caller then redoes the batch with gens_sdf_value) -- laid out for throughput
 * (k6v_sdf_value_f16.hip): the 512^3 lattice of extract_geometry (implicit_surface.py:407-427) and the value-only passes of the opt-in
 * "f16x2" arithmetic.  A wavefront owns 32 points and all 128 hidden units; activations stay in registers between the layers because
 * the weights are packed in the order the accumulators come out in; one weight stream per 128 points goes through LDS.
 *   units: DEVICE, 16-byte aligned, gens_sdf_value_f16_units(n_levels) x 8192 bytes: per 16-deep K block of the six layers
 *   [4 feature tiles][hi, lo][64 lanes][8 halfs] in the slot order of gens_amd.ops._value_slots, pre-scaled by 100 / ln 2 on the
 *   columns fed by unscaled inputs, zero padded to whole chunks of four blocks.
 *   w_out: DEVICE (2, 64 + 8 * NC) float32: row 0 of lin6 in the accumulator / slot order of each lane half. */
int gens_sdf_value_f16(const float* const* vols_packed, const int* dims, int n_levels, const void* units, const float* w_out,
                       float b_last, float scale, const float* pts, const int64_t* index, int64_t n, const int32_t* n_device,
                       float* sdf_out, int* overflow_flag, void* stream);
/* number of 8 KB K blocks in the weight stream of gens_sdf_value_f16 (64 for 3 levels, 80 for 5; 0 = unsupported level count) */
int gens_sdf_value_f16_units(int n_levels);

/* Value AND gradient with SPLIT operands on the f16 matrix cores (k6gh_sdf_grad_f16.hip): gens_sdf_grad's dataflow and outputs,
 * gens_sdf_value_f16's arithmetic contract (hi*hi + hi*lo + lo*hi, float32 accumulation, softplus' kept in float32) -- the value +
 * gradient pass of render_core (implicit_surface.py:179-191 -> sdf_network.py:98-154) under the opt-in "f16x2" arithmetic.  Three or
 * five volume levels (BASELINE config[1] / confs/gens.conf:63-67); GENS_ELIMIT otherwise.
 *   pieces: DEVICE, 16-byte aligned, gens_sdf_grad_f16_pieces(n_levels) x 1024 bytes in the order of gens_amd.ops._pack_grad_pieces:
 *   [64 lanes][8 halfs] per (K block, output tile, hi | lo).
 *   w_out: the output row of gens_sdf_grad (same layout).   g_scale: a power of two the gradients travel multiplied by (lo parts stay
 *   normal halfs); the result is divided by it.
 *   stash: DEVICE, 16-byte aligned, gens_sdf_grad_f16_stash_bytes() bytes, ZEROED ONCE by the caller and then left alone.
 *   overflow_flag: DEVICE int, OR-ed with 1 when an input, a hidden unit or a gradient leaves the half range or is not a number: the
 *   caller redoes the batch with gens_sdf_grad. */
int gens_sdf_grad_f16(const float* const* vols_packed, const int* dims, int n_levels, const void* pieces, const float* w_out,
                      float b_last, float scale, float g_scale, const float* pts, const int64_t* index, int64_t n,
                      const int32_t* n_device, float* sdf_out, float* grad_out, void* stash, int* overflow_flag, void* stream);
int64_t gens_sdf_grad_f16_stash_bytes(void);
int gens_sdf_grad_f16_stash_reset(void* stash, void* stream);      /* as gens_sdf_grad_stash_reset */
/* number of 1 KB pieces in the weight stream of gens_sdf_grad_f16, padding included (0 = unsupported level count) */
int gens_sdf_grad_f16_pieces(int n_levels);

/* The same network with float32-accurate products on the bf16 matrix cores (k6b_sdf_bf16x3.hip): every float32 operand is split into
 * THREE round-to-nearest bfloat16 terms x0 + x1 + x2 and a product is x2 y0 + x1 y1 + x0 y2 + x1 y0 + x0 y1 + x0 y0 with float32
 * accumulation (the dropped terms are below ~2^-26 relative); bfloat16 has float32's exponent range, so there is no overflow flag.  The
 * dataflow of gens_sdf_grad_f16.  Three or five volume levels; GENS_ELIMIT otherwise.  gens_sdf_value_bf16x3 runs the forward half of
 * gens_sdf_grad_bf16x3: every accumulator receives the same products in the same order, so the two return the same float32 sdf for the
 * same point.
 *   pieces: DEVICE, 16-byte aligned, 1024-byte pieces in the order of gens_amd.ops._pack_grad_pieces(terms=3, hid3=layout[2]):
 *   [64 lanes][8 bfloat16] per (K block, output tile, x0 | x1 | x2).  gens_sdf_grad_bf16x3: gens_sdf_bf16x3_pieces(n_levels) of them.
 *   gens_sdf_value_bf16x3: the gradient kernel's stream, of which it reads the forward prefix; where gens_sdf_bf16x3_layout says tile-major
 *   (a development build of the three-level kernel), the value-only stream order="tile" of layout[0] pieces, [tile][block][term] in a layer.
 *   w_out: the output row of gens_sdf_grad (same layout).
 *   stash: gens_sdf_grad_f16's (gens_sdf_grad_f16_stash_bytes() bytes, zeroed once; the same buffer may serve both kernels). */
int gens_sdf_value_bf16x3(const float* const* vols_packed, const int* dims, int n_levels, const void* pieces, const float* w_out,
                          float b_last, float scale, const float* pts, const int64_t* index, int64_t n, const int32_t* n_device,
                          float* sdf_out, void* stream);
int gens_sdf_grad_bf16x3(const float* const* vols_packed, const int* dims, int n_levels, const void* pieces, const float* w_out,
                         float b_last, float scale, const float* pts, const int64_t* index, int64_t n, const int32_t* n_device,
                         float* sdf_out, float* grad_out, void* stash, void* stream);
/* number of 1 KB pieces in the weight stream of gens_sdf_value_bf16x3 / gens_sdf_grad_bf16x3, padding included (0 = unsupported level count) */
int gens_sdf_bf16x3_pieces(int n_levels);
/* how this build's kernels walk the stream: out[0] pieces of the forward half, padding included (what gens_sdf_value_bf16x3 reads), out[1] 1 if
 * gens_sdf_value_bf16x3 takes the tile-major value-only stream at this level count, 0 if the forward prefix of the gradient kernel's stream,
 * out[2] hidden K blocks of forward layer 3 (7 at three levels, 8 at five).  out: HOST, 3 ints. */
int gens_sdf_bf16x3_layout(int n_levels, int out[3]);
/* residency of one instantiation (grad: 0 = gens_sdf_value_bf16x3's kernel, 1 = gens_sdf_grad_bf16x3's) on the current device, at the launcher's
 * block and LDS sizes: out[0] registers per lane (hipFuncAttributes.numRegs), out[1] scratch bytes per lane (localSizeBytes), out[2] dynamic LDS
 * bytes of a launch, out[3] resident workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor).  out: HOST, 4 ints. */
int gens_sdf_bf16x3_residency(int n_levels, int grad, int out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * K21  depth-wise 2-D convolutions of the MnasNet trunk (k21_depthwise.hip): nn.Conv2d(c, c, k, padding = k / 2, stride, groups = c,
 *      bias = False) with k in {3, 5}, stride in {1, 2} -- torchvision's MNASNet layers used by feature_network_mnasnet.py:53-103 -- for which
 *      MIOpen falls back to its naive kernels on gfx950.  NCHW float32, contiguous.
 *   in (n, c, h, w), weight (c, 1, k, k), out / grad_out (n, c, oh, ow) with oh = (h + 2 (k / 2) - k) / stride + 1 (ow likewise).
 *   wgrad: partial (gens_depthwise_conv2d_wgrad_parts(...), c, k, k) receives per-slice sums; the weight gradient is their sum over axis 0
 *   in slice order (deterministic).  Other kernel sizes / strides: GENS_ELIMIT (the caller keeps its own convolution for those).
 * ---------------------------------------------------------------------------------------------------------- */
int gens_depthwise_conv2d_fwd(const float* in, const float* weight, int n, int c, int h, int w, int k, int stride, float* out, void* stream);
int gens_depthwise_conv2d_dgrad(const float* grad_out, const float* weight, int n, int c, int h, int w, int k, int stride, float* grad_in,
                                void* stream);
int gens_depthwise_conv2d_wgrad_parts(int n, int c, int h, int w, int k, int stride);
int gens_depthwise_conv2d_wgrad(const float* in, const float* grad_out, int n, int c, int h, int w, int k, int stride, float* partial,
                                void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K22  BatchNorm2d in training mode (batch statistics) [+ the ReLU that follows it] of the MnasNet trunk (k22_batchnorm.hip): the
 *      nn.BatchNorm2d(c, momentum = 1 - 0.9997) [+ nn.ReLU] pairs of torchvision's MNASNet used by feature_network_mnasnet.py:53-103.
 *      NCHW float32 contiguous, x / y / grad_* (n, c, hw).  gamma / beta (c) or NULL (no affine).
 *   fwd: y = [max](((x - mean_c) * rstd_c) * gamma_c + beta_c[, 0]) with the batch's mean and BIASED variance; mean_rstd (c, 2) receives
 *        (mean, rstd) for the backward pass; running_mean / running_var (c) or NULL are moved by `momentum` (running_var with the unbiased
 *        variance), num_batches_tracked (DEVICE int64 or NULL) is incremented -- nn.BatchNorm2d's bookkeeping.
 *   bwd: grad_x (or NULL), grad_gamma, grad_beta (c, or NULL) from grad_y; relu: the decision y > 0 is recomputed from x.
 *   scratch: DEVICE, gens_batchnorm2d_scratch_doubles(n, c, hw) doubles, contents irrelevant before and after.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t gens_batchnorm2d_scratch_doubles(int n, int c, int hw);
int gens_batchnorm2d_train_fwd(const float* x, const float* gamma, const float* beta, int n, int c, int hw, float eps, float momentum, int relu,
                               float* y, float* mean_rstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                               double* scratch, void* stream);
int gens_batchnorm2d_train_bwd(const float* x, const float* grad_y, const float* mean_rstd, const float* gamma, const float* beta, int n, int c,
                               int hw, int relu, float* grad_x, float* grad_gamma, float* grad_beta, double* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K20  the reference's sampler boundary in full generality (k20_grid_sample.hip): what cuda_gridsample.py:7-14 exports and K2 does not
 *      cover -- grid_sample_2d, padding_mode 'border', align_corners=False, batches, channel counts that are not multiples of four.
 *     forward            F.grid_sample(bilinear) = aten::grid_sampler_2d / _3d        (cuda_gridsample.py:28, 79)
 *     backward           aten::grid_sampler_2d_backward / _3d_backward                 (cuda_gridsample.py:38-50, 94-108)
 *     backward-backward  gridsample_grad2.grad2_2d / grad2_3d                          (gridsample_cuda.cpp:26-56, gridsample_cuda.cu:27-533)
 *   ndim      2 or 3;  in_size HOST int[ndim]: the input's spatial shape, slowest axis first ((H, W) or (D, H, W))
 *   input     (n, c, *in_size) contiguous float32 (the reference's NCHW / NCDHW);  grid (n, n_out, ndim), last axis (x, y[, z]) -> (W, H[, D])
 *   out / grad_out / gg_out  (n, c, n_out);  grad_grid / gg_grid (n, n_out, ndim)
 *   padding_mode  0 = 'zeros', 1 = 'border' (the two the reference asserts, cuda_gridsample.py:8,13; it passes the index, :32,83)
 *   grad_input    like input, ACCUMULATES (float atomics): zero it first, as the reference does (gridsample_cuda.cu:553-555, 620-622); NULL = not
 *                 wanted (bwd) / the reference's unused output (bwd2).  gg_input: like input or NULL (`grad2_grad_input is None`, :113-114).
 * ---------------------------------------------------------------------------------------------------------- */
int gens_grid_sample_fwd(const float* input, const float* grid, int ndim, int n, int c, const int* in_size, int64_t n_out,
                         int padding_mode, int align_corners, float* out, void* stream);
int gens_grid_sample_bwd(const float* grad_out, const float* input, const float* grid, int ndim, int n, int c, const int* in_size,
                         int64_t n_out, int padding_mode, int align_corners, float* grad_input, float* grad_grid, void* stream);
int gens_grid_sample_bwd2(const float* gg_input, const float* gg_grid, const float* grad_out, const float* input, const float* grid,
                          int ndim, int n, int c, const int* in_size, int64_t n_out, int padding_mode, int align_corners,
                          float* gg_out, float* grad_input, float* grad_grid, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K17  the SDF network of a training / fine-tune step: value, gradient, `smooth` vector and the loss backward
 *      (sdf_network.py:98-154: SDFNetwork.sdf, SDFNetwork.gradient with create_graph twice; their autograd backward under
 *      loss.backward(); call sites implicit_surface.py:179-191,257,305,490; sampler Function pair cuda_gridsample.py:71-123,
 *      whose second-backward outputs are constants in the loss backward: third order through the sampler is dropped)
 *   Architecture and n_levels as gens_sdf_mlp, scale = 1 (confs/gens.conf:78).  All buffers are caller-allocated device memory.
 *   gens_sdf_train_pack: w[0..5] / b[0..5]: HOST arrays of device pointers to the EFFECTIVE (weight norm applied) row-major
 *     matrices (128 x 27, 128 x K, 101 x K, 128 x K x 3; K = 128 + 20 n_levels) and biases of lin0..lin5; writes the forward /
 *     transposed B streams wf[l] ([4][ceil((K_l + 1) / 8)][64] float4, bias in reduction row K_l) and wb[l] ([ceil(K_l / 32)][16][64]
 *     float4) that the other entry points (and gens_sdf_mlp) read.
 *   index / n / n_device (all three entry points) as in gens_sdf_mlp: point i of the launch is pts[index[i]] and its results (cotangents)
 *     live at row index[i] of the dense arrays; only min(n, *n_device) points exist -- the masked evaluation of
 *     implicit_surface.py:174-191 with the count left on the device (gens_compact_points).  NULL index = identity, NULL n_device = n.
 *   gens_sdf_train_fwd: pts -> y (N), g (N, 3) = dy/dx, s (N, 3) = d(sum_k g_k)/dx, written at index[i].  w_last: row 0 of lin6 (K
 *     floats), b_last: DEVICE pointer to its bias.  stash: scratch of gens_sdf_train_stash_bytes(n, 0) bytes.
 *   gens_sdf_train_bwd: cotangents y_bar (N), g_bar (N, 3), s_bar (N, 3) (NULL = zero; read at index[i]) -> operand rows of the
 *     weight-gradient products, POINT-major: npad = 32 ceil(n / 32) points x 4 sweeps, the rows of the live points being the
 *     contiguous range [0, 4 * 32 ceil(n_live / 32)) (rows of padding points inside it contribute zero, rows beyond it are NOT written:
 *     pass the count to gens_gemm_tn_batch_live):
 *       lop (npad, 4, 6, 128), rh (5, npad, 4, 128), re (npad, 4, KP - 128), r0 (npad, 4, 32), KP = 8 ceil((K + 1) / 8):
 *       dL/dW_l[:, :128]  = lop[:, :, l, :]^T rh[l - 1]                  (l = 1..5; layer 3's columns are [h_2 | pe] / sqrt 2)
 *       dL/dW_l[:, 128:K] , dL/db_l = lop[:, :, l, :]^T re               (column K - 128 of re is the bias input)
 *       dL/dW_0, dL/db_0  = lop[:, :, 0, :]^T r0                         (column 27 = bias input)
 *       dL/dw_last, dL/db_last = column sums of w6_part (npad / 16, KP): columns [0, K) and column K (zero rows for dead workgroups)
 *     (gens_gemm_tn_batch runs the products in one launch) and f_hat, mu_f, lam_f (npad, 4 n_levels) for
 *     gens_sdf_train_scatter.  stash: gens_sdf_train_stash_bytes(n, 1) bytes.
 *   gens_sdf_train_scatter: adds dL/dvolume into g_vols[l] (planar (4, X, Y, Z), pre-zeroed or accumulating):
 *       w f_hat + (grad w . s_bar) mu_f + (grad w . g_bar) lam_f per corner  (float atomics).
 * ---------------------------------------------------------------------------------------------------------- */
/*   gens_sdf_train_pack_wn: gens_sdf_train_pack from the RAW weight-normed parameters (nn.utils.weight_norm, sdf_network.py:90-91:
 *     W = g v / |v| per output row): v / g / b = HOST arrays of the 7 device pointers weight_v (rows_l, cols_l), weight_g (rows_l), bias
 *     (rows_l) of lin0..lin6; scale: 7 caller-allocated arrays of rows_l floats (g / |v|, kept for the backward); also writes the effective
 *     output row w_last (K floats) and its bias b_last (1).  Two launches.
 *   gens_sdf_train_wgrad: the parameter gradients of a step in one launch -- cc = gens_gemm_tn_batch's result for the eleven products in
 *     the order (l = 1..5: [lop_l^T rh_l (128 x 128) | lop_l^T re (128 x KP - 128)], then lop_0^T r0 (128 x 32)), w6_sum (KP) = the column
 *     sums of w6_part -> dv[l] (rows_l, cols_l), dg[l] (rows_l), db[l] (rows_l) for lin0..lin6, weight norm's backward included. */
int gens_sdf_train_pack_wn(const float* const* v, const float* const* g, const float* const* b, int n_levels, float* const* scale,
                           float* const* wf, float* const* wb, float* w_last, float* b_last, void* stream);
int gens_sdf_train_wgrad(const float* const* v, const float* const* g, int n_levels, const float* cc, const float* w6_sum,
                         float* const* dv, float* const* dg, float* const* db, void* stream);
int64_t gens_sdf_train_stash_bytes(int64_t n, int backward);
int gens_sdf_train_pack(const float* const* w, const float* const* b, int n_levels, float* const* wf, float* const* wb, void* stream);
int gens_sdf_train_fwd(const float* const* vols_packed, const int* dims, int n_levels, const float* const* wf,
                       const float* const* wb, const float* w_last, const float* b_last, const float* pts, const int64_t* index,
                       int64_t n, const int32_t* n_device, void* stash, float* y_out, float* g_out, float* s_out, void* stream);
int gens_sdf_train_bwd(const float* const* vols_packed, const int* dims, int n_levels, const float* const* wf,
                       const float* const* wb, const float* w_last, const float* pts, const int64_t* index, int64_t n,
                       const int32_t* n_device, const float* y_bar, const float* g_bar, const float* s_bar, void* stash, float* lop,
                       float* rh, float* re, float* r0, float* f_hat, float* mu_f, float* lam_f, float* w6_part, void* stream);
int gens_sdf_train_scatter(const int* dims, int n_levels, const float* pts, const float* g_bar, const float* s_bar,
                           const float* f_hat, const float* mu_f, const float* lam_f, const int64_t* index, int64_t n,
                           const int32_t* n_device, float* const* g_vols, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K7  lookup_feature + BlendingNetwork.forward fused, inference only
 *     (projector.py:278-349 followed by blending_network.py:69-118, as called from implicit_surface.py:196-199)
 *   feats / hw / imgs / w2c / intr / c2w / nv as in gens_lookup_feature_fwd (n_levels <= 5).
 *   weights: HOST array of 21 device pointers in the order
 *     ray_dir_fc.0 W,b  ray_dir_fc.2 W,b  base_fc.0 W,b  base_fc.2 W,b  vis_fc.0 W,b  vis_fc.2 W[0:32],b[0:32]  vis_fc.2 W[32]
 *     vis_fc2.0 W,b  vis_fc2.2 W  rgb_fc.0 W,b  rgb_fc.2 W,b  rgb_fc.4 W
 *   (matrices as grouped MFMA B streams -- the layout documented at gens_sdf_mlp, K padded to a multiple of 8 --
 *   biases zero-padded to a multiple of 32; gens_amd.ops.BlendPlan builds them);
 *   scalars: HOST float[4] = { vis_fc.2 bias[32], vis_fc2.2 bias, rgb_fc.4 bias, |s| }.
 *   index as in gens_sdf_mlp.  rgb_out (N_total, 3); vis_out (N_total, S) uint8 or NULL, written at index[i].
 * ---------------------------------------------------------------------------------------------------------- */
int gens_blend_views(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c,
                     const float* intr, const float* c2w, int nv, const float* const* weights, const float* scalars,
                     const float* pts, const int64_t* index, int64_t n, const int32_t* n_device, float* rgb_out, uint8_t* vis_out,
                     void* stream);

/* gens_blend_views for TWO, THREE or FOUR source views (nv = 3, 4, 5: the view counts of the shipped configurations -- num_src_view = 2
 * in the test protocol and the fine-tune configs, confs/gens.conf:24, confs/gens_finetune.conf:15; 4 in training, confs/gens.conf:9) in
 * the transposed dataflow of gens_sdf_value (k7t_blend.hip): one wavefront owns 64 (point, view) rows (three views: 48 + 16 dead rows),
 * the weights are the A operand of v_mfma_f32_16x16x4_f32, the activations of the eleven layers stay in registers in "quad layout", the
 * mean / variance columns of base_fc.0 are multiplied once per point.
 * Same inputs and outputs as gens_blend_views except the weights (the same stream for every view count):
 *   wstream: DEVICE, 16-byte aligned, (gens_blend_views_t_groups(n_levels) + 2) x 1 KB: A fragments in consumption order
 *   (gens_amd.ops._pack_blend_t), the two trailing groups zero;  tab: DEVICE (10, 4, 8) float32: accumulator-layout biases and the
 *   three single-output rows per lane group;  scalars: HOST float[4] as gens_blend_views.
 * gens_blend_views4 / gens_blend_views4_groups: the ABI-4 names (nv = 5 only). */
int gens_blend_views_t(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                       const float* c2w, int nv, const float* wstream, const float* tab, const float* scalars, const float* pts,
                       const int64_t* index, int64_t n, const int32_t* n_device, float* rgb_out, uint8_t* vis_out, void* stream);
int gens_blend_views_t_groups(int n_levels);
/* gens_blend_pack_t: wstream / tab / the four scalars of gens_blend_views_t from the 23 RAW nn.Linear parameters of a BlendingNetwork
 * (HOST array of device pointers in the order of gens_blend_train_fwd), in one launch; scalars_dev: DEVICE float[4].
 * gens_blend_views_t_dev: gens_blend_views_t with those scalars read from device memory -- the forward pass of a TRAINING step, whose
 * colour network changes every step (gens_blend_train_bwd recomputes what it needs). */
int gens_blend_pack_t(const float* const* weights, int n_levels, float* wstream, float* tab, float* scalars_dev, void* stream);
int gens_blend_views_t_dev(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                           const float* c2w, int nv, const float* wstream, const float* tab, const float* scalars_dev, const float* pts,
                           const int64_t* index, int64_t n, const int32_t* n_device, float* rgb_out, uint8_t* vis_out, void* stream);
int gens_blend_views4(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                      const float* c2w, int nv, const float* wstream, const float* tab, const float* scalars, const float* pts,
                      const int64_t* index, int64_t n, const int32_t* n_device, float* rgb_out, uint8_t* vis_out, void* stream);
int gens_blend_views4_groups(int n_levels);

/* gens_blend_views_t with its large products on the bf16 matrix pipe, float32-accurate (k7b_blend_bf16x3.hip): every float32 operand
 * is three round-to-nearest bf16 terms, a product the six significant cross terms on v_mfma_f32_16x16x32_bf16 with float32
 * accumulation; the products with K <= 16 stay on v_mfma_f32_16x16x4_f32.  Same arguments, outputs and limits as gens_blend_views_t
 * (nv = 3..5, n_levels <= 5) except the stream:
 *   wstream: DEVICE, 16-byte aligned, (gens_blend_bf16x3_groups(n_levels) + 2) x 3 KB: groups of three 1 KB pieces in consumption
 *   order (gens_amd.ops._pack_blend_b) -- the three bf16 planes of one (M tile, K block of 32), or float32 fragments in
 *   gens_blend_views_t's layout (first and last group) -- the two trailing groups zero;  tab, scalars: gens_blend_views_t's. */
int gens_blend_views_bf16x3(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                            const float* c2w, int nv, const void* wstream, const float* tab, const float* scalars, const float* pts,
                            const int64_t* index, int64_t n, const int32_t* n_device, float* rgb_out, uint8_t* vis_out, void* stream);
int gens_blend_bf16x3_groups(int n_levels);
/* residency of gens_blend_views_bf16x3's kernel for n_levels (1..5) and nv (3..5) on the current device, at the launcher's block size (one
 * wave): out[0] registers per lane (hipFuncAttributes.numRegs), out[1] scratch bytes per lane (localSizeBytes), out[2] static LDS bytes of a
 * workgroup (sharedSizeBytes), out[3] resident workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor).  out: HOST, 4 ints. */
int gens_blend_bf16x3_residency(int n_levels, int nv, int out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * K18  lookup_feature + BlendingNetwork.forward of a training / fine-tune step, and their backward
 *      (projector.py:278-349, blending_network.py:69-118 as called from implicit_surface.py:196-199; first order only)
 *   feats / hw / imgs / w2c / intr / c2w / nv as in gens_lookup_feature_fwd (n_levels <= 5).
 *   weights: HOST array of 23 device pointers to the RAW nn.Linear parameters (row major (out, in)) in the order
 *     ray_dir_fc.0 W,b  ray_dir_fc.2 W,b  base_fc.0 W,b  base_fc.2 W,b  vis_fc.0 W,b  vis_fc.2 W,b  vis_fc2.0 W,b  vis_fc2.2 W,b
 *     rgb_fc.0 W,b  rgb_fc.2 W,b  rgb_fc.4 W,b  s
 *   index / n / n_device as in gens_sdf_mlp: point i of the launch is pts[index[i]], its colour / flags / cotangent live at row index[i]
 *     of the dense arrays, only min(n, *n_device) points exist (NULL index = identity, NULL n_device = n).
 *   fwd: pts -> rgb_out (N, 3), vis_out (N, S) uint8 (NULL to skip), written at index[i].
 *   bwd: g_rgb (N, 3) cotangent of rgb_out -> for each of the 11 layers the operand rows of its weight-gradient product over
 *     rows = gens_blend_train_rows(n, nv) = 32 ceil(n / floor(32 / S)) (under a device-side count only the rows of the first
 *     ceil(n_live / floor(32 / S)) workgroups are written: gens_gemm_tn_batch_live):  r_ops[l] (rows, even(in_l + 1)) = [layer input | 1 | 0],
 *     l_ops[l] (rows, even(out_l)) = cotangent of the pre-activation (zero padded; even(x) = x rounded up to a multiple of 2):
 *     [dW_l | db_l] = the leading out_l x (in_l + 1) block of l_ops[l]^T r_ops[l]   (gens_gemm_tn_batch);
 *     g_feat (n, S, 3 + 4 n_levels), COMPACT (row i = point i of the launch): cotangent of the looked-up rows for
 *     gens_lookup_feature_bwd[_idx] (NULL to skip);  s_part (rows / 32): partial sums of d loss / d |s| (zero for dead workgroups).
 * ---------------------------------------------------------------------------------------------------------- */
int64_t gens_blend_train_rows(int64_t n, int nv);
int gens_blend_train_fwd(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                         const float* c2w, int nv, const float* const* weights, const float* pts, const int64_t* index, int64_t n,
                         const int32_t* n_device, float* rgb_out, uint8_t* vis_out, void* stream);
int gens_blend_train_bwd(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                         const float* c2w, int nv, const float* const* weights, const float* pts, const int64_t* index, int64_t n,
                         const int32_t* n_device, const float* g_rgb, float* const* r_ops, float* const* l_ops, float* g_feat,
                         float* s_part, void* stream);
/* The same backward with the weight-gradient sums INSIDE the launch (round 4): persistent workgroups -- gens_blend_train_acc_parts(n, nv) of them --
 * multiply L^T [R | 1] of their row tiles out of LDS on the matrix cores, the sums in registers, and leave one block of
 * gens_blend_train_acc_floats(n_levels) floats each in `parts` (parts x floats); `cc` (floats) = their sum in part order = the eleven blocks
 * even(out_l) x even(in_l + 1), concatenated, that gens_gemm_tn_batch returns for l_ops / r_ops above (the input of gens_blend_train_wgrad).  No
 * operand rows: 619 MB per launch neither written nor read again. */
int gens_blend_train_acc_parts(int64_t n, int nv);
int gens_blend_train_acc_floats(int n_levels);
int gens_blend_train_bwd_acc(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                             const float* c2w, int nv, const float* const* weights, const float* pts, const int64_t* index, int64_t n,
                             const int32_t* n_device, const float* g_rgb, float* g_feat, float* s_part, float* parts, float* cc, void* stream);
/* The same backward TRANSPOSED (round 6; two to four source views, nv = 3 .. 5 -- other counts: gens_blend_train_bwd_acc): a wave owns 16 (point,
 * view) rows and all of their forward, reverse and weight-gradient work -- the weights of the eleven layers in LDS as the A operand of
 * v_mfma_f32_16x16x4_f32, the activations in registers from layer to layer and, in [channel][row] order, in a wave-private LDS store the weight-
 * gradient products read both operands from; four independent waves per workgroup, one persistent workgroup per compute unit, no barrier behind the
 * weight load.  gens_blend_train_t_parts(n, nv) = the number of workgroups = blocks of gens_blend_train_acc_floats(n_levels) floats in `parts` AND
 * entries of s_part (one partial of d loss / d |s| per workgroup; 0 = nothing to launch or a view count this kernel is not built for); cc, g_feat as in
 * gens_blend_train_bwd_acc.  Results equal gens_blend_train_bwd_acc's up to float32 summation order.
 * gens_blend_train_bwd_t_dump additionally leaves the operand rows r_ops / l_ops of gens_blend_train_bwd (same widths) for
 * rows = 16 ceil(n / (16 / G)) rows, G = 2 (nv = 3) or 4 lanes per point: row 16 tile + G point + view (three source views: every fourth row is
 * empty) -- the two kernels compared layer by layer (tests). */
int gens_blend_train_t_parts(int64_t n, int nv);
int gens_blend_train_bwd_t(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                           const float* c2w, int nv, const float* const* weights, const float* pts, const int64_t* index, int64_t n,
                           const int32_t* n_device, const float* g_rgb, float* g_feat, float* s_part, float* parts, float* cc, void* stream);
int gens_blend_train_bwd_t_dump(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                                const float* c2w, int nv, const float* const* weights, const float* pts, const int64_t* index, int64_t n,
                                const int32_t* n_device, const float* g_rgb, float* g_feat, float* s_part, float* parts, float* cc,
                                float* const* r_ops, float* const* l_ops, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K9  the two F.grid_sample(align_corners=True) reads of surface_patch_warp   (projector.py:406-416)
 *   image (H, W, C_pad) texels of one view; xy (P, 2) PIXEL coordinates (the normalise/un-normalise pair of
 *   :404-405 and align_corners=True cancel); out (P, C).  bwd: g_out (P, C) -> g_xy (P, 2), overwritten.
 *   gens_upsample2d_into restates F.interpolate(mode="bilinear") (implicit_surface.py:316-325) writing channels
 *   [c_off, c_off+C) of a (n, H, W, C_pad_dst) texel tensor from src (n, C, hs, ws) NCHW.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_patch_sample_fwd(const float* image, int h, int w, int c, const float* xy, int64_t p, float* out,
                          void* stream);
int gens_patch_sample_bwd(const float* image, int h, int w, int c, const float* xy, const float* g_out, int64_t p,
                          float* g_xy, void* stream);
int gens_upsample2d_into(const float* src, int n, int c, int hs, int ws, float* dst, int h, int w, int c_pad_dst,
                         int c_off, void* stream);
/* ... and the whole cat([f0, up(f1), up(f2), ...], 1) of implicit_surface.py:313-326 in ONE launch (ABI 12): srcs[i] is map i, (n, C_i, hs_i, ws_i)
 * NCHW with chw[3 i .. 3 i + 2] = (C_i, hs_i, ws_i); every texel of dst (n, H, W, C_pad_dst) is written whole, its pad channels with zeros (no
 * fill beforehand); the values are gens_upsample2d_into's bit for bit. */
int gens_upsample2d_cat(const float* const* srcs, const int* chw, int n_maps, int n, float* dst, int h, int w, int c_pad_dst,
                        void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K13  compute_LNCC, the photometric patch statistic of the loss     (models/losses/ncc.py:7-55, loss.py:36)
 *   ref (1, B, P, C), src (S, B, P, C) contiguous float32 (render_core's ref_gray_val / sampled_gray_val; P = 121, C = 12);
 *   S * C <= 64.  ncc (B): mean over channels of clamp(1 - cc, 0, 2), mean of the two smallest source views;
 *   sel (B, 2) int32: the two selected source indices (consumed by the backward).
 *   bwd: g_ncc (B) -> g_ref like ref, g_src like src, both overwritten.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_lncc_fwd(const float* ref, const float* src, int64_t n_rays, int n_src, int n_patch, int n_ch, float* ncc, int32_t* sel,
                  void* stream);
int gens_lncc_bwd(const float* ref, const float* src, const float* g_ncc, const int32_t* sel, int64_t n_rays, int n_src, int n_patch,
                  int n_ch, float* g_ref, float* g_src, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K12  iso-surface extraction of the SDF lattice: replaces mcubes.marching_cubes(u, threshold)
 *      (implicit_surface.py:423; PyMCubes==0.1.4, requirements.txt:11 -- third-party, classic marching cubes)
 *   u (X, Y, Z) float32, z fastest (the lattice of implicit_surface.py:407-421); iso = threshold.
 *   gens_mc_classify: per lattice point p  vmask[p] bit a = the edge p -> p + e_a straddles iso (a = x, y, z),
 *     vcount[p] = popcount, cases[p] = Bourke case index of the cell with origin p (bit n: u[corner n] < iso),
 *     tcount[p] = tri_count[cases[p]] (0 where p is not a cell origin).  tri_count: DEVICE (256) uint8.
 *   The caller turns vcount / tcount into exclusive scans voff / toff (int32) and allocates
 *     vertices (V, 3) float64 in INDEX coordinates and triangles (T, 3) int32.
 *   gens_mc_emit: vertex of edge (p, a) = p + e_a (iso - u_p) / (u_q - u_p) in float64, stored at voff[p] + rank of a;
 *     triangles of cell p from tri_table (DEVICE (256, table_stride) int8 edge ids, -1 padded; gens_amd/mc_tables.py)
 *     at toff[p].  Order: vertices by (p, a), triangles by (p, table order).
 * ---------------------------------------------------------------------------------------------------------- */
int gens_mc_classify(const float* u, int x, int y, int z, float iso, const uint8_t* tri_count, uint8_t* vmask,
                     uint8_t* vcount, uint8_t* cases, uint8_t* tcount, void* stream);
int gens_mc_emit(const float* u, int x, int y, int z, float iso, const int8_t* tri_table, int table_stride,
                 const uint8_t* vmask, const int32_t* voff, const uint8_t* cases, const uint8_t* tcount, const int32_t* toff,
                 double* vertices, int32_t* triangles, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K10  tv_regularization, one level per call                      (implicit_surface.py:135-150)
 *   vol (4, X, Y, Z), mask (X, Y, Z); partial (n_blocks, 4) per-block sums [tx_num, ty_num, tz_num, mx_count]
 *   (n_blocks = gens_tv_blocks(x*y*z)); the host finishes sqrt((tx+ty+tz)/(count+1e-8)) * 0.5^level (Q13).
 * bwd: g_vol (4,X,Y,Z) = coef * d(tx_num+ty_num+tz_num)/d vol, overwritten; coef = g * 0.5^level / (2*tv*(count+1e-8)).
 * ---------------------------------------------------------------------------------------------------------- */
int gens_tv_blocks(int64_t n_voxels);
int gens_tv_fwd(const float* vol, const float* mask, int x, int y, int z, float* partial, void* stream);
int gens_tv_bwd(const float* vol, const float* mask, int x, int y, int z, float coef, float* g_vol, void* stream);
/* the same with the coefficient = coef * coef_dev[0], coef_dev a device scalar (the upstream gradient stays on the device: no host sync) */
int gens_tv_bwd_scaled(const float* vol, const float* mask, int x, int y, int z, float coef, const float* coef_dev, float* g_vol,
                       void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K11  the lattice of extract_geometry                            (implicit_surface.py:407-418)
 *   pts (count, 3): lattice points first .. first+count-1 of a res^3 grid in x-major order, coordinates equal to
 *   torch.linspace(bmin, bmax, res).
 * ---------------------------------------------------------------------------------------------------------- */
int gens_lattice_points(const float* bmin3_host, const float* bmax3_host, int res, int64_t first, int64_t count,
                        float* pts, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K23  the ray-cast half of the validation-mesh cleaning: replaces clean_mesh_outside_frustum (utils/clean_mesh.py:38-106),
 *      pyembree's intersects_first through trimesh and trimesh's face-adjacency components
 *   gens_mesh_grid (HOST struct, device pointers inside): a uniform grid of nx * ny * nz cubic cells of edge `cell` from (lo_x, lo_y, lo_z)
 *     over a triangle mesh; vertices (V, 3) float64, triangles (n_faces, 3) int32 (indices < V: the caller's check); cell_start
 *     (cells + 1) int32 = exclusive scan of gens_mesh_grid_count's counts; cell_faces (cell_start[cells]) int32 face ids, cell by cell.
 *     1 .. 512 cells per axis; the box must hold every vertex.
 *   gens_mesh_grid_count: counts (cells) int32, ACCUMULATES: per cell the faces whose closed AABB (widened by 1e-5 cells) overlaps it.
 *   gens_mesh_grid_fill: writes cell_faces (any order inside a cell); cursor (cells) int32 zero-filled scratch.
 *   gens_ray_first_hit: rays (n_rays, 3) float32 origins / directions -> face (n_rays) int32 (-1: miss) and t (n_rays) float32 (+inf: miss,
 *     in units of |d|): the lexicographically smallest (t, face) over the faces hit at t > 0 from either side, watertight (Woop, Benthin,
 *     Wald 2013, in float64).
 *   gens_view_rays_hit_faces: the rays of clean_mesh.py:50-66 for the hu x wu upsampled pixels of nv views (hu = int(h * upscale)),
 *     generated in the kernel; a pixel casts iff masks (nv, h, w) float32 at its nearest source pixel (F.interpolate's rule with
 *     inv_scale = (float)(1 / upscale)) is > 0.  cams (nv, 21) float32: K^-1[:3, :3] row-major, then c2w[:3, :4] row-major.
 *     flags (n_faces) uint8 and any_miss (1) int32 ACCUMULATE: 1 for every face some ray hits first, 1 if some cast ray misses.
 *   gens_face_cc_hook: union-find over pairs (n_pairs, 2) int32 face ids; parent (n_faces) int32 starts as 0 .. n_faces - 1 and is updated
 *     in place (larger roots hooked under smaller ones).  gens_face_cc_compress: label (n_faces) int32 = the root of every face = the
 *     smallest face index of its component.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const double* vertices;
    const int32_t* triangles;
    const int32_t* cell_start;
    int32_t* cell_faces;
    int64_t n_faces;
    float lo_x, lo_y, lo_z, cell;
    int nx, ny, nz;
} gens_mesh_grid;
int gens_mesh_grid_count(const gens_mesh_grid* grid, int32_t* counts, void* stream);
int gens_mesh_grid_fill(const gens_mesh_grid* grid, int32_t* cursor, void* stream);
int gens_ray_first_hit(const gens_mesh_grid* grid, const float* rays_o, const float* rays_d, int64_t n_rays, int32_t* face, float* t,
                       void* stream);
int gens_view_rays_hit_faces(const gens_mesh_grid* grid, const float* masks, const float* cams, int nv, int h, int w, int hu, int wu,
                             float inv_scale, uint8_t* flags, int32_t* any_miss, void* stream);
int gens_face_cc_hook(const int32_t* pairs, int64_t n_pairs, int32_t* parent, int64_t n_faces, void* stream);
int gens_face_cc_compress(const int32_t* parent, int64_t n_faces, int32_t* label, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K24  the three hot steps of the DTU scoring (evaluation/dtu_eval.py), all geometry in float64 as the script computes it.  Every new
 *      entry checks its arguments before any launch (null pointers, negative sizes, a radius / density / cap that is not positive:
 *      GENS_EINVAL).  The ABI version stays 12: no existing entry changes.
 *   gens_mesh_sample_count / _emit (dtu_eval.py:11-20, 61-78): vertices (n_vertices, 3) float64, triangles (n_triangles, 3) int32.
 *     count: counts (n_triangles) int64 = the lattice points of every triangle ((i + 0.5) / n1 + (j + 0.5) / n2 < 1 with the script's
 *     n1, n2; 0 for a triangle of zero area, with an index out of range, or with n1 or n2 = 0; 2^40 for a triangle with more than 2^20
 *     lattice steps along an edge, which emit skips -- the caller's total shows it).  emit: offsets (n_triangles) int64 = the exclusive
 *     scan of the counts, total = their sum (< 2^31); out (total, 3) float64, triangle by triangle, i major, j minor, each point
 *     (v1 k0 + v2 k1) + p0 in the script's operations.
 *   gens_point_grid (HOST struct, device pointers inside): nx * ny * nz (< 2^31) cubic cells of edge `cell` from (lo_x, lo_y, lo_z) over
 *     points (n, 3) float64; a point outside the box counts for the nearest border cell.  cell_start (cells + 1) int32 = the exclusive scan
 *     of gens_point_grid_count's counts (which ACCUMULATE); gens_point_grid_fill (cursor: (cells) int32 zero-filled scratch) writes
 *     cell_points (n) int32 = the point ids cell by cell (any order inside a cell) and sorted (n, 3) = their coordinates in that order.
 *     count / fill read `points`; the two entries below read `sorted`, `cell_start` and `cell_points`.
 *   gens_radius_downsample_round (dtu_eval.py:94-102): one round of the sequential greedy's mask over the cell-ordered cloud.  rank (n)
 *     int32 = the visiting position of the point in every slot; states (n) uint8, 0 undecided, 1 kept, 2 removed: state_out = state_in
 *     with every undecided point decided whose earlier-visited neighbours within the radius (d^2 <= radius^2) are all decided --
 *     removed if one of them is kept, else kept.  *undecided (int32) ACCUMULATES the points still undecided.  radius <= cell
 *     (GENS_ELIMIT otherwise).  Starting from zeros, rounds until nothing is undecided give exactly the script's mask.
 *   gens_nearest_point (:127-130, 140-142): for queries (n_queries, 3) float64 the distance to the nearest grid point and its id, the
 *     smallest id among equal distances; +inf and -1 where nothing is closer than max_dist (+inf: no cap).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const double* points;
    double* sorted;
    const int32_t* cell_start;
    int32_t* cell_points;
    int64_t n;
    double lo_x, lo_y, lo_z, cell;
    int nx, ny, nz;
} gens_point_grid;
int gens_mesh_sample_count(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double density,
                           int64_t* counts, void* stream);
int gens_mesh_sample_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double density,
                          const int64_t* offsets, int64_t total, double* out, void* stream);
int gens_point_grid_count(const gens_point_grid* grid, int32_t* counts, void* stream);
int gens_point_grid_fill(const gens_point_grid* grid, int32_t* cursor, void* stream);
int gens_radius_downsample_round(const gens_point_grid* grid, const int32_t* rank, double radius, const uint8_t* state_in, uint8_t* state_out,
                                 int32_t* undecided, void* stream);
int gens_nearest_point(const gens_point_grid* grid, const double* queries, int64_t n_queries, double max_dist, double* dist, int32_t* index,
                       void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K25  the device pieces of the DTU mesh finalising step (evaluation/clean_meshes.py).  Every entry checks its arguments before any launch.
 *   gens_dilate_u8 (:124-127, :213-216): grey-scale dilation of interleaved uint8 images in (n, h, w, c), c = 1 or 3, into out
 *     (n, h, w, channels), the first `channels` <= c channels of every pixel.  The structuring element has kh rows of kw columns (both odd,
 *     at most 63), anchored at its centre; half_spans (kh) HOST ints: row i holds the columns kw / 2 - half_spans[i] .. kw / 2 +
 *     half_spans[i] (negative: the row is empty).  Pixels outside the image do not take part (a border of 0).  Bit-equal to the maximum
 *     over the element.
 *   gens_vertex_mask_votes (:101-141): points (n_points, 3) float64; proj (nv, 3, 4) float32 (the first three rows of K4 @ E); masks
 *     (nv, h, w) uint8, set where > 128.  votes (n_points) int32 = the number of views whose mask, framed by one pixel of ones, holds the
 *     point's projection: q = P[:, :3] x + P[:, 3] in float64, q / q[2], rint, + 1, inside iff 0 <= u <= w, 0 <= v <= h and (u == 0 or
 *     v == 0 or masks[v - 1][u - 1] > 128).  A projection that is not finite (q[2] == 0) counts as outside.
 *   gens_view_rays_hit_counts (:212-246; the kernel lives beside K23's in k23_mesh_cull.hip): the rays of gen_rays_from_single_image for the
 *     h x w pixels of nv views, generated in the kernel as gens_view_rays_hit_faces generates them; a pixel casts iff masks (nv, h, w)
 *     uint8 is > 128 there; the origin is advanced to o + d * dep_min (a float32 product, then a float32 sum).  cams (nv, 21) as for
 *     gens_view_rays_hit_faces.  flags (nv, n_faces) uint8 and any_miss (nv) int32 ACCUMULATE, per view: 1 for every face some ray of the
 *     view hits first, 1 if some cast ray of the view misses.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_dilate_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int c, int channels, int kw, int kh, const int* half_spans_host,
                   void* stream);
int gens_vertex_mask_votes(const double* points, int64_t n_points, const float* proj, const uint8_t* masks, int nv, int h, int w,
                           int32_t* votes, void* stream);
int gens_view_rays_hit_counts(const gens_mesh_grid* grid, const uint8_t* masks, const float* cams, int nv, int h, int w, float dep_min,
                              uint8_t* flags, int32_t* any_miss, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K26  GenS.filter_volume (gens.py:87-122): the mask pyramid restricted to a dilated band around the surface, two launches for all levels.
 *   u (D0, D0, D0) float32, indexed [ix, iy, iz]: the level-0 lattice of -sdf on linspace(-1, 1, D0)^3 (ImplicitSurface.sdf_grid).
 *   dims (n_levels) HOST ints with dims[l] == dims[0] >> l and dims[0] a multiple of 1 << (n_levels - 1); at most GENS_MAX_LEVELS levels
 *   (GENS_ELIMIT beyond); dims[0]^3 < 2^31.  masks_in / masks_out: HOST arrays of device pointers to (D_l^3) floats indexed [x, y, z]
 *   (in place is allowed: masks_out[l] == masks_in[l]); bits_out: HOST array of device pointers to ceil(D_l^3 / 32) uint32 words each, in
 *   gens_pack_mask_bits' format.  band_words: scratch, ceil(D0^3 / 32) uint32 words (the band as bits, left there for the caller).
 *   counts: two device int64, SET by the call: band voxels, band voxels after dilation.
 *     band[i] = |u[i]| < thresh (a NaN: 0) and sqrt(x^2 + y^2 + z^2) < 1 in float32 at gens_lattice_points' coordinates;
 *     dil     = the 3 x 3 x 3 maximum of band, neighbours outside the cube ignored (F.max_pool3d(band, 3, 1, 1));
 *     out_l[x, y, z] = in_l[x, y, z] * dil[x << l, y << l, z << l] (a float product: the chain of nearest halvings picks, it does not pool);
 *     bits_l = out_l > 0.
 *   Every pointer must be non-null and 4-byte aligned, counts 8-byte aligned.  Arguments are checked before any launch.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_filter_masks(const float* u, float thresh, const float* const* masks_in, float* const* masks_out, uint32_t* const* bits_out,
                      const int* dims, int n_levels, uint32_t* band_words, int64_t* counts, void* stream);
/* The two launches of gens_filter_masks one at a time, for a caller that edits the band in between (K27: keep its largest component).
 *   gens_filter_band: the first launch.  SETS counts[0] (band voxels) and writes band_words; u, thresh, d0 = dims[0] as above.
 *   gens_filter_levels: the second launch from the caller's band_words.  SETS counts[1] (band voxels after dilation) and leaves counts[0]
 *   alone; everything else as above.  gens_filter_band followed by gens_filter_levels is gens_filter_masks. */
int gens_filter_band(const float* u, float thresh, int d0, uint32_t* band_words, int64_t* counts, void* stream);
int gens_filter_levels(const float* const* masks_in, float* const* masks_out, uint32_t* const* bits_out, const int* dims, int n_levels,
                       const uint32_t* band_words, int64_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K27  clean_volume (utils/tools.py:34-50: skimage.measure.label(mask, connectivity=3), regionprops, keep the largest region): the largest
 *      connected component of a bit volume, six launches, nothing waits inside a launch.
 *   bits_in / bits_out: ceil(nx * ny * nz / 32) uint32 words in gens_pack_mask_bits' format, bit (i & 31) of word (i >> 5) = voxel i in C
 *   order of the (nx, ny, nz) volume; any positive extents with nx * ny * nz < 2^31 (GENS_ELIMIT beyond); bits past the last voxel are
 *   ignored on input and zero on output; bits_out must not be bits_in.  connectivity: 3 (26 neighbours) or 1 (6 neighbours); a neighbour
 *   outside the volume does not exist.  scratch: gens_components_scratch_bytes(nx, ny, nz) bytes, 8-byte aligned (16 bytes + one int32
 *   parent per voxel: 67 MB at 256^3; 0 for extents the call refuses).
 *     root of a set voxel = the smallest linear index of its component (a min-index union: the same whatever order the atomics land in);
 *     winner = the component of largest size, a tie to the one whose first voxel comes first in C order (np.argmax over regionprops);
 *     bits_out = the winner's voxels.
 *   results: four device int64, SET by the call: the number of components; the winner's size; its root (-1 when the volume is empty); its
 *   label number = 1 + the number of components whose first voxel precedes the winner's (skimage's and scipy's numbering; 0 when empty).
 *   An empty volume gives empty bits_out and zero components.  Every pointer non-null; bits 4-byte, scratch and results 8-byte aligned.
 *   Arguments are checked before any launch.
 *   gens_unpack_mask_bits: the inverse of gens_pack_mask_bits, mask[i] = 1.0f or 0.0f for bit i, n >= 1 floats.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t gens_components_scratch_bytes(int nx, int ny, int nz);
int gens_largest_component(const uint32_t* bits_in, int nx, int ny, int nz, int connectivity, uint32_t* bits_out, void* scratch,
                           int64_t* results, void* stream);
int gens_unpack_mask_bits(const uint32_t* bits, int64_t n, float* mask, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K28  The two-level lattice of extract_geometry (implicit_surface.py:407-427): the network is evaluated on every brick-th lattice point
 *      and inside the bricks that can contain the iso-surface; six streaming launches around the caller's evaluator (ops.sparse_lattice).
 *   res = R >= 2 lattice points per axis with R^3 < 2^31 (GENS_ELIMIT beyond: all point indices are 32-bit); brick = B >= 1 cells.
 *   C = ceil((R - 1) / B) + 1 coarse points per axis, coarse index i = fine index min(i * B, R - 1); (C - 1)^3 bricks in C order
 *   [bx, by, bz], brick b between the coarse points b and b + 1 of each axis.  The brick that DECIDES for fine index i is min(i / B, C - 2).
 *   Point bricks: fine index i is OWNED by point brick i / B of P = ceil(R / B) per axis (P == C - 1 unless (R - 1) % B == 0: then the
 *   plane R - 1 is a point brick of its own, decided by the brick below it).  A list entry is a point brick's C-order number in the P^3
 *   grid and stands for B^3 rows in brick-local C order [lx, ly, lz], fine index e * B + l per axis.
 *   Coordinates: gens_lattice_points' formula at the fine index, bit for bit.  bmin3_host / bmax3_host: three HOST floats each.
 *     gens_sparse_coarse_points: pts (count, 3) = the coarse points first .. first + count - 1 in C order of the C^3 grid.
 *     gens_sparse_classify: uc (C^3) = u at the coarse points -> flags ((C - 1)^3) bytes: 1 if a corner of the brick is non-finite, or
 *       has |u - t| <= margin (float32; margin >= 0), or the 8 corners disagree on u < t; else 0.
 *     gens_sparse_brick_points: pts (count * B^3, 3) for the entries list[first .. first + count); an index past R - 1 is clamped to it.
 *     gens_sparse_fill: u (R^3, 16-byte aligned) <- for every fine point the value of uc at its deciding brick's lowest corner.
 *     gens_sparse_scatter: sdf (count * B^3) in gens_sparse_brick_points' row order -> u[fine point] = -sdf[row] for the rows whose
 *       indices are all <= R - 1 (the others are the clamped duplicates).  An entry outside the P^3 grid is skipped.
 *     gens_sparse_leaks: leaks (one device int64, 8-byte aligned, SET by the call) = the number of lattice edges (p, p + e_axis) with
 *       (u[p] < t) != (u[q] < t) and flags == 0 at the deciding brick of p or of q.
 *   list: n_list int64 on the DEVICE (gens_compact_valid's output); first >= 0, count >= 0, first + count <= n_list (GENS_EINVAL);
 *   B <= 1024 and count * B^3 < 2^31 / 3 rows per call (GENS_ELIMIT).  Every pointer non-null (a zero count needs none).  Arguments are
 *   checked before any launch.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_sparse_coarse_points(const float* bmin3_host, const float* bmax3_host, int res, int brick, int64_t first, int64_t count, float* pts,
                              void* stream);
int gens_sparse_classify(const float* uc, int res, int brick, float t, float margin, uint8_t* flags, void* stream);
int gens_sparse_brick_points(const float* bmin3_host, const float* bmax3_host, int res, int brick, const int64_t* list, int64_t n_list,
                             int64_t first, int64_t count, float* pts, void* stream);
int gens_sparse_fill(const float* uc, int res, int brick, float* u, void* stream);
int gens_sparse_scatter(const float* sdf, int res, int brick, const int64_t* list, int64_t n_list, int64_t first, int64_t count, float* u,
                        void* stream);
int gens_sparse_leaks(const float* u, int res, int brick, const uint8_t* flags, float t, int64_t* leaks, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K29  Marching cubes on the bricks of K28's two-level lattice (ops.brick_marching_cubes): the mesh gens_mc_classify / gens_mc_emit return
 *      for the lattice K28 builds, without that lattice.  K28's terms (R, B, C, P, deciding and point bricks, the active rule, the fill =
 *      uc at the deciding brick's lowest corner, the leak rule) hold unchanged; u = -sdf.
 *   Limits: res = R >= 2, 2 <= brick = B <= 8 (GENS_EINVAL); C^3 < 2^31 and P^3 < 2^31 (GENS_ELIMIT) -- not R^3.  Per-axis indices are
 *   32-bit, flat fine-lattice indices (the keys) 64-bit.  Arguments are checked before any launch; every pointer non-null unless the list
 *   or range is empty.
 *     gens_brick_coarse_points / gens_brick_points: gens_sparse_coarse_points / gens_sparse_brick_points under these limits, bit-equal to
 *       gens_lattice_points at the same per-axis index; count < 2^31 / 3 rows per call.
 *     gens_brick_active: gens_sparse_classify's rule: uc (C^3) -> flags ((C - 1)^3) bytes.
 *     (These three launch K28's kernels, csrc/k28_sparse_lattice.hip; the rest is csrc/k29_brick_mcubes.hip.  The limits of both families
 *     and every rule K12, K28 and K29 share are written once, in csrc/lattice.h.)
 *     gens_brick_emit_flags: emit[X] = 1 if a brick of X + {0,1}^3 (clipped to the (C - 1)^3 grid) is active.  Every cell of K28's lattice
 *       with corners on both sides of t, and every crossing edge, starts at a point decided by such a brick.
 *   The per-brick calls take `list`: n_list (< 2^31) int64 point-brick numbers on the DEVICE, the point bricks whose deciding brick emits
 *   (an entry outside the P^3 grid emits nothing); entry k owns rows k * B^3 .. of the per-point arrays, brick-local C order.
 *   store: (evaluated point bricks, B^3) u in gens_brick_points' row order; pslot (P^3) int32: a point brick's row of store or -1.
 *     gens_brick_mc_classify: per point vmask / cases as gens_mc_classify defines them (0 for an index past R - 1) and rank (uint16) = the
 *       vertices of the brick's earlier points; counts (3, n_list) int32 = the bricks' vertices, triangles and leaks (gens_sparse_leaks'
 *       rule on the edges its points own).  tri_count: the 256 bytes of gens_mc_classify.
 *     gens_brick_mc_emit: voff / toff (n_list) int64 = exclusive scans of the counts; eslot (P^3) int32: a point brick's index in `list`
 *       or -1.  Vertex of edge (p, a): gens_mc_emit's float64 expression, at voff[brick] + rank (+ earlier axes); vkey = 3 flat(p) + a.
 *       Triangles (vertex ids through eslot; -1 for an owner outside the list, which the covering argument excludes) at toff[brick] + the
 *       triangles of the brick's earlier points; tkey = flat(cell).  Sorting by the keys gives gens_mc_emit's order.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_brick_coarse_points(const float* bmin3_host, const float* bmax3_host, int res, int brick, int64_t first, int64_t count, float* pts,
                             void* stream);
int gens_brick_points(const float* bmin3_host, const float* bmax3_host, int res, int brick, const int64_t* list, int64_t n_list, int64_t first,
                      int64_t count, float* pts, void* stream);
int gens_brick_active(const float* uc, int res, int brick, float t, float margin, uint8_t* flags, void* stream);
int gens_brick_emit_flags(const uint8_t* active, int res, int brick, uint8_t* emit, void* stream);
int gens_brick_mc_classify(const float* uc, const float* store, const int32_t* pslot, const uint8_t* active, int res, int brick,
                           const int64_t* list, int64_t n_list, float iso, const uint8_t* tri_count, uint8_t* vmask, uint8_t* cases,
                           uint16_t* rank, int32_t* counts, void* stream);
int gens_brick_mc_emit(const float* uc, const float* store, const int32_t* pslot, const int32_t* eslot, int res, int brick, const int64_t* list,
                       int64_t n_list, float iso, const int8_t* tri_table, int table_stride, const uint8_t* tri_count, const uint8_t* vmask,
                       const uint8_t* cases, const uint16_t* rank, const int64_t* voff, const int64_t* toff, double* vertices,
                       int32_t* triangles, int64_t* vkey, int64_t* tkey, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K30  Per-vertex attributes of an extracted mesh (ImplicitSurface.vertex_attributes): the two streaming launches around the network
 *      kernels (gens_sdf_grad*, gens_blend_views*), csrc/k30_vertex_attrs.hip.  Arguments are checked before any launch: a negative n,
 *      resolution < 2, a null pointer that n > 0 would dereference, n_src outside 1 .. 255: GENS_EINVAL; n >= 2^31: GENS_ELIMIT.  n == 0
 *      succeeds without a launch.  The ABI version stays 12: no existing entry changes.
 *   gens_vertex_points: vertices (n, 3) float64 in lattice-index coordinates (gens_mc_emit / gens_brick_mc_emit) -> points (n, 3) float32 =
 *     the float32 rounding of v / (resolution - 1.0) * span + lo, evaluated per component in float64 in that order, un-fused: the
 *     vertices extract_geometry returns (implicit_surface.py:424-425), rounded once.  span / lo: the box's extent and lower corner as the
 *     caller's float64 arithmetic sees them (extract_geometry: the float32 difference b_max - b_min widened).
 *   gens_vertex_pack: grad (n, 3) float32 = d sdf / dx, color (n, 3) float32, vis (n, n_src) uint8 in-frustum flags ->
 *     normals (n, 3) float32 = g / sqrt((gx^2 + gy^2) + gz^2) in float64, rounded once; (0, 0, 0) where a component is not finite or the
 *       norm is 0 (a gradient whose float32 squares would underflow still normalises);
 *     colors (n, 3) uint8 = trunc(min(max(c * 256, 0), 255)) (implicit_surface.py:455), 0 for a component that is not finite;
 *     seen (n) uint8 = 1 if any of the vertex' n_src flags is set.
 *     grad == NULL: normals is not written; color == NULL: colors and seen are not written (vis is not read).  Both NULL: GENS_EINVAL.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_vertex_points(const double* vertices, int64_t n, int resolution, double span_x, double span_y, double span_z, double lo_x,
                       double lo_y, double lo_z, float* points, void* stream);
int gens_vertex_pack(const float* grad, const float* color, const uint8_t* vis, int n_src, int64_t n, float* normals, uint8_t* colors,
                     uint8_t* seen, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K31  Sphere tracing of the surface along rays (ops.sphere_trace, ImplicitSurface.render_surface), csrc/k31_surface_trace.hip: the
 *      streaming launches between the network evaluations.  tests/surface_trace_reference.py restates all of it in numpy.
 *
 *   Definition.  g(p) = sdf(p) + threshold; the surface is g = 0; g > 0 is the side K12 calls u < iso (u = -sdf), g <= 0 the other side
 *   (-0.0 counts as 0).  A ray is p(t) = o + t d in float32; d need not be unit and t counts in units of d, like z_vals.  Parameters:
 *   lipschitz L > 0 (an assumed bound on |d sdf| per unit length -- the heuristic of the sparse lattice), min_step > 0 in
 *   world units, max_steps >= 1, refine >= 0.  Per ray: float32 t, t_lo, t_hi, g_lo, g_hi, t_end, |d|; a one-byte status; a step count.
 *   Every float32 operation below is rounded on its own, in the order written; points handed to the evaluator are o + t * d, un-fused.
 *     Begin.  Slab test against [lo, hi] intersected with [near, far]: per axis (lo - o) / d and (hi - o) / d, ordered; an axis with d = 0
 *       contributes (-inf, +inf) if lo <= o <= hi and otherwise the ray misses.  t0 = max(near, entries), t_end = min(far, exits).
 *       Non-finite o or d: BAD.  |d| = 0 or not t0 < t_end: MISS.  Else LIVE at t = t0.  |d| = sqrt((dx^2 + dy^2) + dz^2) in float64 from the
 *       float32 components, rounded once.
 *     March.  One round evaluates g at p(t) for every LIVE ray (its evaluation number k = steps + 1):
 *       g not finite                 BAD
 *       g <= 0 and k == 1            INSIDE (the ray enters the box below the surface: not a hit, the mesh is open there too)
 *       g <= 0 later                 BRACKET, (t_hi, g_hi) = (t, g); (t_lo, g_lo) is the previous round's
 *       g > 0 and t == t_end         MISS (the exit point itself was sampled)
 *       g > 0 and k == max_steps     EXHAUSTED
 *       g > 0 otherwise              (t_lo, g_lo) = (t, g); t = min(t + max(g / L, min_step) / |d|, t_end)
 *     Refine.  `refine` rounds on the BRACKET rays: g at t_m = 0.5 (t_lo + t_hi); g <= 0 replaces the hi end, anything else the lo end.
 *       Then t = t_lo + (t_hi - t_lo) (g_lo / (g_lo - g_hi)) and the status is HIT: marching cubes' own rule on a crossing edge, on a
 *       segment of at most min_step 2^-refine.
 *     Pack, per ray, with rot = inverse(c2ws[0][:3,:3]) (9 floats on the device, row-major) and rot v = (v0 rot[k][0] + v1 rot[k][1]) +
 *       v2 rot[k][2]: depth = t (rot d)_z for HIT and 0 otherwise (the reference's z_val * cos, implicit_surface.py:298); normal = K30's unit
 *       normal of the gradient at the hit point; normal_img = min(max((rot normal) 128 + 128, 0), 255) in float32; img = K30's 8-bit
 *       colour; seen = K30's; hit = (status == HIT).  Everything is 0 where the ray is not a hit.
 *
 *   gens_trace_state: the rays (rays_o, rays_d (n, 3)) and the per-ray state on the device; `points` (n, 3) holds the NEXT point of every ray
 *     that needs an evaluation (a LIVE ray's p(t), a BRACKET ray's p(t_m)) and, after the final refine round, the hit point; `live` (n) is 1
 *     for LIVE rays (what gens_compact_valid takes); t of a BRACKET ray is t_m.  steps counts the march evaluations.
 *   gens_trace_begin: near / far: one float each (per_ray = 0) or (n) (per_ray = 1) on the device; lo / hi: 3 HOST floats each.  Writes all
 *     of the state (rays that are not LIVE: t = t_end = 0, point 0).
 *   gens_trace_march: sdf (m): the evaluator's values at the points of the rays idx[0 .. m) (int64, device; NULL: rays 0 .. m - 1).  Entries
 *     outside 0 .. n - 1 and rays that are not LIVE are left alone.
 *   gens_trace_refine: the same for BRACKET rays; sdf == NULL skips the bisection (refine = 0: final only); final != 0 interpolates and
 *     sets HIT, else the next mid-point is written.
 *   gens_trace_gather: out (m, 3) = points[idx[j]] (rows outside 0 .. n - 1: zeros).
 *   gens_surface_pack: rows j < m of grad / color / vis (n_src flags per row) belong to ray idx[j] (NULL: ray j); status, t, rays_d and the
 *     outputs are per ray (n).  Any output pointer may be NULL (not written); grad == NULL: no normals; color == NULL: no img / seen.
 *   Arguments are checked before any launch: null pointers, negative counts, lipschitz / min_step not positive and finite, max_steps < 1,
 *   n_src outside 1 .. 255: GENS_EINVAL; n or m >= 2^31 (gather: 3 m): GENS_ELIMIT.  n == 0 / m == 0 succeed without a launch.  ABI stays 12.
 * ---------------------------------------------------------------------------------------------------------- */
#define GENS_TRACE_LIVE 0
#define GENS_TRACE_HIT 1
#define GENS_TRACE_MISS 2
#define GENS_TRACE_INSIDE 3
#define GENS_TRACE_EXHAUSTED 4
#define GENS_TRACE_BAD 5
#define GENS_TRACE_BRACKET 6
typedef struct {
    const float *rays_o, *rays_d;
    float *t, *t_lo, *t_hi, *g_lo, *g_hi, *t_end, *dlen;
    uint8_t* status;
    int32_t* steps;
    float* points;
    uint8_t* live;
    int64_t n;
} gens_trace_state;
typedef struct {
    const float *grad, *color;
    const uint8_t* vis;
    int n_src;
    const int64_t* idx;
    int64_t m, n;
    const uint8_t* status;
    const float *t, *rays_d, *rot;
    float *depth, *normal, *normal_img;
    uint8_t *img, *seen, *hit;
} gens_surface_pack_args;
int gens_trace_begin(const gens_trace_state* s, const float* near, const float* far, int per_ray, const float* lo, const float* hi, void* stream);
int gens_trace_march(const gens_trace_state* s, const float* sdf, const int64_t* idx, int64_t m, float threshold, float lipschitz,
                     float min_step, int max_steps, void* stream);
int gens_trace_refine(const gens_trace_state* s, const float* sdf, const int64_t* idx, int64_t m, float threshold, int final, void* stream);
int gens_trace_gather(const float* points, const int64_t* idx, int64_t m, int64_t n, float* out, void* stream);
int gens_surface_pack(const gens_surface_pack_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K32  Fusion of per-view depth maps into a consistency-filtered point cloud (ops.fuse_depth_maps, ops.fused_points,
 *      ImplicitSurface.fuse_surface), csrc/k32_depth_fusion.hip.  tests/depth_fusion_reference.py restates all of it in numpy.
 *
 *   Definition.  All arithmetic is float64, every operation rounded on its own, in the order written; no square root: distances are
 *   compared squared.  A NaN makes a comparison false, hence no vote; nothing special-cases it.
 *     depth (nv, H, W) float32: each view's z-depth in its own camera; a pixel is usable iff its depth is finite and > 0.
 *     cams (nv, 24) float64 per view: P = K[:3,:3] w2c[:3,:4] (12, row-major), B = inverse(K[:3,:3] w2c[:3,:3]) (9, row-major), the camera
 *       centre c (3).  Pixel (x, y), integers, is the ray through K^-1 [x, y, 1].  Below
 *         B [x, y, 1] = (B[i][0] x + B[i][1] y) + B[i][2]                    per row i
 *         P [X, 1]    = ((P[i][0] X0 + P[i][1] X1) + P[i][2] X2) + P[i][3]   per row i.
 *     pairs (nv, k) int32: row r lists the source views that vote for view r; an entry outside 0 .. nv - 1 is skipped (-1 pads a row).
 *     For a usable pixel (r, y, x) with depth d:  X = c_r + d (B_r [x, y, 1]);  n = 0, dsum = 0;  for each listed source s, in list order:
 *       q = P_s [X, 1]; no vote unless q_z > 0.  xs = q_x / q_z, ys = q_y / q_z, x0 = floor(xs), y0 = floor(ys).
 *       No vote unless 0 <= x0, x0 + 1 <= W - 1, 0 <= y0, y0 + 1 <= H - 1, and unless the taps d00 = depth[s, y0, x0], d01 = [s, y0, x0 + 1],
 *       d10 = [s, y0 + 1, x0], d11 = [s, y0 + 1, x0 + 1] are all usable.  fx = xs - x0, fy = ys - y0,
 *       ds = (d00 (1 - fx) + d01 fx) (1 - fy) + (d10 (1 - fx) + d11 fx) fy,   Xs = c_s + ds (B_s [xs, ys, 1]),
 *       q' = P_r [Xs, 1]; no vote unless q'_z > 0.  ex = q'_x / q'_z - x, ey = q'_y / q'_z - y.
 *       Vote iff ex ex + ey ey < pix_tol pix_tol and |q'_z - d| / d < rel_tol (both strict), and, with a normal map (nv, H, W, 3) float32,
 *       (n_a0 n_b0 + n_a1 n_b1) + n_a2 n_b2 >= normal_cos for n_a = normal[r, y, x], n_b = normal[s, floor(ys + 0.5), floor(xs + 0.5)].
 *       On a vote n += 1, dsum += q'_z.
 *     votes[r, y, x] = min(n, 255); keep = (n >= min_views); fused = (d + dsum) / (n + 1) where kept, else 0 (float64); an unusable pixel
 *     has 0 votes.  point = c_r + fused (B_r [x, y, 1]).
 *   gens_fuse_depth_maps: one thread per reference pixel, a workgroup on 16 x 16 pixels of one view (8 x 8 per wave) -> votes, keep (nv, H, W)
 *     uint8, fused (nv, H, W) float64.  normal == NULL: no normal test.  All pointers are device pointers.
 *   gens_fused_points: list (n_list) int64 flat pixel indices (r H + y) W + x (gens_compact_valid of keep) -> points (n_list, 3) float64, and
 *     normals (n_list, 3) float32 / colors (n_list, 3) uint8 copied from normal (nv, H, W, 3) / img (nv, H, W, 3) uint8 at the pixel (a map
 *     and its output are given together or both NULL).  An entry outside the maps gives zero rows.
 *   Arguments are checked before any launch: negative sizes, k < 0, pix_tol / rel_tol negative or not finite, min_views < 1, a NaN
 *   normal_cos with a normal map, null pointers: GENS_EINVAL; nv H W or n_list >= 2^31: GENS_ELIMIT.  nv H W == 0 / n_list == 0 succeed
 *   without a launch.  The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_fuse_depth_maps(const float* depth, const double* cams, const int32_t* pairs, const float* normal, int nv, int h, int w, int k,
                         double pix_tol, double rel_tol, int min_views, double normal_cos, uint8_t* votes, uint8_t* keep, double* fused,
                         void* stream);
int gens_fused_points(const double* fused, const double* cams, const int64_t* list, int64_t n_list, int nv, int h, int w, const float* normal,
                      const uint8_t* img, double* points, float* normals, uint8_t* colors, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K33  Mesh simplification by vertex clustering with quadric-optimal representatives (Lindstrom's out-of-core simplification;
 *      ops.simplify_mesh, io.simplify_mesh, ImplicitSurface.extract_geometry(simplify=)), csrc/k33_mesh_simplify.hip.
 *      tests/mesh_simplify_reference.py restates all of it in numpy.
 *
 *   Definition.  All arithmetic is float64, every operation rounded on its own, in the order written; no square root.
 *     Inputs: vertices (V, 3) float64, triangles (T, 3) int32, cell > 0, origin (3), reg > 0 (default 1e-3).
 *     1. Cell of a vertex p:  c_a = floor((p_a - origin_a) / cell) per axis, which needs 0 <= c_a < 2^21;  key = c_z 2^42 + c_y 2^21 + c_x
 *        (int64).  The distinct keys in ascending order are the clusters (a cluster's rank is its place in that order); a cluster's members
 *        are its vertices in ascending vertex index.
 *     2. A triangle survives iff its three vertices lie in three different clusters.  Among surviving triangles with the same set of three
 *        clusters, whatever the orientation, the one with the smallest triangle index is kept.  Kept triangles are emitted in ascending
 *        input index with their own vertex order; output vertices are the clusters a kept triangle references, numbered in ascending key
 *        order.
 *     3. Quadric of a cluster, in cell units about the cluster's cell centre:  ctr_a = origin_a + (c_a + 0.5) cell,  q = (p - ctr) / cell.
 *        For every SURVIVING triangle (before duplicate removal) that has a vertex in the cluster, in ascending triangle index, each once,
 *        with its vertices q0, q1, q2 in stored order:  e1 = q1 - q0, e2 = q2 - q0,  n = e1 x e2 (n_x = e1_y e2_z - e1_z e2_y,
 *        n_y = e1_z e2_x - e1_x e2_z, n_z = e1_x e2_y - e1_y e2_x: two rounded products and one subtraction each),
 *        d = -((n_x q0_x + n_y q0_y) + n_z q0_z);  A_ij += n_i n_j for the six entries of the symmetric A,  b_i += n_i d.
 *        m = (the sum of the members' q in member order) / their count.
 *     4. Representative:  tr = (A00 + A11) + A22.  If not tr > 0, x = m.  Otherwise lambda = reg tr, M = A with lambda added on the
 *        diagonal, r_a = lambda m_a - b_a, and M x = r is solved by the adjugate:
 *          c00 = M11 M22 - M12 M12,  c01 = M02 M12 - M01 M22,  c02 = M01 M12 - M02 M11,
 *          c11 = M00 M22 - M02 M02,  c12 = M01 M02 - M00 M12,  c22 = M00 M11 - M01 M01,
 *          det = (M00 c00 + M01 c01) + M02 c02,
 *          x_0 = ((c00 r0 + c01 r1) + c02 r2) / det,  x_1 = ((c01 r0 + c11 r1) + c12 r2) / det,  x_2 = ((c02 r0 + c12 r1) + c22 r2) / det.
 *        If not det > 0, or any |x_a| <= 0.5 is false (a NaN included), x = m (the cluster "fell back", as it does when not tr > 0).
 *        The output vertex is ctr_a + x_a cell.  The regulariser pulls towards the members' mean only along directions the planes do not
 *        fix: a flat cluster gives the mean projected onto the plane, an edge cluster the mean projected onto the edge, a corner the corner.
 *     5. Source vertex: the member with the smallest ((q_0 - x_0)^2 + (q_1 - x_1)^2) + (q_2 - x_2)^2, the first such member on ties.
 *        Attributes are never averaged: callers gather any per-vertex array with it (normals[source]).
 *   Guaranteed: every output vertex lies in its cluster's closed cell up to the rounding of the last multiply-add, hence within sqrt(3) cell
 *   of its source vertex.  NOT guaranteed: topology (clustering can pinch sheets together, leave non-manifold edges and drop components
 *   smaller than a cell), and any distance to the true surface.
 *
 *   gens_cluster_keys: one thread per vertex -> keys (V) int64; -1 where a c_a is outside 0 .. 2^21 - 1 or not a number (callers refuse
 *     such input beforehand).
 *   gens_cluster_triangles: one thread per triangle; vertex_cluster (V) int32 = each vertex's cluster rank -> ranks (T, 3) int32 (the three
 *     ranks in stored order), survive (T) uint8, triple (T, 3) int32 (the ranks ascending).  A vertex index outside 0 .. V - 1 gives rank -1
 *     and a triangle that does not survive.
 *   gens_cluster_solve: one thread per output cluster j = 0 .. n_out - 1, cluster out_clusters[j].  cluster_keys (C) int64 ascending;
 *     entries (3 T) int32: the values 3 t + k sorted stably by the rank of vertex k of triangle t, entry_start (C + 1) int32 the segment of
 *     each cluster in it; members (V) int32: the vertex indices sorted stably by key, member_start (C + 1) int32.  The thread walks both
 *     segments in order (steps 3 to 5) -> out_vertices (n_out, 3) float64, source (n_out) int32, fell_back (n_out) uint8.  Entries,
 *     members and indices outside their ranges are skipped, never read through.
 *   All pointers are device pointers.  Arguments are checked before any launch: negative sizes, cell / reg not positive and finite, an
 *   origin that is not finite, n_clusters > n_vertices, n_out > n_clusters, null pointers: GENS_EINVAL; V or 3 T >= 2^31: GENS_ELIMIT.
 *   V == 0, T == 0, n_out == 0 succeed without a launch.  The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const double* vertices;       /* (V, 3) */
    const int32_t* triangles;     /* (T, 3) */
    const uint8_t* survive;       /* (T) */
    const int64_t* cluster_keys;  /* (C) */
    const int32_t *entries, *entry_start, *members, *member_start, *out_clusters;
    int64_t n_vertices, n_triangles, n_clusters, n_out;
    double origin[3], cell, reg;
    double* out_vertices;         /* (n_out, 3) */
    int32_t* source;              /* (n_out) */
    uint8_t* fell_back;           /* (n_out) */
} gens_cluster_solve_args;
int gens_cluster_keys(const double* vertices, int64_t n_vertices, double origin_x, double origin_y, double origin_z, double cell, int64_t* keys,
                      void* stream);
int gens_cluster_triangles(const int32_t* triangles, int64_t n_triangles, const int32_t* vertex_cluster, int64_t n_vertices, int32_t* ranks,
                           uint8_t* survive, int32_t* triple, void* stream);
int gens_cluster_solve(const gens_cluster_solve_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K34  Texture atlases for triangle meshes (ops.texture_points / texture_snap / texture_pack / texture_uv, ImplicitSurface.texture_mesh,
 *      extract_geometry(texture=)), csrc/k34_mesh_texture.hip.  tests/mesh_texture_reference.py restates all of it in numpy.
 *
 *   Definition.  Arithmetic is float64 from the float32 inputs, every operation rounded on its own, in the order written; results are
 *   rounded once to float32.
 *     Inputs: points (V, 3) float32 in the model's frame, triangles (T, 3) int32, texels = S, an integer with 3 <= S <= 64 (the tile edge).
 *     1. Layout.  Every triangle gets P = S (S + 1) / 2 texels.  Triangle f lives in tile f >> 1, half f & 1.  A tile is S + 1 columns by S
 *        rows.  With n_tiles = ceil(T / 2):  cols = ceil(sqrt(n_tiles)) in exact integers, rows = ceil(n_tiles / cols) (both 0 for T = 0).
 *        The atlas is H = rows S by W = cols (S + 1), uint8 RGB, row 0 at the top; tile q sits at tile column q % cols and tile row q / cols.
 *     2. Texels.  The local texels of a triangle are (i', j') with i', j' >= 0 and i' + j' <= S - 1.  Sample number k = 0 .. P - 1
 *        enumerates them with j' as the outer and i' as the inner index (row j' holds S - j' texels); sample s = f P + k.  Half 0 maps
 *        (i', j') to the tile-local column and row (i, j) = (i', j'), half 1 to (S - i', S - 1 - j'), a half turn: half 0 takes i + j <= S - 1,
 *        half 1 takes i + j >= S, so every texel of a tile belongs to exactly one triangle.  The pixel of a texel is
 *        x = (q % cols) (S + 1) + i,  y = (q / cols) S + j.
 *     3. Points.  With A, B, C the triangle's corners in stored order, a = i' / (S - 2) and b = j' / (S - 2):
 *        p = (A + a (B - A)) + b (C - A), component by component.  The corners sit at the local texels (0, 0), (S - 2, 0) and (0, S - 2),
 *        where p is A, B and C.  Texels with i' + j' = S - 1 lie just outside the triangle, on its plane: they exist so that bilinear
 *        filtering at any point of the triangle reads this triangle's texels only.  A triangle with an index outside 0 .. V - 1 has NaN
 *        points (the index is never read through).  Longest edge of a triangle (the default step limit of 5): with
 *        e(P, Q) = ((Q_x - P_x)^2 + (Q_y - P_y)^2) + (Q_z - P_z)^2:  m = e(A, B); if e(B, C) > m, m = e(B, C); if e(C, A) > m, m = e(C, A);
 *        the edge is sqrt(m) rounded to float32 (NaN for a triangle with a bad index).
 *     4. Corner coordinates.  With (x, y) the pixel of a corner's texel:  u = (x + 0.5) / W,  v = 1 - (y + 0.5) / H (origin bottom-left, as
 *        OBJ expects) -> uv (T, 3, 2) float32.
 *     5. Optional snap, one round:  g = sdf + threshold (K31's g),  n2 = (gx^2 + gy^2) + gz^2,  t = g / n2,  step = t grad per component,
 *        len2 = (step_x^2 + step_y^2) + step_z^2.  The step is taken, p_a <- p_a - step_a (float32 state), iff g and n2 are finite, n2 > 0
 *        and len2 <= limit limit, with limit the sample's own (a float32, widened) or one max_move for all.  Otherwise p is kept.
 *        The guard: value and gradient are evaluated again at the new point (the next round's evaluation, and one more after the last
 *        round), and where |g| there is not <= |g| at the step's origin (a NaN included) the point goes back to the origin with the
 *        origin's value and gradient -- a later round repeats that step and is turned back again.  So no point ends with a larger |g|
 *        than it began with, as the evaluator sees it.  Nothing else is promised about convergence.
 *     6. Colour: K30's rule (csrc/pack_rules.h): trunc(clip(256 c, 0, 255)), 0 where c is not finite; seen = some source view has the point
 *        in its frustum.  Texels no triangle owns (the tail of the last tile row, the second half of the last tile when T is odd) are not
 *        written: callers zero the atlas and the seen plane first.
 *   NOT promised: anything under mip-mapping (tiles have no gutters wider than the one texel row), and seam-free colour across triangle
 *   edges (two triangles sample the same edge at the same points only up to their different extrapolations).
 *
 *   gens_texture_points: one thread per sample of [s0, s1) (a chunk may begin and end inside a triangle) -> out (s1 - s0, 3) float32 and,
 *     if edge is not NULL, edge (s1 - s0) float32 (the longest edge of the sample's triangle).
 *   gens_texture_snap: one thread per sample: points (n, 3) float32 in place, value (n) float32 = sdf, grad (n, 3) float32, limit (n)
 *     float32 or NULL (then max_move > 0 applies to all) -> taken (n) uint8 (1 where the step was taken).
 *   gens_texture_keep_better: one thread per sample: where |value + threshold| <= |prev_value + threshold| is false, points (n, 3), value (n)
 *     and grad (n, 3) are overwritten, in place, with prev_points, prev_value and prev_grad -> reverted (n) uint8.
 *   gens_texture_pack: color (s1 - s0, 3) float32 and vis (s1 - s0, n_src) uint8 of samples [s0, s1) -> the three bytes of each sample's
 *     texel in atlas (H, W, 3) uint8 and its flag in seen (H, W) uint8, written by one thread with byte stores (no two samples share a pixel).
 *   gens_texture_uv: one thread per triangle -> uv (n_faces, 3, 2) float32.
 *   All pointers are device pointers.  Arguments are checked before any launch: texels outside 3 .. 64, negative sizes, a sample range
 *   outside 0 .. T P, n_src outside 1 .. 255, a threshold that is not finite, no limit and max_move not positive, null pointers:
 *   GENS_EINVAL; V, T or the samples of one launch >= 2^31: GENS_ELIMIT.  An empty range, n == 0 and T == 0 succeed without a launch.
 *   The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_texture_points(const float* points, int64_t n_vertices, const int32_t* triangles, int64_t n_faces, int texels, int64_t s0, int64_t s1,
                        float* out, float* edge, void* stream);
int gens_texture_snap(float* points, const float* value, const float* grad, const float* limit, double max_move, float threshold, int64_t n,
                      uint8_t* taken, void* stream);
int gens_texture_keep_better(float* points, float* value, float* grad, const float* prev_points, const float* prev_value, const float* prev_grad,
                             float threshold, int64_t n, uint8_t* reverted, void* stream);
int gens_texture_pack(const float* color, const uint8_t* vis, int n_src, int64_t n_faces, int texels, int64_t s0, int64_t s1, uint8_t* atlas,
                      uint8_t* seen, void* stream);
int gens_texture_uv(int64_t n_faces, int texels, float* uv, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K35  Depth, normal and colour maps of a triangle mesh at the first hits of rays (ops.shade_mesh_hits / render_mesh,
 *      ImplicitSurface.render_mesh, validate(mesh_render=)), csrc/k35_mesh_shade.hip: the shading behind K23's gens_ray_first_hit.
 *      tests/mesh_render_reference.py restates all of it in numpy.
 *
 *   Definition.  Arithmetic is float64 from the stored inputs (float64 vertices, float32 rays, t, vertex normals; bytes), every operation
 *   rounded on its own, in the order written; results are rounded once.  dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z.  A, B, C are the
 *   corners of the ray's face in stored order.
 *     1. Hit.  A ray is a hit iff 0 <= face < T, t is finite and > 0, the face's three indices lie in 0 .. V - 1 and the nine coordinates
 *        of its corners are finite (gens_ray_first_hit never returns such a face; planted input may name one).  A face or vertex index
 *        outside its range is never read through.  Every output of a ray that is not a hit is 0.
 *     2. Depth = t (rot d)_z in float32: K31's pack rule, the same device function (csrc/pack_rules.h), so the mesh map and the surface
 *        map of one ray differ only through t.
 *     3. Barycentrics.  p = o + t d per component;  e1 = B - A,  e2 = C - A,  w = p - A;  d11 = dot(e1, e1),  d12 = dot(e1, e2),
 *        d22 = dot(e2, e2),  w1 = dot(w, e1),  w2 = dot(w, e2);  den = d11 d22 - d12 d12;  b = (d22 w1 - d12 w2) / den,
 *        c = (d11 w2 - d12 w1) / den.  If den > 0 is false (a NaN included), or b or c is not finite: (a, b, c) = (1, 0, 0).  Otherwise
 *        b and c that are not > 0 become 0;  s = b + c;  if s > 1: b = b / s, c = c / s;  a = (1 - b) - c, and an a that is not > 0
 *        becomes 0.  This is the least-squares foot of p in the face's plane, clamped into the face: the hit point of a watertight float64
 *        test lies in the face up to rounding, so the clamp removes that rounding only.  0 <= a, b, c <= 1 always.  bary = (a, b, c)
 *        rounded to float32; everything below uses the float64 values.
 *     4. Normal.  Flat: n = e1 x e2 = (e1_y e2_z - e1_z e2_y,  e1_z e2_x - e1_x e2_z,  e1_x e2_y - e1_y e2_x), each component negated if
 *        orient = 1.  Smooth: n = (a n_A + b n_B) + c n_C per component, from vertex_normals; orient does not enter.  normal = K30's unit
 *        normal of n (csrc/pack_rules.h): n / sqrt((n_x^2 + n_y^2) + n_z^2), rounded once; (0, 0, 0) where a component is not finite or
 *        the norm is 0.  normal_img = K31's, from the float32 normal: min(max((rot normal) 128 + 128, 0), 255) in float32.
 *        gens_mc_emit and gens_brick_mc_emit wind their triangles so that e1 x e2 points along + grad sdf (out of the object, towards the
 *        side K12 calls u < iso): orient = 0 is the default of every caller, orient = 1 is for meshes wound the other way.
 *     5. Colour from vertices (no atlas).  Per channel x = (a c_A + b c_B) + c c_C on the uint8 values; img = floor(x + 0.5) clamped to
 *        0 .. 255.  seen = 1 iff every corner whose weight is > 0 has vertex_seen != 0.
 *     6. Colour from the atlas (K34's layout, texels = S).  x = b (S - 2),  y = c (S - 2);  i0 = floor(x),  j0 = floor(y);  fx = x - i0,
 *        fy = y - j0.  The taps are the local texels (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1) with the weights
 *        (1 - fx)(1 - fy),  fx (1 - fy),  (1 - fx) fy,  fx fy.  A tap whose weight is not > 0 is not read and its term is 0; another
 *        tap's term is weight times the byte at K34's pixel of that local texel of the face (tile face >> 1, half face & 1).  Per channel
 *        x = ((term00 + term10) + term01) + term11; img as in 5.  seen = 1 iff every tap with a weight > 0 has atlas_seen != 0.
 *        Since 0 <= b, c <= 1, every tap read has 0 <= i', j' <= S - 1: a texel of the face's own tile.  Up to the roundings of step 3
 *        it also has i' + j' <= S - 1, a texel of the face itself: the rule does not cross the seams between tile halves.  At the
 *        corners A, B, C the colour is that of the local texels (0, 0), (S - 2, 0), (0, S - 2), bit for bit.
 *   NOT promised: anti-aliasing, mip-maps, lighting, a rasteriser.  One sample per ray.
 *
 *   gens_mesh_shade: one thread per ray.  vertices (V, 3) float64, triangles (T, 3) int32 (what gens_mesh_grid holds); rays_o, rays_d
 *     (n, 3) float32; face (n) int32 and t (n) float32 as gens_ray_first_hit wrote them; rot: 9 floats (K31's).  Optional (NULL: absent):
 *     vertex_normals (V, 3) float32, vertex_colors (V, 3) uint8, vertex_seen (V) uint8; atlas (atlas_h, atlas_w, 3) uint8, atlas_seen
 *     (atlas_h, atlas_w) uint8 with texels = S.  With an atlas, colour and seen come from it and the vertex colours are not read.
 *     shading: 0 flat, 1 smooth; orient: 0 as wound, 1 reversed.  Outputs, any of which may be NULL (not written, and what only it needs
 *     is not read): hit (n) uint8, bary (n, 3) float32, depth (n) float32, normal (n, 3) float32, normal_img (n, 3) float32, img (n, 3)
 *     uint8, seen (n) uint8.  All pointers are device pointers.
 *   Arguments are checked before any launch.  GENS_EINVAL: a null argument block; negative n, V or T; shading or orient outside 0 .. 1;
 *     with an atlas, texels outside 3 .. 64 or atlas_h, atlas_w that are not K34's layout of T and S; atlas_seen without an atlas; smooth
 *     shading without vertex_normals; img or seen requested with neither vertex_colors nor an atlas; seen requested without the seen
 *     plane of the colour's source; with n > 0 and some output requested, a null pointer the launch would dereference (face, t,
 *     triangles with T > 0, vertices with V > 0, rays_d, rays_o and rot where a requested output needs them).  GENS_ELIMIT: n, V or
 *     T >= 2^31.  n == 0, and no output requested, succeed without a launch.  The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const double* vertices;
    const int32_t* triangles;
    int64_t n_vertices, n_faces;
    const float *rays_o, *rays_d;
    const int32_t* face;
    const float* t;
    int64_t n;
    const float* rot;
    const float* vertex_normals;
    const uint8_t *vertex_colors, *vertex_seen;
    const uint8_t *atlas, *atlas_seen;
    int64_t atlas_h, atlas_w;
    int texels, shading, orient;
    uint8_t* hit;
    float *bary, *depth, *normal, *normal_img;
    uint8_t *img, *seen;
} gens_mesh_shade_args;
int gens_mesh_shade(const gens_mesh_shade_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K36  Exact point-to-mesh distance: for every query the nearest point of a triangle mesh, over K23's gens_mesh_grid
 *      (ops.closest_point_on_mesh, ops.mesh_distance, io.compare_meshes, python -m gens_amd.compare_meshes,
 *      ImplicitSurface.extract_geometry(simplify_error=)), csrc/k36_mesh_distance.hip.  tests/mesh_distance_reference.py restates all of it
 *      in numpy, as brute force over all faces.
 *
 *   Definition.  Arithmetic is float64, every operation rounded on its own, in the order written; the quotients are the correctly rounded
 *   ones; there is no square root.  dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z.  q is the query; a, b, c are the corners of face f in stored
 *   order.  Differences, products with a scalar and sums of points are per component.
 *     (a) d2(q, f), the closest point p(q, f) and the region code -- the region walk of Ericson, Real-Time Collision Detection, 5.1.5.
 *         ab = b - a,  ac = c - a,  ap = q - a;  n = ab x ac = (ab_y ac_z - ab_z ac_y,  ab_z ac_x - ab_x ac_z,  ab_x ac_y - ab_y ac_x).
 *         If n_x == 0 and n_y == 0 and n_z == 0 the face is DEGENERATE: the degenerate path below.  Otherwise
 *           d1 = dot(ab, ap), d2' = dot(ac, ap);  bp = q - b:  d3 = dot(ab, bp), d4 = dot(ac, bp);  cp = q - c:  d5 = dot(ab, cp),
 *           d6 = dot(ac, cp);  vc = d1 d4 - d3 d2',  vb = d5 d2' - d1 d6,  va = d3 d6 - d5 d4;  e = d4 - d3,  g = d5 - d6
 *         and the FIRST of these tests that holds decides (all of them non-strict, <= and >=, so a query on a border between two regions
 *         belongs to the earlier one):
 *           1. d1 <= 0 and d2' <= 0:                region 1 (vertex a),  p = a
 *           2. d3 >= 0 and d4 <= d3:                region 2 (vertex b),  p = b
 *           3. vc <= 0 and d1 >= 0 and d3 <= 0:     region 4 (edge ab),   den = d1 - d3,  v = d1 / den,  p = a + v ab
 *           4. d6 >= 0 and d5 <= d6:                region 3 (vertex c),  p = c
 *           5. vb <= 0 and d2' >= 0 and d6 <= 0:    region 6 (edge ca),   den = d2' - d6,  w = d2' / den,  p = a + w ac
 *           6. va <= 0 and e >= 0 and g >= 0:       region 5 (edge bc),   den = e + g,  w = e / den,  p = b + w (c - b)
 *           7. va >= 0 and vb >= 0 and vc >= 0:     region 0 (interior),  den = (va + vb) + vc,  v = vb / den,  w = vc / den,
 *                                                   p = (a + v ab) + w ac
 *         A quotient is formed only where its den > 0 (STRICT): where the deciding test is 3, 5, 6 or 7 and den > 0 is false, and where no
 *         test holds (rounding can leave va, vb, vc with signs that no point of the plane has), the degenerate path is taken.  So no
 *         division yields a NaN for finite input whose products stay in range, every v and w lies in 0 .. 1, and p lies in the face up to
 *         the rounding of its own sums.  Then  u = q - p,  d2 = (u_x u_x + u_y u_y) + u_z u_z.
 *         The degenerate path, region 7: for the segments (a, b), (b, c), (c, a) in this order, (p0, p1) with e = p1 - p0:  l = dot(e, e);
 *         t = dot(q - p0, e) / l if l > 0, else 0 (a segment of zero length is its end point);  t = 0 unless t > 0;  t = 1 if t > 1;
 *         s = p0 + t e;  its d2 as above.  The smallest d2 wins, the first segment on ties (a later one replaces only with <).
 *     (b) The result of a query is the lexicographically smallest (d2, f) over ALL faces f of the mesh, a face whose d2 is NaN left out (a
 *         brute-force definition: the grid is only how the kernel finds it), with p and the region of that face.  With max_dist finite the
 *         result stands only if d2 <= max_dist max_dist (one rounded product; NON-strict and on squares -- K24's gens_nearest_point takes the
 *         root and keeps d < max_dist, strictly, as the DTU script does; this one has no root to take).  Otherwise, and for a mesh without
 *         faces:  d2 = +inf,  face = -1,  p = (NaN, NaN, NaN),  region = 255.  A query with a coordinate that is not finite:  d2 = NaN and the
 *         same face, p and region.
 *   The walk.  The query's cell is floor((q - lo) (1 / cell)) per axis clamped into the grid (lo and cell widened from float32, as
 *     gens_mesh_grid_count computes a face's cells).  For r = 0, 1, 2, ... the cells at Chebyshev distance exactly r from it that lie in
 *     the grid are visited, none twice.  gens_mesh_grid_count lists a face in every cell its AABB overlaps, widened OUTWARDS by 1e-5 cell, so
 *     a face listed in no cell of the block [c - r, c + r]^3 lies wholly beyond one of the block's sides, by at least 1e-5 cell less the
 *     rounding of its cell coordinates (at most 512 x 4 x 2^-53 < 3e-13 cell); a face clamped into a border cell is listed there, so the
 *     sides on the grid's border have nothing beyond them.  bound = the smallest, over the block's sides that are not on the border, of
 *     max(s (1 - 2^-40) - 2^-30, 0) cells, s = the side's coordinate less the query's (or the reverse) in cells, times cell.  The margin
 *     covers the rounding of the query's cell coordinate ((|s| + 513) 4 x 2^-53 cells), of 1 / cell and of bound^2, and of d2: the p of
 *     the rule lies within 4 x 2^-53 x (the largest |coordinate| of the face) of the face, which is below 1e-5 cell while
 *     (|lo| + 512 cell) / cell < 2^32 -- checked, GENS_ELIMIT; ops.build_mesh_grid's boxes stay below 2^29.  The widening of the lists is
 *     therefore slack on top of the margin, not something the margin has to win back.  The walk stops after ring r when the best
 *     d2 < bound^2, STRICTLY: every unvisited face then has a larger d2, so none can win, and none can tie and win on its index -- with <=
 *     a face with an equal d2 and a smaller index, one ring further out, would change the answer.  It also stops when
 *     bound^2 > max_dist^2 (nothing unvisited can pass the cap) and when the block covers the grid: after at most max(nx, ny, nz) rings.
 *     A face listed in several cells is evaluated once per listing met; d2 is a pure function of (q, f), so that changes nothing.
 *   NOT promised: a sign, a distance to anything but the triangles as stored, a cost bound for queries far from every face (a query at the
 *     centre of a sphere reads every cell of the grid; a coarse level over the grid would bound that and is not built).
 *
 *   gens_mesh_closest_point: one thread per query.  grid: as ops.build_mesh_grid / gens_mesh_grid_{count,fill} make it (vertex indices
 *     < V are the caller's check, as for every user of the grid; face ids in cell_faces outside 0 .. n_faces - 1 and list bounds outside
 *     0 .. cell_start[cells] are skipped, never read through).  queries (n, 3) float64; dist2 (n) float64; face (n) int32; optional (NULL:
 *     not written) point (n, 3) float64 and region (n) uint8.  All device pointers.
 *   Arguments are checked before any launch.  GENS_EINVAL: a null grid; n_queries < 0; n_faces < 0; max_dist not > 0 (a NaN included; +inf:
 *     no cap); with n_queries > 0, null queries, dist2 or face; with faces too, a null pointer in the grid.  GENS_ELIMIT: n_queries or
 *     n_faces >= 2^31; a grid outside K23's limits (1 .. 512 cells per axis, a positive finite cell, a finite corner) or the ratio above.
 *     n_queries == 0 succeeds without a launch.  n_faces == 0 does not launch the walk: one fill writes the results of (b).
 *     The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_mesh_closest_point(const gens_mesh_grid* grid, const double* queries, int64_t n_queries, double max_dist, double* dist2,
                            int32_t* face, double* point /* (n, 3) or NULL */, uint8_t* region /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K37  The undirected edge table of a triangle mesh, its topology, Baerentzen-Aanaes pseudonormals and the sign of K36's distance
 *      (ops.mesh_topology, ops.signed_distance_to_mesh, ops.mesh_distance(signed=True), io.mesh_report, python -m gens_amd.mesh_report,
 *      ImplicitSurface.extract_geometry(topology=)), csrc/k37_mesh_topology.hip.  tests/mesh_topology_reference.py restates all of it in
 *      numpy with dicts and loops.  vertices (V, 3) float64, triangles (T, 3) int32; V < 2^31 and 3 T < 2^31.
 *
 *   Definitions.
 *     A face is VALID when its three indices lie in [0, V) and are pairwise distinct.  Other faces are counted and take part in nothing
 *       else.  A valid face of zero area takes part in the topology and contributes a zero normal.
 *     Half-edge h = 3 t + k runs from t[k] to t[(k + 1) % 3].  An EDGE is the unordered pair (lo, hi) of a valid face's half-edge; its id is
 *       its rank in ascending (lo, hi); its key is (lo << 32) | hi.  A CORNER is (t, k), id 3 t + k, at vertex t[k].
 *     The USES of an edge are its half-edges in ascending h -- what a stable sort of the keys leaves; the order is part of the rule.
 *     Edge class: 1 boundary (one use), 2 manifold (two uses, one lo -> hi and one hi -> lo), 3 flipped (two uses in the same direction),
 *       4 non-manifold (three or more uses).
 *     FANS.  For every edge of class 2 or 3 and each of its two endpoints v, the corners that the edge's two faces have at v are joined.
 *       The fans of a vertex are the resulting classes of its corners; a class is named by its smallest corner id.
 *     Vertex flag byte: bit 0 referenced (by a valid face), bit 1 on a class-1 edge, bit 2 on a class-4 edge, bit 3 on a class-3 edge,
 *       bit 4 fans > 1 (a pinch).  A vertex is MANIFOLD when bit 0 is set and bits 2 and 4 are clear.
 *     Normals, float64, every operation rounded on its own, dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z, cross as in K36:
 *       face: c = (b - a) x (c - a), l = sqrt(dot(c, c)); c / l per component where l > 0 and finite, else (0, 0, 0); (0, 0, 0) for a face
 *         that is not valid.
 *       edge: the sum of the face normals of its uses, in ascending h, starting from 0, per component.
 *       vertex: over its corners in ascending corner id, starting from 0: sum + angle * n_face per component, with u, v the edge vectors
 *         from the corner's vertex to the face's next and previous vertex, angle = atan2(sqrt(dot(u x v, u x v)), dot(u, v)); a corner
 *         whose angle is not finite is left out.  Neither sum is normalised.
 *     The sign of a K36 result (dist2, face, point, region) for the query q:  NaN unless face is in [0, T) and dist2 is finite and >= 0;
 *       +0 where dist2 == 0; otherwise n = the face normal (region 0), the vertex normal of t[face][region - 1] (regions 1 - 3; none if that
 *       vertex has any of the flag bits 1 - 4), the edge normal of edge_of_halfedge[3 face + region - 4] (regions 4 - 6; none unless that
 *       edge has class 2); s = dot(q - point, n); the result is sqrt(dist2) if s > 0, -sqrt(dist2) if s < 0, NaN where there is no n (region
 *       7 and 255 included) or s is 0 or NaN.  Positive is the side the face normals point to: the sign follows the mesh's own orientation.
 *       For a closed, oriented, manifold mesh the angle-weighted normal decides inside / outside exactly at every point of the surface
 *       (Baerentzen and Aanaes, Signed distance computation using the angle weighted pseudonormal, 2005).
 *
 *   gens_mesh_edge_keys: per half-edge, key (3 T) int64 and forward (3 T) uint8 (1: the half-edge runs lo -> hi).  Half-edges of faces that
 *     are not valid get the key INT64_MAX, which sorts last, and forward 0.
 *   gens_mesh_edge_classify: per edge.  edge_key (E) int64: the distinct keys in ascending order without INT64_MAX; seg_start (E + 1) int32:
 *     where each key's run begins in the sorted half-edges; order (3 T) int32: the half-edge ids in (stably) sorted order; forward: as
 *     above, indexed by half-edge.  Writes edges (E, 2) int32 (lo, hi), edge_count (E), edge_forward (E) (uses that run lo -> hi),
 *     edge_halfedges (E, 2) (the two smallest h, -1 where there is none), edge_class (E) uint8 and the inverse map edge_of_halfedge (3 T)
 *     int32 (first filled with -1: what half-edges of faces that are not valid keep).  Entries of order outside [0, 3 T) and run bounds
 *     outside [0, 3 T] are skipped / clamped, never read through.
 *   gens_mesh_fan_pairs: per edge, pairs (2 E, 2) int32: rows 2 e and 2 e + 1 hold, for an edge of class 2 or 3, the corner ids that the
 *     faces of its two smallest half-edges have at lo and at hi; (-1, -1) for other edges.  The rows go through gens_face_cc_hook /
 *     gens_face_cc_compress with 3 T nodes (ids below zero are skipped there); a root is the smallest corner id.
 *   gens_mesh_vertex_classify: per vertex.  corner_order (3 T') int32: the corner ids of valid faces stably sorted by their vertex (the
 *     caller may pad it to 3 T entries; only [corner_start[0], corner_start[V]) is read); corner_start (V + 1) int32; corner_label (3 T) from
 *     the compress launch.  Writes valence (V) int32, fans (V) int32 (the number of corners of the vertex that are their own label) and
 *     flags (V) uint8.  n_halfedges is 3 T; ids outside their ranges are skipped.
 *   gens_mesh_pseudonormals: three launches -- faces, then edges and vertices, which read the face normals.  face_normal (T, 3),
 *     edge_normal (E, 3), vertex_normal (V, 3) float64.  One thread walks one segment in order: no atomics, deterministic.
 *   gens_mesh_distance_sign: per query, signed (n) float64 by the rule above.  queries (n, 3), dist2 (n), face (n), point (n, 3),
 *     region (n) as gens_mesh_closest_point wrote them.
 *   Arguments are checked before any launch.  GENS_EINVAL: a negative count; more edges than half-edges; a half-edge count that is no
 *     multiple of 3; a null pointer that the given counts would have the launch read or write.  GENS_ELIMIT: V, 3 T or n_queries >= 2^31.
 *     Counts of zero succeed without the launch they would size.  The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_mesh_edge_keys(const int32_t* triangles, int64_t n_faces, int64_t n_vertices, int64_t* key, uint8_t* forward, void* stream);
int gens_mesh_edge_classify(const int64_t* edge_key, const int32_t* seg_start, const int32_t* order, const uint8_t* forward, int64_t n_edges,
                            int64_t n_halfedges, int32_t* edges, int32_t* edge_count, int32_t* edge_forward, int32_t* edge_halfedges,
                            uint8_t* edge_class, int32_t* edge_of_halfedge, void* stream);
int gens_mesh_fan_pairs(const int32_t* triangles, int64_t n_faces, const int32_t* edges, const int32_t* edge_halfedges,
                        const uint8_t* edge_class, int64_t n_edges, int32_t* pairs, void* stream);
int gens_mesh_vertex_classify(const int32_t* corner_order, const int32_t* corner_start, const int32_t* corner_label,
                              const int32_t* edge_of_halfedge, const uint8_t* edge_class, int64_t n_vertices, int64_t n_halfedges,
                              int64_t n_edges, int32_t* valence, int32_t* fans, uint8_t* flags, void* stream);
int gens_mesh_pseudonormals(const double* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_faces, int64_t n_edges,
                            const int32_t* seg_start, const int32_t* order, const int32_t* corner_start, const int32_t* corner_order,
                            double* face_normal, double* edge_normal, double* vertex_normal, void* stream);
int gens_mesh_distance_sign(const double* queries, int64_t n_queries, const double* dist2, const int32_t* face, const double* point,
                            const uint8_t* region, const int32_t* triangles, int64_t n_faces, int64_t n_vertices, int64_t n_edges,
                            const double* face_normal, const double* edge_normal, const double* vertex_normal,
                            const int32_t* edge_of_halfedge, const uint8_t* edge_class, const uint8_t* vertex_flags, double* signed_out,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K38  Mesh repair: drop invalid and duplicate faces, split pinches and non-manifold edges, drop small components, re-orient, close small
 *      holes (ops.repair_mesh, io.repair_mesh, python -m gens_amd.repair_mesh, ImplicitSurface.extract_geometry(repair=)),
 *      csrc/k38_mesh_repair.hip.  tests/mesh_repair_reference.py restates all of it in numpy with dicts and loops.  vertices (V, 3) float64,
 *      triangles (T, 3) int32; V < 2^31 and 3 T < 2^31.  VALID, half-edge, corner, edge class, fan, face component: K37's definitions.
 *
 *   The stages, in this order.  Each is an option; every one is deterministic (no float atomics, nothing depends on launch order).
 *     a. DEDUPE.  Faces that are not VALID are dropped (always: a face with an index outside the vertices has no place in the result).  With
 *        the option on, among valid faces with the same vertex SET, in any winding, the one with the smallest face id survives.  The
 *        survivors keep their order.
 *     b. SPLIT.  Take K37's topology of the surviving faces.  Every referenced vertex v with fans[v] = k becomes k vertices at v's position,
 *        one per fan; a corner takes the copy of its fan.  New ids: the original vertices in ascending id, within a vertex its fans in
 *        ascending label (the smallest corner id).  Unreferenced vertices are dropped.  Off: vertices and indices stay as they are.
 *        ONE ROUND SUFFICES (the bound on rounds is 1).  Proof.  Fans join only across edges of class 2 and 3, which have exactly two uses,
 *        so around a vertex a every face of a fan is joined to at most one other face across each of its two edges at a: a fan is a path or
 *        a cycle of faces.  (i) An edge (a, b) of class 2 or 3 joins its two faces' corners at a and at b, so both uses name the same pair of
 *        copies: the edge survives with its two uses and its class.  (ii) A use of an edge (a, b) of class 1 or 4 is an edge across which
 *        nothing is joined, so within its fan at a its face is an END of a path; a path has two ends, so at most two uses of (a, b) name the
 *        copy a' of that fan, and no edge at a' has more than two uses: no class-4 edge is left.  (iii) The corners at a copy a' are those
 *        of one old fan, and the class-2 and class-3 edges that joined them survive by (i), so a' has one fan: no pinch is left.  Two uses
 *        that pair up on a new edge by (ii) lie in one fan, hence were already in one face component: the components do not change.
 *     c. SMALL COMPONENTS (min_component_faces = m, 0 = off).  In K37's topology of the split mesh, faces whose face_component has fewer
 *        than m faces are dropped, and with them the vertices no face refers to any more; both keep their order.
 *     d. ORIENT.  A union-find on 2 T' nodes, node 2 f + s.  An edge of class 2 with the faces fa, fb of its two half-edges joins (fa, 0) -
 *        (fb, 0) and (fa, 1) - (fb, 1); an edge of class 3 joins (fa, 0) - (fb, 1) and (fa, 1) - (fb, 0).  Labels are smallest members.  A
 *        component is NON-ORIENTABLE where label(f, 0) == label(f, 1): its faces are left alone and it is counted.  Otherwise the faces
 *        with label(f, 0) < label(f, 1) are the side of the component's smallest face, min(label(f, 0), label(f, 1)) / 2.  The side with more
 *        faces keeps its winding; on a tie the smallest face's side does.  Every face of the other side becomes (a, c, b).  The sides are
 *        counted by sort and search.
 *     e. FILL (max_hole_edges = n, 0 = off; needs b and d).  In K37's topology of the oriented mesh every boundary vertex has exactly two
 *        class-1 edges, so the union of the class-1 edges over the vertices gives the loops, named by their smallest vertex.  A loop of
 *        3 <= length <= n edges is closed, unless one of its edges belongs to a face of a non-orientable component or all of them belong to
 *        one face (a lone triangle: its closing face would have that face's vertex set, which (a) drops from a second pass).  The boundary half-edge
 *        a -> b of a closed loop gets the face (b, a, c): c is a new vertex at the loop's centroid -- the float64 sum of the loop's vertices
 *        in ascending vertex id, starting from 0, per component, then divided by their number -- or, for a loop of 3, the loop's third
 *        vertex, and then only the loop's smallest boundary half-edge gets a face.  New faces follow the kept faces in ascending boundary
 *        half-edge id, new vertices follow the kept vertices in ascending loop name.  Longer loops stay open.  A centroid fan over a
 *        strongly non-planar loop can intersect itself or the mesh; that is not detected.
 *     Results: vertices' (V', 3) float64, kept ones bit-identical to their sources; triangles' (T', 3) int32; vertex_source (V') int32, the
 *       original vertex or -1 for a centroid; face_source (T') int32, the original face or -1 for a fill face; face_flipped (T') bool.
 *
 *   gens_mesh_face_keys: per face, key_major (T) int64 = the smallest index and key_minor (T) int64 = (middle << 32) | largest; both
 *     INT64_MAX for a face that is not valid.  Two stable sorts (minor, then major) leave equal triples adjacent in ascending face id.
 *   gens_mesh_split_corners: per vertex, one thread walks the vertex's corners (corner_order, corner_start, corner_label as in
 *     gens_mesh_vertex_classify) in ascending corner id.  vertex_base (V) int32: the exclusive prefix sum of K37's fans.  A corner that is
 *     its own label is the r-th root of the walk: new_corner[c] = vertex_base[v] + r and vertex_source[that] = v; another corner takes
 *     new_corner[label], which the same thread wrote before.  new_corner (3 T) int32 is first filled with -1, what corners of faces that
 *     are not valid keep; vertex_source (n_new) int32.  A root whose id would reach n_new is skipped.
 *   gens_mesh_orient_pairs: per edge, pairs (2 E, 2) int32: the two joins of (d) for an edge of class 2 or 3, with fa, fb the faces of
 *     edge_halfedges' two entries; (-1, -1) for other edges.  The rows go through gens_face_cc_hook / gens_face_cc_compress with 2 T nodes.
 *   gens_mesh_apply_flips: per face, out = (a, c, b) where flip (T) uint8 is not zero, else (a, b, c).
 *   gens_mesh_loop_centroids: per loop, one thread walks loop_vertices [loop_start[l], loop_start[l + 1]) -- the n_rim boundary vertices
 *     sorted by loop name, then id -- and writes the centroid to row loop_slot[l] of centroids (n_centroids, 3) float64; a slot outside
 *     [0, n_centroids) writes nothing.
 *   gens_mesh_fill_emit: per boundary half-edge.  rim_halfedges (n_rim) int32 in ascending order; rim_slot (n_rim) int32: the row of faces
 *     (n_fill, 3) int32 to write, outside [0, n_fill) for none; loop_of_vertex (V) int32: the loop's rank, -1 off the boundary; loop_apex
 *     (n_loops) int32: the id of the loop's centroid vertex, below zero for a loop of three, whose third vertex is found by a walk of the
 *     loop's segment.  A row that cannot be formed (an id outside its range) is written as (-1, -1, -1).
 *   Arguments are checked before any launch.  GENS_EINVAL: a negative count; more edges than half-edges, more new vertices than
 *     half-edges, more loops than rim vertices, more centroids than loops, more rim half-edges than vertices or than half-edges, more fill
 *     faces than rim half-edges; a half-edge count that is no multiple of 3; a null pointer that the given counts would have the launch
 *     read or write.  GENS_ELIMIT: V or 3 T >= 2^31.  Counts of zero succeed without the launch they would size.  Ids outside their
 *     ranges are skipped, never read through.  The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_mesh_face_keys(const int32_t* triangles, int64_t n_faces, int64_t n_vertices, int64_t* key_major, int64_t* key_minor, void* stream);
int gens_mesh_split_corners(const int32_t* corner_order, const int32_t* corner_start, const int32_t* corner_label, const int32_t* vertex_base,
                            int64_t n_vertices, int64_t n_halfedges, int64_t n_new, int32_t* new_corner, int32_t* vertex_source, void* stream);
int gens_mesh_orient_pairs(const int32_t* edge_halfedges, const uint8_t* edge_class, int64_t n_edges, int64_t n_faces, int32_t* pairs,
                           void* stream);
int gens_mesh_apply_flips(const int32_t* triangles, const uint8_t* flip, int64_t n_faces, int32_t* out, void* stream);
int gens_mesh_loop_centroids(const double* vertices, int64_t n_vertices, const int32_t* loop_start, const int32_t* loop_vertices,
                             int64_t n_loops, int64_t n_rim, const int32_t* loop_slot, int64_t n_centroids, double* centroids, void* stream);
int gens_mesh_fill_emit(const int32_t* triangles, int64_t n_faces, int64_t n_vertices, const int32_t* rim_halfedges, const int32_t* rim_slot,
                        int64_t n_rim, const int32_t* loop_of_vertex, const int32_t* loop_start, const int32_t* loop_vertices,
                        const int32_t* loop_apex, int64_t n_loops, int64_t n_fill, int32_t* faces, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K39  Mesh fairing: Laplacian and Taubin smoothing with uniform or cotangent weights, the vertex Laplacian and the dihedral roughness of
 *      the edges (ops.smooth_mesh, ops.mesh_laplacian, ops.mesh_roughness, ops.smoothing_weights, io.smooth_mesh,
 *      python -m gens_amd.smooth_mesh, python -m gens_amd.mesh_report --roughness, ImplicitSurface.extract_geometry(smooth=)),
 *      csrc/k39_mesh_fairing.hip.  tests/mesh_smooth_reference.py restates all of it in numpy with dicts and loops.  vertices (V, 3)
 *      float64, triangles (T, 3) int32 and K37's table of that mesh (E edges); V < 2^31 and 3 T < 2^31.  VALID, half-edge, edge, edge
 *      class, uses, vertex flags, face normals: K37's definitions.  float64; every operation is rounded on its own, in the order written.
 *
 *   Definitions.
 *     1. NEIGHBOURS.  N(i) = the other ends of the edges of K37's table that end at i, every class, each edge once however many faces use
 *        it, in ascending vertex index: nbr_start (V + 1) int32, nbr_vertex (2 E) int32, nbr_edge (2 E) int32 (the edge's id).  One sort
 *        of the 2 E keys (from << 32) | to gives all three.
 *     2. WEIGHTS, per edge, from the input positions, kept through all iterations.  "uniform": w_e = 1.  "cotangent": for a valid face t and
 *        k = 0, 1, 2 let P = t[(k + 2) % 3] (the corner opposite half-edge h = 3 t + k), Q = t[k], R = t[(k + 1) % 3]; u = Q - P, v = R - P;
 *        d = (u_x v_x + u_y v_y) + u_z v_z; n = u x v (K36's cross); l = sqrt((n_x^2 + n_y^2) + n_z^2); cot_h = d / l if l > 0 and the
 *        quotient is finite, else 0; 0 for half-edges of faces that are not valid.  w_e = the sum of cot_h over the edge's uses in
 *        ascending h, starting from 0; then w_e = 0 unless w_e > 0 (negatives and NaN are clamped, which keeps every step a convex
 *        combination of the vertex and its neighbours for a factor in (0, 1]).
 *     3. LAPLACIAN of vertex i.  S = (0, 0, 0), W = 0; for j in N(i) in order: W = W + w_ij; S_a = S_a + w_ij (p_j,a - p_i,a).
 *        delta_i,a = S_a / W if W > 0 and W is finite, else 0.
 *     4. STEP with factor f.  q_i,a = p_i,a + f delta_i,a.  q_i = p_i, bit for bit, for a pinned vertex and for a vertex whose delta is 0 by
 *        the "else" of (3) (no neighbours, or no positive weight: p + f 0 would turn a -0.0 into +0.0, and such a vertex is promised not to
 *        move).  A step reads one buffer and writes another.
 *     5. PINNED: the caller's mask, if any; with fix_boundary every vertex with K37's flag bit 1 (on a class-1 edge).  Unreferenced
 *        vertices have no neighbours and never move.
 *     6. SMOOTH (n, lambda, mu): n times a step with f = lambda, then, unless mu == 0, a step with f = mu.  mu == 0 is plain Laplacian
 *        smoothing; lambda in (0, 1], mu in [-2, -lambda) is Taubin's (A signal processing approach to fair surface design, 1995).  n = 0
 *        returns a copy.  The triangles are untouched.
 *     7. DIHEDRAL ROUGHNESS per edge: for an edge of class 2 whose two uses' face normals n1, n2 (K37's unit normals) both have a non-zero
 *        component, theta_e = atan2(sqrt(dot(c, c)), dot(n1, n2)) with c = n1 x n2 and K37's dot; NaN for every other edge.
 *     Not here: re-projection onto the SDF's zero set, weights recomputed per iteration, implicit fairing, feature detection, volume
 *     rescaling.
 *
 *   gens_mesh_corner_cot: per half-edge, cot (3 T) float64 by (2).
 *   gens_mesh_edge_weights: per edge, one thread walks the edge's run [edge_start[e], edge_start[e + 1]) of halfedge_order (3 T) int32 --
 *     K37's seg_start and order, the half-edges stably sorted by edge key -- and writes weight (E) float64 by (2).
 *   gens_mesh_laplacian_step: per vertex, one thread walks [nbr_start[i], nbr_start[i + 1]) in order.  weight (E) float64 or NULL for
 *     uniform; pinned (V) uint8 or NULL; n_neighbours = 2 E.  Writes out (V, 3) by (4) and, where given, delta (V, 3) by (3) and
 *     weight_sum (V) (W); each of the three may be NULL, not all.  No atomics: deterministic.  None of the three may be `in` (neighbours
 *     read it), and no two of them may be the same buffer; overlaps other than equal pointers are the caller's to avoid.
 *   gens_mesh_dihedral: per edge, angle (E) float64 by (7) from K37's face_normal (T, 3), edge_halfedges (E, 2), edge_class (E).
 *   Arguments are checked before any launch.  GENS_EINVAL: a negative count; more edges than half-edges; a half-edge count that is no
 *     multiple of 3; n_neighbours != 2 E; a factor outside [-2, 1] or NaN; an output equal to `in` or to another output; no output; a null pointer that the given counts would
 *     have the launch read or write.  GENS_ELIMIT: V, 3 T or 2 E >= 2^31.  Counts of zero succeed without a launch.  Ids outside their
 *     ranges are skipped, never read through.  The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_mesh_corner_cot(const double* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_faces, double* cot, void* stream);
int gens_mesh_edge_weights(const double* cot, const int32_t* edge_start, const int32_t* halfedge_order, int64_t n_edges, int64_t n_halfedges,
                           double* weight, void* stream);
int gens_mesh_laplacian_step(const double* in, int64_t n_vertices, const int32_t* nbr_start, const int32_t* nbr_vertex, const int32_t* nbr_edge,
                             int64_t n_neighbours, const double* weight /* (E) or NULL */, int64_t n_edges, const uint8_t* pinned /* or NULL */,
                             double factor, double* out /* (V, 3) or NULL */, double* delta /* (V, 3) or NULL */,
                             double* weight_sum /* (V) or NULL */, void* stream);
int gens_mesh_dihedral(const double* face_normal, int64_t n_faces, const int32_t* edge_halfedges, const uint8_t* edge_class, int64_t n_edges,
                       double* angle, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K40  Generalised winding numbers (Jacobson, Kavan, Sorkine-Hornung: Robust inside-outside segmentation using generalized winding
 *      numbers, 2013), exact and with a far field over clusters (after Barill et al.: Fast winding numbers for soups and clouds, 2018,
 *      first order only): an inside test that needs no connectivity (ops.build_winding_plan, ops.winding_number, ops.mesh_inside,
 *      ops.signed_distance_to_mesh(sign="winding"), ops.mesh_distance(sign="winding"), io.compare_meshes(sign=),
 *      python -m gens_amd.compare_meshes --signed --sign winding), csrc/k40_mesh_winding.hip.  tests/winding_reference.py restates all of
 *      it in numpy.  vertices (V, 3) float64, triangles (T, 3) int32; V < 2^31 and 3 T < 2^31.  VALID: K37's rule (three different
 *      indices, all in [0, V)).  float64; every operation is rounded on its own, in the order written; dot(u, v) = (u_x v_x + u_y v_y) +
 *      u_z v_z, |u| = sqrt(dot(u, u)), cross as in K36.
 *
 *   Definitions.
 *     1. SOLID ANGLE of a valid face (a, b, c) at the query q (Van Oosterom and Strackee, 1983): A = a - q, B = b - q, C = c - q;
 *        num = dot(A, B x C); den = (((|A| |B|) |C| + dot(A, B) |C|) + dot(B, C) |A|) + dot(C, A) |B|; Omega = 2 atan2(num, den).  A face
 *        that is not valid adds nothing.  A query on a vertex or in the plane of a face gets what the formula gives, which is finite
 *        (atan2(+-0, x) is +-0 or +-pi): on a face the face counts as 0, or as +-2 pi where den < 0 -- half of the jump across it --; nothing
 *        is special-cased.
 *     2. w(q) = (the sum of Omega over the faces) / (4 pi): 1 inside a closed mesh whose normals point outwards, 0 outside, -1 inside an
 *        inside-out mesh (which therefore reads as "outside everywhere": repair_mesh re-orients), k where k sheets enclose q, a smooth
 *        fraction near a hole.  NaN for a query with a coordinate that is not finite.
 *     3. PLAN ORDER.  face_order (T) int32: the faces stably sorted by the Morton key of their centroid ((a + b) + c) / 3 -- 10 bits per
 *        axis over the bounding box of the valid faces' centroids, x the most significant of each triple; faces that are not valid last --
 *        ties by face index.  LEAF l = the faces at positions 64 l .. 64 l + 63 of that order, NODE k = the leaves 64 k .. 64 k + 63.  Any
 *        permutation of the faces is a correct plan (the order only decides how tight the clusters are); the kernels take it as given.
 *     4. MOMENTS of a leaf, over its valid faces in position order, sums starting from 0: with n_f = (b - a) x (c - a), a_f = 0.5 |n_f|,
 *        g_f = ((a + b) + c) / 3:  count; area = sum a_f; normal = sum 0.5 n_f; S = sum a_f g_f; M = sum g_f; centre p = S / area if
 *        area > 0, else M / count; radius2 = max over the faces' corners v of dot(v - p, v - p).  A leaf with count 0 is EMPTY: zeros, and
 *        it is skipped everywhere.  Of a node, over its leaves that are not empty in order: count = sum count_l; area = sum area_l;
 *        normal = sum normal_l; S = sum area_l p_l; M = sum count_l p_l; p as above; r = max (|p_l - p| + sqrt(radius2_l)), which is no
 *        smaller than the distance from p to any corner; radius2 = r r.
 *     5. FAR FIELD of a cluster (leaf or node) with area, normal N, centre p, radius2 for the query q and beta2 = beta beta:
 *        D = p - q, d2 = dot(D, D).  The cluster is ACCEPTED if d2 > beta2 radius2.  Then d = sqrt(d2), r = sqrt(radius2) and it stands for
 *        the solid angle  dot(N, D) / (d2 d)  with an error of at most  err = (area r) / (2 pi ((g g) g)), g = d - r, in units of w:
 *        w is the integral of g(y - q) . n over the surface with g(y) = y / (4 pi |y|^3), whose Jacobian I / (4 pi |y|^3) - 3 y y^T /
 *        (4 pi |y|^5) has eigenvalues 1 / (4 pi |y|^3) (twice) and -2 / (4 pi |y|^3), so an operator norm of 1 / (2 pi |y|^3); every
 *        point y of the cluster is within r of p and at least d - r from q, so |g(y - q) - g(p - q)| <= r / (2 pi (d - r)^3), and the
 *        integral of that over the cluster's area is err.  (The dipole replaces g(y - q) by g(p - q) and the integral of n is N.)
 *     6. TRAVERSAL.  total = 0, bound = 0.  For each node k that is not empty, in order: if beta > 0 and the node is accepted: part = its
 *        dipole, bound = bound + err.  Else part = 0 and for each of its leaves l that is not empty, in order: if beta > 0 and the leaf is
 *        accepted: leaf = its dipole, bound = bound + err; else leaf = 0 and, for its faces in position order, leaf = leaf + Omega;
 *        then part = part + leaf.  Then total = total + part.  w = total / (4 pi).  beta = 0 accepts nothing: the exact sum, in this
 *        tree's order, and bound = 0.  |w(beta) - w(0)| <= bound up to rounding.  The tree is fixed and a query's sums are its own: its
 *        bits do not depend on the other queries of the call, their number, or the run.
 *     Not here: expansion terms beyond the dipole, a deeper tree, sorting the queries, splitting one query's nodes over workgroups,
 *     orientation guessing, self-intersection tests, voxelisation.
 *
 *   gens_winding_plan: the mesh (read by gens_mesh_winding_moments only), face_order, and what the moments launch writes and the query
 *     reads: corners (64 L, 9) float64 -- a, b, c of the face at each position, NINE ZEROS for a face that is not valid or a position
 *     past T (the solid angle of such a triple is +-0 at every query: it adds nothing) --, and per leaf (L = ceil(T / 64)) and per node
 *     (K = ceil(L / 64)) count int32, area, normal (, 3), centre (, 3), radius2 float64.
 *   gens_mesh_winding_moments: one thread per leaf, then one per node (4).  Indices in face_order and triangles outside their ranges
 *     make the face not valid; they are never read through.
 *   gens_mesh_winding_number: one query per lane; queries (n, 3) float64 -> w (n) and, unless NULL, bound (n) (NaN where w is).
 *     beta = 0: exact; else a finite number > 1 (so that d > r in (5)).  Reads the plan's corners and moments only.
 *   Arguments are checked before any launch.  GENS_EINVAL: a null plan; a negative count; leaf or node counts that are not the ceilings
 *     above; beta that is neither 0 nor a finite number > 1; two of queries, w, bound equal; a null pointer that the counts would have a
 *     launch read or write.  GENS_ELIMIT: V, 3 T or n >= 2^31.  T = 0: moments launch nothing, the query writes 0 (NaN).  n = 0 succeeds
 *     without a launch.  The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const double* vertices;      /* (V, 3) */
    const int32_t* triangles;    /* (T, 3) */
    const int32_t* face_order;   /* (T) */
    double* corners;             /* (64 L, 9) */
    int32_t* leaf_count;         /* (L) */
    double *leaf_area, *leaf_normal, *leaf_centre, *leaf_radius2;      /* (L), (L, 3), (L, 3), (L) */
    int32_t* node_count;         /* (K) */
    double *node_area, *node_normal, *node_centre, *node_radius2;      /* (K), (K, 3), (K, 3), (K) */
    int64_t n_vertices, n_faces, n_leaves, n_nodes;
} gens_winding_plan;
int gens_mesh_winding_moments(const gens_winding_plan* plan, void* stream);
int gens_mesh_winding_number(const gens_winding_plan* plan, const double* queries, int64_t n_queries, double beta, double* w,
                             double* bound /* (n) or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K41  Self-intersections of a triangle mesh: which pairs of its faces intersect, decided exactly or not at all
 *      (ops.mesh_self_intersections, io.mesh_report(self_intersections=True), python -m gens_amd.mesh_report --self-intersections,
 *      ImplicitSurface.extract_geometry(self_intersections=True)), csrc/k41_mesh_intersect.hip.  tests/mesh_intersect_reference.py decides
 *      the same question in rational arithmetic from the set definition.  A report only: nothing is removed or repaired.
 *      vertices (V, 3) float64, triangles (T, 3) int32; V < 2^31 and 3 T < 2^31.  VALID: K37's rule (three different indices, all in [0, V)).
 *
 *   Definitions, in exact real arithmetic on the float64 coordinates.  A face is the closed convex hull of its three corner positions.
 *     1. A valid face (a, b, c) is DEGENERATE when (b - a) x (c - a) is exactly the zero vector.  Degenerate faces are counted and take
 *        part in no pair (marching cubes emits them).
 *     2. The AABB of a face is the component-wise min / max of its corners (exact in float64).  A CANDIDATE is a pair s < t of valid faces
 *        that are not degenerate, share k < 3 vertex INDICES, and whose closed AABBs overlap (<= on all three axes).  A pair with k = 3 is a
 *        duplicate in K38's sense: counted (duplicate_pairs), not a candidate.  Sharing is by index only: two unwelded vertices at one
 *        position are not shared, and faces touching there intersect.
 *     3. A candidate pair INTERSECTS iff: k = 0: Ts and Tt have a common point; k = 1 (vertex v): they have a common point other than v's
 *        position; k = 2 (edge e): they have a common point that is not on the segment e (a flat fold).
 *     4. PREDICATE FORM, what the kernel evaluates (derived in DESIGN.md, section 5r).  orient3d(a, b, c, d) = det [a - d; b - d; c - d]
 *        = (a_z - d_z) ((b_x - d_x)(c_y - d_y) - (c_x - d_x)(b_y - d_y)) + (b_z - d_z) ((c_x - d_x)(a_y - d_y) - (a_x - d_x)(c_y - d_y))
 *        + (c_z - d_z) ((a_x - d_x)(b_y - d_y) - (b_x - d_x)(a_y - d_y)); orient2d(p, q, r) = (p_u - r_u)(q_v - r_v) - (p_v - r_v)(q_u - r_u).
 *        k = 0: some edge of one face meets the other closed face (6 segment-face tests: the 6 plane sides orient3d(face, corner) and the
 *               9 edge-edge values orient3d(s_i, s_i+1, t_j, t_j+1), each used by both directions -- all 15 four-subsets of the six corners).
 *        k = 1: with Ts = (v, a, b), Tt = (v, c, d): segment ab meets Tt or segment cd meets Ts.
 *        k = 2: with e = ab and the opposite corners c, d: orient3d(a, b, c, d) = 0 and ((b - a) x (c - a)) . ((b - a) x (d - a)) > 0.
 *        A closed segment pq meets a face (a, b, c) that is not degenerate: the plane signs of p and q (orient3d(a, b, c, .)) strictly
 *        equal: no.  Opposite, or exactly one zero: yes iff orient3d(p, q, a, b), orient3d(p, q, b, c), orient3d(p, q, c, a) are all >= 0
 *        or all <= 0.  Both zero: in two dimensions, after dropping the first axis whose component of (b - a) x (c - a) is certainly not
 *        zero: an end of pq in the closed face (three orient2d against the face's own orientation), or pq meets an edge (two closed
 *        segments meet iff neither has both ends strictly on one side of the other; four zeros: on one line, they meet iff their boxes
 *        do -- exact coordinate comparisons).
 *     5. CERTIFIED SIGNS.  Every predicate returns -, 0, + or ?.  It is evaluated in float64, every operation rounded once (the file is
 *        built without contraction), as a tree of height h: h = 3 for orient2d (difference, product, difference), h = 6 for orient3d and
 *        the k = 2 dot product (difference, product, difference, product, sum, sum).  By induction over the tree |computed - exact| <=
 *        ((1 + e)^h - 1) P, e = 2^-53, P = the tree with every operation replaced by the sum of absolute values (the permanent), and the
 *        permanent as computed is >= (1 - e)^h P, so |computed - exact| <= c e P~ with c = h + 1: c = 4 for orient2d, 7 for the two others,
 *        taken as 8.  |value| > c 2^-53 P~ (and |value| > 2^-600, P~ finite: no underflow or overflow can have voided the bound, given (6))
 *        gives the sign.  Otherwise the predicate is evaluated again with error-free transformations -- two_sum for each difference and sum,
 *        fma for each product's tail, a product that is not 0 and below 2^-900 counting as inexact --: if every operation was exact the
 *        value is the exact one and its sign (0 included) is returned; else ?.  There is no expansion-arithmetic fallback.
 *        A pair whose decision needs a ? is UNDECIDED; the decision does not wait for predicates it does not need: one face strictly on
 *        one side of the other's plane (for k = 1: its two other corners) decides DISJOINT alone; for k = 2 a dot product that is
 *        certainly <= 0 decides DISJOINT whatever orient3d says, and a certainly non-zero orient3d whatever the dot product says; a
 *        segment whose ends are strictly on one side meets nothing; three edge signs of which two certainly differ say no as soon as one
 *        end of the segment is certainly off the plane.
 *     6. A valid face whose degeneracy cannot be certified -- some component of (b - a) x (c - a) is ?, and none is certainly non-zero --
 *        is UNCERTAIN; so is a valid face with a coordinate that is not finite or beyond 2^100 in magnitude.  It is counted, it is
 *        treated as not degenerate in (2), and all its candidate pairs are UNDECIDED.
 *     7. The first face of a pair in (4) is the one whose index row (i0, i1, i2) is lexicographically smaller, not the one with the
 *        smaller face number: a pair's verdict does not depend on how the faces are numbered.
 *   Broad phase over K23's gens_mesh_grid as ops.build_mesh_grid builds it: a candidate is processed in exactly one cell, the one that
 *     holds the lower corner of the intersection of the two AABBs: per axis max(i0_s, i0_t) with i0 = gens_mesh_grid_count's
 *     clamp(floor((min - lo) / cell - 1e-5)) evaluated by the same float64 expression on the same float32 box.  That expression is
 *     monotone in the coordinate, and the upper index i1 uses + 1e-5: min_s <= max_t gives i0_s <= i1_t, so the cell lies in both faces'
 *     ranges, i.e. in both lists, and no other cell claims the pair: exactly once, without atomics.
 *
 *   gens_mesh_isect_faces: one thread per face -> face_class (T) uint8: 0 not valid, 1 ordinary, 2 degenerate, 3 uncertain; face_box
 *     (T, 6) float64: min x, y, z, max x, y, z (zeros for a face that is not valid).
 *   gens_mesh_isect_count: one lane per entry of the cell lists (n_entries = cell_start[cells]); the lane of (cell, position x) walks the
 *     positions y > x of its cell, 128 per workgroup row (gridDim.y = ceil(longest_list / 128), at most 65535; rows stride over the
 *     rest), so a long list is spread over its entries' lanes and over workgroups.  ACCUMULATES into: cell_counts (cells, 2) int32: the
 *     pairs the cell will emit, intersecting and undecided; totals (3) int64: candidates, duplicate pairs, candidates decided DISJOINT
 *     by one strict plane separation alone; face_flags (4 ceil(T / 4)) uint8, 4-byte aligned (integer atomicOr on its words): bit 0 for a
 *     face of an intersecting pair, bit 1 of an undecided one.  face_class and face_box: gens_mesh_isect_faces' of the same mesh.
 *   gens_mesh_isect_emit: the same walk; pairs (n_out, 2) int32 (s < t) and kinds (n_out) uint8 (1 intersecting, 2 undecided) at
 *     out_start[cell] + a ticket from cursor[cell]; out_start (cells + 1) int32 = the exclusive scan of cell_counts' row sums, cursor
 *     (cells) int32 zero-filled, n_out = out_start[cells].  The order inside a cell is not defined: the op sorts by (s << 32) | t.
 *   Arguments are checked before any launch.  GENS_EINVAL: a null pointer that a launch would read or write, a negative size, face_flags
 *     or totals misaligned.  GENS_ELIMIT: V, 3 T, n_entries or n_out >= 2^31; a grid outside K23's limits.  T = 0, n_entries = 0 (and
 *     n_out = 0 for emit) succeed without a launch.  Indices in cell_faces and triangles outside their ranges are skipped, never read
 *     through.  The ABI version stays 12: no existing entry changes.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_mesh_isect_faces(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_faces, uint8_t* face_class,
                          double* face_box, void* stream);
int gens_mesh_isect_count(const gens_mesh_grid* grid, int64_t n_vertices, int64_t n_entries, int64_t longest_list, const uint8_t* face_class,
                          const double* face_box, int32_t* cell_counts, int64_t* totals, uint8_t* face_flags, void* stream);
int gens_mesh_isect_emit(const gens_mesh_grid* grid, int64_t n_vertices, int64_t n_entries, int64_t longest_list, const uint8_t* face_class,
                         const double* face_box, const int32_t* out_start, int32_t* cursor, int64_t n_out, int32_t* pairs, uint8_t* kinds,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K14  C (m x n) = A^T B for tall row-major operands A (k x m), B (k x n), k >> m, n: the weight-gradient product of the training
 *      step (dW = dY^T X, what aten::mm computes inside torch.nn.functional.linear's backward; the reference reaches it through
 *      autograd from sdf_network.py:98-123 and blending_network.py:69-118).  Exact float32 (fp32 MFMA), K split into slabs whose
 *      partial results are added in a fixed order (deterministic).  workspace: gens_gemm_tn_slabs(k, m, n) * m * n floats.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_gemm_tn_slabs(int64_t k, int m, int n);
int gens_gemm_tn(const float* a, const float* b, int64_t k, int m, int n, float* workspace, float* c, void* stream);
/* Up to 12 products C_p (m_p x n_p) = A_p^T B_p over the same k rows in one launch; A_p / B_p are column blocks of row-major buffers
 * with leading dimensions lda[p] / ldb[p] (HOST arrays of device pointers / ints).  c: the C_p concatenated (row major each).
 * workspace: gens_gemm_tn_batch_workspace(count, m, n, k) floats.  Partial sums are added in a fixed order (deterministic). */
int64_t gens_gemm_tn_batch_workspace(int count, const int* m, const int* n, int64_t k);
int gens_gemm_tn_batch(int count, const float* const* a, const int* lda, const float* const* b, const int* ldb, const int* m,
                       const int* n, int64_t k, float* workspace, float* c, void* stream);
/* The same with the number of rows that EXIST left on the device: only the first min(k, k_rows ceil(*k_live / k_div)) rows of the
 * operands are read -- *k_live work items of the producer, k_div of which share a workgroup that wrote k_rows rows (gens_sdf_train_bwd:
 * 32 points -> 128 rows; gens_blend_train_bwd: floor(32 / S) points -> 32 rows) under a device-side point count. */
int gens_gemm_tn_batch_live(int count, const float* const* a, const int* lda, const float* const* b, const int* ldb, const int* m,
                            const int* n, int64_t k, const int32_t* k_live, int k_div, int k_rows, float* workspace, float* c,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K15  the 3 x 3 x 3 convolutions of the cost-volume U-Net (reg_network.py:7-50: nn.Conv3d(k=3, padding=1, stride 1 | 2) and
 *      nn.ConvTranspose3d(k=3, stride=2, padding=1, output_padding=1), i.e. aten::convolution / convolution_backward as MIOpen runs
 *      them), batch 1, float32.  A coarse tensor P (cp, X, Y, Z) and a fine tensor Q (cq, sX, sY, sZ) are tied by W[cp][cq][27]:
 *        gather    P[a][o] = bias[a] + sum W[a][b][t] Q[b][s o + t - 1]      Conv3d forward (a = out, b = in), ConvTranspose3d dgrad
 *        scatter2  Q[b][i] = sum W[a][b][t] P[a][(i + 1 - t) / 2]            ConvTranspose3d forward (a = in, b = out), Conv3d(s=2) dgrad
 *        wgrad     dW[a][b][t] = sum_o P[a][o] Q[b][s o + t - 1]             both weight gradients, in W's own layout
 *      dims_p = {X, Y, Z} (host).  Weight layouts (the host permutes the small tensor): gather w (cq, 27, cpp), cpp = cp rounded up
 *      to 8 (cp > 4) or 4, zero-filled; scatter2 w (cp, 27, cqp), cqp likewise from cq.  bias may be NULL.  A stride-1 scatter is a
 *      gather with the 27 taps reversed and the channel roles swapped.  wgrad writes partial sums (parts, cpp4, cqp8, 27) with
 *      parts = gens_conv3d_wgrad_parts(...), cpp4 = cp rounded up to 4, cqp8 = cq rounded up to 8; the caller adds over `parts`
 *      (fixed order: deterministic).  Every tensor must be smaller than 2 GiB.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_conv3d_gather(const float* q, const float* w, const float* bias, int cp, int cq, const int* dims_p, int stride,
                       float* p, void* stream);
int gens_conv3d_scatter2(const float* p, const float* w, int cp, int cq, const int* dims_p, float* q, void* stream);
int gens_conv3d_wgrad_parts(int cp, int cq, const int* dims_p);
/* the number of parts gens_conv3d_wgrad writes for THIS stride (the stride-1 matrix-core kernel cuts the volume its own way); the workspace
 * of a call must hold gens_conv3d_wgrad_parts_strided(cp, cq, dims_p, stride) parts */
int gens_conv3d_wgrad_parts_strided(int cp, int cq, const int* dims_p, int stride);
int gens_conv3d_wgrad(const float* p, const float* q, int cp, int cq, const int* dims_p, int stride, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K16  InstanceNorm3d (affine=False, biased variance) + ReLU after every convolution of the U-Net (reg_network.py:16-17,39-40:
 *      aten::instance_norm + aten::relu_ and their backward), batch 1, float32 planes x (c, n).
 *        gens_instnorm_stats           partials (c, blocks, 2) float64: sums of x and x^2 per workgroup, blocks = gens_instnorm_blocks(c, n)
 *        gens_instnorm_relu_fwd        y = max((x - mean) * rstd, 0), mean_rstd (c, 2) float32
 *        gens_instnorm_relu_bwd_stats  partials (c, blocks, 2) float64: sums of g and g xhat, g = gy [xhat > 0], xhat = (x - mean) * rstd
 *        gens_instnorm_relu_bwd        gx = rstd (g - m1 - xhat m2), g_means (c, 2) float32 = {m1 = mean(g), m2 = mean(g xhat)}
 *        gens_instnorm_finish          partials -> (c, 2) float32 in one launch, float64 inside: mode 0 = (mean, 1 / sqrt(max(E[x^2] - mean^2, 0) + eps))
 *                                      from gens_instnorm_stats' partials, mode 1 = (m1, m2) from gens_instnorm_relu_bwd_stats' (eps ignored)
 *      A batch (nn.InstanceNorm2d of the feature decoder, feature_network_mnasnet.py:29-50) is n * c planes: pass c = n * c.
 * ---------------------------------------------------------------------------------------------------------- */
int gens_instnorm_blocks(int c, int64_t n);
int gens_instnorm_stats(const float* x, int c, int64_t n, double* partials, void* stream);
int gens_instnorm_finish(const double* partials, int c, int64_t n, double eps, int mode, float* out, void* stream);
int gens_instnorm_relu_fwd(const float* x, const float* mean_rstd, int c, int64_t n, float* y, void* stream);
/* the same + skip (c, n): the decoder blocks add the encoder's tensor right after norm + ReLU (reg_network.py:158) */
int gens_instnorm_relu_add_fwd(const float* x, const float* mean_rstd, const float* skip, int c, int64_t n, float* y, void* stream);
int gens_instnorm_relu_bwd_stats(const float* x, const float* gy, const float* mean_rstd, int c, int64_t n, double* partials, void* stream);
int gens_instnorm_relu_bwd(const float* x, const float* gy, const float* mean_rstd, const float* g_means, int c, int64_t n, float* gx,
                           void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * K19  step-boundary kernels of a training step: what the reference does with dozens of scalar-sized PyTorch launches around the
 *      hot-path kernels, each in ONE launch on the device and without host synchronisation (k19_step.hip).
 *
 * gens_scene_setup: the camera constants of a scene --
 *     w2c = inverse(c2ws)                                  (volume.py:34, projector.py:322)
 *     ks[l] = intrs with rows 0-1 times 0.5^l, l < 8       (volume.py:24-25, projector.py:317-318; Q2)
 *     rot_inv = inverse(c2ws[0, :3, :3])                   (implicit_surface.py:242,245)
 *     kinv_ref = inverse(intrs)[0, :3, :3]                 (projector.py:364)
 *   written to `cams`, gens_scene_cams_floats(nv) floats laid out as
 *     [w2c nv x 16][ks GENS_MAX_LEVELS x nv x 16][rot_inv 9 + 3 pad][kinv_ref 9 + 3 pad][status: int32, bit 0 = a singular matrix][3 pad].
 *   Inverses: float64 Gauss-Jordan with partial pivoting, rounded once to float32; a singular matrix gives NaNs and sets the status bit
 *   (torch.inverse raises: the host checks the bit where it synchronises anyway).
 * gens_pack_maps / gens_unpack_maps: gens_pack_nchw / gens_unpack_nhwc for up to 8 maps in one launch; src / dst: HOST arrays of device
 *   pointers, nchw: HOST int[4 * n_maps] = (n, C, H, W) per map.
 * gens_compact_points: the index list of a step's masked SDF evaluation (implicit_surface.py:121-124,174-177,256-257,484-497): rows
 *   [0, n_ray_pts) are ray samples with flags from gens_ray_points (none set: the first min(10, n) of them, Q7), the next n_always rows
 *   are always selected (the random points), the rest are the pseudo points with their own flags.  idx (n) int64: selected rows in
 *   increasing order; counts (3) int32 = {selected, selected ray samples, selected pseudo points}.  n < 2^24; two launches (counts per
 *   workgroup, ordered write); scratch: gens_compact_points_scratch(n) 4-byte words of device memory.
 *   Optional outputs of the same launch (NULL to skip): the values the reference's dense tensors hold for UNSELECTED rows (Q8) --
 *   y_fill (n): 100 for ray samples, 0 for pseudo points (implicit_surface.py:125,497); g_fill / s_fill (n, 3): 0; rgb_fill
 *   (n_ray_pts, 3): 0; vis_fill (n_ray_pts, n_src): 0 -- and scalars (4) = {max of z (nz floats; :301), inv_s = clip(exp(10 variance),
 *   1e-6, 1e6) (variance_network.py:11, :206), 1 / inv_s, 1 if inv_s is inside the clip range else 0}.
 * gens_tv_levels_fwd / _bwd: tv_regularization (implicit_surface.py:135-150; Q13) of all levels.  vols[l] (4, X, Y, Z), masks[l]
 *   (X, Y, Z): HOST arrays of device pointers; dims HOST int[3 * n_levels]; Z % 4 == 0, 16-byte aligned planes.
 *   fwd: partial: scratch of gens_tv_levels_blocks(dims, n_levels) float4; out (1 + n_levels): out[0] = tv_reg, out[1 + l] = the
 *   level's backward coefficient 0.5^l / (2 tv_l den_l).  bwd: g (1) = d loss / d tv_reg (DEVICE) -> g_vols[l] (overwritten).
 * ---------------------------------------------------------------------------------------------------------- */
/* gens_patch_warp_fwd / _bwd: surface_patch_warp (projector.py:353-437 as called from implicit_surface.py:301-328) in one launch each.
 *   rays_o, rays_d (B, 3); z (B) = the clamped crossing depth z_vals_sdf0 (:300-303), the only differentiable input; g0 (B, 3) = the SDF
 *   gradient at the surface point, un-normalised (normalised and rotated into the reference camera in-kernel, :308-310; used detached);
 *   c2ws, intrs (nv, 4, 4), kinv_ref (3, 3) = inverse(intrs)[0, :3, :3] (gens_scene_setup); tex (nv, H, W, C_pad) texels of the warp
 *   features (gens_upsample2d_into), C <= 16 channels; patch: odd patch size (11).
 *   fwd -> ref (1, B, P, C), sampled (nv - 1, B, P, C), P = patch^2 in row-major (y, x) order.  bwd: g_sampled -> g_z (B), overwritten. */
int gens_patch_warp_fwd(const float* rays_o, const float* rays_d, const float* z, const float* g0, int64_t n_rays, const float* c2ws,
                        const float* intrs, const float* kinv_ref, int nv, const float* tex, int h, int w, int c, int patch, float* ref,
                        float* sampled, void* stream);
int gens_patch_warp_bwd(const float* rays_o, const float* rays_d, const float* z, const float* g0, int64_t n_rays, const float* c2ws,
                        const float* intrs, const float* kinv_ref, int nv, const float* tex, int h, int w, int c, int patch,
                        const float* g_sampled, float* g_z, void* stream);
/* gens_loss_fwd / _bwd: Loss.forward (models/losses/loss.py:24-93) in one launch, its backward in one launch.  The argument block: */
typedef struct {
    const float *color, *target;            /* color_fine, targets["color"]: (B, 3) */
    const uint8_t* valid;                   /* valid_mask (B) */
    int64_t b;
    const float* sparse;                    /* sparse_sdf (n_sparse) */
    int64_t n_sparse;
    float sparse_scale;
    const float* pseudo;                    /* pseudo_sdf (n_pseudo) or NULL */
    int64_t n_pseudo;
    const float *ncc, *mid_in;              /* compute_LNCC's result (B), mid_inside_sphere (B) */
    const float *depth, *pseudo_depth_t, *depth_t;      /* render_depth (B); targets["pseudo_depth"], targets["depth"] (B) or NULL */
    const float *ge, *se, *tv;              /* gradient_error, smooth_error, tv_reg: DEVICE scalars */
    float w_color, w_igr, w_sparse, w_mfc, w_smooth, w_tv, w_pseudo_sdf, w_pseudo_depth;
    float* out;                             /* (16): loss, color, eikonal, sparse, mfc, smooth, tv, depth, pseudo_sdf, pseudo_depth, 4 denominators, 2 spare */
    const float* g;                         /* backward: d L / d loss, DEVICE scalar */
    float *g_color, *g_sparse, *g_pseudo, *g_ncc, *g_depth, *g_scalars;      /* backward outputs (NULL to skip); g_scalars (3): ge, se, tv */
} gens_loss_args;
int gens_loss_fwd(const gens_loss_args* args, void* stream);
int gens_loss_bwd(const gens_loss_args* args, void* stream);
/* gens_coarse_z: the coarse depths of a render (implicit_surface.py:356-363) in one launch: z (B, n) = near + (far - near) * steps[j]
 *   (+ (t_rand[ray] - 0.5) * 2 / n when t_rand != NULL); near / far: one float each (per_ray = 0) or (B) (per_ray = 1); steps (n) =
 *   torch.linspace(0, 1, n).
 * gens_blend_train_wgrad: the 23 parameter gradients of a BlendingNetwork in one launch from cc = gens_gemm_tn_batch's result for
 *   gens_blend_train_bwd's eleven products and s_part (n_part); n_feat = 3 + 4 n_levels; grads: HOST array of 23 device pointers (row-major
 *   weights and biases in the order of gens_blend_train_fwd, then s). */
int gens_coarse_z(const float* near, const float* far, int per_ray, const float* steps, const float* t_rand, int64_t n_rays, int n, float* z,
                  void* stream);
int gens_blend_train_wgrad(const float* cc, const float* s_part, int n_part, const float* s, int n_feat, float* const* grads, void* stream);
int64_t gens_scene_cams_floats(int nv);
int gens_scene_setup(const float* c2ws, const float* intrs, int nv, float* cams, void* stream);
int gens_pack_maps(const float* const* src, float* const* dst, const int* nchw, int n_maps, void* stream);
int gens_unpack_maps(const float* const* src, float* const* dst, const int* nchw, int n_maps, void* stream);
/* Views taken out of up to 16 per-scene maps in one launch (ABI 12): dst[k][j] = src[k][index[j]], j < n_sel, where a view of map k is
 * floats_per_view[k] contiguous floats (a multiple of 4; both sides 16-byte aligned) and src[k] holds views_in_src[k] of them; index: n_sel int64 on the
 * DEVICE (negative values count from the end, as torch's).  What fine-tuning's `self.features[i][view_ids]` (gens.py:151-153) does to the frozen
 * pyramid -- here for the maps and their texel / warp layouts together. */
int gens_select_views(const float* const* src, float* const* dst, const int* floats_per_view, const int* views_in_src, int n_maps,
                      const int64_t* index, int n_sel, void* stream);
int64_t gens_compact_points_scratch(int64_t n);   /* 4-byte words of scratch for n rows */
int gens_compact_points(const uint8_t* valid, int64_t n_ray_pts, int64_t n_always, int64_t n, int64_t* idx, int32_t* counts,
                        float* y_fill, float* g_fill, float* s_fill, float* rgb_fill, uint8_t* vis_fill, int n_src, const float* z,
                        int64_t nz, const float* variance, float* scalars, int32_t* scratch, void* stream);
int gens_tv_levels_blocks(const int* dims, int n_levels);
int gens_tv_levels_fwd(const float* const* vols, const float* const* masks, const int* dims, int n_levels, float* partial, float* out,
                       void* stream);
int gens_tv_levels_bwd(const float* const* vols, const float* const* masks, const int* dims, int n_levels, const float* out,
                       const float* g, float* const* g_vols, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GENS_HIP_H */
