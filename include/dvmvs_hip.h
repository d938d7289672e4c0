/*
 * dvmvs_hip.h -- C ABI of the MI355X (gfx950) plane-sweep depth kernels.
 *
 * The reference (ardaduz/deep-video-mvs) has no FFI layer: its hot path is a set of Python functions over torch
 * tensors.  This header is the boundary a maintainer binds instead (ctypes stub shown in
 * INTEGRATION.md).  Each entry point names the reference interface it replaces.
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer to contiguous fp32 data unless the comment says "host array" or the parameter is named
 *     *_host (the host-side sweep plan: those functions make no HIP call at all);
 *   - tensors are NCHW, batch-major, exactly as the reference lays them out;
 *   - the caller (PyTorch) allocates and owns every buffer including outputs and workspaces;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); no entry point synchronises,
 *     allocates, or keeps global state, so calls are re-entrant and capturable into a hipGraph;
 *   - return value: 0 on success, a positive hipError_t on a HIP failure, a negative DVMVS_E* on a bad argument.
 *     Nothing is enqueued when the return value is negative.
 */
#ifndef DVMVS_HIP_H
#define DVMVS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 4 (round 4) = ABI 3 + additions, no signature of ABI 3 changed: variant 3 of dvmvs_cost_volume_fwd, the host-side sweep plan
 * (dvmvs_sweep_plan_stats / _select_variant / _work_list / dvmvs_sweep_plan, dvmvs_cost_volume_planned_fwd), the bottleneck convolution
 * (dvmvs_bottleneck_conv_*, dvmvs_partial_sums_bias_act_fwd, dvmvs_lstm_gates_partials_fwd) and two training gradients
 * (dvmvs_upsample2x_bwd, dvmvs_depthwise_conv_bwd).
 * ABI 5 = ABI 4 + the direct convolution of the larger maps and the depth heads (dvmvs_direct_conv_*, dvmvs_conv_head_fwd).
 * ABI 6 (round 5) = ABI 5 + variant 6 of dvmvs_cost_volume_fwd (the correlate-then-interpolate sweep on the fp32 matrix cores) and the
 * one-launch re-projection of the frame path (dvmvs_depth_reproject_estimate_fwd), dvmvs_sweep_plan6 / dvmvs_sweep_mfma_estimate,
 * dvmvs_nchw_to_nhwc, dvmvs_copy_batch; no earlier signature changed.
 * ABI 7 (round 6) = ABI 6 + dvmvs_direct_conv_dual_fwd (the direct convolution with a second, channels-last copy of its output written in the
 * same epilogue: the frame engine's keyframe features reach the MFMA sweep without a transposing launch); no earlier signature changed.
 * Variant 6 of dvmvs_cost_volume_fwd runs as one persistent 16-wave workgroup per CU where the problem allows (csrc/sweep_mfma.hip): same
 * arguments, bit-identical volumes.
 * ABI 8 (round 6) = ABI 7 + the 1x1 convolution with bias, ReLU and the residual add in its store path (dvmvs_pointwise_conv_*); no earlier
 * signature changed; dvmvs_bottleneck_conv_up2x_fwd and the 32x40 stride-2 shape of dvmvs_bottleneck_conv_fwd; dvmvs_host_pointer_device_visible, dvmvs_upsample2x_pair_fwd.
 * ABI 9 = ABI 8 + marching cubes on a voxel volume (dvmvs_marching_cubes_*); no earlier signature changed.
 * ABI 10 = ABI 9 + the RGB SAD sweep of the MVDepthNet / GP-MVS baselines (dvmvs_rgb_sweep_fwd) and GP-MVS's filter step
 * (dvmvs_gp_filter_step); no earlier signature changed.
 * ABI 11 = ABI 10 + the DPSNet baseline's plane volume (dvmvs_dps_volume_fwd) and its up-sampling soft-argmin (dvmvs_dps_regress_fwd);
 * no earlier signature changed.
 * ABI 11, later addition: dvmvs_preprocess_* (frame pre-processing on the device); no earlier signature changed.  The number stays 11:
 * a library built before the addition reports the same version and simply lacks the two symbols, which a binding must check for.
 * ABI 11, later addition: dvmvs_depth_errors_* (depth evaluation on the device); no earlier signature changed, the number stays 11 by the
 * same rule.
 * ABI 11, later addition: dvmvs_tsdf_raycast_* (ray-casting a fused TSDF volume from camera views); no earlier signature changed, the
 * number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_tsdf_integrate_frames* (fusing a batch of frames into a TSDF volume in one launch); no earlier signature
 * changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_nearest_* and dvmvs_distance_metrics_fwd (exact nearest-point distances between point clouds and the 3-D
 * reconstruction metrics); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_consistency_matrices and dvmvs_depth_consistency_fwd (filtering depth maps by multi-view geometric
 * consistency); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_surface_sample_* and dvmvs_voxel_* (point sets for the 3-D metrics: area-weighted samples of a triangle
 * mesh, one point per occupied voxel of a cloud); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_mesh_raster_* and dvmvs_mesh_visibility_fwd (rasterising a triangle mesh to depth maps, and the vertices
 * that depth maps show); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_icp_* and dvmvs_transform_points_fwd (registering a point cloud to another by trimmed ICP on the device);
 * no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_direct_conv_shape (which workgroup shape of the direct convolution a problem runs with; a host query);
 * no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_mesh_components_* and dvmvs_mesh_filter_* (connected components of a triangle mesh and their removal by
 * size); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_knn_fwd, dvmvs_radius_count_fwd and dvmvs_outlier_statistics_fwd (the k nearest neighbours of points,
 * neighbours within a radius, statistical outlier scores); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_point_normals_fwd (oriented normals of points from rows of nearest neighbours); no earlier signature
 * changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_icp_plane_* (registering a point cloud to another with normals by point-to-plane ICP); no earlier
 * signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_implicit_* (the implicit moving-least-squares signed distance of an oriented point cloud on a voxel grid,
 * and the trimming of the mesh that marching cubes makes of it); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_mesh_simplify_* and dvmvs_voxel_downsample_runs (simplifying a triangle mesh by vertex clustering with
 * quadric error representatives); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_mesh_smooth_* (smoothing a triangle mesh by the Laplacian and Taubin filters; vertex normals from the
 * faces); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_sparse_neighbours and dvmvs_sparse_extract_* (marching cubes straight from the pool of the sparse TSDF
 * volume); no earlier signature changed, the number stays 11 by the same rule.
 * ABI 11, later addition: dvmvs_sparse_raycast_* (ray-casting the sparse TSDF volume straight from its pool); no earlier signature
 * changed, the number stays 11 by the same rule. */
#define DVMVS_ABI_VERSION 11
#define DVMVS_MAX_MEASUREMENTS 8      /* measurement frames fused per launch */
#define DVMVS_MAX_DEPTH_LEVELS 256    /* sweep planes per launch */

#define DVMVS_LAYOUT_NCHW 0           /* [B,C,H,W] contiguous: the reference's layout */
#define DVMVS_LAYOUT_NHWC 1           /* [B,H,W,C] contiguous ("channels last") */

#define DVMVS_EINVAL (-1)             /* null pointer / non-positive dimension / out-of-range count */
#define DVMVS_EUNSUPPORTED (-2)       /* shape outside what the kernels were built for */
#define DVMVS_ELIBRARY (-3)           /* a call into MIOpen failed (dvmvs_conv_bias_act_fwd) */

typedef void* dvmvs_stream_t;         /* hipStream_t */

/* ABI / build identification. */
int dvmvs_abi_version(void);
const char* dvmvs_build_arch(void);   /* "gfx950" */
const char* dvmvs_error_string(int code);
/* Launches an empty kernel named dvmvs::trace_marker_kernel (profiling: brackets a region of a kernel trace). */
int dvmvs_trace_marker(dvmvs_stream_t stream);

/*
 * Small pose algebra: WHERE IT IS EVALUATED, AND WHY IT IS AN ARGUMENT (ABI 3).
 *
 * The reference derives three tiny matrices per frame from the camera poses with fp32 torch ops on the host side of its
 * hot functions:
 *   sweep constants   E = inverse(pose2) * pose1,  Hm = K R K^-1,  kt = K t        (/root/reference/dvmvs/utils.py:51-56)
 *   splat transform   inverse(reference_pose) * measurement_pose                   (utils.py:121)
 *   warp transform    inverse(previous_pose) * current_pose                        (dvmvs/convlstm.py:30)
 * Their fp32 round-off (cancellation in the relative translation, ~5e-7 m) moves sample positions by up to 3e-4 px on the
 * nearest plane -- more than everything else on the path together -- so "results identical to the reference" requires
 * the very same matrices.  The entry points below therefore take them as DEVICE ARRAYS, computed by the caller exactly as
 * the reference computes them (the Python surface does it with the reference's own torch expressions, see
 * deep-video-mvs_amd/dvmvs/pose_algebra.py), and do no pose algebra themselves.
 *   Hm  [B,M,9]   row-major 3x3 per (batch item, measurement frame)
 *   kt  [B,M,3]
 * For callers that prefer accuracy over bit-parity (or want no host involvement at all) dvmvs_sweep_matrices and
 * dvmvs_relative_pose evaluate the same algebra on the device in fp64 and round once ("exact" mode).
 */

/*
 * Hm[b,m] = K[b] R K[b]^-1, kt[b,m] = K[b] t with [R|t] = inverse(pose2s[m][b]) * pose1[b]; fp64 on the device, rounded once.
 * Opt-in alternative to the reference's fp32 host algebra (utils.py:51-56).
 *   pose1 [B,4,4]   pose2s host array of M device pointers, each [B,4,4]   K [B,3,3]   Hm [B,M,9] out   kt [B,M,3] out
 */
int dvmvs_sweep_matrices(const float* pose1, const float* const* pose2s, const float* K, float* Hm, float* kt,
                         int B, int M, dvmvs_stream_t stream);

/*
 * Fused plane-sweep warp + feature correlation over all planes and all measurement frames, written once.
 * Replaces dvmvs.utils.calculate_cost_volume_by_warping (M == 1) and dvmvs.utils.cost_volume_fusion (M >= 1):
 *   /root/reference/dvmvs/utils.py:45-86 and :89-107 (everything after the small pose algebra of :51-56, see above).
 *
 *   image1      [B,C,H,W]   reference-frame features
 *   image2s     host array of M device pointers, each [B,C,H,W] measurement-frame features
 *   Hm          [B,M,9]     K R K^-1 per (batch item, measurement frame)
 *   kt          [B,M,3]     K t
 *   cost_volume [B,D,H,W]   out; plane 0 = max_depth ... plane D-1 = min_depth, uniform in inverse depth
 *   dot_product 1: sum_c(f1*warp(f2))/C   0: sum_c|f1-warp(f2)|  (utils.py:81-84); result is the mean over M
 *   variant     0 = pick the fastest kernel for the shape; 1 = force the generic reference-order kernel (taps through
 *               the vector L1); 2 = force the LDS-tiled sweep in its default configuration (dot_product only); 3 = the
 *               LDS-tiled sweep in its wide-baseline configuration (72 KB sample boxes, 512-thread workgroups: faster where
 *               the default one has to split or queue runs of planes, slower on easy pairs -- dvmvs_sweep_select_variant
 *               decides from the matrices); 4 / 5 = configurations 2 / 3 as ONE launch: no second pass, a run that cannot be staged is
 *               gathered inline by the sweep kernel (what dvmvs_sweep_plan returns when its plan queues nothing; also what a NULL
 *               workspace gives); 6 = the correlate-then-interpolate sweep on the fp32 matrix cores (csrc/sweep_mfma.hip: the 32-channel dot
 *               product per measurement CELL on v_mfma_f32_16x16x4_f32, four table look-ups per (pixel, plane, frame); up to 32 channels,
 *               either layout, any image size, no workspace, no work list, no host plan; since round 6 one persistent 16-wave workgroup per CU
 *               that gives every SIMD the same mix of work, for one batch item with >= 4096 (pixel group, 16-plane chunk) items whose
 *               K t / depth table fits in LDS, D * M <= 512); 7 = variant 6 as one work item per workgroup for every shape (what 6 falls back
 *               to; bit-identical to 6: the comparison kernel of tests and bench).  Each is bit-reproducible; they differ in fp32
 *               summation order.
 *   image2_layout DVMVS_LAYOUT_NCHW, or DVMVS_LAYOUT_NHWC when the MEASUREMENT maps are stored channels-last (a keyframe's
 *               features are reused as measurement features by later frames, so a runner converts them once per
 *               keyframe).  Supported by the LDS-tiled dot-product kernel (C % 4 == 0, H*W >= 4096); image1 and
 *               cost_volume are always NCHW.
 *   workspace   optional device scratch of dvmvs_cost_volume_workspace_bytes(B, M, H, W, D) bytes for the two-pass form of
 *               the LDS-tiled sweep: runs of planes whose sample footprint does not fit in LDS (magnified or behind-camera
 *               views) are queued there by the sweep launch and finished by a second, finely grained gather launch that
 *               is spread over the whole chip, in a fixed order (the volume is bit-reproducible run to run).
 *               CONTRACT: the first 16 bytes must be zero when a call starts.  Every call leaves them zero again, so the
 *               owner zero-fills the buffer once, when it allocates it; a buffer must not be shared by calls that may
 *               overlap in time (different streams).  With workspace == NULL (or too small) such runs are gathered inline
 *               by the sweep kernel itself (one launch, long tail on wide-baseline / forward-motion pairs).
 */
size_t dvmvs_cost_volume_workspace_bytes(int B, int M, int H, int W, int D);
int dvmvs_cost_volume_fwd(const float* image1, const float* const* image2s, const float* Hm, const float* kt,
                          float* cost_volume, int B, int M, int C, int H, int W, int D,
                          double min_depth, double max_depth, int dot_product, int variant, int image2_layout,
                          float* workspace, size_t workspace_bytes, dvmvs_stream_t stream);

/*
 * HOST-side model of the LDS-tiled sweep's run plan (no HIP call, no device memory): Hm_host / kt_host are HOST copies of the
 * matrices the launch will get -- they are on the host before the launch anyway (see "small matrices" above).
 *   configuration 0 = default (variant 2), 1 = wide-baseline (variant 3)
 *   stats[8] out: staged runs, LDS records of all staged runs, runs entirely outside the image, runs queued for the second
 *                 pass, planes of those runs, workgroups with at least one queued run, the largest number of staged runs of
 *                 one workgroup (all workgroups are resident at once: the longest chain is the launch's span), the largest
 *                 number of queued planes of one workgroup
 * dvmvs_sweep_select_variant returns the variant (2 or 3) the cost model built on those numbers expects to be faster for this
 * keyframe pair (negative DVMVS_E* on bad arguments); a captured frame graph per variant is replayed accordingly.
 */
int dvmvs_sweep_plan_stats(const float* Hm_host, const float* kt_host, int B, int M, int H, int W, int D,
                           double min_depth, double max_depth, int configuration, long long* stats);
int dvmvs_sweep_select_variant(const float* Hm_host, const float* kt_host, int B, int M, int H, int W, int D,
                               double min_depth, double max_depth);

/*
 * Work list of the LDS-tiled sweep, built on the HOST from the host copies of the matrices (no HIP call).  All workgroups of a sweep
 * launch are resident at once, so the launch lasts as long as its slowest workgroup; on wide-baseline / forward-motion pairs a few
 * (tile, 8-plane chunk) pairs need 5-8 staged runs instead of 2.  The list cuts those into plane sub-ranges of at most 3 staged runs
 * that separate workgroups process in parallel.  Upload it (dvmvs_sweep_work_list_bytes(B, H, W, D) bytes; the returned value is the
 * number of 32-bit words actually used, negative on error) and pass the DEVICE copy to dvmvs_cost_volume_planned_fwd, which is
 * dvmvs_cost_volume_fwd with that one extra argument (NULL = static numbering; used only together with a workspace).  `configuration`
 * as for dvmvs_sweep_plan_stats; it must match the variant of the launch (2 -> 0, 3 -> 1; 0 picks the default configuration).
 * Results do not depend on the list beyond fp32 summation order (a cut can turn a queued run into staged ones); with a given list the
 * volume is bit-reproducible.
 */
size_t dvmvs_sweep_work_list_bytes(int B, int H, int W, int D);
/* dvmvs_sweep_select_variant + dvmvs_sweep_work_list in one walk (what a frame loop calls once per keyframe): `variant` 0 = decide,
 * 2 / 3 = that configuration; leaves the chosen configuration's work list in work_list_host and returns the variant to launch with
 * (2 / 3, or 4 / 5 = the same configuration without a second pass when the plan queues nothing for it; negative on error). */
int dvmvs_sweep_plan(const float* Hm_host, const float* kt_host, int B, int M, int H, int W, int D, double min_depth, double max_depth,
                     int variant, unsigned int* work_list_host, size_t work_list_bytes);
/* ABI 6: HOST-side work estimate of variant 6 (the correlate-then-interpolate sweep) for batch item 0 of these matrices, no HIP call:
 * stats[4] = mean 16-cell tiles per wave, mean passes per wave, mean strips beyond the first per wave, fraction of waves whose footprint
 * cannot be bounded from its corners (behind-camera / non-finite); sampled on every sixth pixel group row / column (25 us at 160 x 128 x 64).
 * dvmvs_sweep_plan6 uses it. */
int dvmvs_sweep_mfma_estimate(const float* Hm_host, const float* kt_host, int B, int M, int H, int W, int D, double min_depth, double max_depth,
                              double* stats);
/* dvmvs_sweep_plan with variant 6 as a candidate.  Since round 6 (ABI 7) a single-item launch (B == 1, H * W >= 4096) always gets variant 6: the
 * work list is left EMPTY (header count 0: a tiled launch on it does nothing), neither the estimate nor the tiled plan runs, the call is a few
 * nanoseconds -- variant 6 in its persistent form is the faster kernel on 255 of the sample scene's 285 keyframe pairs and within 1 - 7 us on the
 * rest (profiles/r06_sweep_all_pairs_v6_vs_tiled.json; round 5 took it below 14 estimated tiles per wave: profiles/r05_sweep_selection.md).
 * Lock-step batches (B > 1) get the tiled plan as dvmvs_sweep_plan makes it.  For callers whose measurement maps are channels-last (what variant 6
 * is fast with) and have at most 32 channels. */
int dvmvs_sweep_plan6(const float* Hm_host, const float* kt_host, int B, int M, int H, int W, int D, double min_depth, double max_depth,
                      unsigned int* work_list_host, size_t work_list_bytes);
/* [B,C,H,W] -> [B,H,W,C] (C <= 64, a multiple of 4), one launch: how a keyframe's features enter a channels-last feature cache. */
int dvmvs_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, dvmvs_stream_t stream);
/* n <= 8 contiguous device-to-device copies of n_floats[j] floats (a multiple of 4; 16-byte aligned pointers; host arrays of n entries) in
 * ONE launch -- the small copies a frame step makes in front of its graph (features into the feature cache, measurement maps and the next
 * image into the buffers the graph reads).  Ranges must not overlap each other (the copies run concurrently). */
int dvmvs_copy_batch(const float* const* srcs, float* const* dsts, const long long* n_floats, int n, dvmvs_stream_t stream);
/* (ABI 8) A source of dvmvs_copy_batch may also be PINNED HOST memory that the device sees at the same address (the frame engine's parameter
 * block rides up in the frame's copy batch instead of a blit launch of its own): 1 when p is such memory for the current device, else 0. */
int dvmvs_host_pointer_device_visible(const void* p);
int dvmvs_sweep_work_list(const float* Hm_host, const float* kt_host, int B, int M, int H, int W, int D,
                          double min_depth, double max_depth, int configuration, unsigned int* work_list_host, size_t work_list_bytes);
int dvmvs_cost_volume_planned_fwd(const float* image1, const float* const* image2s, const float* Hm, const float* kt,
                                  float* cost_volume, int B, int M, int C, int H, int W, int D,
                                  double min_depth, double max_depth, int dot_product, int variant, int image2_layout,
                                  float* workspace, size_t workspace_bytes, const unsigned int* work_list, dvmvs_stream_t stream);

/*
 * Gradient of the fused cost volume (dot_product mode) w.r.t. both feature maps; poses/K carry no gradient
 * (autograd through utils.py:75-82; the sampling grid is data).
 *   grad_cost   [B,D,H,W]
 *   Hm, kt      as for the forward
 *   grad_image1 [B,C,H,W]   out (overwritten)
 *   grad_image2s host array of M device pointers, each [B,C,H,W]; MUST be zero-filled by the caller (the gradient is ADDED to
 *               it -- by a gather without atomics, so the result is bit-reproducible); an entry may be NULL to skip that frame.
 */
int dvmvs_cost_volume_bwd(const float* grad_cost, const float* image1, const float* const* image2s,
                          const float* Hm, const float* kt, float* grad_image1, float* const* grad_image2s,
                          int B, int M, int C, int H, int W, int D,
                          double min_depth, double max_depth, dvmvs_stream_t stream);

/*
 * Depth-conditioned inverse warp of the ConvLSTM hidden state.
 * Replaces dvmvs.utils.warp_frame_depth (/root/reference/dvmvs/utils.py:205-258; normalize_points=False,
 * bilinear) and, with zero_invalid != 0, the caller's mask h[depth <= 0.01] = 0 (dvmvs/convlstm.py:32-41).
 *   image_src     [B,C,H,W]
 *   depth_dst     [B,1,H,W]
 *   src_trans_dst [B,4,4]
 *   camera_matrix [B,3,3]
 *   out           [B,C,H,W]
 */
int dvmvs_hidden_warp_fwd(const float* image_src, const float* depth_dst, const float* src_trans_dst,
                          const float* camera_matrix, float* out, int B, int C, int H, int W,
                          int zero_invalid, dvmvs_stream_t stream);

/*
 * Gradient of the hidden-state warp w.r.t. image_src.  As in the reference the validity mask is NOT applied to
 * the gradient (convlstm.py:41 mutates .data outside autograd).  grad_src [B,C,H,W] MUST be zero-filled.
 */
int dvmvs_hidden_warp_bwd(const float* grad_out, const float* depth_dst, const float* src_trans_dst,
                          const float* camera_matrix, float* grad_src, int B, int C, int H, int W,
                          dvmvs_stream_t stream);

/*
 * out[b] = inverse(a[b]) * c[b] for 4x4 matrices (evaluated in fp64, rounded once to fp32): the "exact" alternative to
 * the reference's fp32 torch.bmm(torch.inverse(previous_pose), current_pose) (dvmvs/convlstm.py:30, utils.py:121).
 */
int dvmvs_relative_pose(const float* a, const float* c, float* out, int B, dvmvs_stream_t stream);

/*
 * ConvLSTM gate fusion given the 4*hidden-channel convolution output (split order i,f,o,g):
 *   i,f,o = sigmoid; g = celu(LN_hw(cc_g)); c' = LN_hw(f*c + i*g); h' = o*celu(c').  LN: biased variance,
 *   eps 1e-5, no affine; celu alpha = 1.
 * Replaces /root/reference/dvmvs/convlstm.py:45-59.
 *   combined_conv [B,4*hidden,H,W]   c_cur [B,hidden,H,W]   h_next, c_next [B,hidden,H,W] out; c_next may be c_cur (in-place state update)
 */
int dvmvs_lstm_gates_fwd(const float* combined_conv, const float* c_cur, float* h_next, float* c_next,
                         int B, int hidden, int H, int W, dvmvs_stream_t stream);

/*
 * Backward of the gate fusion: recomputes the gates from (combined_conv, c_cur).
 *   grad_h, grad_c [B,hidden,H,W] (either may be NULL = zero)   grad_cc [B,4*hidden,H,W], grad_c_cur out
 */
int dvmvs_lstm_gates_bwd(const float* grad_h, const float* grad_c, const float* combined_conv,
                         const float* c_cur, float* grad_cc, float* grad_c_cur,
                         int B, int hidden, int H, int W, dvmvs_stream_t stream);

/*
 * Gradients of two frame-path ops for training (BASELINE.json configs[4]); both are gathers / fixed-order reductions without
 * atomics, i.e. bit-reproducible (csrc/train_ops.hip).
 *   dvmvs_upsample2x_bwd      adjoint of dvmvs_upsample2x_fwd (x2 bilinear, align_corners; /root/reference/dvmvs/fusionnet/model.py:59,114):
 *                             grad_out [B,C,2H,2W] -> grad_in [B,C,H,W]
 *   dvmvs_depthwise_conv_bwd  depthwise k x k (3 or 5), padding k/2, stride 1 or 2 (the MnasNet layers): grad_out [B,C,OH,OW], in [B,C,H,W],
 *                             weight [C,1,k,k] -> grad_in [B,C,H,W] and / or grad_weight [C,1,k,k] (either pointer may be NULL);
 *                             workspace: dvmvs_depthwise_conv_bwd_workspace_bytes() bytes of caller-owned scratch for the weight
 *                             gradient's slice sums (0 bytes -> may be NULL)
 */
int dvmvs_upsample2x_bwd(const float* grad_out, float* grad_in, int B, int C, int H, int W, dvmvs_stream_t stream);
size_t dvmvs_depthwise_conv_bwd_workspace_bytes(int B, int C, int H, int W, int kernel_size, int stride);
int dvmvs_depthwise_conv_bwd(const float* grad_out, const float* in, const float* weight, float* grad_in, float* grad_weight,
                             float* workspace, int B, int C, int H, int W, int kernel_size, int stride, dvmvs_stream_t stream);

/*
 * 3x3, padding-1 convolutions on the bottleneck maps of a 320x256 frame (8x10, 16x20 with stride 1 or 2, and -- ABI 8 -- 32x40 with
 * stride 2: the layer that takes the 1/8 map down) as a weight-streaming
 * fp32 MFMA GEMM with a DETERMINISTIC split-K (csrc/bottleneck_conv.hip).  Replaces, for those shapes only, the nn.Conv2d of the
 * ConvLSTM cell (/root/reference/dvmvs/convlstm.py:43-44: 1024 -> 2048 channels) and the 256 / 512-channel layers around it
 * (fusionnet/model.py:167-305), which MIOpen solves with split-K kernels that accumulate with float atomics (results vary from
 * run to run).  Inference only (no gradient); the other convolutions of an inference frame have their own entries below (dvmvs_direct_conv_*,
 * dvmvs_pointwise_conv_*, dvmvs_depthwise_conv_fwd); training convolutions stay on MIOpen.
 *   dvmvs_bottleneck_conv_pack    weight [C_out,C_in,3,3] -> packed (dvmvs_bottleneck_conv_packed_bytes; C_in % 16 == 0), once
 *   dvmvs_bottleneck_conv_splits  number S of partial sums for a problem, DVMVS_EUNSUPPORTED for shapes the kernel does not take
 *   dvmvs_bottleneck_conv_fwd     x [B,C_in,H_in,W_in] -> partials [S][B][C_out][H_out*W_out]: partial s holds the contribution of
 *                                 input channels [s*C_in/S, (s+1)*C_in/S); their sum in ascending s is the convolution
 *   dvmvs_partial_sums_bias_act_fwd  dst[b,c,:] = act(sum_s partials[s,b,c,:] + bias[c]); activation 0 none / 1 ReLU; dst batch
 *                                 item b starts at dst + b*dst_batch_stride (a channel slice of a concatenation buffer)
 *   dvmvs_lstm_gates_partials_fwd dvmvs_lstm_gates_fwd on a convolution output that arrives as n_partials partial sums
 */
size_t dvmvs_bottleneck_conv_packed_bytes(int C_out, int C_in);
int dvmvs_bottleneck_conv_pack(const float* weight, float* packed, int C_out, int C_in, dvmvs_stream_t stream);
int dvmvs_bottleneck_conv_splits(int B, int C_out, int C_in, int H_in, int W_in, int stride);
int dvmvs_bottleneck_conv_fwd(const float* x, const float* packed, float* partials, int B, int C_in, int H_in, int W_in, int C_out,
                              int stride, dvmvs_stream_t stream);
/* (ABI 8) dvmvs_bottleneck_conv_fwd on the 2x bilinear up-sampling (align_corners = True: dvmvs_upsample2x_fwd's values, bit for bit) of
 * x [B,C_in,H_in/2,W_in/2], interpolated while the input is staged -- the decoder's first up-convolution without the up-sampling launch in
 * front of it (/root/reference/dvmvs/fusionnet/model.py UpconvolutionLayer).  H_in x W_in = 16 x 20 (the up-sampled map), stride 1; same
 * split count and partial-sum layout as dvmvs_bottleneck_conv_fwd for that shape. */
int dvmvs_bottleneck_conv_up2x_fwd(const float* x, const float* packed, float* partials, int B, int C_in, int H_in, int W_in, int C_out,
                                   dvmvs_stream_t stream);
int dvmvs_partial_sums_bias_act_fwd(const float* partials, int n_partials, float* dst, long long dst_batch_stride, const float* bias,
                                    int B, int C, int HW, int activation, dvmvs_stream_t stream);
int dvmvs_lstm_gates_partials_fwd(const float* conv_partials, int n_partials, const float* c_cur, float* h_next, float* c_next,
                                  int B, int hidden, int H, int W, dvmvs_stream_t stream);

/*
 * Dense 3x3 / 5x5 convolutions ("same" padding k/2, stride 1 or 2) of the 1/8 ... full-resolution maps of a frame as a direct fp32-MFMA
 * convolution with bias + ReLU in its store path, and the one-output-channel 3x3 depth heads (csrc/direct_conv.hip).  Replace, for the
 * problems dvmvs_direct_conv_tile accepts, the nn.Conv2d + BatchNorm(folded) + ReLU of the cost-volume encoder / decoder, the FPN's
 * smoothing layers and the stem (/root/reference/dvmvs/fusionnet/model.py:167-305, dvmvs/layers.py conv_layer) at inference; no
 * gradient.  Deterministic: input-channel splits are added through LDS in a fixed order.
 *   dvmvs_direct_conv_tile          0 when the kernel does not take the problem (output width not a multiple of 40, C_out % 16 != 0,
 *                                   other kernel sizes / strides: the caller keeps its library convolution); else the number of
 *                                   16-channel output tiles per wave (1 or 2) the weights have to be packed for
 *   dvmvs_direct_conv_shape         (ABI 11, later addition) which of the kernel's workgroup shapes the problem runs with: 0 when
 *                                   dvmvs_direct_conv_tile is 0; 1 = 4 rows x 80 columns x 32 channels per workgroup (tile 2),
 *                                   2 = 2 x 40 x 32 (tile 2), 3 = 1 x 80 x 16 (tile 1), 4 = 2 x 40 x 16 (tile 1).  With kernel_size and
 *                                   stride it names the one of the 16 compiled kernels that a launch runs; host only, for tests and tools
 *   dvmvs_direct_conv_pack          weight [C_out,C_in,k,k] -> packed (dvmvs_direct_conv_packed_bytes), once per (layer, n_tile)
 *   dvmvs_direct_conv_fwd           x [B,C_in,H,W] (batch item b at x + b*x_batch_stride, 0 = dense) -> dst [B,C_out,H/stride,W/stride]
 *                                   (batch item b at dst + b*dst_batch_stride, 0 = dense: a channel slice of a concatenation buffer);
 *                                   bias may be NULL; activation 0 none, 1 ReLU; DVMVS_EINVAL when n_tile is not the problem's
 *   dvmvs_direct_conv_dual_fwd      (ABI 7) the same, and when dst_nhwc is not NULL the same values once more as a dense channels-last map
 *                                   [B,H/stride,W/stride,C_out] (DVMVS_LAYOUT_NHWC: what variant 6 of the sweep reads one 128-byte line per cell)
 *   dvmvs_conv_head_fwd             3x3, padding 1, ONE output channel: weight [1,C_in,3,3]; dst [B,1,H,W]; bias may be NULL (raw
 *                                   convolution output when also activation == 0); activation / p0 / p1 as dvmvs_bias_act_fwd
 */
int dvmvs_direct_conv_tile(int B, int C_in, int H, int W, int C_out, int kernel_size, int stride);
int dvmvs_direct_conv_shape(int B, int C_in, int H, int W, int C_out, int kernel_size, int stride);
size_t dvmvs_direct_conv_packed_bytes(int C_out, int C_in, int kernel_size, int n_tile);
int dvmvs_direct_conv_pack(const float* weight, float* packed, int C_out, int C_in, int kernel_size, int n_tile, dvmvs_stream_t stream);
int dvmvs_direct_conv_fwd(const float* x, long long x_batch_stride, const float* packed, int n_tile, const float* bias, float* dst,
                          long long dst_batch_stride, int B, int C_in, int H, int W, int C_out, int kernel_size, int stride, int activation,
                          dvmvs_stream_t stream);
int dvmvs_direct_conv_dual_fwd(const float* x, long long x_batch_stride, const float* packed, int n_tile, const float* bias, float* dst,
                               long long dst_batch_stride, float* dst_nhwc, int B, int C_in, int H, int W, int C_out, int kernel_size, int stride,
                               int activation, dvmvs_stream_t stream);
int dvmvs_conv_head_fwd(const float* x, long long x_batch_stride, const float* weight, const float* bias, float* dst,
                        long long dst_batch_stride, int B, int C_in, int H, int W, int activation, float p0, float p1, dvmvs_stream_t stream);

/*
 * (ABI 8) 1x1 convolutions (stride 1, no padding, one group) of a frame as an fp32-MFMA GEMM straight from the NCHW map, with the bias add,
 * ReLU and the residual add of dvmvs_bias_act_fwd in its store path (csrc/pointwise_conv.hip).  Replace the nn.Conv2d(k = 1) +
 * BatchNorm(folded) (+ ReLU) (+ residual) of the MnasNet feature extractor's expansion / projection layers and of the feature pyramid's
 * lateral layers (/root/reference/dvmvs/fusionnet/model.py:20-124; torchvision's _InvertedResidual) at inference: one launch instead of a
 * library GEMM + an epilogue launch.  No gradient.  Deterministic: input-channel splits are added through LDS in a fixed order.
 *   dvmvs_pointwise_conv_supported  1 when dvmvs_pointwise_conv_fwd takes the problem (C_in % 4 == 0, H*W % 4 == 0, activation 0 / 1, mode 2 only
 *                                   for even H and W % 4 == 0), else 0: the caller keeps its library convolution
 *   dvmvs_pointwise_conv_pack       weight [C_out,C_in] -> packed (dvmvs_pointwise_conv_packed_bytes), once per layer
 *   dvmvs_pointwise_conv_fwd        x [B,C_in,H,W] (batch item b at x + b*x_batch_stride, 0 = dense) -> dst [B,C_out,H,W] (batch item b at
 *                                   dst + b*dst_batch_stride, 0 = dense: a channel slice of a concatenation buffer; 16-byte aligned):
 *                                   dst = act(conv + bias) + residual.  bias may be NULL; activation 0 none, 1 ReLU; residual_mode 0 none,
 *                                   1 residual [B,C_out,H,W], 2 residual [B,C_out,H/2,W/2] nearest-up-sampled (batch item b at residual +
 *                                   b*residual_batch_stride, 0 = dense) -- the meaning of dvmvs_bias_act_fwd's arguments;
 *                                   splits: input-channel splits per output tile, 1 ... 16, 0 = chosen from the problem size
 */
int dvmvs_pointwise_conv_supported(int B, int C_in, int H, int W, int C_out, int activation, int residual_mode);
size_t dvmvs_pointwise_conv_packed_bytes(int C_out, int C_in);
int dvmvs_pointwise_conv_pack(const float* weight, float* packed, int C_out, int C_in, dvmvs_stream_t stream);
int dvmvs_pointwise_conv_fwd(const float* x, long long x_batch_stride, const float* packed, const float* bias, const float* residual,
                             long long residual_batch_stride, int residual_mode, float* dst, long long dst_batch_stride, int B, int C_in,
                             int H, int W, int C_out, int activation, int splits, dvmvs_stream_t stream);

/*
 * Forward splat (z-buffer, farthest wins) of the previous full-resolution depth into the current view at half
 * resolution; untouched pixels are 0.  No host round trip, order-independent (atomic max on the float bits).
 * Replaces dvmvs.utils.get_non_differentiable_rectangle_depth_estimation (/root/reference/dvmvs/utils.py:110-154).
 *   transformation [B,4,4]  inverse(reference_pose) * measurement_pose (utils.py:121), computed by the caller (see above)
 *   previous_depth [B,1,Hf,Wf]   full_K, half_K [B,3,3]
 *   out [B,1,Hf/2,Wf/2]  (zeroed by this call)
 * If out_lowres != NULL it also receives the nearest-neighbour down-sampling by `lowres_factor` that the call
 * site applies next (fusionnet/run-testing.py:187-189): [B,1,(Hf/2)/f,(Wf/2)/f].
 */
int dvmvs_depth_reproject_fwd(const float* transformation, const float* previous_depth, const float* full_K,
                              const float* half_K, float* out, float* out_lowres, int lowres_factor,
                              int B, int full_height, int full_width, dvmvs_stream_t stream);
/*
 * The frame path's form of the above: only the decimated estimate [B,1,(Hf/2)/f,(Wf/2)/f] is produced.  `zbuffer`
 * [B,Hf/2,Wf/2] is caller-owned scratch that MUST be all-zero when the call starts; the call leaves it all-zero again (the
 * decimation kernel clears it), so the owner zero-fills it once: two launches per frame instead of three.
 */
int dvmvs_depth_reproject_lowres_fwd(const float* transformation, const float* previous_depth, const float* full_K,
                                     const float* half_K, float* zbuffer, float* out_lowres, int lowres_factor,
                                     int B, int full_height, int full_width, dvmvs_stream_t stream);

/*
 * ABI 6.  The frame path in ONE launch: the ConvLSTM reads only rows / columns 0, f, 2f, ... of the estimate
 * (fusionnet/run-testing.py:176-189), so the splat goes straight into `estimate` [B,1,Hf/2/f,Wf/2/f] -- bit-identical to
 * out_lowres of the functions above -- which MUST be all-zero when the call starts.  `estimate_to_clear` (optional, another
 * buffer of that shape) is zero-filled by the same launch: a caller that alternates between two estimate buffers from frame
 * to frame zero-fills them once and never launches a clear.
 */
int dvmvs_depth_reproject_estimate_fwd(const float* transformation, const float* previous_depth, const float* full_K,
                                       const float* half_K, float* estimate, float* estimate_to_clear, int lowres_factor,
                                       int B, int full_height, int full_width, dvmvs_stream_t stream);

/*
 * Frame-path epilogues (not part of the reference's function list; they replace ATen elementwise / copy launches that sit
 * between MIOpen convolutions on the per-frame path, /root/reference/dvmvs/layers.py:39-65 and fusionnet/model.py:57,112,231-232,290-303).
 * At batch 1 a frame is ~250 launches of a few microseconds each, so what these buy is launches, not FLOPs.
 *   dvmvs_bias_act_fwd:     dst[b,c,:,:] = act(x[b,c,:,:] + bias[c]) [+ residual]; x is a dense [B,C,H,W] convolution output, dst may
 *                           be x (in place) or a CHANNEL SLICE of a larger buffer: batch item b starts at dst + b * dst_batch_stride
 *                           (in floats), its C planes are dense -- a torch.cat of convolution outputs is then never copied.
 *                           bias may be NULL; activation 0 none, 1 ReLU, 2 sigmoid, 3 sigmoid then the decoder's depth mapping
 *                           1 / (p0 * s + p1) (fusionnet/model.py:231-232,297-303); residual_mode 0 none, 1 residual [B,C,H,W]
 *                           (MnasNet shortcut), 2 residual [B,C,H/2,W/2] nearest-up-sampled on the fly (FPN top-down sum).
 *   dvmvs_bias_act_inplace: the same with dst = x (activations 0..2).
 *   dvmvs_upsample2x_fwd:   torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True);
 *                           in [B,C,H,W] -> out [B,C,2H,2W], batch item b at out + b * out_batch_stride (0 = dense).  With
 *                           pre_activation != 0 (1 ReLU, 2 sigmoid) the input is a raw convolution output and
 *                           act(in + pre_bias[c]) (pre_bias may be NULL) is applied to the taps on the fly.
 */
int dvmvs_bias_act_fwd(const float* x, float* dst, long long dst_batch_stride, const float* bias, const float* residual,
                       int residual_mode, int B, int C, int H, int W, int activation, float p0, float p1, dvmvs_stream_t stream);
int dvmvs_bias_act_inplace(float* x, const float* bias, const float* residual, int residual_mode, int B, int C, int H, int W,
                           int activation, dvmvs_stream_t stream);
int dvmvs_upsample2x_fwd(const float* in, float* out, long long out_batch_stride, const float* pre_bias, int pre_activation,
                         int B, int C, int H, int W, dvmvs_stream_t stream);
/* (ABI 8) Two dvmvs_upsample2x_fwd of maps of the same size [B,C1,H,W] and [B,C2,H,W] in ONE launch: job 1 without pre-activation, job 2 with
 * pre_bias2 / pre_activation2 (a decoder level's feature map and its one-channel depth head, /root/reference/dvmvs/fusionnet/model.py:262-296);
 * the same values bit for bit. */
int dvmvs_upsample2x_pair_fwd(const float* in1, float* out1, long long out1_batch_stride, int C1, const float* in2, float* out2,
                              long long out2_batch_stride, const float* pre_bias2, int pre_activation2, int C2, int B, int H, int W,
                              dvmvs_stream_t stream);
/*
 *   dvmvs_conv_bias_act_fwd: a dense convolution (square kernel K, zero padding, no dilation, one group) WITH its epilogue, as one
 *                           MIOpen fusion plan (convolution + bias [+ ReLU]): out = act(conv(x, weight) + bias[c]).  The convolution
 *                           is MIOpen's in either form; what this saves is the dvmvs_bias_act_fwd launch after it, for the problems
 *                           MIOpen gives to its fp32 Winograd kernel (for the others the plan is slower than convolution + epilogue:
 *                           the caller times both at warm-up, dvmvs/engine.py).  x [B,Cin,H,W], weight [Cout,Cin,K,K], bias [Cout],
 *                           out [B,Cout,Ho,Wo] with batch item b at out + b * out_batch_stride (0 = dense); activation 0 none, 1 ReLU.
 *                           The first call of a problem builds (compiles) its plan -- not inside a stream capture; later calls only
 *                           launch.  DVMVS_EUNSUPPORTED: MIOpen has no fused plan for the problem; DVMVS_ELIBRARY: a MIOpen call failed.
 */
int dvmvs_conv_bias_act_fwd(const float* x, const float* weight, const float* bias, float* out, long long out_batch_stride,
                            int B, int Cin, int H, int W, int Cout, int K, int stride, int padding, int activation, dvmvs_stream_t stream);
/*
 *   dvmvs_depthwise_conv_fwd: depthwise convolution (groups == C, weight [C,1,k,k], k in {3,5}, padding k/2, stride 1|2)
 *                           with bias (may be NULL) and activation fused; in [B,C,H,W] -> out [B,C,OH,OW].  The MnasNet
 *                           depthwise layers of the feature extractor (torchvision mnasnet _InvertedResidual).  With pre_relu != 0
 *                           the input is the RAW output of the preceding 1x1 expansion convolution and relu(in + pre_bias[c])
 *                           (pre_bias may be NULL) is applied to every in-bounds tap on the fly.
 */
int dvmvs_depthwise_conv_fwd(const float* in, const float* weight, const float* bias, const float* pre_bias, int pre_relu, float* out,
                             int B, int C, int H, int W, int kernel_size, int stride, int activation, dvmvs_stream_t stream);

/*
 * TSDF fusion of one RGB-D frame into a voxel volume, in place.  Replaces the `integrate` CUDA kernel the reference's
 * reconstruction script compiles with pycuda (/root/reference/sample-data/run-tsdf-reconstruction.py:79-152) and the
 * per-"gpu loop" launches around it (:240-268): one launch covers the whole volume.
 *   tsdf_vol, weight_vol, color_vol [dim_x,dim_y,dim_z]   (z fastest; colour folded as b * 65536 + g * 256 + r)
 *   origin_*, voxel_size    world position of voxel (0,0,0) and the voxel edge, metres
 *   cam_intr [3,3], cam_pose [4,4] camera-to-world        (device pointers)
 *   color_im, depth_im [im_h,im_w]   folded colour and depth in metres (0 = invalid)
 *   trunc_margin            truncation distance (the reference uses 5 voxels);  obs_weight  weight of this observation
 */
int dvmvs_tsdf_integrate(float* tsdf_vol, float* weight_vol, float* color_vol, int dim_x, int dim_y, int dim_z,
                         float origin_x, float origin_y, float origin_z, float voxel_size, const float* cam_intr,
                         const float* cam_pose, const float* color_im, const float* depth_im, int im_h, int im_w,
                         float trunc_margin, float obs_weight, dvmvs_stream_t stream);

/*
 * Marching cubes on a voxel volume: the mesh of the iso-surface value == level, with shared vertices in a fixed order.  Replaces
 * scikit-image's marching_cubes_lewiner in the reference's get_mesh / get_point_cloud (run-tsdf-reconstruction.py:313-351).
 *   vol [X,Y,Z] (z fastest), color_vol the same shape, folded as b * 65536 + g * 256 + r (may be NULL: no colours)
 *   A corner is inside when value < level.  Each voxel owns its +x, +y, +z edges; vertices are numbered by (linear index of the
 *   owner, axis x < y < z); triangles by (linear index of the cube's lowest corner, table order of csrc/marching_cubes_tables.h),
 *   counter-clockwise seen from the side of increasing values, where the normals point.  A volume with a dimension below 2 has
 *   V = F = 0.  Exact formulas: csrc/marching_cubes.hip.
 * Two calls, with one host read of V and F between them to size the outputs:
 *   dvmvs_marching_cubes_workspace_bytes   host only, no HIP call: 4 bytes per voxel + 24 per 256 voxels (0 for a bad shape)
 *   dvmvs_marching_cubes_count             counts_dev (device int64 [2]) <- V, F; keeps per-block offsets in the workspace
 *   dvmvs_marching_cubes_emit              with the SAME workspace, after _count: verts, normals [V,3] float32 (verts in world
 *                                          units: index * voxel_size + origin), colors [V,3] uint8 RGB (only when color_vol is
 *                                          given), faces [F,3] int32.  V and F as read from counts_dev; each below 2^31.
 */
size_t dvmvs_marching_cubes_workspace_bytes(int X, int Y, int Z);
int dvmvs_marching_cubes_count(const float* vol, int X, int Y, int Z, float level, void* workspace, size_t workspace_bytes,
                               long long* counts_dev, dvmvs_stream_t stream);
int dvmvs_marching_cubes_emit(const float* vol, const float* color_vol, int X, int Y, int Z, float level, float ox, float oy, float oz,
                              float voxel_size, void* workspace, float* verts, float* normals, unsigned char* colors, int* faces,
                              long long V, long long F, dvmvs_stream_t stream);

/*
 * Baselines (ABI 10): MVDepthNet and GP-MVS, the reference's dvmvs/baselines/{mvdepthnet,gpmvs}/run-testing.py.
 *
 * dvmvs_rgb_sweep_fwd: cost_volume_fusion(..., dot_product=False) of a 3-channel image (utils.py:45-107), written into a channel
 * slice of a caller-owned tensor; with copy_image = 1 the reference image goes into channels 0..2 of the same tensor, so one launch
 * yields the encoders' torch.cat((image, cost_volume), 1) input.  Bit-identical to dvmvs_cost_volume_fwd(dot_product = 0,
 * variant = 1) on the same arguments.  No gradient.
 *   image1      [B,3,H,W]   reference image            image2s  host array of M device pointers, each [B,3,H,W]
 *   Hm, kt      [B,M,9], [B,M,3] as for dvmvs_cost_volume_fwd; min_depth, max_depth, D as there (plane 0 = max_depth)
 *   out         [B,Cout,H,W]  the volume goes to channels [channel_offset, channel_offset + D); nothing else is written except,
 *               with copy_image = 1, channels 0..2 (= image1); every other channel keeps its contents
 *   Returns DVMVS_EUNSUPPORTED for C != 3, M > DVMVS_MAX_MEASUREMENTS, D > DVMVS_MAX_DEPTH_LEVELS or Cout * H * W >= 2^31;
 *   DVMVS_EINVAL for a null pointer, a non-positive dimension or depth, copy_image not 0 / 1, or a slice that overruns Cout or
 *   (copy_image = 1) overlaps channels 0..2.
 *
 * dvmvs_gp_filter_step: one step of GP-MVS's Kalman filter over the N = 512 * 8 * 10 bottleneck columns (run-testing.py:179-193), in
 * float64 like the reference's numpy:  M <- A M;  v = y - M[0];  M <- M + k v;  z = relu(float32(M[0])).
 *   state  [2,N] float64, in place (the reference's M)   y [N] fp32 (the encoder's conv5, read in place)   z [N] fp32 out
 *   a00..a11  A = expm(F dt) row-major;  k0, k1  the Kalman gain (host algebra of the poses: dvmvs.baselines.runner)
 *   reset  1 = start from M = 0 (a scene's first frame; the old state is not read), 0 = continue
 *   Returns DVMVS_EINVAL for a null pointer, N <= 0 or reset not 0 / 1; DVMVS_EUNSUPPORTED for N > 2^30.
 */
int dvmvs_rgb_sweep_fwd(const float* image1, const float* const* image2s, const float* Hm, const float* kt, float* out,
                        int B, int M, int C, int H, int W, int D, double min_depth, double max_depth, int Cout,
                        int channel_offset, int copy_image, dvmvs_stream_t stream);
int dvmvs_gp_filter_step(double* state, const float* y, float* z, int N, double a00, double a01, double a10, double a11,
                         double k0, double k1, int reset, dvmvs_stream_t stream);

/*
 * DPSNet baseline (ABI 11): the reference's dvmvs/baselines/dpsnet/dpsnet.py.  Forward only.
 *
 * dvmvs_dps_volume_fwd: the plane volume of one measurement frame (dpsnet.py:343-351, the loop of inverse_warp calls), in the layout
 * Conv3d reads.  Channels 0..C-1 hold the reference features at every plane; channels C..2C-1 the measurement features warped to
 * plane i, whose depth is fp32(mindepth) * nlabel / (i + 1e-16) (plane 0 lies at ~3.2e17, as in the reference).  Warp convention
 * (dpsnet.py:36-120, not the one of dvmvs_cost_volume_fwd): cam = (Kinv [x,y,1]) depth; p = (K pose)[:, :3] cam + (K pose)[:, 3];
 * Z = max(p_z, 1e-3); gx = 2 (p_x / Z) / (w - 1) - 1, gy likewise with h; gx or gy outside [-1, 1] becomes 2 (the sample reads
 * zeros); bilinear, zeros padding, align_corners = True.  K pose is taken in fp32 by the kernel.
 *   ref, meas  [B,C,h,w]      pose [B,3,4] (reference camera -> measurement camera)      K, Kinv [B,3,3] at the feature resolution
 *   out        [B,2C,nlabel,h,w], every element written
 *   Returns DVMVS_EINVAL for a null pointer, a non-positive dimension or mindepth; DVMVS_EUNSUPPORTED for C > 64,
 *   nlabel > DVMVS_MAX_DEPTH_LEVELS, B > 65535 or h * w >= 2^24.
 *
 * dvmvs_dps_regress_fwd: up-sampling, softmax and expectation (dpsnet.py:373-383):
 *   c = interpolate(costs, [nlabel,H,W], trilinear, align_corners = False)   (per plane: bilinear, half-pixel centres, clamped borders)
 *   pred = sum_i softmax(c)_i * i;      depth = mindepth * nlabel / (pred + 1e-16)
 * The costs are interpolated, then the softmax is taken (not the other way round).
 *   costs [B,nlabel,h,w] (= [B,1,nlabel,h,w])      depth [B,1,H,W] out      pred [B,H,W] out, or null: not written
 *   Returns DVMVS_EINVAL for a null costs / depth pointer, a non-positive dimension or mindepth; DVMVS_EUNSUPPORTED for
 *   nlabel > DVMVS_MAX_DEPTH_LEVELS, B > 65535, or h * w or H * W >= 2^30.
 */
int dvmvs_dps_volume_fwd(const float* ref, const float* meas, const float* pose, const float* K, const float* Kinv, float* out,
                         int B, int C, int h, int w, int nlabel, double mindepth, dvmvs_stream_t stream);
int dvmvs_dps_regress_fwd(const float* costs, float* depth, float* pred, int B, int nlabel, int h, int w, int H, int W,
                          double mindepth, dvmvs_stream_t stream);

/*
 * Frame pre-processing (ABI 11, later addition): dvmvs/dataset_loader.py's PreprocessImage.apply_rgb / apply_depth on the camera's raw
 * 8-bit frames and 16-bit depth maps, one launch per call for N frames.
 *
 * dvmvs_preprocess_rgb_fwd: centre crop, bilinear resampling (half-pixel centres, clamped edges, no anti-aliasing: resize_bilinear),
 * optional colour normalisation, HWC -> CHW.
 *   src   uint8 [N,H,W,3] interleaved RGB; row y of frame n starts at src + (n * H + y) * src_row_stride bytes (src_row_stride >= 3 W)
 *   dst   fp32 [N,3,new_h,new_w]; frame n starts at dst + n * dst_batch_stride elements (>= 3 new_h new_w: a slot of a larger buffer),
 *         its three planes are dense; 16-byte stores when new_w % 4 == 0 and dst and the stride are 16-byte aligned, scalar stores otherwise
 *   crop_x, crop_y   columns / rows dropped on EACH side before resampling (PreprocessImage.crop_x / crop_y); w = W - 2 crop_x, h likewise
 *   normalize  1: (v / scale - mean_host[c]) / std_host[c] with fp32(scale) and the two HOST arrays of 3 floats; 0: the resampled
 *              0..255 values (scale, mean_host, std_host are not read and may be null)
 * Arithmetic contract: xs = max((x + 0.5) * (w / new_w) - 0.5, 0), x0 = min(floor(xs), w - 1), x1 = min(x0 + 1, w - 1),
 * fx = fp32(xs - x0) in DOUBLE, rows likewise: tap indices and weights are bit-identical to the host function's.  Then in fp32, every
 * operation rounded (no FMA contraction), in the host's order: top = a (1 - fx) + b fx; bottom likewise; top (1 - fy) + bottom fy;
 * / scale; - mean; / std, with correctly rounded divisions.
 *
 * dvmvs_preprocess_depth_fwd: crop, nearest resampling (source index min(int(x * (w / (double)new_w)), w - 1): resize_nearest), and
 * fp32((double)d / scaling): the fp32 rounding of load_depth_png + apply_depth.
 *   src   uint16 [N,H,W] dense      dst   fp32 [N,new_h,new_w] dense
 *
 * Both return DVMVS_EINVAL for a null src / dst, N < 1, a non-positive size, a negative crop or one that leaves no pixels, a row or
 * batch stride smaller than a row / an output frame, normalize not 0 / 1, and -- with normalize = 1 -- a null mean_host / std_host,
 * fp32(scale) == 0 or a std_host[c] == 0; scaling == 0.  DVMVS_EUNSUPPORTED for N > 65535 or a frame whose offsets do not fit the
 * kernels' 32-bit indices: src_row_stride or H * src_row_stride >= 2^31 bytes, 3 new_h new_w >= 2^31 elements, dst_batch_stride >= 2^40
 * elements (depth: H W or new_h new_w >= 2^31).
 */
int dvmvs_preprocess_rgb_fwd(const unsigned char* src, float* dst, int N, int H, int W, long long src_row_stride, int crop_x, int crop_y,
                             int new_h, int new_w, long long dst_batch_stride, double scale, const float* mean_host,
                             const float* std_host, int normalize, dvmvs_stream_t stream);
int dvmvs_preprocess_depth_fwd(const unsigned short* src, float* dst, int N, int H, int W, int crop_x, int crop_y, int new_h, int new_w,
                               double scaling, dvmvs_stream_t stream);

/*
 * Depth evaluation (ABI 11, later addition): the eight metrics of dvmvs/errors.py::compute_errors (the reference's dvmvs/errors.py:4-28)
 * for n_frames (ground truth, prediction) pairs in ONE launch.
 *   gt, pred   fp32 [n_frames, pixels] dense; the base pointers need 4-byte alignment only and pixels may be any positive number: a
 *              frame whose two rows are 16-byte aligned is read with 16-byte loads, any other with scalar loads, with the same result
 *   max_depth  fp32; +inf = no upper bound
 *   metrics    fp32 [n_frames, 8] out: abs_error, abs_relative_error, abs_inverse_error, squared_relative_error, rmse, ratio_125,
 *              ratio_125_2, ratio_125_3
 *   counts     int [n_frames, 4] out, or null: n and the three inlier counts
 *   workspace  dvmvs_depth_errors_workspace_bytes(n_frames, pixels) bytes, 8-byte aligned: per-frame integer tickets followed by the
 *              per-workgroup partial sums.  The ticket words (the first 4 n_frames bytes) must be ZERO before the first call; every
 *              call leaves them zero, so consecutive calls need no memset.  Calls that share a workspace must be ordered (one stream).
 * Arithmetic contract.  A pixel takes part iff gt >= 0.5f && gt <= max_depth (a NaN gt fails both).  Per pixel, in fp32, every
 * operation rounded, no FMA contraction, correctly rounded divisions -- compute_errors' elementwise operations on fp32 arrays:
 *   d = gt - pred;  |d|;  |d| / gt;  |1 / gt - 1 / pred|;  d d / gt;  d d;  ratio = max(gt / pred, pred / gt) where a NaN operand
 *   gives NaN (np.maximum, not fmaxf).
 * ratio < 1.25f, < 1.5625f, < 1.953125f are counted as integers; a NaN ratio is never an inlier.  pred is not filtered: a zero,
 * negative, infinite or NaN prediction gives what IEEE arithmetic gives numpy (inf / NaN in the affected metrics).  The five sums are
 * accumulated in fp64 in an order that is a function of `pixels` alone (per-thread strided partial sums, a fixed tree in the workgroup,
 * per-workgroup partial sums added by index by the workgroup that draws the frame's last ticket; no floating-point atomics): results
 * are bit-identical run to run, for any n_frames, and for either load width.  Row: fp32(sum / n) for the first four metrics,
 * fp32(sqrt(sum / n)) for rmse, fp32(count_k) / fp32(n) for the ratios (both exact below 2^24); n = 0 gives eight NaNs.
 * Returns DVMVS_EINVAL for a null gt / pred / metrics / workspace, n_frames < 1, pixels < 1, a NaN max_depth, a pointer that is not
 * 4-byte (workspace: 8-byte) aligned; DVMVS_EUNSUPPORTED for pixels >= 2^24 (fp32 no longer holds the counts exactly) or
 * n_frames > 65535.  dvmvs_depth_errors_workspace_bytes returns 0 for sizes the entry point refuses.
 */
size_t dvmvs_depth_errors_workspace_bytes(int n_frames, long long pixels);
int dvmvs_depth_errors_fwd(const float* gt, const float* pred, int n_frames, long long pixels, float max_depth, float* metrics,
                           int* counts, void* workspace, dvmvs_stream_t stream);

/*
 * TSDF ray-casting (ABI 11, later addition): depth, world-space normal and colour of the first zero crossing of a fused volume along
 * every pixel's ray, for n_views cameras in ONE launch.  The reference project has no ray-caster: the definition is this project's own.
 *   tsdf_vol, weight_vol, color_vol [dim_x,dim_y,dim_z]   the volumes of dvmvs_tsdf_integrate (z fastest); color_vol may be NULL when rgb is
 *   origin_*, voxel_size    world position of voxel (0,0,0) and the voxel edge, metres
 *   mask                    brick mask written by dvmvs_tsdf_raycast_mask for the SAME volume contents, or NULL = dense march.  Both
 *                           give the same bits; a mask built before the volume changed is stale and must not be passed.
 *   cam_intr [n_views,3,3], cam_pose [n_views,4,4] camera-to-world   (device pointers)
 *   near, far               depth range in metres: 0 <= near < inf; far may be +inf
 *   step                    sample spacing along the ray in voxels, 0 < step <= 5 (the truncation)
 *   depth [n_views,im_h,im_w] fp32 out (0 = no surface); normal [n_views,im_h,im_w,3] fp32 out or NULL; rgb [n_views,im_h,im_w,3] uint8
 *   out or NULL.
 * Per pixel (u, v), in fp32, every operation rounded, no FMA contraction, correctly rounded divisions and square roots:
 *   d_c = ((u - cx) / fx, (v - cy) / fy, 1);  o_g = (t - origin) / voxel_size;  d_g = (R d_c) / voxel_size with each row of R d_c summed left
 *   to right;  g(z) = o_g + z d_g is the ray in voxel coordinates and z is the camera depth.
 *   [z0, z1] = the slab intersection of the ray with the box [0, dim - 1]^3 cut to [near, far]; a component d_g == 0 contributes
 *   (-inf, +inf) when o_g lies in its slab and nothing otherwise.  A non-finite o_g, d_g, z0, z1 or step / |d_g|, or z0 > z1: a miss.
 *   dz = step / |d_g|;  n = min(floor((z1 - z0) / dz), n_cap), n_cap = floor(sqrt(sum (dim - 1)^2) / step) + 2 evaluated in double;
 *   z_k = z0 + float(k) dz for k = 0..n (never accumulated).
 *   f_k = trilinear tsdf at g(z_k) clamped to the box, in the cell i0 = min(floor(g), dim - 2), as lerp(a, b, w) = a (1 - w) + b w along
 *   z, then y, then x.  Sample k is valid when all eight corner weights of its cell are > 0.
 *   Hit: the first k >= 1 with samples k - 1 and k valid and f_{k-1} > 0 >= f_k;  depth = z_{k-1} + dz (f_{k-1} / (f_{k-1} - f_k)).
 *   Normal at the hit point g* = clamp(o_g + depth d_g): per axis the difference of the same trilinear tsdf at clamp(g* + 1 voxel) and
 *   clamp(g* - 1 voxel), the three differences divided by their Euclidean norm; (0,0,0) when one of the six samples is invalid, the norm
 *   is zero, or on a miss.  Colour: the folded colour voxel at rint(g*) per axis (clamped), decoded as dvmvs_marching_cubes_emit decodes a
 *   vertex colour; 0 on a miss.
 * dvmvs_tsdf_raycast_mask_bytes: host only, no HIP call: one byte per 8x8x8 brick of cells,
 *   ceil((dim_x - 1) / 8) * ceil((dim_y - 1) / 8) * ceil((dim_z - 1) / 8); 0 for a shape the entry points refuse.
 * dvmvs_tsdf_raycast_mask: mask[brick] (z fastest) <- 1 when a corner of one of the brick's cells has weight > 0 && tsdf <= 0, else 0.
 * Returns DVMVS_EINVAL for a null tsdf_vol / weight_vol / cam_intr / cam_pose / depth (mask entry point: mask), rgb without color_vol,
 * a dimension below 2, n_views, im_h or im_w < 1, voxel_size <= 0, step outside (0, 5], near < 0 or not finite, a NaN far;
 * DVMVS_EUNSUPPORTED for dim_y * dim_z >= 2^31, 2^26 bricks or more, im_h * im_w >= 2^31, im_h > 16 * 65535, n_views > 65535,
 * ceil(im_w / 16) * ceil(im_h / 16) * n_views >= 2^24 (a launch of 256-thread workgroups holds fewer than 2^32 threads), or a
 * march of 2^20 samples or more (n_cap).  Nothing is enqueued in either case.
 */
size_t dvmvs_tsdf_raycast_mask_bytes(int dim_x, int dim_y, int dim_z);
int dvmvs_tsdf_raycast_mask(const float* tsdf_vol, const float* weight_vol, int dim_x, int dim_y, int dim_z, unsigned char* mask,
                            dvmvs_stream_t stream);
int dvmvs_tsdf_raycast_fwd(const float* tsdf_vol, const float* weight_vol, const float* color_vol, int dim_x, int dim_y, int dim_z,
                           float origin_x, float origin_y, float origin_z, float voxel_size, const unsigned char* mask,
                           const float* cam_intr, const float* cam_pose, int n_views, int im_h, int im_w, float near, float far, float step,
                           float* depth, float* normal, unsigned char* rgb, dvmvs_stream_t stream);

/*
 * TSDF fusion of a batch of frames (ABI 11, later addition): dvmvs_tsdf_integrate applied to n_frames frames in index order, in ONE pass
 * over the volume, with the SAME BITS as n_frames calls of dvmvs_tsdf_integrate: a thread owns its voxels for the launch, loads them once,
 * applies the frames 0..n_frames-1 in registers with that kernel's float32 statements and stores a voxel only if a frame updated it.
 *   tsdf_vol, weight_vol, color_vol, dim_*, origin_*, voxel_size, trunc_margin   as dvmvs_tsdf_integrate
 *   cam_intr [n_frames,3,3], cam_pose [n_frames,4,4] camera-to-world, depth [n_frames,im_h,im_w] fp32 metres   (device pointers)
 *   rgb_u8 [n_frames,im_h,im_w,3] uint8 RGB or NULL; folded [n_frames,im_h,im_w] fp32 (b * 65536 + g * 256 + r) or NULL   (device pointers):
 *                           exactly one of the two; 8-bit colour is folded in the kernel, exactly
 *   obs_weight_host         HOST array of n_frames weights, read during the call (it travels in the kernel arguments)
 *   max_depth               a depth > max_depth counts as 0 (invalid); +inf = no clamp; a NaN depth stays NaN and, as in the dense kernel,
 *                           is integrated with dist = 1
 *   workspace               dvmvs_tsdf_integrate_frames_workspace_bytes(n_frames) bytes on the device, 4-byte aligned, written by a first
 *                           kernel of the call (the largest clamped depth of every frame) and read by the fusion kernel: no host read.  Calls
 *                           that share it must be ordered (one stream)
 *   tile_stats              device long long[2] or NULL; when given, the call ADDS to element 0 the number of (tile, frame) pairs its
 *                           culling kept and to element 1 the number of tiles that loaded the volume (integer atomics, one thread per
 *                           workgroup).  For tests and benchmarks
 * The volume is cut into tiles, one workgroup each.  A frame is dropped for a tile only when no voxel of the tile can pass that frame's
 * per-voxel tests (behind the camera, outside the four image sides, beyond the frame's largest depth + trunc_margin), with margins that
 * cover the float32 error of the per-voxel projection (derivation in csrc/tsdf_fuse.hip); a tile that no frame can touch makes no volume
 * access.  A launch takes 64 frames; more are split into consecutive launches in frame order by the call.
 * dvmvs_tsdf_integrate_frames_workspace_bytes: host only, no HIP call; 0 for n_frames <= 0, non-decreasing in n_frames.
 * Returns DVMVS_EINVAL for a null tsdf_vol / weight_vol / color_vol / cam_intr / cam_pose / depth / obs_weight_host / workspace, both or neither
 * of rgb_u8 and folded, a dimension, image size or n_frames < 1, voxel_size or trunc_margin <= 0, a NaN max_depth; DVMVS_EUNSUPPORTED for
 * dim_y * dim_z >= 2^31, im_h * im_w >= 2^31, n_frames > 65535 or 2^31 tiles or more.  Nothing is enqueued in either case.
 */
size_t dvmvs_tsdf_integrate_frames_workspace_bytes(int n_frames);
int dvmvs_tsdf_integrate_frames(float* tsdf_vol, float* weight_vol, float* color_vol, int dim_x, int dim_y, int dim_z, float origin_x,
                                float origin_y, float origin_z, float voxel_size, const float* cam_intr, const float* cam_pose,
                                const unsigned char* rgb_u8, const float* folded, const float* depth, int n_frames, int im_h, int im_w,
                                float trunc_margin, const float* obs_weight_host, float max_depth, void* workspace, long long* tile_stats,
                                dvmvs_stream_t stream);

/*
 * Nearest-point distances between point clouds and the 3-D reconstruction metrics (ABI 11, later addition).  The reference project has
 * nothing for this: the definitions are this project's own (the metrics are those of the Atlas / NeuralRecon / SimpleRecon evaluations).
 *   target [M,3], query [N,3]   fp32, contiguous, 4-byte aligned, FINITE (a precondition; not checked on the device)
 *   workspace         dvmvs_nearest_workspace_bytes(M) bytes on the device, 16-byte aligned: written by dvmvs_nearest_build, read by
 *                     dvmvs_nearest_distance_fwd.  It holds a header (the targets' bounding box, the cell edge and the dimensions of a
 *                     uniform grid over the box, all computed on the device), the cells' end offsets and a copy of the targets sorted by
 *                     cell with their original indices.  The host sizes it from M alone and never reads it.  Header, for tests and tools:
 *                     float mn[3], mx[3], inv_h, h_lo; int dim[3], ncells (48 bytes); cell_a(x) = int((clamp(x, mn_a, mx_a) - mn_a) * inv_h).
 *   query_workspace   dvmvs_nearest_query_workspace_bytes(N, M) bytes on the device, 16-byte aligned, scratch of one query call (the
 *                     queries binned by the same grid, so that a wave works on neighbouring cells).  Calls that share it must be ordered.
 *   dist [N] fp32 out; index [N] int32 out or NULL
 * Arithmetic contract.  d2(q, t) = (dx dx + dy dy) + dz dz with dx = q.x - t.x, dy, dz likewise; every operation rounded to fp32, no FMA
 * contraction.  dist[i] = sqrt(min over j of d2(query_i, target_j)), the square root correctly rounded; index[i] = the SMALLEST j that
 * attains the minimum.  The minimum does not depend on the order of evaluation, so dist and index are bit-identical to a brute force over
 * all j, run to run, on any stream.  The search visits the cells around the query's cell (for a query outside the box: the cell of its
 * clamp onto the box) in growing Chebyshev rings and stops only, and never before ring 1, when the best d2 is provably smaller than that of every unvisited
 * target (bound and its fp32 margins: csrc/nearest_points.hip); otherwise it goes on until it has visited the whole grid.  Degenerate
 * target sets (one point, coincident, collinear, coplanar) are legal.  The float32 result is within 4 * 2^-24 * d of the exact distance.
 * dvmvs_nearest_distance_fwd with N == 0 enqueues nothing and returns 0.
 * dvmvs_distance_metrics_fwd: dist_a [Na] (prediction -> ground truth), dist_b [Nb] (ground truth -> prediction), fp32 threshold ->
 *   row fp32 [6]: acc = mean(dist_a), comp = mean(dist_b), chamfer = (acc + comp) / 2, precision = count(dist_a < threshold) / Na,
 *   recall = count(dist_b < threshold) / Nb, fscore = 2 P R / (P + R) (0 when P + R == 0);  counts long long [2] out or NULL: the two
 *   counts.  The sums run in fp64 in ONE workgroup in an order that is a function of (Na, Nb) alone; the means, shares, chamfer and
 *   fscore are formed in fp64 from them and rounded to fp32 once each.
 * The two *_workspace_bytes: host only, no HIP call; 0 for M <= 0 (N <= 0) or above 2^28 points; non-decreasing in M (and N).
 * Returns DVMVS_EINVAL for a null target / workspace (with N > 0: query / query_workspace / dist), M < 1, N < 0, workspace_bytes or
 * query_workspace_bytes too small,
 * a misaligned pointer; metrics: a null dist_a / dist_b / row, Na or Nb < 1, a NaN threshold, counts not 8-byte aligned;
 * DVMVS_EUNSUPPORTED above 2^28 points.  Nothing is enqueued in either case.
 */
size_t dvmvs_nearest_workspace_bytes(long long M);
size_t dvmvs_nearest_query_workspace_bytes(long long N, long long M);
int dvmvs_nearest_build(const float* target, long long M, void* workspace, size_t workspace_bytes, dvmvs_stream_t stream);
int dvmvs_nearest_distance_fwd(const float* query, long long N, const float* target, long long M, const void* workspace,
                               void* query_workspace, size_t query_workspace_bytes, float* dist, int* index, dvmvs_stream_t stream);
int dvmvs_distance_metrics_fwd(const float* dist_a, long long Na, const float* dist_b, long long Nb, float threshold, float* row,
                               long long* counts, dvmvs_stream_t stream);

/*
 * Depth-map consistency (ABI 11, later addition): keeps the pixels of N depth maps that enough neighbouring views agree on.  The reference
 * project has nothing for this: the definition is this project's own (the geometric check of the MVSNet family's fusion step).
 *   depth   [N,H,W] fp32, dense.  A pixel is VALID iff it is finite and > 0
 *   K       [N,3,3] fp32; only fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2] are read
 *   pose    [N,4,4] fp32, camera-to-world, rigid (only the top three rows are read)
 *   sources [N,S] int32 device table, 0 <= S <= 16: slot j of frame r names a source frame s = sources[r][j] of the same batch.  A slot with
 *           s < 0, s >= N or s == r is SKIPPED, on the device (no host read).  A frame named twice counts twice.  May be NULL when S == 0
 *   pixel_threshold, relative_threshold   fp32 (usual values 1.0 and 0.01); min_views >= 0; average 0 / 1
 *
 * Step A, dvmvs_consistency_matrices: one thread per (r, j), float64 from the float32 inputs, no FMA contraction, each result rounded once
 * to fp32.  With pose = [R|t] and a -> b meaning "from frame a's pixels to frame b's":
 *   Rab[i][j] = (Rb[0][i] Ra[0][j] + Rb[1][i] Ra[1][j]) + Rb[2][i] Ra[2][j]                       (inv_rigid(pose_b) pose_a, rotation)
 *   ti[i]     = -((Rb[0][i] tb[0] + Rb[1][i] tb[1]) + Rb[2][i] tb[2])                              (inv_rigid = (R^T, -R^T t))
 *   tab[i]    = ((Rb[0][i] ta[0] + Rb[1][i] ta[1]) + Rb[2][i] ta[2]) + ti[i]
 *   M = K_b Rab:  M[0][j] = fx_b Rab[0][j] + cx_b Rab[2][j],  M[1][j] = fy_b Rab[1][j] + cy_b Rab[2][j],  M[2][j] = Rab[2][j]
 *   A = M K_a^-1: A[i][0] = M[i][0] (1 / fx_a),  A[i][1] = M[i][1] (1 / fy_a),
 *                 A[i][2] = (M[i][0] (-(cx_a / fx_a)) + M[i][1] (-(cy_a / fy_a))) + M[i][2]
 *   b = K_b tab:  b[0] = fx_b tab[0] + cx_b tab[2],  b[1] = fy_b tab[1] + cy_b tab[2],  b[2] = tab[2]
 *   matrices [N,S,2,12] fp32 out: [r][j][0] = (A row-major, b) for a = r, b = s;  [r][j][1] = (A', b') for a = s, b = r.  A skipped slot is
 *   written as 24 zeros.  S == 0 writes nothing.
 *
 * Step B, dvmvs_depth_consistency_fwd: one launch for all N frames; fp32 throughout, every operation rounded (no FMA contraction), divisions
 * correctly rounded, in exactly this order for pixel (u, v) of frame r with valid d and each non-skipped slot j (u, v as fp32):
 *   1. p[i] = d * ((A[i][0] u + A[i][1] v) + A[i][2]) + b[i];  require p.z > 0;  us = p.x / p.z, vs = p.y / p.z;
 *      require 0 <= us <= W - 1 and 0 <= vs <= H - 1
 *   2. x0 = min(floor(us), W - 2), y0 = min(floor(vs), H - 2), wx = us - x0, wy = vs - y0;  the four taps t00 = depth[s][y0][x0],
 *      t01 = [y0][x0 + 1], t10 = [y0 + 1][x0], t11 = [y0 + 1][x0 + 1] must all be valid;
 *      top = t00 + wx (t01 - t00), bot = t10 + wx (t11 - t10), ds = top + wy (bot - top)
 *   3. q[i] = ds * ((A'[i][0] us + A'[i][1] vs) + A'[i][2]) + b'[i];  require q.z > 0;  du = q.x / q.z - u, dv = q.y / q.z - v
 *   4. the slot is CONSISTENT iff du du + dv dv < pixel_threshold^2 (squared once, in fp32; no square root anywhere) and
 *      |q.z - d| / d < relative_threshold
 *   5. count = number of consistent slots;  fused = (d + sum of q.z over the consistent slots, in slot order) / fp32(count + 1)
 *   6. out_depth [N,H,W] fp32 = count >= min_views ? (average ? fused : d) : 0;  0 for an invalid d
 *      count     [N,H,W] uint8 or NULL: the count; 0 for an invalid d
 *      points    [N,H,W,3] fp32 or NULL: world position of the pixel at z = out_depth: xn = (u - cx) / fx, yn = (v - cy) / fy,
 *                X = z xn, Y = z yn, Z = z, world[i] = ((P[i][0] X + P[i][1] Y) + P[i][2] Z) + P[i][3] with K_r, P = pose_r;
 *                zeros where out_depth is 0
 *   A map with H < 2 or W < 2 has no tap cell: every slot is inconsistent.
 * matrices: step A's output for the same K, pose and sources.  out_depth must not overlap depth.
 * Every output element has one writer and no value crosses threads: the results depend on nothing but the inputs -- a frame filtered alone
 * with its sources gives the bits it has inside a larger batch with re-indexed sources, and two calls give the same bits.
 * Both return DVMVS_EINVAL for a null K / pose / matrices (with S > 0: sources; pixels: depth / out_depth), N < 1, S outside [0,16],
 * H or W < 1, a NaN threshold, min_views < 0, average not 0 / 1, a pointer to 32-bit words that is not 4-byte aligned; DVMVS_EUNSUPPORTED
 * for N > 65535 or 3 H W >= 2^31 (offsets inside a frame are 32-bit).  Nothing is enqueued in either case.
 */
int dvmvs_consistency_matrices(const float* K, const float* pose, const int* sources, float* matrices, int N, int S,
                               dvmvs_stream_t stream);
int dvmvs_depth_consistency_fwd(const float* depth, const float* K, const float* pose, const int* sources, const float* matrices,
                                float* out_depth, unsigned char* count, float* points, int N, int S, int H, int W,
                                float pixel_threshold, float relative_threshold, int min_views, int average, dvmvs_stream_t stream);

/*
 * Point sets for the 3-D reconstruction metrics (ABI 11, later addition): samples of a triangle mesh in proportion to its faces' areas, and
 * the voxel down-sampling of a point cloud.  The reference project has nothing for this: the definitions are this project's own (the
 * protocol is that of the Atlas / NeuralRecon / TransformerFusion / SimpleRecon evaluations); dvmvs/errors.py restates them in numpy
 * (sample_surface, voxel_down_sample) and the device reproduces those bit for bit.  No float atomics; no FMA contraction; every entry
 * runs on `stream`; the host reads `counts` once between a *_count and its *_emit, to size the output.
 *
 * Surface sampling.  verts [V,3] fp32, faces [F,3] int32, density > 0 (points per square metre), seed (32 bits).
 *   1. A_f = int64(rint(sqrt(n2) * 0.5 * 2^32)) with, in fp64 from the fp32 corners a, b, c of face f: e1 = b - a, e2 = c - a,
 *      cx = e1.y e2.z - e1.z e2.y, cy = e1.z e2.x - e1.x e2.z, cz = e1.x e2.y - e1.y e2.x, n2 = (cx cx + cy cy) + cz cz; every operation
 *      rounded.  A face with an index outside [0, V) has A_f = 0 and no vertex is read for it.  cum_f = A_0 + ... + A_f, exact.  An A_f that
 *      is not below 2^63 (or not a number), or a total of 2^63 and more (2^31 square metres), is an error: counts[1] = 1, N = 0.
 *   2. D = max(int64(rint(2^32 / density)), 1); t_k = k D + (D >> 1); N = 0 if cum_{F-1} <= D >> 1, else (cum_{F-1} - (D >> 1) - 1) / D + 1;
 *      sample k belongs to the face f with cum_{f-1} <= t_k < cum_f (found by binary search, one thread per sample).
 *   3. lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32).  r0 = lowbias32(seed),
 *      r1 = lowbias32(seed + 1); h1 = uint32(k) 0xC13FA9A9 + r0, h2 = uint32(k) 0x91E10DA5 + r1; u = fp32(h1 >> 8) 2^-24, v likewise from h2;
 *      if u + v > 1 (fp32): u = 1 - u, v = 1 - v;  p = (a + u (b - a)) + v (c - a) per component in fp32, every operation rounded.
 *   workspace   dvmvs_surface_sample_workspace_bytes(F) bytes on the device, 8-byte aligned: written by _count (it holds cum), read by _emit
 *   counts      long long [3] on the device, out of _count: N, the status (0, or 1 = the error of step 1) and cum_{F-1}
 *   points [N,3] fp32 out, in ascending k;  face [N] int32 out or NULL: the face of each sample
 * dvmvs_surface_sample_emit takes the N that _count of the same mesh and density produced; N == 0 enqueues nothing and returns 0.
 *
 * Voxel down-sampling.  points [N,3] fp32, FINITE, N >= 1; inv_voxel = fp32(1 / fp64(voxel)), computed by the host.
 *   mn = the per-axis minimum of the cloud (exact); cell c_a = int32((x_a - mn_a) inv_voxel): one fp32 subtraction, one fp32 product, each
 *   rounded, then truncation; a c_a of 2^21 or more (or a coordinate that is not finite) is an error: status 1, and that cell counts as 0.
 *   key = (c_x << 42) | (c_y << 21) | c_z.  dvmvs_voxel_keys writes key [N] int64 (and mn into the workspace).  The CALLER sorts the keys
 *   stably with their indices 0 .. N-1 (both int64).  dvmvs_voxel_downsample_count takes the sorted arrays: counts long long [2] on the
 *   device receives M, the number of distinct keys, and the status of dvmvs_voxel_keys for the same workspace.  dvmvs_voxel_downsample_emit
 *   writes out [M,3] fp32, the voxels in ascending key order: out[m][a] = fp32((0.0 + x_i0 + x_i1 + ...) / n), the sum in fp64 over the
 *   voxel's points in ascending index, the division in fp64, one rounding;  count [M] int32 out or NULL: n.  One thread per voxel walks a
 *   copy of the points in sorted order: linear in N.
 *   workspace   dvmvs_voxel_downsample_workspace_bytes(N) bytes on the device, 16-byte aligned, shared by the three calls of one cloud
 * The two *_workspace_bytes: host only, no HIP call; 0 for F (N) <= 0 or above 2^28; non-decreasing.
 * Every entry returns DVMVS_EINVAL for a null or misaligned pointer (verts may be null when V == 0), F < 1, N < 1 (surface emit: N < 0),
 * V < 0, a density or inv_voxel that is not positive and finite, M outside [1, N], a workspace that is too small, an N for which t_k does
 * not fit 63 bits; DVMVS_EUNSUPPORTED for F, N above 2^28 or V above 2^31 - 1.  Nothing is enqueued in either case.
 */
size_t dvmvs_surface_sample_workspace_bytes(long long F);
int dvmvs_surface_sample_count(const float* verts, long long V, const int* faces, long long F, double density, void* workspace,
                               size_t workspace_bytes, long long* counts, dvmvs_stream_t stream);
int dvmvs_surface_sample_emit(const float* verts, long long V, const int* faces, long long F, double density, unsigned int seed,
                              const void* workspace, long long N, float* points, int* face, dvmvs_stream_t stream);
size_t dvmvs_voxel_downsample_workspace_bytes(long long N);
int dvmvs_voxel_keys(const float* points, long long N, float inv_voxel, void* workspace, size_t workspace_bytes, long long* keys,
                     dvmvs_stream_t stream);
int dvmvs_voxel_downsample_count(const float* points, long long N, const long long* sorted_keys, const long long* sorted_index,
                                 void* workspace, size_t workspace_bytes, long long* counts, dvmvs_stream_t stream);
int dvmvs_voxel_downsample_emit(long long N, long long M, const void* workspace, float* out, int* count, dvmvs_stream_t stream);

/*
 * Mesh rasterisation (ABI 11, later addition): the depth and the face of a triangle mesh at every pixel of n_views cameras, with a
 * z-buffer, in ONE call; and which vertices a set of depth maps shows.  The reference project has no rasteriser: the definition is this
 * project's own; tests/mesh_raster_reference.py restates it in numpy and the device reproduces that bit for bit.
 *   verts [V,3] fp32 world space; faces [F,3] int32; cam_intr [n_views,3,3] (fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2]);
 *   cam_w2c [n_views,3,4] WORLD-TO-CAMERA (R | t), row-major; near > 0, finite; far (may be +inf); cull_backfaces 0 / 1;
 *   large_box >= 1: see "work" below, it cannot change a result (DVMVS_MESH_RASTER_LARGE_BOX is the measured choice).
 * fp32 throughout, every operation rounded (no FMA contraction), divisions correctly rounded, in exactly this order for view r, face f:
 *   1. A face with an index outside [0, V) is skipped; no vertex is read for it.  Camera space, per corner j (a, b, c in the face's order):
 *      p_j[i] = ((M[i][0] x + M[i][1] y) + M[i][2] z) + M[i][3].  A face with a coordinate that is not finite is skipped.
 *   2. Plane of the UNCLIPPED triangle: e1 = b - a, e2 = c - a; nx = e1.y e2.z - e1.z e2.y, ny = e1.z e2.x - e1.x e2.z,
 *      nz = e1.x e2.y - e1.y e2.x; na = (nx a.x + ny a.y) + nz a.z; lo = fmaxf(fminf(fminf(a.z, b.z), c.z), near),
 *      hi = fmaxf(fmaxf(a.z, b.z), c.z).  With cull_backfaces the face is skipped unless na < 0 (it then shows the camera the side from which
 *      its corners run counter-clockwise, the outside of a dvmvs_marching_cubes_emit mesh).
 *   3. Near plane: corner j is BEHIND when p_j.z < near.  Three behind: the face is skipped.  None: one triangle (a, b, c).  Otherwise the
 *      corners are rotated, keeping their cyclic order, to (v0, v1, v2) with v0 the odd one out, and the point where the edge from a corner
 *      g behind to a corner h in front meets the plane is clip(g, h): t = (near - g.z) / (h.z - g.z), x = g.x + t (h.x - g.x), y likewise,
 *      z = near (always from the corner behind, so two faces that share the edge compute the same point).
 *      One behind (v0): piece 0 = (clip(v0,v1), v1, v2), piece 1 = (clip(v0,v1), v2, clip(v0,v2)).
 *      Two behind (v1, v2): piece 0 = (v0, clip(v1,v0), clip(v2,v0)).
 *   4. Every corner of a piece is projected and snapped to 8 sub-pixel bits: xp = (x / z) fx + cx, sx = rintf(256 xp), the same in y.  A piece
 *      with |sx| or |sy| above 2^29 (2^21 pixels) or not a number at a corner is LEFT OUT and adds one to overflow[r]; else X = (int) sx.
 *   5. Coverage, in int64 (no product exceeds 2^61): area = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0); a piece with area 0 is skipped; with
 *      area < 0 its corners 1 and 2 are exchanged.  For the edges i -> j = 0 -> 1, 1 -> 2, 2 -> 0: dx = Xj - Xi, dy = Yj - Yi,
 *      E(u, v) = dx (256 v - Yi) - dy (256 u - Xi): pixel (u, v), sampled AT its integer coordinates as the ray-caster's, is covered when
 *      for every edge E > 0, or E == 0 and the edge is a top or left one: dy < 0, or dy == 0 and dx > 0.  Two pieces that share an edge
 *      cover each sample on it exactly once.  Only pixels inside the image are looked at.
 *   6. Depth of a covered pixel: dx = (u - cx) / fx, dy = (v - cy) / fy, den = (nx dx + ny dy) + nz, z = fminf(fmaxf(na / den, lo), hi).
 *      fmaxf and fminf return their other operand for a NaN, so z is finite and near <= lo <= z <= hi whatever na / den is (a grazing
 *      triangle).  z depends on (r, f, u, v) alone, not on the piece.  A pixel with z > far is not written.
 *   7. Z-buffer: key = (bits of z << 32) | f, a 64-bit unsigned atomic minimum per pixel (positive floats order as their bits): the nearest
 *      depth wins and, at equal depths, the lowest face index; the result does not depend on the order of arrival.
 *   8. depth [n_views,im_h,im_w] fp32 out (0 = nothing), face [n_views,im_h,im_w] int32 out (-1 = nothing), overflow [n_views] int32 out.
 * Work: a piece whose box of candidate pixels holds at most large_box pixels is rasterised by the thread of its (view, face); a larger one is
 * appended, once per 16x16 tile of the image grid that its box meets, to a list in the workspace that resident workgroups then stride
 * over, one pixel per lane; the length of the list is read on the device.
 *   workspace   dvmvs_mesh_raster_workspace_bytes(n_views, F, im_h, im_w) bytes on the device, 16-byte aligned.  Every call writes what it
 *               reads first (keys, list length): no initial state is needed, and a buffer may serve calls of different sizes in turn.
 * dvmvs_mesh_raster_workspace_bytes: host only, no HIP call; 0 for a shape that dvmvs_mesh_raster_fwd refuses.
 * dvmvs_mesh_raster_cameras: cam_w2c [n_views,3,4] fp32 out <- the top three rows of the inverse of cam_pose [n_views,4,4] fp32
 * (camera-to-world), computed in fp64 by cofactors from the fp32 entries and rounded once; one thread per view.
 *
 * Vertex visibility: count [V] int32 out, the number of views r that SEE vertex i, which is when, with p = the camera-space point of step 1
 * and fp32 operations in this order: p.z >= near;  xp = (p.x / p.z) fx + cx, yp likewise, 0 <= xp <= im_w - 1 and 0 <= yp <= im_h - 1;  and
 * p.z <= D (1 + relative) + absolute, evaluated as (D * (1.0f + relative)) + absolute, for D the largest depth[r] value > 0 among the
 * pixels (floor(xp) + {0,1}, floor(yp) + {0,1}) that are inside the image (not seen when there is none; a NaN is never the largest).
 * depth [n_views,im_h,im_w] fp32: any depth maps, normally the rasteriser's.  One thread per vertex, the views in order.
 *
 * The rasteriser and the visibility return DVMVS_EINVAL for a null or misaligned pointer (4 bytes; workspace: 16), V, F, n_views, im_h or
 * im_w < 1, large_box < 1, near
 * not positive and finite, a NaN far / relative / absolute, cull_backfaces not 0 / 1, a workspace that is too small; DVMVS_EUNSUPPORTED for
 * n_views > 65535, F > 2^28, V > 2^31 - 1, im_h or im_w > 16384, n_views im_h im_w >= 2^31, or 2 n_views F tiles >= 4e18 (tiles: the 16x16
 * tiles of the image grid).  dvmvs_mesh_raster_cameras: DVMVS_EINVAL for a null or misaligned pointer or n_views < 1, DVMVS_EUNSUPPORTED for
 * n_views > 65535.  Nothing is enqueued in either case.
 */
#define DVMVS_MESH_RASTER_LARGE_BOX 64
size_t dvmvs_mesh_raster_workspace_bytes(long long n_views, long long n_faces, long long im_h, long long im_w);
int dvmvs_mesh_raster_cameras(const float* cam_pose, float* cam_w2c, int n_views, dvmvs_stream_t stream);
int dvmvs_mesh_raster_fwd(const float* verts, long long V, const int* faces, long long F, const float* cam_intr, const float* cam_w2c,
                          int n_views, int im_h, int im_w, float near, float far, int cull_backfaces, int large_box, void* workspace,
                          size_t workspace_bytes, float* depth, int* face, int* overflow, dvmvs_stream_t stream);
int dvmvs_mesh_visibility_fwd(const float* verts, long long V, const float* depth, const float* cam_intr, const float* cam_w2c,
                              int n_views, int im_h, int im_w, float near, float relative, float absolute, int* count,
                              dvmvs_stream_t stream);

/*
 * Registration of a point cloud to another by trimmed ICP (ABI 11, later addition; csrc/registration.hip).  The reference project has
 * nothing for this: the definition is this project's own (the step the Tanks-and-Temples evaluation takes before precision and recall).
 * The whole loop is enqueued by one call; no host read happens inside it, and the result stays on the device.
 *   source [N,3], target [M,3]   fp32, contiguous, 4-byte aligned, finite (not checked)
 *   grid_workspace     the target's grid: dvmvs_nearest_build(target, M, ...) into dvmvs_nearest_workspace_bytes(M) bytes
 *   query_workspace    dvmvs_nearest_query_workspace_bytes(N, M) bytes, scratch of the loop's nearest queries
 *   state              dvmvs_icp_workspace_bytes(N, max_iterations) bytes on the device, 16-byte aligned, any contents.  In 8-byte words:
 *                        [0, 16)   T, fp64 4x4 row-major: takes source coordinates into the target's frame
 *                        [16]      iterations (int64): the iterations that were recorded below
 *                        [17]      status (int64): 0 running, 1 converged, 2 too few correspondences, 3 iteration limit
 *                        [18, 36)  the moments of the last recorded iteration, fp64: n | sum p' [3] | sum q [3] | sum p' q^T [9, row-major:
 *                                  entry 3 a + b is sum p'_a q_b] | sum |p'|^2 | sum d^2
 *                        [36, 36 + I), [36 + I, 36 + 2 I), [36 + 2 I, 36 + 3 I) with I = max_iterations: per iteration the inlier count
 *                                  (int64), the fitness and the RMSE (fp64); entries at and after `iterations` are not written
 *                      and, from the next multiple of 256 bytes on, the loop's scratch: p' [N,3] fp32, d [N] fp32, j [N] int32 and the
 *                      partial sums [ceil(N / 1024), 18] fp64 (each rounded up to 256 bytes).
 *   init_host          16 doubles on the HOST (row-major 4x4, read before the call returns), or NULL for the identity
 * Iteration k = 0, 1, ... with T_0 = init:
 *   1. A = every entry of T_k[:3,:4] rounded to fp32; p' = ((A00 x + A01 y) + A02 z) + A03 and likewise for y and z: every operation
 *      rounded to fp32, no FMA contraction.
 *   2. (d_i, j_i) = dvmvs_nearest_distance_fwd of p'_i in target (the distance and the smallest index); q_i = target[j_i].
 *   3. Pair i is an inlier when d_i <= max_distance, compared in fp32 (+inf keeps every pair).
 *   4. The 18 moments above over the inliers, in fp64 from the fp32 values: the products p'_a q_b, p'_a p'_a and d d are exact,
 *      |p'|^2 = (xx + yy) + zz.  Order of the additions, a function of N alone: the points are cut into consecutive blocks of 1024; in a
 *      block, "thread" t of 256 adds the terms of its points t, t + 256, t + 512, t + 768 in that order from 0.0; the threads of each
 *      group of 64 are combined by the xor butterfly (v[l] += v[l ^ m] for m = 32, 16, 8, 4, 2, 1), the 4 groups are added in order.
 *      The block sums b = 0, 1, ... are then added by 64 "lanes": lane l adds b = l, l + 64, ... in order from 0.0, then the same
 *      butterfly.  A trimmed point is skipped, which equals adding an exact +0.0.
 *   5. n = the count, rmse_k = sqrt(sum d^2 / n) (0 when n = 0), fitness_k = n / N: recorded at entry k; iterations = k + 1.  They
 *      describe T_k.  If n < 3: status 2, T stays, stop.  Else if k >= 1 and |rmse_k - rmse_{k-1}| < tolerance and
 *      |fitness_k - fitness_{k-1}| < tolerance: status 1, T stays, stop.
 *   6. Solve, fp64 with +, -, *, / and sqrt only, nothing contracted: pbar = sum p' / n, qbar = sum q / n,
 *      S_ab = sum p'_a q_b - (sum p'_a * sum q_b) / n.  Horn's symmetric matrix
 *        [ (Sxx+Syy)+Szz  Syz-Szy        Szx-Sxz        Sxy-Syx       ]
 *        [                (Sxx-Syy)-Szz  Sxy+Syx        Szx+Sxz       ]
 *        [                               (Syy-Sxx)-Szz  Syz+Szy       ]
 *        [                                              (Szz-Sxx)-Syy ]
 *      is diagonalised by cyclic Jacobi sweeps over (p, q) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3): a zero A_pq is skipped; otherwise
 *      theta = (A_qq - A_pp) / (2 A_pq), t = +-1 / (|theta| + sqrt(theta theta + 1)) with the sign of theta (+ for 0),
 *      c = 1 / sqrt(t t + 1), s = t c; for every k the columns A_kp <- c A_kp - s A_kq, A_kq <- s A_kp + c A_kq (old values on the right),
 *      then the rows A_pk, A_qk by the same formulas, then A_pq = A_qp = 0, then the columns p, q of V (V starts as the identity) like
 *      A's.  Before each sweep: stop when every off-diagonal is exactly zero; at most 16 sweeps.  The quaternion (w, x, y, z) is the
 *      column of V of the largest diagonal entry (the lowest index on a tie), divided by sqrt(((ww + xx) + yy) + zz) and negated when
 *      w < 0.  R = [1-2(yy+zz) 2(xy-wz) 2(xz+wy); 2(xy+wz) 1-2(xx+zz) 2(yz-wx); 2(xz-wy) 2(yz+wx) 1-2(xx+yy)]: never a reflection.
 *      s = 1, or with with_scale s = (sum over a, b in row-major order of R_ab S_ba, from 0.0) / (sum |p'|^2 - ((sx sx + sy sy) + sz sz) / n)
 *      with (sx, sy, sz) = sum p' (Umeyama); a denominator that is not > 0: status 2, T stays, stop.  M = s R,
 *      t_a = qbar_a - ((M_a0 pbar_0 + M_a1 pbar_1) + M_a2 pbar_2), and for a < 3
 *      T_{k+1}[a][c] = ((M_a0 T_k[0][c] + M_a1 T_k[1][c]) + M_a2 T_k[2][c]) + t_a T_k[3][c]; row 3 stays.  If k + 1 = max_iterations:
 *      status 3.
 * The transform, moments and solve kernels of an iteration read the status on the device and do nothing once it is not 0 (the nearest-point
 * query between them cannot, and repeats a query that nothing reads), so a larger max_iterations cannot change
 * a result that stopped earlier.  The result is bit-identical run to run, on any stream, for any alignment of the inputs.
 * dvmvs_transform_points_fwd: out[i] = step 1 applied to points[i] with T (16 doubles on the DEVICE, 8-byte aligned); out may be points.
 * dvmvs_icp_workspace_bytes: host only; 0 for N <= 0 or above 2^28 and for max_iterations outside [1, 1024]; non-decreasing in N.
 * Returns DVMVS_EINVAL for a null or misaligned pointer (fp32: 4 bytes; workspaces and state: 16; T: 8), N or M < 1, max_iterations < 1,
 * with_scale not 0 / 1, a max_distance that is NaN or <= 0, a tolerance that is NaN or negative, an init that is not finite, a
 * state or query workspace that is too small; DVMVS_EUNSUPPORTED above 2^28 points or 1024 iterations.  Nothing is enqueued when a negative
 * code is returned: these checks cover everything the nearest-point launcher inside the loop refuses, so from inside the loop only a
 * positive hipError_t of a launch can come back, after earlier launches of the call have been enqueued.
 */
size_t dvmvs_icp_workspace_bytes(long long N, int max_iterations);
int dvmvs_icp_fwd(const float* source, long long N, const float* target, long long M, const void* grid_workspace, void* query_workspace,
                  size_t query_workspace_bytes, float max_distance, int with_scale, int max_iterations, double tolerance,
                  const double* init_host, void* state, size_t state_bytes, dvmvs_stream_t stream);
int dvmvs_transform_points_fwd(const float* points, long long N, const double* T, float* out, dvmvs_stream_t stream);

/*
 * Point-to-plane registration (ABI 11, later addition; csrc/registration.hip): the loop above with the target's normals, for surfaces made
 * of planes, along which point-to-point correspondences slide.  The definition is this project's own (dvmvs/errors.py::
 * register_points_plane is its host form, the same bits).  Arguments as dvmvs_icp_fwd, without with_scale, and
 *   target_normals [M,3]  fp32, contiguous, 4-byte aligned.  A row that is all zero or holds a value that is not finite is "no normal".
 *                         Neither the length nor the sign of a normal is looked at: every term below is even in it.
 *   state              dvmvs_icp_plane_workspace_bytes(N, max_iterations) bytes on the device, 16-byte aligned, any contents.  In 8-byte words:
 *                        [0, 16)   T; [16] iterations; [17] status: 0 running, 1 converged, 2 too few correspondences, 3 iteration limit,
 *                                  4 degenerate geometry
 *                        [18, 48)  the moments of the last recorded iteration, fp64: n | sum J_a J_b for a <= b, row-major (00, 01, .., 05,
 *                                  11, .., 55) [21] | sum J_a r [6] | sum r^2 | sum d^2
 *                        [48, 48 + I), .., [48 + 3 I, 48 + 4 I) with I = max_iterations: per iteration the inlier count (int64), the
 *                                  fitness, the RMSE of the plane residual and the RMSE of the point distance (fp64)
 *                      and, from the next multiple of 256 bytes on, the loop's scratch as in dvmvs_icp_fwd with partial sums [.., 30].
 * Iteration k = 0, 1, ... with T_0 = init:
 *   1., 2. as in dvmvs_icp_fwd: p' and (d_i, j_i); q_i = target[j_i], n_i = target_normals[j_i].
 *   3. Pair i is an inlier when d_i <= max_distance (fp32) and n_i is a normal.  An index outside [0, M) is skipped and never addressed.
 *   4. Per inlier, in fp64 from the fp32 values, every product and sum rounded, nothing contracted: p = p'_i, o = p'_0 (the first moved
 *      point, inlier or not), r = ((p0 - q0) n0 + (p1 - q1) n1) + (p2 - q2) n2, e = p - o,
 *      c = (e1 n2 - e2 n1, e2 n0 - e0 n2, e0 n1 - e1 n0), J = (c0, c1, c2, n0, n1, n2).  The 30 moments above are added in the order of
 *      dvmvs_icp_fwd's step 4.
 *   5. rmse_k = sqrt(sum r^2 / n), rmse_point_k = sqrt(sum d^2 / n) (both 0 when n = 0), fitness_k = n / N: recorded at entry k;
 *      iterations = k + 1.  If n < 6: status 2, T stays, stop.  Else if k >= 1 and |rmse_k - rmse_{k-1}| < tolerance and
 *      |fitness_k - fitness_{k-1}| < tolerance: status 1, T stays, stop.
 *   6. A = sum J J^T (6x6 symmetric), b = sum J r; x with A x = -b by LDL^T without pivoting, fp64 with +, -, *, / only:
 *        for j = 0 .. 5:  d = A_jj; for k = 0 .. j-1: d = d - (L_jk L_jk) D_k;
 *                         if not d > 2^-30 A_jj: status 4, T stays, stop;  D_j = d;
 *                         for i = j+1 .. 5:  s = A_ij; for k = 0 .. j-1: s = s - (L_ik L_jk) D_k;  L_ij = s / d
 *        for i = 0 .. 5:  s = -b_i; for k = 0 .. i-1: s = s - L_ik x_k;  x_i = s
 *        for i = 0 .. 5:  x_i = x_i / D_i
 *        for i = 5 .. 0:  s = x_i; for k = i+1 .. 5: s = s - L_ki x_k;  x_i = s
 *      (the constant 2^-30 is part of the definition: a single plane or two planes leave a pivot at rounding level, every well-posed
 *      scene stays orders of magnitude above it).
 *   7. x = (alpha, beta, gamma, t0, t1, t2).  qx = alpha / 2, qy = beta / 2, qz = gamma / 2, norm = sqrt(((1 + qx qx) + qy qy) + qz qz),
 *      w = 1 / norm, qx = qx / norm (qy, qz likewise); R from (w, qx, qy, qz) by the formula of dvmvs_icp_fwd's step 6;
 *      s_a = (o_a - ((R_a0 o_0 + R_a1 o_1) + R_a2 o_2)) + t_a, and for a < 3
 *      T_{k+1}[a][c] = ((R_a0 T_k[0][c] + R_a1 T_k[1][c]) + R_a2 T_k[2][c]) + s_a T_k[3][c]; row 3 stays.  If k + 1 = max_iterations: status 3.
 * dvmvs_icp_plane_workspace_bytes and the return codes: as dvmvs_icp_workspace_bytes and dvmvs_icp_fwd (target_normals among the pointers).
 */
size_t dvmvs_icp_plane_workspace_bytes(long long N, int max_iterations);
int dvmvs_icp_plane_fwd(const float* source, long long N, const float* target, const float* target_normals, long long M,
                        const void* grid_workspace, void* query_workspace, size_t query_workspace_bytes, float max_distance,
                        int max_iterations, double tolerance, const double* init_host, void* state, size_t state_bytes,
                        dvmvs_stream_t stream);

/*
 * Connected components of a triangle mesh, and their removal by size (ABI 11, later addition; csrc/mesh_components.hip).  The reference
 * project has nothing for this: the definition is this project's own (dvmvs/components.py is its host form; Open3D's
 * cluster_connected_triangles and remove_triangles_by_mask are the usual tools).  Everything that decides a result is an integer.
 *   faces [F,3] int32, verts [V,3] fp32 (normals [V,3] fp32, colors [V,3] uint8), contiguous, 4-byte aligned; V, F in [0, 2^28].
 * A face is VALID when its three indices lie in [0, V); an invalid face joins nothing and no vertex is read for it.
 *   labels [V] int32        the smallest vertex index reachable from v over the edges of valid faces (v itself when no valid face uses v)
 *   face_labels [F] int32   labels[faces[f][0]], -1 for an invalid face
 *   face_count [V] int32    at r: the valid faces of the component whose label is r; 0 at every vertex that is no label of a face
 *   area [V] int64          at r: the sum of A_f over those faces, A_f of dvmvs_surface_sample_count's definition (units of 2^-32 m^2);
 *                           only with verts (both NULL otherwise)
 *   result [2] int64        {the number of r with face_count[r] > 0, status}: status 1 when a valid face's area is not finite or does not
 *                           fit or the mesh's total area is 2^63 units or more (decided exactly, from separately summed upper and lower
 *                           halves; the areas of bad faces count as 0), status 2 when the labelling gave up (below); 0 otherwise.
 * The labelling is a lock-free union-find over the vertices: parent[v] = v; one thread per valid face (a, b, c) unites (a, b) and (b, c);
 * labels[v] = the end of v's chain, written to a separate array.  A union finds both roots and hooks the larger under the smaller by a
 * compare-and-swap of parent[larger] that expects `larger`; when it fails it continues from the value the compare-and-swap returned.
 * Invariant: parent[v] <= v always, an entry only ever decreases, and every write to parent during the unions is an atomic (that
 * compare-and-swap, or the atomicMin of path halving).  A stale read can therefore cost a retry and never a wrong hook, and the smallest
 * vertex of a component is never hooked: the labels are the canonical ones whatever the schedule.  A union makes at most 65536
 * compare-and-swaps, then sets status 2.
 * dvmvs_mesh_filter_count: root r is KEPT when face_count[r] > 0, face_count[r] >= min_faces and area[r] >= min_area_units; with
 * keep_largest only the one r of all with face_count[r] > 0 that has the greatest area (ties: the greater face count, then the smaller r),
 * and it only if it passes the thresholds.  A face is kept when it is valid and its label is kept, a vertex when its label is kept (the
 * vertices that kept faces use).  counts [3] int64 = {V', F', status} with the status of `result` (V' = F' = 0 unless it is 0).
 * dvmvs_mesh_filter_emit (with V_out = V', F_out = F' of the count call of the same arguments and workspace): kept vertices and kept faces
 * in their original order, the faces re-indexed; normals / colors are gathered alongside (each NULL with its output); vertex_index
 * [V'] and face_index [F'] (int32, each may be NULL): the old indices.
 * workspace: dvmvs_mesh_components_workspace_bytes(V, F) bytes, 16-byte aligned, the same block for the three calls of one mesh (fwd
 * initialises it; count leaves what emit reads).  dvmvs_mesh_components_workspace_bytes: host only; 0 for V or F outside [0, 2^28].
 * Every entry returns DVMVS_EINVAL for a null or misaligned pointer that a non-empty side needs, a negative V or F (emit: V or F < 1, V_out
 * or F_out outside [0, V] / [0, F]), verts without area or the reverse, a negative threshold, keep_largest not 0 / 1, a workspace that is
 * too small; DVMVS_EUNSUPPORTED for V or F above 2^28.  Nothing is enqueued in either case.  The results are bit-identical run to run.
 */
size_t dvmvs_mesh_components_workspace_bytes(long long V, long long F);
int dvmvs_mesh_components_fwd(const float* verts, long long V, const int* faces, long long F, void* workspace, size_t workspace_bytes,
                              int* labels, int* face_labels, int* face_count, long long* area, long long* result, dvmvs_stream_t stream);
int dvmvs_mesh_filter_count(const int* labels, const int* face_labels, const int* face_count, const long long* area, const long long* result,
                            long long V, long long F, long long min_area_units, long long min_faces, int keep_largest, void* workspace,
                            size_t workspace_bytes, long long* counts, dvmvs_stream_t stream);
int dvmvs_mesh_filter_emit(const float* verts, const int* faces, const float* normals, const unsigned char* colors, const int* labels,
                           const int* face_labels, const int* face_count, const long long* area, long long V, long long F,
                           long long min_area_units, long long min_faces, int keep_largest, void* workspace, size_t workspace_bytes,
                           long long V_out, long long F_out, float* verts_out, int* faces_out, float* normals_out, unsigned char* colors_out,
                           int* vertex_index, int* face_index, dvmvs_stream_t stream);

/*
 * Simplifying a triangle mesh by vertex clustering with quadric error representatives (ABI 11, later addition; csrc/mesh_simplify.hip).
 * The reference project has nothing for this: the definition is this project's own (dvmvs/simplify.py is its host form and states every
 * step; Lindstrom 2000 is the method, Open3D's simplify_vertex_clustering the usual tool).
 *   verts [V,3] fp32, faces [F,3] int32 (normals [V,3] fp32, colors [V,3] uint8), contiguous, 4-byte aligned; V in [1, 2^28], F in [0, 2^28].
 * Arithmetic: fp64 from the fp32 inputs with +, -, *, / and sqrt only, every operation correctly rounded, nothing contracted.
 *   1. The clusters are the voxels of dvmvs_voxel_keys(verts, V, fp32(1 / voxel)) in ascending key order, the cluster mean m_c is
 *      dvmvs_voxel_downsample_emit's point (fp64 sum in ascending vertex index, one division, one rounding).
 *   2. The quadric of cluster c: over its incidences (f, j), face f valid (three indices in [0, V)) and corner j in c, in ascending
 *      3 f + j: o = fp64(m_c), p_k = fp64(verts[faces[f][k]]) - o, e1 = p_1 - p_0, e2 = p_2 - p_0, n = (e1y e2z - e1z e2y, e1z e2x -
 *      e1x e2z, e1x e2y - e1y e2x), d = -((nx p0x + ny p0y) + nz p0z); A_cd += n_c n_d (the upper triangle), b_c += d n_c, from 0.0.
 *   3. With average = 0: the cyclic Jacobi of dvmvs_point_normals_fwd on A (pairs (0,1), (0,2), (1,2), a zero A_pq skipped, at most 16
 *      sweeps, stop before a sweep when the three off-diagonals are exactly zero) -> l_0..2 and the columns v_0..2; l_max = l_0, replaced by
 *      l_1 when l_1 > l_max, then by l_2 likewise; column i is kept when l_i > 1e-3 l_max; x = (0, 0, 0), and per kept column in column
 *      order x_k += (-(((v_0i b_0 + v_1i b_1) + v_2i b_2) / l_i)) v_ki.  When l_max > 0 and |x_k| <= voxel for every k (false for a NaN)
 *      the cluster's vertex is fp32(o + x), otherwise m_c.  With average = 1 it is m_c.  `voxel` is fp64(fp32(the cell edge)).
 *   4. normals': the fp64 sum of the members' normals in ascending vertex index, each component divided by len = sqrt((xx + yy) + zz),
 *      rounded to fp32; zeros unless 0 < len < inf.  colors': per channel rint(fp64(sum) / n), halves to even.
 *   5. A face is kept when it is valid, its three clusters differ, and no face of smaller index has the same clusters up to rotation.
 *   6. The clusters that kept faces use keep their order and are renumbered; the faces are re-indexed and keep their order.
 * Call sequence for one mesh, every call on one stream, `voxel_workspace` the block of the voxel entries and `workspace` this block's:
 *   dvmvs_voxel_keys(verts, V, ...) -> a stable sort of the keys (sorted_keys, sorted_index int64 [V]) -> dvmvs_voxel_downsample_count
 *   (-> voxel_counts int64 [2] on the device) -> dvmvs_mesh_simplify_keys (-> incidence_keys int32 [3F]: the cluster of corner j of
 *   face f at 3 f + j, INT_MAX for an invalid face; third int32 [F] and pair int64 [F]: of the rotation of the face's clusters that
 *   puts the smallest first, (x, y, z), z and (x << 28) | y; INT_MAX and INT64_MAX for a face that step 5 drops for its own corners) ->
 *   stable sorts of incidence_keys (incidence_sorted, incidence_order int64 [3F]) and of third (third_order int64 [F]) ->
 *   dvmvs_mesh_simplify_pair_keys (out[s] = pair[third_order[s]]) -> a stable sort of out (pair_sorted, pair_order int64 [F]) ->
 *   dvmvs_mesh_simplify_count -> counts [3] int64 = {V', F', status}: status 1 when dvmvs_voxel_keys found a cell index of 2^21 or
 *   more or a coordinate that is not finite (V' = F' = 0 then) -> dvmvs_mesh_simplify_emit with V_out = V', F_out = F':
 *   verts_out [V',3], faces_out [F',3], normals_out / colors_out (each NULL when the count call had no such input), vertex_cluster [V]
 *   int32 (the output vertex of every input vertex, -1 where its cluster kept no face) and face_index [F'] int32 (the old index of
 *   every output face); each of the last two may be NULL.
 * One thread owns a cluster and walks its members and its incidences serially; no float atomics, no float value crosses threads: the
 * results are bit-identical run to run.  No index read from memory becomes an address before it is checked against its array's size.
 * dvmvs_mesh_simplify_workspace_bytes: host only; 0 for V or F outside [0, 2^28].  The block is 16-byte aligned.
 * dvmvs_voxel_downsample_runs (csrc/surface_sample.hip; host only, enqueues nothing): where dvmvs_voxel_downsample_count left, in its
 * workspace for N points, the first sorted slot of every voxel (starts int32 [M]) and the points in sorted order (fp32 [N,3]).
 * Every entry returns DVMVS_EINVAL for a null or misaligned pointer that a non-empty side needs, V < 1, F < 0, a voxel that is not positive
 * and finite, average not 0 / 1, V_out or F_out outside [0, V] / [0, F], a workspace that is too small; DVMVS_EUNSUPPORTED for V or F
 * above 2^28.  Nothing is enqueued in either case.
 */
size_t dvmvs_mesh_simplify_workspace_bytes(long long V, long long F);
int dvmvs_voxel_downsample_runs(long long N, const void* workspace, const int** starts, const float** sorted_points);
int dvmvs_mesh_simplify_keys(const int* faces, long long V, long long F, const long long* sorted_index, const void* voxel_workspace,
                             const long long* voxel_counts, void* workspace, size_t workspace_bytes, int* incidence_keys, int* third,
                             long long* pair, dvmvs_stream_t stream);
int dvmvs_mesh_simplify_pair_keys(const long long* pair, const long long* third_order, long long F, long long* out, dvmvs_stream_t stream);
int dvmvs_mesh_simplify_count(const float* verts, const float* normals, const unsigned char* colors, long long V, const int* faces,
                              long long F, double voxel, int average, const long long* sorted_index, const void* voxel_workspace,
                              const long long* voxel_counts, const int* incidence_sorted, const long long* incidence_order,
                              const int* third, const long long* third_order, const long long* pair_sorted, const long long* pair_order,
                              void* workspace, size_t workspace_bytes, long long* counts, dvmvs_stream_t stream);
int dvmvs_mesh_simplify_emit(long long V, long long F, void* workspace, size_t workspace_bytes, long long V_out, long long F_out,
                             float* verts_out, int* faces_out, float* normals_out, unsigned char* colors_out, int* vertex_cluster,
                             int* face_index, dvmvs_stream_t stream);

/*
 * Smoothing a triangle mesh (the umbrella Laplacian filter and Taubin's lambda / mu filter) and area-weighted vertex normals from the
 * faces (ABI 11, later addition; csrc/mesh_smooth.hip).  The reference project has nothing for this: the definition is this project's own
 * (dvmvs/smooth.py is its host form and states every step; Open3D's filter_smooth_laplacian, filter_smooth_taubin and
 * compute_vertex_normals are the usual tools).
 *   verts [V,3] fp32, faces [F,3] int32 (fallback [V,3] fp32), contiguous, 4-byte aligned; V in [1, 2^28], F in [0, 2^28].
 * Arithmetic: fp64 from the fp32 inputs with +, -, *, / and sqrt only, every operation correctly rounded, nothing contracted.
 *   1. A face counts when its three indices lie in [0, V) and are pairwise different; every other face takes no part.
 *   2. Rows: N(v) is the set of distinct u that share a counting face with v, in ascending u.  A counting face (a, b, c) emits the
 *      directed pairs (a,b), (b,a), (b,c), (c,b), (c,a), (a,c); boundary[v] is set when some pair (v, u) is emitted exactly once over all
 *      counting faces (an edge of one face; not an edge of two faces, whatever their orientation, nor of three).
 *   3. A step with factor s, all reads from the previous iterate: when n = |N(v)| is 0, or fixed_boundary and boundary[v], the
 *      position's bits are copied; otherwise per component S = (((0.0 + x_u1) + x_u2) + ...) over N(v) in order, m = S / fp64(n),
 *      x' = fp32(x_v + s * (m - x_v)).  The iterate between steps is fp32.
 *   4. taubin = 0: `iterations` steps with lam.  taubin = 1: per iteration a step with lam, then one with mu.  No step: verts_out = verts.
 *   5. Vertex normals: over the incidences (f, j) of a vertex, the counting faces f whose corner j it is, in ascending 3 f + j, the sum
 *      from 0.0 of n_f = e1 x e2 = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), e1 = p1 - p0, e2 = p2 - p0 of the fp32
 *      positions taken as fp64 (area-weighted, not normalised per face); len = sqrt((xx + yy) + zz); each component divided by len and
 *      rounded to fp32; unless 0 < len < inf the row of `fallback`, or (0, 0, 0) where fallback is NULL.
 * Coordinates that are not finite are outside the contract (the result is unspecified; nothing is addressed out of bounds).
 * Call sequence for one mesh, every call on one stream, `workspace` this block's:
 *   dvmvs_mesh_smooth_keys -> pair_keys int64 [6F]: (a << 32) | b of the six pairs of face f from 6 f, INT64_MAX for a face that does not
 *   count; corner_keys int32 [3F]: the vertex of corner j of face f at 3 f + j, INT_MAX likewise (either may be NULL, not both) ->
 *   a sort of pair_keys (values only; equal keys are identical) -> dvmvs_mesh_smooth_rows: offsets int32 [V+1], neighbours int32 [6F] (the
 *   first offsets[V] are used: the host never needs that number) and the boundary flags, in the workspace -> dvmvs_mesh_smooth_steps:
 *   ALL steps of the call, one launch per step, between two buffers of the workspace that hold the positions as 16-byte float4 (packed
 *   = 1: as 12-byte fp32 x 3, a tool's comparison), the last step into verts_out [V,3]; verts is never written and may not be verts_out.
 *   dvmvs_mesh_smooth_rows_export copies the rows out: offsets int64 [V+1], neighbours int32 [6F] (-1 past offsets[V]), boundary uint8 [V].
 *   dvmvs_mesh_smooth_normals (needs no rows): corner_sorted int32 [3F] and corner_order int64 [3F] are a STABLE sort of corner_keys;
 *   normals [V,3] may not be verts.
 * One lane owns a vertex and walks its row or its incidences serially, in the order above; no float atomics, no float value crosses
 * threads, no barrier across workgroups: the results are bit-identical run to run.  No index read from memory becomes an address before it
 * is checked against its array's size.  Nothing is read back by the host anywhere in the sequence.
 * dvmvs_mesh_smooth_workspace_bytes: host only; 0 for V or F outside [0, 2^28].  The block is 16-byte aligned.
 * Every entry returns DVMVS_EINVAL for a null or misaligned pointer that a non-empty side needs, V < 1 (keys: V < 0), F < 0, iterations < 0,
 * lam outside (0, 1], a mu that is not finite or, with taubin, outside [-1, -lam), a flag that is not 0 / 1, a workspace that is too small;
 * DVMVS_EUNSUPPORTED for V or F above 2^28 or more than 1024 iterations.  Nothing is enqueued in either case.
 */
size_t dvmvs_mesh_smooth_workspace_bytes(long long V, long long F);
int dvmvs_mesh_smooth_keys(const int* faces, long long V, long long F, long long* pair_keys, int* corner_keys, dvmvs_stream_t stream);
int dvmvs_mesh_smooth_rows(const long long* pair_sorted, long long V, long long F, void* workspace, size_t workspace_bytes,
                           dvmvs_stream_t stream);
int dvmvs_mesh_smooth_rows_export(long long V, long long F, const void* workspace, size_t workspace_bytes, long long* offsets,
                                  int* neighbours, unsigned char* boundary, dvmvs_stream_t stream);
int dvmvs_mesh_smooth_steps(const float* verts, long long V, long long F, int iterations, int taubin, double lam, double mu,
                            int fixed_boundary, int packed, void* workspace, size_t workspace_bytes, float* verts_out,
                            dvmvs_stream_t stream);
int dvmvs_mesh_smooth_normals(const float* verts, long long V, const int* faces, long long F, const int* corner_sorted,
                              const long long* corner_order, const float* fallback, void* workspace, size_t workspace_bytes, float* normals,
                              dvmvs_stream_t stream);

/*
 * The k nearest neighbours of points, neighbours within a radius, and statistical outlier scores (ABI 11, later addition;
 * csrc/point_neighbours.hip).  The reference project has nothing for this: the definitions are this project's own (dvmvs/outliers.py is
 * their host form; Open3D's remove_statistical_outlier and remove_radius_outlier are the usual tools).  The two searches run on the grid
 * of the nearest-point block above and take its arguments:
 *   target [M,3], query [N,3]   fp32, contiguous, 4-byte aligned, FINITE (a precondition; not checked on the device)
 *   workspace         the target's grid: dvmvs_nearest_build(target, M, ...) into dvmvs_nearest_workspace_bytes(M) bytes; not changed
 *   query_workspace   dvmvs_nearest_query_workspace_bytes(N, M) bytes, 16-byte aligned, scratch of one call.  Calls that share it must be
 *                     ordered.
 * Arithmetic contract, that of the nearest-point block: d2(q, t) = (dx dx + dy dy) + dz dz, every operation rounded to fp32, no FMA
 * contraction; distances are sqrt(d2), correctly rounded.
 * dvmvs_knn_fwd: the CANDIDATES of query i are the targets j with d2(query_i, target_j) <= cap2 = fl(max_distance * max_distance) in fp32
 *   (max_distance = inf: all) and, with exclude_same_index = 1, j != i (by index, for a cloud searched against itself: a duplicate point
 *   at distance 0 is a neighbour).  dist [N,k] fp32 and index [N,k] int32: row i holds the k smallest candidates in ascending
 *   lexicographic order of (d2, j), the distance as sqrt(d2); missing slots are (inf, -1).  1 <= k <= 32.  The set of the k smallest
 *   pairs does not depend on the order of evaluation, so the rows are bit-identical to a brute force over all j, run to run, on any
 *   stream.  The search visits the cells around the query's cell in growing Chebyshev rings and stops only, and never before ring 1, when
 *   every unvisited target is provably no candidate (its d2 exceeds cap2) or provably larger than the k-th pair of a full list (bound and
 *   its fp32 margins: csrc/point_neighbours.hip); otherwise it goes on until it has visited the whole grid.  A query with fewer than k
 *   candidates therefore walks the whole grid unless max_distance ends the walk: max_distance is what bounds the work for far outliers.
 * dvmvs_radius_count_fwd: count [N] int32 = min(number of candidates of cap2 = fl(radius * radius), cap), cap >= 1.  The saturation is
 *   part of the definition: the search leaves a query once it has counted cap.
 * dvmvs_outlier_statistics_fwd: dist / index [N,k] as dvmvs_knn_fwd wrote them (a slot counts when its index is >= 0), ratio >= 0 finite.
 *   mean [N] fp32: m_i = the fp64 sum of the counted distances of row i in slot order, divided by their number, rounded to fp32 once; inf
 *     for a row without one.  Point i is VALID when m_i is finite.
 *   stats [4] fp64 = {n, mu, sigma, threshold}: n the valid points, mu = sum of fp64(m_i) over them / n, sigma = sqrt(sum of (m_i - mu)^2
 *     / (n - 1)) (a second pass; 0 for n < 2), threshold = mu + ratio * sigma; n = 0 gives four zeros.  Both sums run in fp64 in ONE
 *     workgroup in the order of dvmvs_distance_metrics_fwd, a function of N alone (thread t of 1024 adds the elements t, t + 1024, ...,
 *     an invalid one adds 0; 64-lane xor butterfly; the 16 waves in order); division and square root are correctly rounded.
 *   keep [N] uint8: 1 where point i is valid and fp64(m_i) <= threshold.  Three launches, nothing read by the host.
 * With N == 0 every entry enqueues nothing and returns 0.
 * Every entry returns DVMVS_EINVAL for a null or misaligned pointer (4 bytes; workspaces 16; stats 8), k outside [1,32], cap < 1, a NaN or
 * negative max_distance / radius / ratio (ratio also: infinite), exclude_same_index not 0 / 1, N < 0, M < 1, a query workspace that is too
 * small; DVMVS_EUNSUPPORTED above 2^28 points.  Nothing is enqueued in either case.  No floating-point atomics are used.
 */
int dvmvs_knn_fwd(const float* query, long long N, const float* target, long long M, const void* workspace, void* query_workspace,
                  size_t query_workspace_bytes, int k, float max_distance, int exclude_same_index, float* dist, int* index,
                  dvmvs_stream_t stream);
int dvmvs_radius_count_fwd(const float* query, long long N, const float* target, long long M, const void* workspace, void* query_workspace,
                           size_t query_workspace_bytes, float radius, int cap, int exclude_same_index, int* count, dvmvs_stream_t stream);
int dvmvs_outlier_statistics_fwd(const float* dist, const int* index, long long N, int k, double ratio, float* mean, unsigned char* keep,
                                 double* stats, dvmvs_stream_t stream);

/*
 * Oriented normals of points from rows of nearest neighbours (ABI 11, later addition; csrc/point_normals.hip).  The reference project has
 * nothing for this: the definition is this project's own (dvmvs/normals.py is its host form; Open3D's estimate_normals followed by
 * orient_normals_towards_camera_location is the usual tool).
 *   points [N,3]      fp32: where normals are wanted (used by the orientation only)
 *   target [M,3]      fp32: the cloud the neighbours come from, usually the same array; M >= 1
 *   index [N,k]       int32, 3 <= k <= 32: row i as dvmvs_knn_fwd(points, target, k, max_distance, exclude_same_index = 0) wrote it (for a
 *                     cloud against itself the point is its own slot 0)
 *   viewpoints [V,3]  fp32 or NULL (then V = 0): where the cloud was seen from
 *   view [N]          int32 or NULL: the viewpoint of every point; NULL needs V <= 1 (every point was seen from viewpoints[0])
 *   normals [N,3] fp32, curvature [N] fp32, valid [N] uint8: the outputs.  Coordinates must be FINITE (a precondition, not checked).
 * All arithmetic is fp64 from the fp32 inputs, +, -, *, / and sqrt only, each operation correctly rounded, no FMA contraction.  Point i:
 *   1. The VALID slots of row i, in slot order, are those with 0 <= j < M: j0, j1, ..., n of them.  A slot that is -1 or any other value
 *      outside [0, M) is skipped and never becomes an address.  n < 3: normal (0,0,0), curvature 0, valid 0.
 *   2. Single-pass moments about the anchor a = target[j0]: for each valid slot in order e = target[j] - a (per component), s_c += e_c,
 *      S_cd += e_c e_d for (c,d) = (0,0), (0,1), (0,2), (1,1), (1,2), (2,2); all sums start from 0.0.  m_c = s_c / n and
 *      C_cd = S_cd / n - m_c m_d, mirrored to be symmetric.
 *   3. A = C is diagonalised by cyclic Jacobi sweeps, the rule of the ICP block above on a 3x3: pairs (p, q) = (0,1), (0,2), (1,2); a zero
 *      A_pq is skipped; otherwise theta = (A_qq - A_pp) / (2 A_pq), t = +-1 / (|theta| + sqrt(theta theta + 1)) with the sign of theta (+
 *      for 0), c = 1 / sqrt(t t + 1), s = t c; the columns p, q of A (new_p = c old_p - s old_q, new_q = s old_p + c old_q), then its rows
 *      p, q likewise, then A_pq = A_qp = 0, then the columns p, q of V (V starts as the identity).  Before each sweep: stop when the three
 *      off-diagonals are exactly zero; at most 16 sweeps.
 *   4. lambda = the smallest diagonal entry, the lowest index on a tie; trace = (A_00 + A_11) + A_22.  If trace is not > 0 (coincident
 *      points): normal 0, curvature 0, valid 0.  Otherwise curvature = fp32(max(lambda, 0) / trace) (a lambda of -0 counts as 0) and
 *      valid 1.
 *   5. The normal is that column of V, (x, y, z), divided by sqrt((x x + y y) + z z); it is negated when the first non-zero of (z, y, x)
 *      is negative: the canonical sign.
 *   6. With viewpoints: v = viewpoints[view[i]], or viewpoints[0] without view; a view[i] outside [0, V) means "unknown" and keeps the
 *      canonical sign.  d = (n_x (v_x - p_x) + n_y (v_y - p_y)) + n_z (v_z - p_z) with p = points[i]; the normal is negated when d < 0
 *      (d = 0 keeps it).  Then each component is rounded to fp32.
 * One point per lane and nothing crosses lanes, so the outputs are bit-identical run to run and on any stream, and equal to the host
 * form.  One launch, nothing read by the host.  N == 0 enqueues nothing and returns 0.
 * DVMVS_EINVAL for a null or misaligned pointer (4 bytes for everything but valid), N < 0, M < 1, k outside [3,32], V < 0, viewpoints
 * NULL with V > 0 or given with V = 0, view without viewpoints, no view with V > 1; DVMVS_EUNSUPPORTED above 2^28 points.  Nothing is
 * enqueued in either case.
 */
int dvmvs_point_normals_fwd(const float* points, long long N, const float* target, long long M, const int* index, int k,
                            const float* viewpoints, long long V, const int* view, float* normals, float* curvature, unsigned char* valid,
                            dvmvs_stream_t stream);

/*
 * Implicit moving-least-squares (IMLS) signed distance of an oriented point cloud on a voxel grid, and the trimming of the mesh that
 * marching cubes makes of it (ABI 11, later addition; csrc/implicit_surface.hip).  The reference project has nothing for this: the
 * definition is this project's own (dvmvs/implicit.py is its host form).
 *   points [M,3], normals [M,3]  fp32, FINITE (a precondition, not checked); a normal of (0,0,0) marks a point without one
 *   grid              origin (three fp32 numbers, finite), voxel > 0 finite, X, Y, Z >= 1 nodes, z fastest, at most 2^31 nodes.  Node
 *                     (i, j, k) lies at x_c = fl(fl(fl(i_c) * voxel) + origin_c) in fp32, the multiply and the add rounded separately.
 *   radius            fp32, finite, > 0: where the weights reach zero, and the max_distance of the search
 * dvmvs_implicit_band_fwd: sets mask [X,Y,Z] uint8 to 1 at a SUPERSET of the nodes that have at least one candidate under the fp32 test
 *   of dvmvs_knn_fwd(nodes, points, ..., max_distance = radius) (derivation: csrc/implicit_surface.hip); other bytes are left as they
 *   were (the caller zeroes the mask).  How many more nodes are marked changes no result.  Points outside the grid mark what lies inside
 *   it; no address is formed from an index outside [0, dim).  Many lanes store the same constant byte: a benign race.
 * dvmvs_implicit_nodes_fwd: nodes [A,3] fp32, the positions of the nodes with the linear indices linear [A] int64 ((i * Y + j) * Z + k,
 *   each inside the grid: a precondition).
 * dvmvs_implicit_values_fwd: index [A,k] int32, 1 <= k <= 32: row a as dvmvs_knn_fwd(nodes, points, k, radius, 0) wrote it.  All
 *   arithmetic is fp64 from the fp32 inputs, +, -, *, / only, each operation correctly rounded, no FMA contraction.  Node a, over its row
 *   in slot order: a slot is USED when 0 <= j < M and normals[j] != (0,0,0) (a slot outside [0, M) never becomes an address).
 *   h2 = fp64(radius) fp64(radius).  For each used slot: e = x - points[j] (exact); d2 = (e_x e_x + e_y e_y) + e_z e_z; t = 1 - d2 / h2,
 *   and t < 0 becomes 0 (the slot still counts); w = (t t) t; s = (n_x e_x + n_y e_y) + n_z e_z; num += w s, den += w, both from 0.0.
 *   The node is VALID when at least min_neighbours (>= 1) slots were used and den > 0: then volume[linear[a]] = fp32(num / den) and
 *   valid[linear[a]] = 1.  Nothing is written for another node: the caller pre-fills volume [total] with fp32(radius), a positive fill,
 *   and valid [total] uint8 with 0.  A linear index outside [0, total) is skipped.  One node per lane and nothing crosses lanes, so the
 *   outputs are bit-identical run to run, on any stream, however the nodes are split into calls, and equal to the host form.
 * dvmvs_implicit_trim_fwd: verts [V,3] fp32 in index space (of marching cubes with origin 0 and voxel size 1) and faces [F,3] int32 ->
 *   keep_vertex [V] uint8: 1 when the nodes floor(pos) and ceil(pos) (componentwise) are inside the grid and both valid;
 *   keep_face [F] uint8: 1 when its three vertices are inside [0, V) and kept.  Two launches.
 * Every entry enqueues on the given stream, reads nothing on the host, and with nothing to do (M, A or V and F of 0) returns 0.
 * DVMVS_EINVAL for a null or misaligned pointer (4 bytes; linear 8; the uint8 arrays none), a negative count, M < 1 (values), k outside
 * [1,32], min_neighbours < 1, total < 1, a radius or voxel that is not finite and > 0, an origin that is not finite, a dimension < 1;
 * DVMVS_EUNSUPPORTED above 2^28 points or candidate nodes of one call, 2^31 nodes, 2^31 - 1 vertices or faces.  Nothing is enqueued in
 * either case.
 */
int dvmvs_implicit_band_fwd(const float* points, long long M, float origin_x, float origin_y, float origin_z, float voxel, int X, int Y,
                            int Z, float radius, unsigned char* mask, dvmvs_stream_t stream);
int dvmvs_implicit_nodes_fwd(const long long* linear, long long A, float origin_x, float origin_y, float origin_z, float voxel, int X,
                             int Y, int Z, float* nodes, dvmvs_stream_t stream);
int dvmvs_implicit_values_fwd(const float* nodes, long long A, const float* points, const float* normals, long long M, const int* index,
                              int k, float radius, int min_neighbours, const long long* linear, long long total, float* volume,
                              unsigned char* valid, dvmvs_stream_t stream);
int dvmvs_implicit_trim_fwd(const float* verts, long long V, const int* faces, long long F, const unsigned char* valid, int X, int Y,
                            int Z, unsigned char* keep_vertex, unsigned char* keep_face, dvmvs_stream_t stream);

/*
 * A TSDF volume without bounds: a hash table of 8 x 8 x 8-voxel bricks over a pool of fixed capacity (ABI 11, later addition;
 * csrc/sparse_volume.hip, csrc/sparse_grid.h).  The reference project has nothing for this: the definitions are
 * this project's own, and dvmvs/sparse.py is the host form of the marking.
 * Lattice.  Voxel v is a signed integer triple at origin + float(v) * voxel_size, evaluated in fp32 as dvmvs_tsdf_integrate evaluates it
 *   (one multiply, one add, no contraction): voxel v here and voxel v of a dense volume with the same origin see the same floats.  Brick
 *   b = floor(v / 8) per component, |b| < 2^20, so float(v) is exact.  Key = ((b_x + 2^20 - 1) << 42) | ((b_y + 2^20 - 1) << 21) |
 *   (b_z + 2^20 - 1), an int64 in [0, 2^63); ascending keys are the bricks in lexicographic (x, y, z) order.  EMPTY = 2^63 - 1 is no brick.
 * State, all device memory of the caller, never reallocated:
 *   table_keys [table_slots] int64, EMPTY where free; table_birth [table_slots] int32, 2^31 - 1 where free; table_slots a power of two.
 *     Where in the table a key sits depends on the schedule; nothing below that is observable does.
 *   fresh [table_slots] int64, EMPTY everywhere between flushes: the keys a flush inserted, in any order.
 *   pool_tsdf, pool_weight, pool_color [max_bricks, 512] fp32, initially 1, 0, 0; local index x * 64 + y * 8 + z.
 *   pool_key [max_bricks] int64, pool_birth [max_bricks] int32: defined for slots < status[0].
 *   status [8] int64, zero at first: [0] bricks allocated (n_bricks <= max_bricks), [1] bricks dropped because the pool was full,
 *     [2] marks dropped because a probe saw the whole table without finding the key or a free slot, [3] pixels that marked nothing
 *     because a sample left |b| < 2^20, was not finite, or spanned more than 4 bricks on an axis, [4] keys inserted by the flush in
 *     progress (0 between flushes), [5..7] zero.
 * A flush of the frames numbered first_frame .. first_frame + n_frames - 1 (the volume counts the frames it is given from 0) is
 *   dvmvs_sparse_mark; a sort of fresh into sorted [table_slots] (ascending, by any device sort); dvmvs_sparse_assign;
 *   dvmvs_sparse_integrate, on one stream.  No entry reads anything on the host.
 * dvmvs_sparse_mark: depth [n,h,w], cam_intr [n,3,3], camera-to-world cam_pose [n,4,4] fp32.  One pixel per lane.  A depth > max_depth
 *   counts as 0; a depth that is zero, negative or not finite marks nothing.  Every other pixel marks exactly the bricks of
 *   dvmvs/sparse.py::mark_bricks, whose fp32 operations, in its order, the kernel repeats (correctly rounded +, -, *, /, sqrt, floor,
 *   ceil; no contraction): samples of the pixel's ray from max(d - trunc, 0) to d + trunc, at most 2 voxels apart (at most 16 intervals;
 *   longer bands are sampled more coarsely with the margin growing to match), each marking the bricks that the box sample +- m meets,
 *   m = 0.501953125 (z + delta / 2) sqrt(1/fx^2 + 1/fy^2) + (delta / 2) sqrt(1 + a^2 + b^2) + slack (derivation in the kernel's header
 *   comment).  A marked brick that is not in the table is inserted (compare-and-swap after a read); its birth becomes the smallest frame
 *   number that marks it (integer atomicMin).  EVERY PROBE LOOP IS BOUNDED BY table_slots; a mark that finds no slot is counted in
 *   status[2] and dropped.
 * dvmvs_sparse_assign: rank r of the non-EMPTY keys of sorted gets pool slot status[0] + r, its key and its birth; ranks at or beyond
 *   max_bricks are dropped and counted in status[1] (their keys stay in the table, so they are never offered again).  Then status[0] is
 *   advanced, status[4] zeroed and fresh refilled with EMPTY.  The pool's layout is therefore deterministic: by flush, ascending key inside.
 * dvmvs_sparse_integrate: one workgroup per pool slot (max_bricks workgroups; those of slots >= status[0], read on the device, return at
 *   once).  A brick's voxels receive, for each frame g = first_frame + f in index order with g >= birth, the per-voxel statements of
 *   dvmvs_tsdf_integrate on that frame after depth > max_depth -> 0, in registers, one load and one store per voxel: the bits of the dense
 *   kernel on that brick under the birth rule, free-space updates (dist = 1) included.  Frames before a brick's birth are not applied --
 *   the one stated difference from the dense volume.  Because birth is a property of the frame numbers, the result does not depend on how
 *   frames are batched into flushes.  Colour as in dvmvs_tsdf_integrate_frames: exactly one of rgb_u8 [n,h,w,3] and folded [n,h,w];
 *   obs_weight_host: n floats on the host.
 * dvmvs_sparse_gather: copies the bricks of slots < n_bricks (a host number: the caller has read status[0]) that lie inside the box of
 *   bricks_x x bricks_y x bricks_z bricks from brick (first_x, first_y, first_z) to their place in dense [8 bricks_x, 8 bricks_y,
 *   8 bricks_z] arrays (z fastest); bricks outside the box are skipped, voxels of no brick are left as the caller filled them.
 * DVMVS_EINVAL for a null pointer, a table_slots that is no power of two, a count < 1 (n_bricks < 0), first_frame < 0, a voxel_size or
 *   trunc_margin that is not finite and > 0, an origin that is not finite (mark), a NaN max_depth, both or neither colour form;
 *   DVMVS_EUNSUPPORTED for 2^31 pixels per frame, frame numbers or pool slots, more than 2^30 table slots.  Nothing is enqueued then.
 */
int dvmvs_sparse_mark(long long* table_keys, int* table_birth, long long table_slots, long long* fresh, long long* status,
                      const float* depth, const float* cam_intr, const float* cam_pose, int n_frames, int im_h, int im_w, float origin_x,
                      float origin_y, float origin_z, float voxel_size, float trunc_margin, float max_depth, int first_frame,
                      dvmvs_stream_t stream);
int dvmvs_sparse_assign(const long long* table_keys, const int* table_birth, long long table_slots, const long long* sorted,
                        long long* fresh, long long* status, long long* pool_key, int* pool_birth, long long max_bricks,
                        dvmvs_stream_t stream);
int dvmvs_sparse_integrate(float* pool_tsdf, float* pool_weight, float* pool_color, const long long* pool_key, const int* pool_birth,
                           const long long* status, long long max_bricks, float origin_x, float origin_y, float origin_z, float voxel_size,
                           const float* cam_intr, const float* cam_pose, const unsigned char* rgb_u8, const float* folded,
                           const float* depth, int n_frames, int im_h, int im_w, float trunc_margin, const float* obs_weight_host,
                           float max_depth, int first_frame, dvmvs_stream_t stream);
int dvmvs_sparse_gather(const float* pool_tsdf, const float* pool_weight, const float* pool_color, const long long* pool_key,
                        long long n_bricks, float* tsdf_vol, float* weight_vol, float* color_vol, int bricks_x, int bricks_y, int bricks_z,
                        int first_x, int first_y, int first_z, dvmvs_stream_t stream);

/*
 * Marching cubes straight from the pool of the sparse volume (ABI 11, later addition; csrc/sparse_extract.hip,
 * csrc/sparse_extract_grid.h).  No dense copy is made: the work and the memory follow the allocated bricks.
 * Definition.  The sparse volume read as an unbounded dense volume: voxel v (|v| < 2^23) holds its brick's pool values when the brick is
 *   allocated (a slot < status[0]) and (tsdf 1, weight 0, colour 0) otherwise.  The mesh is what dvmvs_marching_cubes_* gives on that
 *   volume at level 0: inside = value < 0; a grid edge with exactly one inside endpoint carries one vertex, owned by the voxel at its lower
 *   end; case and triangle tables of csrc/marching_cubes_tables.h, a cube's triangles in table order; one vertex per crossing edge, shared
 *   by every face around it, across brick borders too.  Cubes and owned edges of voxels in UNALLOCATED bricks next to allocated ones count.
 *   Vertex on the +axis edge of voxel a, b = a + e_axis (fp32, no contraction, the statements of the dense kernel with the global signed
 *   index): t = (0 - v_a) / (v_b - v_a); p = float(a_axis) + t on the edge axis, float(a) on the others; position = p * voxel_size +
 *   origin; normal = g_a + t (g_b - g_a) divided by its length (zero stays zero) with g ALWAYS the central difference
 *   (v[+1] - v[-1]) * 0.5 per axis (there is no border); colour = the folded colour voxel at rint(p) (0 where unallocated), decoded as
 *   the dense kernel decodes it.
 * Inputs read: status, pool_key and the pool arrays; the hash table is not.  The key -> slot map is rebuilt: the caller sorts the keys of
 *   the slots < status[0] (every other entry of the sort's input being EMPTY) ascending into sorted [max_bricks] with the slots they came
 *   from in sort_index [max_bricks] (int64), by any device sort.
 * dvmvs_sparse_neighbours: neighbour [max_bricks, 27] int32; for slots < status[0] (read on the device), entry (dx+1)*9 + (dy+1)*3 + (dz+1)
 *   is the pool slot of brick b + d, d in {-1,0,1}^3, or -1 (not allocated, or outside |b| <= 2^20 - 1, then without a search).  The
 *   lookup is a binary search of exactly 32 steps over sorted[0 .. status[0]).  The table describes which bricks exist: it holds until
 *   the next flush.
 * Handling.  A voxel of an allocated brick is handled by that brick.  A voxel w of an unallocated brick u is handled by the allocated brick
 *   of SMALLEST KEY among u + e, e in {0,1}^3 with e_a = 1 only where w's coordinate inside u is 7 on axis a (the bricks its cube touches);
 *   by nobody when none is allocated.  A brick therefore handles voxels of local coordinates -1 .. 7 per axis: its 9^3 lattice, cell
 *   (lx+1)*81 + (ly+1)*9 + (lz+1).
 * dvmvs_sparse_extract_count: one workgroup per pool slot (max_bricks of them; those of slots >= status[0] return at once) stages the
 *   brick's tsdf with the halo -2 .. 9 per axis from its neighbours into LDS (missing neighbours read 1) and writes the owned crossing
 *   edges and the triangles of the voxels it handles to counts[2 slot], counts[2 slot + 1] (int32 [2 max_bricks]).
 * dvmvs_sparse_extract_scan: offsets [2 max_bricks] int64 <- the exclusive prefix sums of counts over the slots < status[0];
 *   summary [5] int64 <- (status[0], status[1], status[2], V, F).  The caller reads summary: the one host read of an extraction.
 * dvmvs_sparse_extract_emit: n_bricks, V, F from summary; vertex_base: workspace, int32 [729 n_bricks].  verts [V,3] fp32, normals [V,3]
 *   fp32, colors [V,3] uint8 RGB (pool_color and colors NULL: no colours), faces [F,3] int32.  ORDER: vertices by (pool slot of the
 *   handling brick, cell of the owner voxel in its lattice, axis x < y < z); faces by (pool slot of the handling brick, cell of the cube's
 *   lowest corner, table order).  The same pool state gives the same bytes.  Stores are guarded by V and F.  No atomics.
 * DVMVS_EINVAL for a null pointer, max_bricks < 1, negative counts; DVMVS_EUNSUPPORTED for 2^31 pool slots, vertices or faces.
 */
int dvmvs_sparse_neighbours(const long long* pool_key, const long long* sorted, const long long* sort_index, const long long* status,
                            long long max_bricks, int* neighbour, dvmvs_stream_t stream);
int dvmvs_sparse_extract_count(const float* pool_tsdf, const int* neighbour, const long long* status, long long max_bricks, int* counts,
                               dvmvs_stream_t stream);
int dvmvs_sparse_extract_scan(const int* counts, const long long* status, long long max_bricks, long long* offsets, long long* summary,
                              dvmvs_stream_t stream);
int dvmvs_sparse_extract_emit(const float* pool_tsdf, const float* pool_color, const long long* pool_key, const int* neighbour,
                              const long long* offsets, long long n_bricks, float origin_x, float origin_y, float origin_z, float voxel_size,
                              int* vertex_base, float* verts, float* normals, unsigned char* colors, int* faces, long long V, long long F,
                              dvmvs_stream_t stream);

/*
 * Ray-casting the sparse volume straight from its pool (ABI 11, later addition; csrc/sparse_raycast.hip, csrc/sparse_raycast_grid.h;
 * DESIGN.md section 4.8t).  No dense copy is made.
 * Definition.  For the brick-aligned box of count_x x count_y x count_z bricks whose first brick is (first_x, first_y, first_z),
 *   dvmvs_sparse_raycast_fwd writes depth, normal and rgb equal BIT FOR BIT to those of dvmvs_tsdf_raycast_fwd with the same origin,
 *   voxel_size, cameras, near, far and step on the dense volume of 8 count voxels per axis whose voxel w holds the pool's voxel of brick
 *   first + (w >> 3) at local index (w & 7) (x * 64 + y * 8 + z) when that brick is allocated (a slot < status[0]) and (tsdf 1,
 *   weight 0, colour 0) otherwise -- what dvmvs_sparse_gather puts there.  The per-pixel statements are those of the dense kernel, one by
 *   one; only where a voxel is read from differs.  skip_empty != 0 jumps over unallocated bricks and over bricks without a crossing
 *   corner with verified jumps; the outputs are the same bits either way.
 * Inputs read: status, pool_key and the pool arrays; the volume's hash table is not.
 * dvmvs_sparse_raycast_index: the render index, index [2 index_slots] int64, index_slots a power of two >= 2 max_bricks.  Entry e =
 *   (key, value); every entry is cleared to (EMPTY, -1), then the key of every slot < status[0] (read on the device) takes the first free
 *   entry on its probe path (splitmix64 finaliser, linear probing, 64-bit compare-and-swap; at most index_slots attempts) with the value
 *   = its slot.  Which entry a key lands in may depend on the schedule; what a lookup returns does not.
 * dvmvs_sparse_raycast_flags: neighbour = the table of dvmvs_sparse_neighbours.  flags [max_bricks] uint8: for slots < status[0], 1 when
 *   one of the 9^3 corners of the brick's cells (local 0 .. 8 per axis: its own voxels and the first layer of its seven forward
 *   neighbours, where allocated) has weight > 0 && tsdf <= 0; the same bit is set in the brick's index value (slot | flag << 32).  Index
 *   and flags describe the pool's CURRENT keys and contents: rebuild them after every flush.
 * dvmvs_sparse_raycast_fwd: depth [N,h,w] fp32; normal [N,h,w,3] fp32 or NULL; rgb [N,h,w,3] uint8 or NULL (then pool_color may be NULL).
 *   One lane per pixel, an 8x8 tile per wave, 16x16 per workgroup, one grid plane per view.  Every dereferenced pool slot comes from an
 *   index value or a neighbour entry checked against [0, min(status[0], max_bricks)).
 * Refusals, all before anything is enqueued.  DVMVS_EINVAL: a null pointer; max_bricks < 1; index_slots not a power of two or
 *   < 2 max_bricks; n_views, im_h, im_w or a count < 1; a box that leaves [-2^20, 2^20] bricks; voxel_size <= 0; step outside (0, 5];
 *   near < 0 or not finite; far NaN.  DVMVS_EUNSUPPORTED: 2^31 pool slots; a count above 2^21; h * w >= 2^31; more than 65535 views or
 *   tile rows; 2^32 threads; a box whose diagonal in steps, floor(|8 count - 1| / step) + 2, reaches 2^20.  The dense entry's limits
 *   Y * Z < 2^31 and 2^26 bricks do not apply: nothing is indexed by the box.
 */
int dvmvs_sparse_raycast_index(const long long* pool_key, const long long* status, long long max_bricks, long long* index,
                               long long index_slots, dvmvs_stream_t stream);
int dvmvs_sparse_raycast_flags(const float* pool_tsdf, const float* pool_weight, const long long* pool_key, const int* neighbour,
                               const long long* status, long long max_bricks, long long* index, long long index_slots, unsigned char* flags,
                               dvmvs_stream_t stream);
int dvmvs_sparse_raycast_fwd(const float* pool_tsdf, const float* pool_weight, const float* pool_color, const long long* status,
                             long long max_bricks, const long long* index, long long index_slots, const int* neighbour,
                             const unsigned char* flags, int first_x, int first_y, int first_z, int count_x, int count_y, int count_z,
                             float origin_x, float origin_y, float origin_z, float voxel_size, int skip_empty, const float* cam_intr,
                             const float* cam_pose, int n_views, int im_h, int im_w, float near, float far, float step, float* depth,
                             float* normal, unsigned char* rgb, dvmvs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DVMVS_HIP_H */
