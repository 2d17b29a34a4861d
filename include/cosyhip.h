/*
 * cosyhip.h -- C ABI of libcosyhip.so: the MI355X (gfx950) implementation of CosyPose's
 * render-and-compare pose-refinement hot path.
 *
 * Each entry point replaces one reference interface (file:line relative to the reference
 * checkout of ylabbe/cosypose); the Python shim in cosypose_amd/ binds them with ctypes
 * (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross this boundary;
 *   - every pointer is a DEVICE pointer unless the parameter name starts with `host_`;
 *   - all geometry tensors are fp32 row-major: poses (B,4,4), intrinsics (B,3,3),
 *     boxes (B,4) = x1,y1,x2,y2 in pixels; frames are fp32 NCHW (N,3,h,w) in [0,1];
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no
 *     allocation and no synchronisation; the caller owns and sizes every output;
 *   - return value: COSY_OK (0) or a negative COSY_E* code; cosy_last_error() gives the
 *     message of the last failure on the calling thread.  Nothing throws across the ABI;
 *   - the library owns only cosy_net_t (packed weights + activation workspace);
 *     distinct nets may be used concurrently from distinct threads/streams.
 */
#ifndef COSYHIP_H
#define COSYHIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COSY_VERSION 100 /* 0.1.0 */

enum { COSY_OK = 0, COSY_EINVAL = -1, COSY_ENOMEM = -2, COSY_EHIP = -3, COSY_ESIZE = -4 };

/* storage/compute type of the backbone activations and weights (accumulation is always fp32) */
enum { COSY_F32 = 0, COSY_BF16 = 1, COSY_F16 = 2 };

typedef struct cosy_net cosy_net_t;
typedef void* cosy_stream_t; /* hipStream_t */

int cosy_version(void);
const char* cosy_last_error(void);

/* ---- backbone: EfficientNet-B3(in_channels=6) + global-avg-pool + Linear(1536,9) ----------
 * Replaces EfficientNet.extract_features (cosypose/models/efficientnet.py:174-190), MBConvBlock.forward
 * (:71-98), Conv2dStaticSamePadding (cosypose/models/efficientnet_utils.py:123-146) and
 * PosePredictor.net_forward (cosypose/models/pose.py:81-87), eval mode.
 *
 * host_params: flat fp32 blob of the reference state_dict in this order (BN tensors as
 * weight,bias,running_mean,running_var; num_batches_tracked omitted):
 *   backbone._conv_stem.weight[40,6,3,3], backbone._bn0;
 *   for i in 0..25: [_expand_conv.weight[Cmid,Cin,1,1], _bn0]  (absent when expand==1),
 *                   _depthwise_conv.weight[Cmid,1,k,k], _bn1,
 *                   _se_reduce.weight[Cse,Cmid,1,1], _se_reduce.bias, _se_expand.weight[Cmid,Cse,1,1], _se_expand.bias,
 *                   _project_conv.weight[Cout,Cmid,1,1], _bn2;
 *   backbone._conv_head.weight[1536,384,1,1], backbone._bn1; pose_fc.weight[9,1536], pose_fc.bias[9].
 * cosy_effnet_b3_param_count() floats in total (10,798,441). */
long cosy_effnet_b3_param_count(void);
int cosy_effnet_b3_out_hw(int H, int W, int* out_h, int* out_w);
int cosy_effnet_b3_create(const float* host_params, size_t n_floats, int dtype, int H, int W, int max_batch,
                          cosy_net_t** out);
int cosy_effnet_b3_destroy(cosy_net_t* net);
size_t cosy_effnet_b3_workspace_bytes(const cosy_net_t* net);

/* Fill the net's 6-channel input from a reference-layout tensor x (B,6,H,W) fp32 NCHW
 * (what torch.cat((images_crop, renders), 1) produces, pose.py:104). */
int cosy_effnet_b3_set_input_nchw(cosy_net_t* net, const float* x, int B, cosy_stream_t stream);

/* Frames (N,3,h,w) fp32 planar -> (N,h,w,4) fp32 interleaved (RGB + pad), the layout cosy_crop_pack samples from.
 * Done once per PosePredictor.forward call (the frames do not change across iterations); out holds N*h*w*4 floats.
 * 0 <= N <= 65535 (one grid row per frame), h, w >= 1; N = 0 is COSY_OK with null pointers; anything else COSY_EINVAL. */
int cosy_frames_to_nhwc4(const float* images, float* out, int N, int h, int w, cosy_stream_t stream);
/* the same from uint8 frames (N,3,h,w) as the datasets deliver them: out = value / 255.f (training/pose_forward_loss.py:24: images.float() / 255.) */
int cosy_frames_u8_to_nhwc4(const unsigned char* images, float* out, int N, int h, int w, cosy_stream_t stream);

/* Fused replacement of deepim_crops_robust's roi_align (cosypose/lib3d/cropping.py:73-74,
 * torchvision 0.4.2 semantics, sampling_ratio=4) + torch.cat with the renders (pose.py:104):
 * writes observed crop -> channels 0..2 and renders (B,3,H,W fp32 NCHW) -> channels 3..5 of
 * the net input.  frames_nhwc4 (N,h,w,4) from cosy_frames_to_nhwc4; im_id (B) int32 index into the frames
 * or NULL for identity (the reference gathers images[im_ids] first, cosypose/integrated/pose_predictor.py:41).
 * The 16 bilinear samples of a pixel are evaluated in separable form (same sum, fp32 rounding differs ~1e-7). */
int cosy_crop_pack(cosy_net_t* net, const float* frames_nhwc4, const int* im_id, const float* boxes_crop,
                   const float* renders, int B, int N, int h, int w, cosy_stream_t stream);

/* Run the backbone on the current input: feat (B,1536) fp32 or NULL, pose9 (B,9) fp32,
 * taps (B,9,16) fp32 or NULL = per-stage probes [mean, mean|x|, 14 strided samples] of the
 * stem, the 7 stage outputs and the head activation (test hook; same probe as the oracle). */
int cosy_effnet_b3_forward(cosy_net_t* net, int B, float* feat, float* pose9, float* taps, cosy_stream_t stream);

/* After cosy_effnet_b3_forward: copy the head activation out as the reference's backbone(x) would return it,
 * (B,1536,h,w) fp32 NCHW (what EfficientNet.forward yields, efficientnet.py:192-204). */
int cosy_effnet_b3_features_nchw(cosy_net_t* net, int B, float* out, cosy_stream_t stream);

/* ---- test probes (parity tests of the fused kernels; never on the hot path) -----------------
 * cosy_effnet_b3_set_probe: the NEXT forwards also copy one whole activation out as fp32 NCHW into `out`
 * (caller-allocated, B x C x HW floats): layer -1 = stem output, 0..25 = output of MBConv block i
 * (MBConvBlock.forward's return value, cosypose/models/efficientnet.py:71-98), 26 = head activation,
 * 100+i = depthwise output of block i (after _bn1 + swish, :83), 200+i = squeeze-excite gate of block i as (B, Cmid)
 * (sigmoid(_se_expand(...)), :85-88); layer -2 switches the probe off.
 * cosy_effnet_b3_block_info: dims[11] = {H, W, Ho, Wo, Cin, Cmid, Cout, front kernel (0 unfused, 1 wave, 2 small, 3 tiled, 4 block 0 behind the
 * fused stem: the stem tensor stays fp32 in registers and is never stored -- a forward with probe -1 or per-stage taps runs the unfused kernels,
 * 5 wave / 6 small with the depthwise taps applied by small MFMAs: the expanded values and the taps are rounded to the storage type), k, s,
 * SE gate applied to the project weights (1) or to the activation rows (0)}. */
int cosy_effnet_b3_set_probe(cosy_net_t* net, int layer, float* out);
int cosy_effnet_b3_block_info(const cosy_net_t* net, int block, int* dims);

/* ---- measurement hook ---------------------------------------------------------------------
 * With profiling enabled every launch of cosy_effnet_b3_forward is bracketed by HIP events recorded on the
 * launch stream (no synchronisation, one hipEventRecord per kernel; up to 24 forwards are retained).
 * cosy_effnet_b3_profile_read blocks until the recorded events have completed and returns one record per
 * launch slot of the schedule: kernel name (as rocprofv3 prints it, abbreviated), layer index, number of
 * timed launches, mean/min duration, and the ALGORITHMIC bytes and flops of one launch (tensor sizes
 * in+out+weights).  Reading resets the accumulation. */
typedef struct {
    char name[64];
    int layer;      /* -1 stem, 0..25 MBConv block, 26 head */
    int n;          /* launches timed */
    float ms_avg, ms_min;
    double bytes;   /* algorithmic HBM bytes of one launch */
    double flops;   /* algorithmic flops of one launch */
    double cbytes;  /* the compulsory part of `bytes`: block inputs / outputs / residuals and weights only -- the tensors that stay
                     * inside an MBConv block (expanded E, depthwise output D, squeeze sums, gates) count as 0 */
} cosy_prof_rec_t;
int cosy_effnet_b3_set_profiling(cosy_net_t* net, int enable);
int cosy_effnet_b3_profile_read(cosy_net_t* net, cosy_prof_rec_t* recs, int cap, int* n_out);

/* ---- sample order of the backbone's launches (tests and A/B timing) --------------------------
 * mode 0: every launch walks the samples of the batch forward.  mode 1 (serpentine): a launch that reads a large
 * activation walks them in the opposite order to the launch that wrote it, so that it starts with what was written
 * last; a new net starts in mode 1.  The order changes no arithmetic: both modes return the same bits.  Takes effect from
 * the next cosy_effnet_b3_forward on this net; any other mode returns COSY_EINVAL. */
int cosy_effnet_b3_set_traversal(cosy_net_t* net, int mode);

/* ---- geometry ---------------------------------------------------------------------------
 * PosePredictor.crop_inputs without the pixel work (cosypose/models/pose.py:45-67):
 * project_points_robust + boxes_from_uv (cosypose/lib3d/camera_geometry.py:18-42), deepim_boxes
 * (cosypose/lib3d/cropping.py:7-47, lamb=1.4, not clamped), get_K_crop_resize (camera_geometry.py:45-87).
 * pts_table (n_obj,P,3) = mesh_db points after sample_points(P, deterministic=True)
 * (cosypose/lib3d/mesh_ops.py:31-41); obj_id (B) int32 rows of pts_table; K is (N,3,3) indexed
 * by im_id (B) or (B,3,3) when im_id is NULL.
 *
 * Argument limits of every entry of this section and the two below (checked on the host, before any launch; a violation
 * returns COSY_EINVAL and cosy_last_error() names the argument): batch sizes B, M, n_seg >= 0, and B = 0 (n_seg = 0)
 * returns COSY_OK at once, with null data pointers allowed; P >= 1, S >= 1; im_h, im_w, out_h, out_w, C >= 1 and
 * sampling_ratio >= 1; every pointer not called optional must be non-null; cosy_roi_align and cosy_dists_add take
 * B <= 65535 (one grid row per item; split larger batches).  The VALUES of obj_id / im_id / n_sym live on the device and
 * are the caller's to keep inside their tables. */
int cosy_crop_geometry(const float* pts_table, const int* obj_id, const float* K, const int* im_id, const float* TCO,
                       int B, int P, float z_min, int im_h, int im_w, int out_h, int out_w, float lamb,
                       float* boxes_rend, float* boxes_crop, float* K_crop, cosy_stream_t stream);

/* torchvision.ops.roi_align(images, [im_id|boxes], (out_h,out_w), sampling_ratio) as the reference
 * calls it (cropping.py:74): out (B,C,out_h,out_w) fp32 NCHW. */
int cosy_roi_align(const float* images, const int* im_id, const float* boxes, int B, int N, int C, int h, int w,
                   int out_h, int out_w, int sampling_ratio, float* out, cosy_stream_t stream);

/* PosePredictor.update_pose for pose_dim=9 (pose.py:69-79): compute_rotation_matrix_from_ortho6d
 * (cosypose/lib3d/rotations.py:6-21) + apply_imagespace_predictions (cosypose/lib3d/cosypose_ops.py:10-31). */
int cosy_pose_update(const float* TCO_in, const float* K_crop, const float* pose9, int B, float* TCO_out,
                     cosy_stream_t stream);

/* TCO_init_from_boxes(z_range=(z,z)) (cosypose_ops.py:121-135) and
 * TCO_init_from_boxes_zup_autodepth (cosypose_ops.py:138-173), as used by
 * CoarseRefinePosePredictor.make_TCO_init (pose_predictor.py:65-74). */
int cosy_tco_init_from_boxes(const float* boxes, const float* K, const int* im_id, int B, float z, float* TCO,
                             cosy_stream_t stream);
int cosy_tco_init_zup_autodepth(const float* boxes, const float* pts_table, const int* obj_id, const float* K,
                                const int* im_id, int B, int P, float* TCO, cosy_stream_t stream);

/* ---- index / assignment ops adjacent to the loop (bit-exact) --------------------------------
 * scatter_argmin (cosypose/csrc/cosypose_cext.cpp:218-245): per segment id in [0,n_seg) the index of the
 * smallest distance, first index wins on ties; out[s] = -1 for an empty segment (the reference's loop reads a missing
 * key of its map there, which yields 0 and lengthens its output). dists (M) fp32, ids (M) int32 on the device.
 * NaN as in the reference's scan: a NaN distance is chosen exactly when it is the segment's first member. */
int cosy_scatter_argmin(const float* dists, const int* ids, int M, int n_seg, int* out, cosy_stream_t stream);

/* expand_ids_for_symmetry (cosypose/csrc/cosypose_cext.cpp:247-259): for item n (in order), for k < n_sym_item[n]:
 * ids_expand[m] = n, sym_ids[m] = k.  n_sym_item (B) int32 = n_symmetries[labels[n]] (the label lookup is the caller's
 * dict).  The caller sizes the outputs with M = sum(n_sym_item); *total (optional, device) receives M. */
int cosy_expand_ids_for_symmetry(const int* n_sym_item, int B, int* ids_expand, int* sym_ids, int* total, cosy_stream_t stream);

/* ---- symmetric pose distances / losses' argmin / ADD(-S) (fp32; index outputs follow the reference's tie rule) ----
 * Points come from a per-object table pts_table (n_obj,P,3) indexed by obj_id (B) int32; obj_id == NULL means the
 * table is already per sample, (B,P,3) -- the layout the reference passes.
 *
 * cosy_symmetric_distance: symmetric_distance_batched (mode 0) / symmetric_distance_batched_fast (mode 1),
 * cosypose/lib3d/symmetric_distances.py:19-57.  sym_table (n_obj,S,4,4) is the identity-padded symmetry table,
 * n_sym (n_obj) the real counts (mode 0 scans only those, like expand_ids_for_symmetry + scatter_argmin: strict <,
 * first wins; mode 1 scans all S rows and takes the first minimum of the mean SQUARED distance, like argmin -- a NaN
 * cost counts as the smallest there, as in torch; in mode 0 it is kept only where it comes first, as in the C++ scan).
 * n_sym == NULL: mode 0 scans all S rows too.
 * -> min_dists (B), best_sym (B) int32, S12 (B,4,4) = sym_table[obj, best]. */
int cosy_symmetric_distance(const float* T1, const float* T2, const int* obj_id, const float* pts_table, const float* sym_table,
                            const int* n_sym, int B, int P, int S, int mode, float* min_dists, int* best_sym, float* S12,
                            cosy_stream_t stream);
/* symmetric_distance_reprojected (cosypose/lib3d/symmetric_distances.py:94-121): per item, over the object's n_sym real symmetries S_k,
 * the mean over its P points of the PIXEL distance between project(K, T1 S_k, p) and project(K, T2, p) (camera_geometry.py:4-15, no z
 * clamp); strict <, first wins.  K (B,3,3); n_obj = rows of the tables (>= B when obj_id is NULL).  -> min_dists (B), best_sym (B) int32,
 * S12 (B,4,4) = sym_table[obj, best].  An item whose object id is outside [0, n_obj) or whose n_sym is <= 0 gets NaN, -1 and a zero S12. */
int cosy_symmetric_distance_reprojected(const float* T1, const float* T2, const float* K, const int* obj_id, const float* pts_table,
                                        const float* sym_table, const int* n_sym, int B, int n_obj, int P, int S, float* min_dists,
                                        int* best_sym, float* S12, cosy_stream_t stream);
/* loss_CO_symmetric with l1 (cosypose/lib3d/cosypose_ops.py:34-46), forward value: per sample the minimum over the S
 * possible ground truths of mean |pred points - gt points| (first minimum wins, a NaN counts as the smallest: torch.min) -> loss (B), min_id (B)
 * int32 (optional), TCO_assign (B,4,4) (optional). */
int cosy_loss_co_symmetric(const float* TCO_possible_gt, const float* TCO_pred, const float* pts_table, const int* obj_id, int B,
                           int S, int P, float* loss, int* min_id, float* TCO_assign, cosy_stream_t stream);
/* loss_refiner_CO_disentangled (cosypose_ops.py:49-82), forward value -> loss (B). */
int cosy_loss_refiner_disentangled(const float* TCO_possible_gt, const float* TCO_input, const float* refiner_outputs,
                                   const float* K_crop, const float* pts_table, const int* obj_id, int B, int S, int P, float* loss,
                                   cosy_stream_t stream);
/* dists_add (symmetric = 0) / dists_add_symmetric (symmetric = 1), cosypose/lib3d/distances.py:5-21 -> dists (B,P,3):
 * gt point minus predicted point (ADD), or minus the NEAREST predicted point (ADD-S; first minimum of the squared
 * distance wins). */
int cosy_dists_add(const float* TXO_pred, const float* TXO_gt, const float* pts_table, const int* obj_id, int B, int P,
                   int symmetric, float* dists, cosy_stream_t stream);

/* ---- pose evaluation (cosypose/evaluation/meters/pose_meters.py:53-92) ----------------------------------------------
 * PoseErrorMeter.compute_errors for B tentative (prediction, ground truth) pairs in one call, on points[:n_points[obj]] of each
 * pair's object: errors (B,8) = norm_avg, xyz_avg[3], TCO_xyz[3], TCO_norm.  The per-point vector is the one cosy_dists_add
 * produces, bit for bit: gt point minus predicted point where mode[b] = 0 (ADD), minus the NEAREST predicted point (first minimum
 * of the squared distance) where mode[b] != 0 (ADD-S); the mode is per pair, so ADD(-S) is one call.  norm_avg = mean of the
 * vectors' norms, xyz_avg = mean of |components|, both accumulated in float64 in a fixed order (per-tile partial sums in the
 * workspace, then tile order): no floating-point atomics, the same bits from run to run, and a pair's result does not depend on
 * what else is in the batch.  TCO_xyz = |t_pred - t_gt|, TCO_norm its norm.
 * pts_table (n_obj,n_max,3), n_points (n_obj) int32 on the device.  B is bounded only by B * ceil(n_max / 1024) < 2^31.
 * Checked on the host before any launch (COSY_EINVAL, cosy_last_error() names the argument): B >= 0, n_obj >= 1, n_max >= 1,
 * every pointer non-null, workspace 16-byte aligned with workspace_bytes >= cosy_pose_errors_workspace_bytes(B, n_max); B = 0
 * returns COSY_OK at once with null pointers.  The VALUES of obj_id / n_points live on the device and are checked there: an
 * obj_id outside [0, n_obj) reads nothing and gives NaN norm_avg / xyz_avg for its pair, n_points is clamped to [0, n_max]
 * (0 points: NaN, the mean of nothing). */
size_t cosy_pose_errors_workspace_bytes(int B, int n_max);
int cosy_pose_errors(const float* TXO_pred, const float* TXO_gt, const int* obj_id, const int* mode, const float* pts_table,
                     const int* n_points, int B, int n_obj, int n_max, float* errors, void* workspace, size_t workspace_bytes,
                     cosy_stream_t stream);

/* ---- training step of the refiner network, fp32, activations NHWC = rows x channels --------------
 * Every piece of cosypose/training/train_pose.py:317-331's step: the 1x1 convolutions and their gradients on the library's own
 * fp32 MFMA GEMMs (cosy_train_gemm / cosy_wgrad below), BatchNorm, depthwise, squeeze-excite scaling, loss gradient, clip +
 * Adam, the squeeze-excite and pose FCs (cosy_se_train_*, cosy_fc_small_*): no rocBLAS on the step.  `workspace` is a device buffer
 * of cosy_train_workspace_bytes() bytes shared by the reductions (deterministic two-stage sums, no atomics). */
size_t cosy_train_workspace_bytes(void);
/* crop + render pack (as cosy_crop_pack) into a caller-owned NHWC8 buffer of element type `dtype` */
int cosy_crop_pack_to(void* x_nhwc8, int dtype, const float* frames_nhwc4, const int* im_id, const float* boxes_crop,
                      const float* renders, int B, int N, int h, int w, int H, int W, cosy_stream_t stream);
/* the same through the per-crop tap tables and the LDS-tiled kernel that cosy_crop_pack runs on the net's own buffer (bit-identical
 * to cosy_crop_pack_to): `workspace` = cosy_crop_pack_workspace_bytes(B, H, W) bytes of device scratch */
size_t cosy_crop_pack_workspace_bytes(int B, int H, int W);
int cosy_crop_pack_to_ws(void* x_nhwc8, int dtype, const float* frames_nhwc4, const int* im_id, const float* boxes_crop,
                         const float* renders, int B, int N, int h, int w, int H, int W, void* workspace, cosy_stream_t stream);
/* nn.BatchNorm2d in train mode (efficientnet.py:49-68; eps 1e-3, momentum 0.01): batch mean / 1/sqrt(biased var + eps)
 * per channel over the M rows; running_mean/var (optional) updated in place with the unbiased variance.  C % 4 == 0
 * (rows are read as 16-byte channel quads), else COSY_EINVAL. */
int cosy_bn_train_stats(const float* x, long M, int C, float eps, float momentum, float* mean, float* rstd, float* running_mean,
                        float* running_var, void* workspace, cosy_stream_t stream);
/* out = act((x-mean)*rstd*gamma+beta) [* rowscale[row/HW]] [+ res];  act 0 none / 1 Swish; rowscale = drop_connect's
 * per-sample mask/keep_prob (efficientnet_utils.py:83-92), res = the block's skip input. */
int cosy_bn_train_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, long M, int C,
                        int act, const float* rowscale, int HW, const float* res, float* out, cosy_stream_t stream);
/* backward of the above (+ SwishImplementation.backward, efficientnet_utils.py:44-48): dgamma, dbeta (accumulated when
 * `accumulate`), dx.  `sums` = 2*C floats of scratch. */
int cosy_bn_train_backward(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, long M, int C, int act, const float* rowscale, int HW, float* dgamma, float* dbeta,
                           int accumulate, float* dx, float* sums, void* workspace, cosy_stream_t stream);
/* the same with the incoming gradient formed on the fly as dout * cgate[sample][c] + cadd[sample][c] * cadd_scale (sample = row / HW; cgate,
 * cadd (B,C)): the squeeze-excite backward of an MBConv block (gradient through the gate multiply + the pooled mean) feeds BatchNorm 1's
 * backward without the sum being stored */
int cosy_bn_train_backward_gated(const float* dout, const float* cgate, const float* cadd, float cadd_scale, const float* x, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, long M, int C, int act, const float* rowscale, int HW,
                                 float* dgamma, float* dbeta, int accumulate, float* dx, float* sums, void* workspace, cosy_stream_t stream);
/* depthwise convolution with the reference's static "same" padding; weights transposed to (k*k, C); C % 4 == 0.
 * Output size: H x W at stride 1, ((H - 2) / 2 + 1) x ((W - 2) / 2 + 1) at stride 2 (arch.conv_out).  Stride 2 needs H >= 2 and
 * W >= 2 (a 1-pixel side has no output under that padding): COSY_EINVAL otherwise, for the forward and both gradients. */
int cosy_dw_train_forward(const float* x, const float* wt, int B, int H, int W, int C, int k, int stride, float* out,
                          cosy_stream_t stream);
int cosy_dw_train_backward_data(const float* dy, const float* wt, int B, int H, int W, int C, int k, int stride, float* dx,
                                cosy_stream_t stream);
/* ... + add (B,H,W,C): dx = conv-transpose(dy) + add in one pass (stride 1): the skip connection's gradient of an MBConv block without expansion */
int cosy_dw_train_backward_data_add(const float* dy, const float* wt, const float* add, int B, int H, int W, int C, int k, int stride, float* dx,
                                    cosy_stream_t stream);
int cosy_dw_train_backward_weight(const float* x, const float* dy, int B, int H, int W, int C, int k, int stride, float* dwt,
                                  void* workspace, cosy_stream_t stream);
/* module_layout = 0 (and cosy_dw_train_backward_weight): the gradient as [tap][channel] (k*k, C), the layout of `wt`;
 * module_layout = 1: as (C, k*k) = the module's _depthwise_conv.weight (C,1,k,k).  The two are transposes of each other bit for bit. */
int cosy_dw_train_backward_weight_ex(const float* x, const float* dy, int B, int H, int W, int C, int k, int stride, float* dw, int module_layout,
                                     void* workspace, cosy_stream_t stream);
/* 1x1 convolutions of the training step on the library's own fp32 MFMA GEMMs (no rocBLAS on the path):
 *   cosy_train_gemm: out (M,N) = A (M,K) . op(W) (+ add (M,N)); op(W) = W^T for W stored (N,K) [w_is_kn = 0: the forward of
 *                    F.conv2d with a 1x1 kernel, efficientnet.py:81,90,188], W for W stored (K,N) [w_is_kn = 1: the data
 *                    gradient dX = dY . W].  K and N multiples of 8 (anything else: COSY_EINVAL before a launch; the same rule
 *                    holds for cosy_train_pack_plan and cosy_train_gemm_packed).  The weights are packed on the device per call.
 *   cosy_wgrad:      dW (N,K) = dY^T (N,M) . X (M,K), dY (M,N), X (M,K) row-major, any shape; deterministic (fixed-order
 *                    combine of per-slab partial tiles).
 * cosy_wgrad_tall / _supported are round 1's names for the same kernel (kept: every shape is supported now). */
int cosy_train_gemm(const float* A, const float* W, int w_is_kn, long M, int K, int N, const float* add, float* out, void* workspace,
                    cosy_stream_t stream);
int cosy_wgrad(const float* dY, const float* X, long M, int N, int K, float* dW, void* workspace, cosy_stream_t stream);
/* The weights of EVERY 1x1 convolution packed in one launch per step (they change once per step, in Adam): cosy_train_pack_plan fills `plan`
 * (host, 8 x int64 per entry: see kernels_train.hip) for n weights given as in cosy_train_gemm and returns the pool size in floats and the grid;
 * the caller uploads the plan, cosy_train_pack_all packs into `pool` (pool_floats floats), cosy_train_gemm_packed is cosy_train_gemm on entry e's
 * packed form at pool + plan[e][1]. */
int cosy_train_pack_plan(int n, const float* const* W, const int* K, const int* N, const int* w_is_kn, long long* plan, long long* pool_floats,
                         long long* n_blocks);
int cosy_train_pack_all(const long long* plan_dev, int n, long long n_blocks, float* pool, cosy_stream_t stream);
int cosy_train_gemm_packed(const float* A, const float* pool, long long packed_offset, long M, int K, int N, const float* add, float* out,
                           cosy_stream_t stream);

int cosy_wgrad_tall_supported(long M, int N, int K);
int cosy_wgrad_tall(const float* dY, const float* X, long M, int N, int K, float* dW, void* workspace, cosy_stream_t stream);
/* per-sample reductions / broadcasts over the HW pixels of a (B,HW,C) activation: mean (adaptive_avg_pool2d),
 * sum of a*a2 (gradient of the squeeze-excite gate), a*g[b,c] (+ add[b,c]*add_scale), v[b,c]*scale broadcast.
 * All of them need C % 4 == 0 (16-byte channel quads), else COSY_EINVAL. */
int cosy_rows_mean(const float* a, int B, int HW, int C, float* out, void* workspace, cosy_stream_t stream);
/* Squeeze-excite without the unscaled activation in memory (efficientnet.py:84-90 in train mode): the per-sample means / dot products take the
 * BatchNorm INPUT `raw` and recompute swish(bn(raw)) per element (the arithmetic of cosy_bn_train_apply), and cosy_bn_train_apply_gated writes
 * swish(bn(raw)) * cgate[sample][c] -- the project conv's input -- directly. */
int cosy_rows_mean_bn(const float* raw, const float* mean, const float* rstd, const float* gamma, const float* beta, int B, int HW, int C, float* out,
                      void* workspace, cosy_stream_t stream);
int cosy_rows_dot_bn(const float* a, const float* raw, const float* mean, const float* rstd, const float* gamma, const float* beta, int B, int HW, int C,
                     float* out, void* workspace, cosy_stream_t stream);
int cosy_bn_train_apply_gated(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, long M, int C, int act,
                              const float* cgate, int HW, float* out, cosy_stream_t stream);
int cosy_rows_dot(const float* a, const float* a2, int B, int HW, int C, float* out, void* workspace, cosy_stream_t stream);
int cosy_rows_scale(const float* a, const float* g, const float* add, float add_scale, int B, int HW, int C, float* out,
                    cosy_stream_t stream);
int cosy_rows_broadcast(const float* v, float scale, int B, int HW, int C, float* out, cosy_stream_t stream);
/* elementwise Swish (kind 0) / sigmoid (kind 1) and their gradients */
/* Squeeze-excite of an MBConv block in the training step (efficientnet.py:85-88 and its autograd), one launch forward, two backward:
 *   forward : h_pre (B,Cse) = pooled (B,C) w_reduce^T + b_reduce;  gate (B,C) = sigmoid(swish(h_pre) w_expand^T + b_expand)
 *   backward: from dgate (B,C): dpooled (B,C), dw_reduce (Cse,C), db_reduce (Cse), dw_expand (C,Cse), db_expand (C); sums over the batch in
 *             sample order (deterministic).  Weight layouts are the module's own (_se_reduce.weight (Cse,C,1,1), _se_expand.weight (C,Cse,1,1)).
 * cosy_fc_small_*: a Linear layer with J <= 16 outputs (models/pose.py:84: pose_fc, J = 9): y = x w^T + bias and its three gradients.
 * They replace torch.addmm / matmul + elementwise launches (rocBLAS at 64 rows). */
int cosy_se_train_forward(const float* pooled, const float* w_reduce, const float* b_reduce, const float* w_expand, const float* b_expand, int B, int C,
                          int Cse, float* h_pre, float* gate, cosy_stream_t stream);
int cosy_se_train_backward(const float* dgate, const float* gate, const float* h_pre, const float* pooled, const float* w_reduce, const float* w_expand,
                           int B, int C, int Cse, float* dpooled, float* dw_reduce, float* db_reduce, float* dw_expand, float* db_expand, void* workspace,
                           cosy_stream_t stream);
int cosy_fc_small_forward(const float* x, const float* w, const float* bias, int B, int C, int J, float* y, cosy_stream_t stream);
int cosy_fc_small_backward(const float* dy, const float* x, const float* w, int B, int C, int J, float* dx, float* dw, float* db, cosy_stream_t stream);
int cosy_act_forward(const float* x, long n, int kind, float* out, cosy_stream_t stream);
int cosy_act_backward(const float* x, const float* dy, long n, int kind, float* dx, cosy_stream_t stream);
/* stem 3x3 stride-2 patches of the NHWC8 input as GEMM rows: cols (B*Ho*Wo, 54), column = (ky*3+kx)*6 + c */
int cosy_stem_im2col(const float* x_nhwc8, int B, int H, int W, float* cols, cosy_stream_t stream);
/* the same with a row stride ld >= 54 (columns 54..ld-1 are written as zeros): ld = 56 gives the 16-byte aligned rows
 * cosy_train_gemm wants */
int cosy_stem_im2col_ld(const float* x_nhwc8, int B, int H, int W, int ld, float* cols, cosy_stream_t stream);
/* gradient of loss_refiner_CO_disentangled (cosypose_ops.py:49-82) wrt refiner_outputs, times the upstream dloss (B) */
int cosy_loss_refiner_disentangled_backward(const float* TCO_possible_gt, const float* TCO_input, const float* refiner_outputs,
                                            const float* K_crop, const float* pts_table, const int* obj_id, int B, int S, int P,
                                            const float* dloss, float* d_refiner_outputs, cosy_stream_t stream);
/* torch.nn.utils.clip_grad_norm_(max_norm, 2) on a flat gradient buffer -> norm_and_coef[0] = total norm,
 * [1] = min(1, max_norm/(norm+1e-6)) (1 when max_norm <= 0); torch.optim.Adam step on flat buffers, gradients scaled by
 * norm_and_coef[1] when given (train_pose.py:325-329). */
int cosy_grad_norm_clip(const float* grads, long n, float max_norm, float* norm_and_coef, void* workspace, cosy_stream_t stream);
int cosy_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, const float* norm_and_coef, cosy_stream_t stream);

/* ---- on-device mesh rasteriser behind renderer.render (interface of BulletBatchRenderer.render,
 * cosypose/rendering/bullet_batch_renderer.py:46-90; camera model of simulator/camera.py:9-33).  verts / colors
 * (n_obj,V,3), faces (n_obj,F,3) int32 (padded), n_faces (n_obj); per crop obj_id, TCO (B,4,4), K (B,3,3) ->
 * rgb (B,3,H,W) in [0,1] (black background, non-finite poses -> black) and optional depth (B,H,W) in metres.
 * Shading = vertex colour x (ambient + diffuse |n.l|), l = light direction in the camera frame (PyBullet's OpenGL shading
 * is third-party: pixel values parity-unpinned).  `scratch`: cosy_render_scratch_bytes(B,V,H,W) bytes.
 * Limits, checked before anything is launched (COSY_EINVAL, cosy_last_error() names the argument): 0 <= B <= 65535 (the batch is
 * the grid's y dimension); H, W, V, F > 0; with B > 0 every pointer except `depth` non-null ("null TCO").  B = 0 returns COSY_OK
 * and touches no pointer.  depth = NULL: no depth is written.  A triangle with any vertex at z <= 0.01 is dropped whole (OpenGL
 * would clip it at the near plane).  The light direction must be a UNIT vector: it is used as given, neither checked nor
 * normalised (cosypose_amd.rasterizer.HipBatchRenderer normalises it for its callers). */
size_t cosy_render_scratch_bytes(int B, int V, int H, int W);
int cosy_render_meshes(const float* verts, const float* colors, const int* faces, const int* n_faces, const int* obj_id,
                       const float* TCO, const float* K, int B, int V, int F, int H, int W, float ambient, float diffuse,
                       float light_x, float light_y, float light_z, float* rgb, float* depth, void* scratch, cosy_stream_t stream);

/* The object set on the device (one row per label, padded to V vertices / F faces) and the shading model.
 * cosy_shade_t.smooth = 1 selects the OpenGL-like model that PyBullet's hardware renderer has in structure
 * (bullet_scene_renderer.py:38-60 -> getCameraImage(ER_BULLET_HARDWARE_OPENGL)): texture x vertex colour, interpolated
 * vertex normals, one-sided Lambert + Blinn-Phong highlight, light fixed in the world frame (= the object's frame: every
 * object is rendered at TWO = identity, bullet_batch_renderer.py:56-59), 8-bit output (quantize = 1:
 * `images.float() / 255`, bullet_batch_renderer.py:83-84).  The shader's constants are third-party: pixel values stay
 * parity-unpinned. */
typedef struct {
    const float* verts;   /* (n_obj,V,3) metres, object frame */
    const float* colors;  /* (n_obj,V,3) in [0,1] */
    const float* normals; /* (n_obj,V,3) unit vertex normals, or NULL (flat shading only) */
    const float* uvs;     /* (n_obj,V,2) texture coordinates, or NULL */
    const float* tex;     /* (n_obj,TH,TW,4) RGB(+pad) fp32 in [0,1], or NULL */
    const int* faces;     /* (n_obj,F,3) */
    const int* n_faces;   /* (n_obj) */
    int V, F, TH, TW;
} cosy_mesh_t;
typedef struct {
    float ambient, diffuse, specular, shininess;
    float light[3];       /* unit vector from the surface towards the light: a precondition, not checked, not normalised */
    int light_frame;      /* 0: camera frame, 1: object (PyBullet world) frame */
    int smooth;           /* 0: flat two-sided face normals, 1: interpolated vertex normals */
    int quantize;         /* 1: round colours to multiples of 1/255 */
} cosy_shade_t;
/* Limits as cosy_render_meshes; in addition smooth = 1 without mesh->normals and mesh->tex without mesh->uvs or with TH / TW <= 0
 * are refused (COSY_EINVAL). */
int cosy_render_meshes_ex(const cosy_mesh_t* mesh, const cosy_shade_t* shade, const int* obj_id, const float* TCO, const float* K, int B,
                          int H, int W, float* rgb, float* depth, void* scratch, cosy_stream_t stream);

/* Render + crop + pack in one pass (replaces renderer.render -> cosy_crop_pack when the renderer is this library's): the
 * resolve pass of the rasteriser also samples the observed frame (roi_align, as cosy_crop_pack) and writes the network's
 * 8-channel NHWC input pixel directly -- no fp32 (B,3,H,W) render tensor is written or read.  K = K_crop (B,3,3); the
 * render resolution is the network's input resolution.  Same limits as cosy_render_meshes_ex (0 <= B <= 65535; H, W, h, w > 0; mesh
 * with V, F > 0 and verts / colors / faces / n_faces; smooth shading needs normals, a texture needs uvs and TH, TW > 0); im_id may
 * be NULL (crop b reads frame b); dtype is COSY_F32, COSY_BF16 or COSY_F16. */
int cosy_render_crop_pack(cosy_net_t* net, const cosy_mesh_t* mesh, const cosy_shade_t* shade, const int* obj_id, const float* TCO,
                          const float* K_crop, const float* frames_nhwc4, const int* im_id, const float* boxes_crop, int B, int N, int h,
                          int w, void* scratch, cosy_stream_t stream);
int cosy_render_crop_pack_to(void* x_nhwc8, int dtype, const cosy_mesh_t* mesh, const cosy_shade_t* shade, const int* obj_id,
                             const float* TCO, const float* K_crop, const float* frames_nhwc4, const int* im_id, const float* boxes_crop,
                             int B, int N, int h, int w, int H, int W, void* scratch, cosy_stream_t stream);

/* ---- scene renderer: many object instances in many views, one shared z-buffer per view (interface of BulletSceneRenderer.render_scene,
 * cosypose/rendering/bullet_scene_renderer.py:12-64; camera model, near plane, non-finite poses and shading as cosy_render_meshes_ex).
 * A ROW is one object instance in one view: obj_id (N), view_id (N) in [0, n_views), TCO (N,4,4), optional color (N,4); K (n_views,3,3);
 * one resolution H x W per call.  Rows may come in any order, a view may have no row.
 *
 * Z-buffer key, 64 bits:  depth bits (32) | slot (COSY_SCENE_SLOT_BITS = 10) | face id (COSY_SCENE_FACE_BITS = 22),
 * slot = the row's rank among the rows of its view, in call order.  Per pixel the smaller depth wins; at equal depth bits the row that
 * comes first in the call; then the smaller face id.  Hence at most COSY_SCENE_MAX_FACES = 2^22 faces per mesh (mesh->F) and
 * COSY_SCENE_MAX_INSTANCES = 2^10 rows per view; a call outside either is refused before any launch.
 *
 * obj_id and view_id are HOST arrays (they are checked, ranked and uploaded by the call); background: 3 HOST floats.  Everything else is
 * device memory.  color: a row with color[r][3] >= 0 is drawn in the flat colour color[r][0..2] in place of the mesh's vertex colours and
 * texture (shading still applies; the alpha value itself is ignored); color[r][3] < 0, or color = NULL: the mesh's own colours.
 * Outputs: rgb (n_views,3,H,W) in [0,1]; optional depth (n_views,H,W) metres; optional mask (n_views,H,W) int32 = the ROW INDEX of the
 * winner.  Background pixels: the background colour, depth 0, mask -1.  Optional per-row statistics (all four pointers or none):
 * px_count_all (N) int32 = pixels of the row's silhouette (covered by any of its live triangles, whatever is in front),
 * px_count_visib (N) int32 = pixels the row wins, bbox_obj / bbox_visib (N,4) float32 = xyxy boxes of inclusive pixel indices of the two
 * sets, (-1,-1,-1,-1) when empty.  Integer atomics only: equal inputs give equal bits.
 * scratch: cosy_render_scene_scratch_bytes(N, n_views, mesh->V, H, W) bytes = [z-buffers (n_views,H,W) u64 | projected vertices (N,V,3) |
 * id table (4 N + n_views + 1 int32) | silhouette bits (N, ceil(H W / 32)) u32 | statistics (N,10) int32], each padded to 32 bytes.  Do
 * not share one scratch between streams.
 * Limits (COSY_EINVAL, cosy_last_error() names the argument): 0 <= N, n_views <= 65535 (grid y); H, W > 0; with N > 0 obj_id, view_id,
 * TCO, K non-null; with n_views > 0 background, rgb, scratch non-null.  N = 0 is legal: every view is background. */
#define COSY_SCENE_FACE_BITS 22
#define COSY_SCENE_SLOT_BITS (32 - COSY_SCENE_FACE_BITS)
#define COSY_SCENE_MAX_FACES (1 << COSY_SCENE_FACE_BITS)
#define COSY_SCENE_MAX_INSTANCES (1 << COSY_SCENE_SLOT_BITS)
size_t cosy_render_scene_scratch_bytes(int N, int n_views, int V, int H, int W);
int cosy_render_scene(const cosy_mesh_t* mesh, const cosy_shade_t* shade, const int* host_obj_id, const int* host_view_id, const float* TCO,
                      const float* color, const float* K, int N, int n_views, int H, int W, const float* background, float* rgb, float* depth,
                      int* mask, int* px_count_all, int* px_count_visib, float* bbox_obj, float* bbox_visib, void* scratch,
                      cosy_stream_t stream);

/* ---- scene-level bundle adjustment (cosypose/multiview/bundle_adjustment.py:164-222), ALL FLOAT64 ----
 * States are 9-D poses (ortho6d rotation, translation; transform_ops.py:54-64): TWO_9d (n_obj,9) of the objects, TCW_9d (n_views,9) of the
 * cameras.  Candidate c observes object cand_obj[c] in view cand_view[c] with pose cand_TCO[c] (n_cand,4,4); K (n_views,3,3).  Points and
 * symmetries come from per-mesh tables pts_table (n_mesh,P,3), sym_table (n_mesh,S,4,4), n_sym (n_mesh) int32; cand_mesh[c] / obj_mesh[o]
 * are the table rows of a candidate's label / an object's label.  The unknowns are ordered objects first: n = 9 (n_obj + n_views), and
 * n_obj + n_views <= 128 (COSY_ESIZE beyond).  Residual r = (c P + point) 2 + (0: x, 1: y), the reference's order.
 *
 * cosy_ba_upload_ids: checks the HOST id arrays against their tables (COSY_EINVAL names the first id outside; nothing is copied or
 *   launched) and copies them into `ids` (3 n_cand + n_obj int32 on the device), the id table every call below takes.
 * cosy_ba_align (:164-173): TCO = TCW[view] TWO[obj]; best symmetry of each candidate against it by the reprojected distance above;
 *   -> dists (n_cand), best_sym (n_cand) int32, TCO_cand_aligned (n_cand,4,4) = cand_TCO S.
 * cosy_ba_linearize (:175-214 and the products of :218-219): errors e = y - yhat (n_res = 2 P n_cand), loss = mean(min(e^2, threshold))
 *   (1 double; the clamp enters the loss only), A = J^T J (n,n), b = J^T e (n) with J the ANALYTIC Jacobian of yhat, accumulated as
 *   per-candidate 18x18 blocks summed in candidate order (no atomics: bit-identical from run to run).  J_obj, J_view (n_res,9) each,
 *   optional: the Jacobian rows with respect to the residual's own object / view (every other entry of the dense row is 0).
 * cosy_ba_solve (:216-222): h = (A + lambda I)^-1 b by Cholesky, lambda > 0; n <= 1152.
 * workspace: cosy_ba_workspace_bytes(n_cand, P, n_obj, n_views) bytes of device scratch (0 for sizes the calls reject) = the larger of
 *   what cosy_ba_linearize needs (190 doubles per candidate) and what cosy_ba_solve needs (n*n doubles for the factor).  The two SHARE it
 *   from offset 0: a solve overwrites the linearisation's scratch, which is dead by then (A and b are complete when cosy_ba_linearize's
 *   launches have run; calls on one stream are ordered).  Do not share one workspace between streams. */
size_t cosy_ba_workspace_bytes(int n_cand, int P, int n_obj, int n_views);
int cosy_ba_upload_ids(const int* host_cand_obj, const int* host_cand_view, const int* host_cand_mesh, const int* host_obj_mesh, int n_cand,
                       int n_obj, int n_views, int n_mesh, int* ids, cosy_stream_t stream);
int cosy_ba_align(const double* TWO_9d, const double* TCW_9d, const double* cand_TCO, const double* K, const int* ids, const double* pts_table,
                  const double* sym_table, const int* n_sym, int n_cand, int n_obj, int n_views, int n_mesh, int P, int S, double* dists,
                  int* best_sym, double* TCO_cand_aligned, cosy_stream_t stream);
int cosy_ba_linearize(const double* TWO_9d, const double* TCW_9d, const double* TCO_cand_aligned, const double* K, const int* ids,
                      const double* pts_table, int n_cand, int n_obj, int n_views, int n_mesh, int P, double residuals_threshold,
                      double* errors, double* loss, double* A, double* b, double* J_obj, double* J_view, void* workspace,
                      cosy_stream_t stream);
int cosy_ba_solve(const double* A, const double* b, int n, double lambda, double* h, void* workspace, cosy_stream_t stream);

/* ---- batched bundle adjustment: G problems per call, the Levenberg-Marquardt loop (bundle_adjustment.py:238-277) on the device ----
 * A batch is the concatenation of G problems that share the mesh tables: candidates (n_cand), objects (n_obj) and views (n_views) are
 * TOTALS over the batch, problem g owns the candidate rows cand_off[g] .. cand_off[g+1], the object rows obj_off[g] .. obj_off[g+1] of
 * TWO_9d (n_obj,9), the view rows view_off[g] .. view_off[g+1] of TCW_9d / K, and candidates name GLOBAL object and view rows.  Its
 * unknowns are ordered as in the single problem (its objects, then its views; n_g = 9 blocks_g, blocks_g <= 128), its parameter offset
 * is 9 (obj_off[g] + view_off[g]) and its A lies at the sum of n_k^2 over the problems before it.
 *
 * cosy_ba_batch_upload: checks the HOST tables (offsets start at 0 and rise, every problem has a candidate, an object and a view and
 *   at most 128 blocks -- COSY_ESIZE beyond --, every id inside ITS problem's rows, mesh ids inside [0, n_mesh)) before anything is
 *   copied, then writes the device `table` (cosy_ba_batch_table_bytes(G, n_cand, n_obj) bytes: the ids, each candidate's problem, the
 *   offsets, the A offsets) and waits for the copy; a_total receives the sum of n_g^2, max_blocks the largest blocks_g.
 * cosy_ba_ctrl_t: the control record of one problem.  loss = the loss at the current state, next_loss = at the updated one.
 * cosy_ba_batch_linearize: align + linearise + accumulate, one launch each over the batch, at the current (which = 0) or the updated
 *   (which = 1) states -> the problem's A, b (in the workspace) and ctrl.loss / ctrl.next_loss.  Workgroups of a problem that is
 *   `finished`, or with which = 0 whose last iteration accepted its step (`prev_update`: A, b and the loss are those of the accepted
 *   state already), leave at once.  The same device code as cosy_ba_align / cosy_ba_linearize: the same bits.
 * cosy_ba_batch_solve_step: one workgroup per problem: the Cholesky of cosy_ba_solve on A_g + lambda_g I, then updated = current + h
 *   (the views' part of h dropped when optimize_cameras = 0).
 * cosy_ba_batch_record: appends (iteration, lambda, loss and, with hist_TWO_9d / hist_TCW_9d given, the current states) as row n_hist
 *   of the problem's history -- hist_iteration / hist_lambda / hist_loss (G, n_hist_rows), hist_TWO_9d (n_hist_rows, n_obj, 9),
 *   hist_TCW_9d (n_hist_rows, n_views, 9) -- and marks the problem `finished` if `done` was set: where the reference appends, then
 *   breaks.  table and the states may be NULL when no state history is asked for.
 * cosy_ba_batch_decide: rho = loss - next_loss; |rho| < eps: done = 1, nothing else; else rho > eps: current = updated, loss =
 *   next_loss, lambda = max(lambda / L_down, 1e-7), prev_update = 1; otherwise (a NaN rho too) lambda = min(lambda L_up, 1e7),
 *   prev_update = 0.  Finished problems are left alone.  table and the states may be NULL: the records alone are then updated.
 * cosy_ba_batch_iterate: iterations n_first .. n_first + n_count - 1, each = linearize(0), record(n), solve_step, linearize(1), decide.
 *   Launches on one stream are the only synchronisation; nothing is read back.
 * workspace: cosy_ba_batch_workspace_bytes(n_cand, n_obj + n_views, a_total) bytes.  Do not share one between streams. */
typedef struct {
    double loss, next_loss, lambda;
    int done, prev_update, finished, n_hist;
} cosy_ba_ctrl_t;
typedef struct {
    int G, n_cand, n_obj, n_views, n_mesh, P, S, max_blocks, n_hist_rows, optimize_cameras;
    long long a_total;
    double residuals_threshold, L_down, L_up, eps;
    const void* table;
    const double *cand_TCO, *K, *pts_table, *sym_table;
    const int* n_sym;
    double *TWO_9d, *TCW_9d, *TWO_9d_updated, *TCW_9d_updated;
    cosy_ba_ctrl_t* ctrl;
    int* hist_iteration;
    double *hist_lambda, *hist_loss, *hist_TWO_9d, *hist_TCW_9d;
    void* workspace;
} cosy_ba_batch_t;
size_t cosy_ba_batch_table_bytes(int G, int n_cand, int n_obj);
size_t cosy_ba_batch_workspace_bytes(int n_cand, int n_blocks, long long a_total);
int cosy_ba_batch_upload(const int* host_cand_obj, const int* host_cand_view, const int* host_cand_mesh, const int* host_obj_mesh,
                         const int* host_cand_off, const int* host_obj_off, const int* host_view_off, int G, int n_mesh, void* table,
                         long long* a_total, int* max_blocks, cosy_stream_t stream);
int cosy_ba_batch_linearize(const cosy_ba_batch_t* batch, int which, cosy_stream_t stream);
int cosy_ba_batch_solve_step(const cosy_ba_batch_t* batch, cosy_stream_t stream);
int cosy_ba_batch_record(cosy_ba_ctrl_t* ctrl, int G, int iteration, int n_hist_rows, const void* table, int n_cand, int n_obj,
                         int n_views, const double* TWO_9d, const double* TCW_9d, int* hist_iteration, double* hist_lambda,
                         double* hist_loss, double* hist_TWO_9d, double* hist_TCW_9d, cosy_stream_t stream);
int cosy_ba_batch_decide(cosy_ba_ctrl_t* ctrl, int G, double L_down, double L_up, double eps, const void* table, int n_cand, int n_obj,
                         double* TWO_9d, double* TCW_9d, const double* TWO_9d_updated, const double* TCW_9d_updated,
                         cosy_stream_t stream);
int cosy_ba_batch_iterate(const cosy_ba_batch_t* batch, int n_first, int n_count, cosy_stream_t stream);

/* ---- multi-view candidate matching, CosyPose stage 2 (cosypose/multiview/ransac.py:19-88, csrc/cosypose_cext.cpp:107-216), float32 ----
 * The scene: cand_poses (n_cand,4,4) TCO of every candidate, cand_mesh (n_cand) int32 row of its label in pts_table (n_mesh,P,3) /
 * sym_table (n_mesh,S,4,4, identity-padded) / n_sym (n_mesh) int32.  Tentative matches are stored once per ORDERED view pair, not per
 * hypothesis: tmatches (n_tm,4) int32 = cand1, cand2, rank of cand1 among the pair's cand1s, rank of cand2 among its cand2s (both
 * < the pair's number of matches); the matches of pair p are rows pair_off[p] .. pair_off[p+1].  max_tm = the longest such list;
 * beyond cosy_ransac_max_tmatches() (4096) the calls return COSY_ESIZE.  All pointers are device pointers.  Ids outside their tables
 * are skipped (no inlier / best_sym -1), never dereferenced; callers check them on the host.
 *
 * cosy_ransac_hypotheses: seeds (H,4) int32 = match1 (a, b), match2 (g, d).  Over the n_sym symmetries S of a's label: the
 *   symmetric_distance_batched_fast distance (as cosy_symmetric_distance, mode 1) of a's label between TC1Og and
 *   ((TC1Oa S) inv(TC2Ob)) TC2Od; the first strict minimum S* -> TC1C2 (H,4,4) = (TC1Oa S*) inv(TC2Ob), best_sym (H), gap (H) = runner-up
 *   distance - minimum (inf with one symmetry); sym_dists (H,S), optional: every symmetry's distance (inf beyond n_sym).  S <= 64.
 * cosy_ransac_score: hypothesis h belongs to view pair hyp_pair[h].  Distance of each of the pair's matches = the same distance between
 *   TC1Oa and TC1C2[h] TC2Ob; inliers: distance <= dist_threshold; ordered by (distance, list position) and walked greedily so that every
 *   cand1 and every cand2 is used once -> n_inliers (H) int32, dists_sum (H) added in that order.  Optional tables, both laid out as the
 *   reference's expanded list (hypothesis h's matches from hyp_dist_off[h] on, (H) int64): dists_out receives the distances, dists_in
 *   REPLACES them (the reference's find_ransac_inliers on given distances; the scene and TC1C2 are then not read and may be NULL / 0).
 * cosy_ransac_best: the hypotheses of pair p are pair_hyps[pair_hyp_off[p] .. pair_hyp_off[p+1]), ascending.  Most inliers, then the
 *   smaller dists_sum, then the lower id, among those with >= n_min_inliers -> best_hyp (n_pairs), -1 for none; with skip_hypothesis_0
 *   hypothesis 0 is never reported (the reference tests `hypothesis_id > 0`).  The winner's walk is repeated and its matches written to
 *   match_cand1/2[pair_off[p] ...], their number to n_matches (n_pairs).
 * Fixed summation orders, no atomics: equal inputs give equal bits. */
int cosy_ransac_max_tmatches(void);
int cosy_ransac_hypotheses(const float* cand_poses, const int* cand_mesh, const float* pts_table, const float* sym_table, const int* n_sym,
                           int n_cand, int n_mesh, int P, int S, const int* seeds, int H, float* TC1C2, int* best_sym, float* gap,
                           float* sym_dists, cosy_stream_t stream);
int cosy_ransac_score(const float* cand_poses, const int* cand_mesh, const float* pts_table, const float* sym_table, int n_cand, int n_mesh,
                      int P, int S, const float* TC1C2, const int* hyp_pair, int H, const int* pair_off, const int* tmatches, int n_pairs,
                      int max_tm, float dist_threshold, const long long* hyp_dist_off, const float* dists_in, float* dists_out,
                      int* n_inliers, float* dists_sum, cosy_stream_t stream);
int cosy_ransac_best(const float* cand_poses, const int* cand_mesh, const float* pts_table, const float* sym_table, int n_cand, int n_mesh,
                     int P, int S, const float* TC1C2, int H, const int* n_inliers, const float* dists_sum, const int* pair_hyp_off,
                     const int* pair_hyps, const int* pair_off, const int* tmatches, int n_pairs, int max_tm, float dist_threshold,
                     int n_min_inliers, int skip_hypothesis_0, const long long* hyp_dist_off, const float* dists_in, int* best_hyp,
                     int* n_matches, int* match_cand1, int* match_cand2, cosy_stream_t stream);

/* ---- training augmentations of PoseDataset.get_data (cosypose/datasets/pose_dataset.py:82-87, datasets/augmentations.py:40-125), uint8 ----
 * images / out (B,3,H,W) uint8, masks (B,H,W) uint8 or NULL, backgrounds (n_bg,3,H,W) uint8 or NULL, params (B) records:
 *   bg      row of `backgrounds` pasted where masks == 0, or -1 (then masks / backgrounds are not read for this image);
 *   flags   COSY_AUG_GATE: the Pillow chain runs (without it the image is only pasted); COSY_AUG_SHARPNESS / _CONTRAST / _BRIGHTNESS /
 *           _COLOR: that ImageEnhance stage runs with its factor below; COSY_AUG_GRAY: the float32 grey conversion runs last;
 *   k       GaussianBlur radius 1, 2 or 3 (read only under COSY_AUG_GATE, where the blur always runs).
 * Every byte equals what Pillow 12 gives for the same record (DESIGN.md section 14 holds the arithmetic): integer box passes, float32
 * products and sums each rounded on their own, an integer sum of L for Contrast's mean.  No floating-point atomics: equal inputs give
 * equal bytes.  out may alias images (images is read by the first launch only, out is written by the last and by the images whose gate
 * is off, point by point).  workspace: cosy_augment_workspace_bytes(B, H, W) bytes, 16-byte aligned; it holds the two intermediate
 * batches and the per-image sums.  A bg outside [-1, n_bg) or a k outside 1..3 under the gate is refused on the device: the image is
 * copied unchanged to out and nothing outside the tables is read (callers check their records on the host). */
enum { COSY_AUG_GATE = 1, COSY_AUG_SHARPNESS = 2, COSY_AUG_CONTRAST = 4, COSY_AUG_BRIGHTNESS = 8, COSY_AUG_COLOR = 16, COSY_AUG_GRAY = 32 };
typedef struct cosy_aug_params {
    int bg, flags, k;
    float sharpness, contrast, brightness, color;
    int reserved; /* 32 bytes per record */
} cosy_aug_params_t;
size_t cosy_augment_workspace_bytes(int B, int H, int W);
int cosy_augment_batch(const unsigned char* images, const unsigned char* masks, const unsigned char* backgrounds, int n_bg,
                       const cosy_aug_params_t* params, int B, int H, int W, unsigned char* out, void* workspace, size_t workspace_bytes,
                       cosy_stream_t stream);

/* ---- BOP pose errors (Hodan et al., "BOP Challenge 2020", section 2.2): MSSD, MSPD and the pixel counts of VSD, float32 ----
 * A pair is one estimate TCO_pred, one ground truth TCO_gt, one object obj_id and one view view_id; lengths in metres, pixel
 * coordinates are integer indices (no + 0.5), K (n_views,3,3) is per view.  Object tables: verts (n_obj,V,3) with n_verts (n_obj)
 * used rows, sym_table (n_obj,S,4,4) with n_sym (n_obj) used rows (the identity first), faces (n_obj,F,3) with n_faces (n_obj).
 * DESIGN.md section 15 states the arithmetic; every product and sum is rounded on its own (no contraction), nothing uses
 * floating-point atomics: equal inputs give equal bits, and a pair's result does not depend on what else is in the call.
 * All three steps check on the host, before any launch (COSY_EINVAL, cosy_last_error() names the argument): counts >= 0, table sizes
 * and H, W > 0, every pointer that is read non-null, workspace 16-byte aligned and at least its *_workspace_bytes; B = 0 (N = 0)
 * returns COSY_OK at once with null pointers.  Ids are device values and are checked there: an obj_id / view_id / instance id outside
 * its table, or a non-finite entry in a pose or in the view's K, reads nothing and gives NaN errors, an empty box and zero counts;
 * n_verts, n_sym and n_faces are clamped to [0, V], [0, S] and [0, F].
 *
 * Step 1.  mssd[b] = min over s < n_sym of max over x of |P_est x - P_gt S x|, mspd[b] the same on the projections
 * (fx X / Z + cx, fy Y / Z + cy), Z not clamped.  The maxima are combined as integer maxima of float bit patterns.  B is bounded by
 * B * ceil(V / 1024) * ceil(S / 8) < 2^31. */
size_t cosy_bop_mssd_mspd_workspace_bytes(int B, int S);
int cosy_bop_mssd_mspd(const float* TCO_pred, const float* TCO_gt, const int* obj_id, const int* view_id, const float* K, const float* verts,
                       const int* n_verts, const float* sym_table, const int* n_sym, int B, int n_obj, int n_views, int V, int S, float* mssd,
                       float* mspd, void* workspace, size_t workspace_bytes, cosy_stream_t stream);
/* Step 2.  An instance is one (object, view, pose).  cosy_bop_instance_boxes: boxes (N,4) int32 = x0, y0, x1, y1 (inclusive) of the
 * instance's vertices beyond the near plane, clipped to the (H,W) frame; empty (x1 < x0 or y1 < y0) when nothing can be drawn, with
 * x1 = y1 = -2 for an instance whose ids lie outside the tables or whose pose or K is not finite (a pair with such an instance gets zero
 * counts in step 3, whatever its other instance shows).  The
 * caller reads the boxes, gives every non-empty box a window of (x1 - x0 + 1) (y1 - y0 + 1) floats at win_offset[n] (int64, in
 * floats) of a store of n_pixels floats = the workspace, and calls cosy_bop_render_windows: window pixel (x - x0, y - y0) receives
 * the depth cosy_render_meshes_ex writes at (x, y) of that instance's (H,W) depth image, bit for bit, 0 = background.  A window that
 * does not fit its box or the store is skipped, never written past. */
int cosy_bop_instance_boxes(const float* TCO, const int* obj_id, const int* view_id, const float* K, const float* verts, const int* n_verts,
                            int N, int n_obj, int n_views, int V, int H, int W, int* boxes, cosy_stream_t stream);
size_t cosy_bop_windows_workspace_bytes(long long n_pixels);
int cosy_bop_render_windows(const float* TCO, const int* obj_id, const int* view_id, const float* K, const float* verts, const int* faces,
                            const int* n_faces, const int* boxes, const long long* win_offset, int N, int n_obj, int n_views, int V, int F, int H,
                            int W, long long n_pixels, void* workspace, size_t workspace_bytes, cosy_stream_t stream);
/* Step 3.  Pair b compares the windows of instances est_inst[b] and gt_inst[b] (both of view inst_view[.]) with the measured depth
 * depth_test (n_views,H,W), 0 = missing, over the union box of the two windows.  counts (B, 2 + n_tau) int32 = |U|, |I|, c_1..c_n_tau
 * with taus (B,n_tau) absolute metres, 1 <= n_tau <= 16, delta the visibility tolerance in metres. */
size_t cosy_bop_vsd_workspace_bytes(int B);
int cosy_bop_vsd_counts(const int* est_inst, const int* gt_inst, const int* inst_view, const int* boxes, const long long* win_offset,
                        const float* windows, long long n_pixels, const float* depth_test, const float* K, const float* taus, float delta, int B,
                        int N, int n_views, int n_tau, int H, int W, int* counts, void* workspace, size_t workspace_bytes,
                        cosy_stream_t stream);

/* ---- BOP ground-truth annotations: what the BOP toolkit's calc_gt_masks.py / calc_gt_info.py write ----
 * Every instance is drawn alone on a canvas of 3H x 3W whose centre third is the (H,W) frame: the caller forms K' = K with cx + W and
 * cy + H (one float32 addition each) and calls cosy_bop_instance_boxes and cosy_bop_render_windows with K' and (3H, 3W).
 * cosy_gt_info then reads boxes (N,4) and win_offset (N) as those two left them, windows = the store of n_pixels floats, inst_view (N)
 * the row of every instance in depth_test (n_views,H,W) (measured depth in metres, 0 = missing) and in K (n_views,3,3), the UNSHIFTED
 * intrinsics, and id_in_segm (N) in [1, 255].  With dist() of section 15 in the frame's coordinates (x = x_canvas - W, y = y_canvas - H),
 * dist_gt of the window depth and t of depth_test:  mask = dist_gt > 0;  V = mask and (dist_gt - t <= delta or t == 0); a NaN in
 * depth_test fails every comparison.  Written in full for every n < N:
 *   counts (N,3) int32 = px_count_all (depth > 0 on the whole canvas), px_count_valid (mask and t > 0), px_count_visib (V);
 *   bbox_obj (N,4) int32 = x, y, w, h of {depth > 0} on the canvas in the frame's coordinates (x, y may be negative, w = max - min);
 *   bbox_visib (N,4) the same of V; both -1, -1, -1, -1 where px_count_visib = 0.
 * Accumulated into (the caller zeroes them once, chunks of instances then share them): composite (n_views,H,W) int32 = the largest
 * id_in_segm whose V holds the pixel; mask, mask_visib (N,H,W) uint8 0 / 1, both optional (null: not written), stored on the part of
 * the frame the instance's window covers.  cosy_gt_composite_u8 narrows n words of the composite to bytes.
 * Checked on the host before any launch (COSY_EINVAL, cosy_last_error() names the argument): N, n_pixels >= 0, n_views, H, W > 0 with
 * 9 H W and N ceil(9 H W / 2048) < 2^31, every pointer that is read or written non-null (windows only when n_pixels > 0), workspace
 * 16-byte aligned and at least cosy_gt_info_workspace_bytes(N); N = 0 (n = 0) returns COSY_OK at once with null pointers.  Checked on
 * the device, where the boxes are: an instance whose box is empty or dead (x1 = -2), whose view lies outside [0, n_views), or whose
 * window does not lie inside the n_pixels of the store as a whole reads nothing and gets zero counts and -1 boxes.  Integer atomics
 * only: equal inputs give equal bytes, and an instance's rows do not depend on what else is in the call. */
size_t cosy_gt_info_workspace_bytes(int N);
int cosy_gt_info(const int* inst_view, const int* id_in_segm, const int* boxes, const long long* win_offset, const float* windows,
                 long long n_pixels, const float* depth_test, const float* K, float delta, int N, int n_views, int H, int W, int* counts,
                 int* bbox_obj, int* bbox_visib, int* composite, unsigned char* mask, unsigned char* mask_visib, void* workspace,
                 size_t workspace_bytes, cosy_stream_t stream);
int cosy_gt_composite_u8(const int* composite, long long n, unsigned char* out, cosy_stream_t stream);

/* ---- object models: what the BOP toolkit's calc_model_info.py writes per model -- the diameter (misc.calc_pts_diameter: the largest
 * distance between two vertices), the axis-aligned box (misc.calc_3d_bbox) -- for a ragged batch of models ----
 * verts: the vertices of all models one after the other, (sum V, 3) row-major, float32 (elem_bytes = 4) or float64 (elem_bytes = 8), in
 * the model's own units; offsets (n + 1) int64 on the DEVICE and host_offsets, the same numbers on the HOST (they size the grid and the
 * workspace and are checked there): model m owns the vertices [offsets[m], offsets[m + 1]), 1 <= V_m < 2^31, and verts holds
 * host_offsets[n] vertices.  out (n) records, written in full for every model:
 *   s_max   the largest SQUARED distance over all vertex pairs, float64, computed as ((dx dx + dy dy) + dz dz) with dx = x_i - x_j formed
 *           in float64 (float32 input is widened first) and every operation rounded on its own: no fused multiply-add, not the form
 *           |a|^2 + |b|^2 - 2 a.b.  Bit-equal to the square of SciPy's cdist; the diameter is the caller's sqrt(s_max) on the host;
 *   i, j    i < j: of all pairs that attain s_max the lexicographically smallest, vertex numbers within the model; the same from run to
 *           run and whatever else is in the call.  V = 1: s_max = 0, i = j = 0.  A pair with a NaN distance never wins;
 *   min, max  per axis over the model's vertices, float64 (NaN coordinates are skipped); the caller forms size = max - min;
 *   n_bad   the number of non-finite coordinates (NaN, +-inf) of the model: the caller refuses the model when it is not 0.
 * Three launches (tile plan, vertex-pair tiles of 512 x 512 over the upper triangle of every model in ONE grid, per-model merge), plain
 * stores only, no atomics: every tile leaves its winner in the workspace, and a model's tiles are merged under one total order (larger s,
 * smaller i, smaller j).  workspace: 16-byte aligned, at least cosy_model_info_workspace_bytes(host_offsets, n) = 8 (n + 1) rounded up to
 * 16, plus 16 bytes per tile; that function returns 0 for n <= 0 and for offsets the call would refuse.
 * Checked on the host before any launch (COSY_EINVAL, cosy_last_error() names the argument): n >= 0, elem_bytes 4 or 8, non-null
 * pointers, host_offsets[0] >= 0 and 1 <= V_m < 2^31, verts aligned to its elements, out to 8 bytes, the workspace's size and alignment;
 * n = 0 returns COSY_OK at once with null pointers.  Checked on the device, where the offsets are read: a model whose device offsets are
 * not 0 <= offsets[m] <= offsets[m + 1] <= host_offsets[n] reads no vertex and gets s_max = 0, i = j = 0, an empty box (min = +inf,
 * max = -inf) and n_bad = -1; device offsets that give more tiles than the host's leave the surplus tiles out (no access outside the
 * workspace), so the two arrays must agree for a meaningful result. */
typedef struct cosy_model_record {
    double s_max;
    double min[3], max[3];
    int i, j;
    long long n_bad; /* 72 bytes per model */
} cosy_model_info_t;
size_t cosy_model_info_workspace_bytes(const long long* host_offsets, int n);
int cosy_model_info(const void* verts, int elem_bytes, const long long* offsets, const long long* host_offsets, int n, cosy_model_info_t* out,
                    void* workspace, size_t workspace_bytes, cosy_stream_t stream);

/* ---- detection side: instance-id masks -> counts, boxes and binary masks; box IoU (cosypose/datasets/utils.py:27-40,
 * datasets/detection_dataset.py:61-80, evaluation/meters/detection_meters.py:31-35) ----
 * masks (B,H,W) of uint8 (COSY_MASK_U8) or int32 (COSY_MASK_I32), contiguous; the base address needs the element's alignment only and
 * W may be odd.  All four functions check on the host, before any launch (COSY_EINVAL, cosy_last_error() names the argument): counts
 * >= 0, H, W > 0 with H W < 2^30, n_ids in [1, 1024], B and N of the mask functions <= 65535, every pointer that is read non-null;
 * B = 0 (N = 0) returns COSY_OK at once with null pointers.  Nothing is allocated; every output is written in full.
 *
 * cosy_mask_instance_stats: stats (B,n_ids,5) int32 = count, x1, y1, x2, y2 of the pixels that hold id i: inclusive pixel indices,
 * the np.min / np.max of np.where; an absent id gives 0, -1, -1, -1, -1.  A pixel whose value lies outside [0, n_ids) is skipped (the
 * scene renderer's -1 background).  Integer atomics only: equal inputs give equal bytes, whatever else is in the batch. */
enum { COSY_MASK_U8 = 0, COSY_MASK_I32 = 1 };
int cosy_mask_instance_stats(const void* masks, int dtype, int B, int H, int W, int n_ids, int* stats, cosy_stream_t stream);
/* out (N,H,W) uint8: out[n] = masks[row_image[n]] == row_id[n] (1 or 0); row_image, row_id (N) int32 on the device.  A row whose image
 * index lies outside [0, B) is written as zeros and reads nothing. */
int cosy_instance_masks(const void* masks, int dtype, const int* row_image, const int* row_id, int B, int H, int W, int N, unsigned char* out,
                        cosy_stream_t stream);
/* xyxy boxes, float32: a, b (N,4) -> iou (N); a (N,4), b (M,4) -> iou (N,M), N M < 2^39.  torchvision.ops.box_iou's arithmetic, every
 * operation rounded to float32 on its own: area = (x2 - x1) (y2 - y1); w = max(min(ax2, bx2) - max(ax1, bx1), 0), h likewise;
 * inter = w h; iou = inter / ((area_a + area_b) - inter).  max, min and the clamp propagate NaN as torch's do, nothing is special-cased:
 * two zero-area boxes at one point give 0 / 0 = NaN, inverted boxes follow the formula. */
int cosy_box_iou_pairs(const float* a, const float* b, int N, float* iou, cosy_stream_t stream);
int cosy_box_iou_matrix(const float* a, const float* b, int N, int M, float* iou, cosy_stream_t stream);

/* ---- Pillow 12's Image.resize of 8-bit images, bilinear and bicubic (BackgroundAugmentation.__call__, cosypose/datasets/
 * augmentations.py:120-124: im_bg.resize((w, h)) of a background of any size), uint8, byte for byte ----
 * DESIGN.md section 17 holds the arithmetic.  An axis of input length `in` and output length `out` has a table of bounds
 * (out,2) int32 = xmin, xmax (first tap and number of taps of every output index) and of coefficients (out,ksize) int32 in 2^-22,
 * computed in double on the HOST by cosy_resize_coeffs (no device, no stream): it writes both, returns ksize = cosy_resize_ksize(in,
 * out, filter), and needs capacity >= out * ksize ints in `k` and 2 * out ints in `bounds`; in, out < 1 or another filter give
 * COSY_EINVAL, a capacity too small COSY_ESIZE (both negative).
 *
 * cosy_resize_u8: n images of C planes each, image i (C,h_i,w_i) contiguous at items[i].src, all resized to out (n,C,H,W).  items and
 * tables are DEVICE memory; tables (n_tables int32) holds the bounds and coefficient tables of the axes the items name by offset (in
 * ints): hb / vb the bounds of the horizontal (w -> W) and vertical (h -> H) axis, hk / vk their coefficients, hks / vks their ksize.
 * ksize 0 means the pass is skipped, which needs w == W (h == H); with both skipped the image is copied.  The horizontal pass comes
 * first and its result is rounded to bytes, as in Pillow.  Two launches: rows (items -> workspace, or -> out where there is no vertical
 * pass), then columns (-> out); workspace is cosy_resize_workspace_bytes(n, C, max_h, W) bytes, 16-byte aligned, with max_h >= every
 * h_i.  Integer arithmetic only; equal inputs give equal bytes.  out needs no alignment.
 * Checked on the host before any launch (COSY_EINVAL, cosy_last_error() names the argument): 0 <= n <= 65535, C, H, W, max_h >= 1,
 * max_h <= 262140, C max_h W and C H W < 2^31, non-null pointers, the workspace size; n = 0 returns COSY_OK at once.  The items live on the
 * device and are checked there: an item with a null src, h or w < 1, h > max_h, a table outside [0, n_tables), or a skipped pass
 * whose lengths differ leaves its image of `out` UNTOUCHED and reads nothing; a bounds entry that would read outside its line (xmin <
 * 0, xmax outside [0, ksize], xmin + xmax > in) leaves that output byte untouched.  Callers build the tables with cosy_resize_coeffs. */
enum { COSY_RESIZE_BILINEAR = 2, COSY_RESIZE_BICUBIC = 3 };   /* Pillow's Image.BILINEAR, Image.BICUBIC */
typedef struct cosy_resize_item {
    const unsigned char* src;
    int h, w;
    int hb, hk, hks;
    int vb, vk, vks; /* 40 bytes per item */
} cosy_resize_item_t;
int cosy_resize_ksize(int in, int out, int filter);
int cosy_resize_coeffs(int in, int out, int filter, int* bounds, int* k, size_t capacity);
size_t cosy_resize_workspace_bytes(int n, int C, int max_h, int W);
int cosy_resize_u8(const cosy_resize_item_t* items, int n, int C, int H, int W, int max_h, const int* tables, long n_tables,
                   unsigned char* out, void* workspace, size_t workspace_bytes, cosy_stream_t stream);

/* ---- The frames' own resize (CropResizeToAspectAugmentation.__call__, cosypose/datasets/augmentations.py:137-192, for a frame of the
 * target aspect): image through float32 bilinear interpolation with half-pixel centres and a truncating cast, mask through nearest ----
 * DESIGN.md section 18 holds the arithmetic.  Everything that divides is computed by the CALLER in float32 and handed over in `tables`
 * (n_tables int32 of DEVICE memory, 16-byte aligned): for an axis n_in -> n_out a tap table (n_out,4) = i0, i1, bits of l0, bits of l1
 * (offset a multiple of 4 ints) and a nearest table (n_out) = source index; and at offset `lut` the bits of the 256 floats
 * float32(u) / 255f.
 *
 * cosy_resize_frames_u8: n frames, frame i an image (3,h_i,w_i) uint8 contiguous at items[i].image and, where items[i].mask is not
 * null, a mask (h_i,w_i) uint8; images go to out_images (n,3,H,W), masks to out_masks (n,H,W) (may be null when no item has a mask).
 * xb / yb: offsets (in ints) of the tap tables of the horizontal (w -> W) and vertical (h -> H) axis, xn / yn of the nearest tables
 * (read only for a mask).  A frame with h == H and w == W is copied and its offsets are not read.  ONE launch, no workspace; per byte
 *   top = fma(lx0, p00, lx1 * p01), bot = fma(lx0, p10, lx1 * p11), v = fma(ly0, top, ly1 * bot), byte = (uint8) trunc(v * 255f)
 * with every product rounded once.  Equal inputs give equal bytes.  The outputs need no alignment.
 * Checked on the host before the launch (COSY_EINVAL, cosy_last_error() names the argument): 0 <= n <= 16383, H, W >= 1, H <= 524280,
 * 3 H W < 2^31, lut + 256 <= n_tables, non-null items / tables / out_images and their alignment; n = 0 returns COSY_OK at once.  The
 * items live on the device and are checked there: an item with a null image (mask), h or w < 1, or a table outside [0, n_tables) or
 * misaligned leaves its frame of out_images (out_masks) UNTOUCHED and reads nothing; a tap or nearest index outside its line is
 * clamped into it. */
typedef struct cosy_frame_item {
    const unsigned char* image;
    const unsigned char* mask;
    int h, w;
    int xb, yb;
    int xn, yn; /* 40 bytes per item */
} cosy_frame_item_t;
int cosy_resize_frames_u8(const cosy_frame_item_t* items, int n, int H, int W, const int* tables, long n_tables, int lut,
                          unsigned char* out_images, unsigned char* out_masks, cosy_stream_t stream);

/* ---- Output side of the detector: the Mask R-CNN heads' raw outputs -> detections (torchvision 0.4.2's roi_heads.postprocess_detections,
 * ops.batched_nms, GeneralizedRCNNTransform.postprocess, maskrcnn_inference + paste_masks_in_image; cosypose/integrated/detector.py:28-50) ----
 * DESIGN.md section 21 holds the arithmetic: float32, one rounding per operation.  Every pointer is DEVICE memory.  All functions check on
 * the host before any launch (COSY_EINVAL, cosy_last_error() names the argument); nothing is allocated.
 *
 * Candidates live in a per-image arena of `cap` slots (a multiple of 64 in [64, cosy_nms_max_candidates() = 16384]): slot s of image b is
 * row b cap + s of cand_boxes (B cap,4), cand_scores, cand_labels (1 .. C-1), cand_src (proposal-in-image (C-1) + label - 1) and cand_keys.
 *
 * cosy_det_decode: class_logits (R,C), box_regression (R,4C), proposals (R,4) xyxy of all B images, image b owning rows
 * [prop_offsets[b], prop_offsets[b+1]) (B+1 int32; a row no image owns is skipped); net_sizes (B,2) float32 = height, width the network
 * saw.  Softmax, BoxCoder.decode with weights (10,10,5,5) and the log(1000/16) clamp, clip to the image, score > score_thresh, both sides
 * >= 1e-2.  Survivors take slots in NO particular order; cand_keys (int64) = b << 52 | (0x7fffffff - score bits) << 21 | cand_src, and an
 * unused slot holds b << 52 | 2^52 - 1: sorting ALL B cap keys ascending lists every image's candidates by descending score, equal scores
 * by ascending cand_src, and its unused slots after them.  counts (B) = survivors of every image, which MAY EXCEED cap: the ones beyond
 * it were dropped and the caller must refuse the result.  max_coord (B) = the largest coordinate among an image's candidates (0 without
 * any).  Limits: 2 <= C <= 4096, B <= 2047, R (C-1) <= 2^21, score_thresh >= 0.  Two launches (initialisation, decode). */
int cosy_nms_max_candidates(void);
int cosy_det_decode(const float* class_logits, const float* box_regression, const float* proposals, const int* prop_offsets,
                    const float* net_sizes, int R, int C, int B, float score_thresh, int cap, float* cand_boxes, float* cand_scores,
                    int* cand_labels, int* cand_src, long long* cand_keys, int* counts, float* max_coord, cosy_stream_t stream);
/* Greedy NMS of B segments in one launch each.  Segment b is the rows [seg_start[b], seg_start[b] + min(seg_count[b], cap)) of `order`
 * (N int64: row -> index into boxes (N,4), labels (N); null = identity), ALREADY sorted by descending score; a segment that does not fit
 * into [0, N) is treated as empty, an index outside [0, N) as a box that suppresses nothing.  With labels (int32), a box is shifted by
 * float(label) * (max_coord[b] + 1) before the IoU (batched_nms); without, max_coord may be null.
 * cosy_nms_mask: mask (B, cap, cap/64) uint64, bit j of word (b, i, c) = "IoU(row i, row 64 c + j) > iou_thresh and 64 c + j > i", written
 * for the 64 x 64 tiles with c >= i / 64 that hold rows of the segment; the IoU is cosy_box_iou_matrix's, bit for bit.
 * cosy_nms_scan: walks the rows in order; a row nothing kept before it suppresses is kept, until max_keep are.  kept (B, max_keep) int32
 * = the kept rows' indices (order[row], or the row) in visiting order, -1 beyond n_kept (B); keep_flags (N uint8, may be null) is zeroed
 * and set at every kept index. */
int cosy_nms_mask(const float* boxes, const long long* order, const int* labels, const float* max_coord, const int* seg_start,
                  const int* seg_count, int B, int N, int cap, float iou_thresh, unsigned long long* mask, cosy_stream_t stream);
int cosy_nms_scan(const unsigned long long* mask, const long long* order, const int* seg_start, const int* seg_count, int B, int N, int cap,
                  int max_keep, int* kept, int* n_kept, unsigned char* keep_flags, cosy_stream_t stream);
/* The kept candidates of an arena (kept, n_kept of cosy_nms_scan with order = the sorted keys' permutation) as B max_keep padded rows:
 * boxes_net (B max_keep,4) as decoded, boxes_frame = x * ratios[b][0], y * ratios[b][1] (ratios (B,2) float32 = width ratio, height
 * ratio), src = cand_src; a row past n_kept[b] holds zeros and src -1.  packed (2 B + 2 B max_keep int32) is what the host needs in one
 * copy: counts (B), n_kept (B), labels (B max_keep, -1 on a padding row), bits of the scores (B max_keep). */
int cosy_det_gather(const int* kept, const int* n_kept, const int* counts, const float* cand_boxes, const float* cand_scores,
                    const int* cand_labels, const int* cand_src, const float* ratios, int B, int cap, int max_keep, float* boxes_net,
                    float* boxes_frame, int* src, int* packed, cosy_stream_t stream);
/* mask_logits (D,C,M,M), boxes (D,4) xyxy in the frame, labels (D) int32 = channel -> out (D,H,W) uint8 (0 / 1), EVERY byte written:
 * sigmoid of the label's channel, zero padding of 1, box expanded by (M+2)/M and truncated toward zero, torch's bilinear upsample
 * (align_corners = False) to the box's integer size; a pixel the box does not reach, and every pixel of a label outside [0, C), holds the
 * value 0; out = value > mask_th for all of them (so 0 outside the box unless mask_th is negative; a NaN mask_th gives 0 everywhere).
 * 1 <= M <= 62, D <= 65535, H W < 2^30.  One launch. */
int cosy_paste_masks(const float* mask_logits, const float* boxes, const int* labels, int D, int C, int M, int H, int W, float mask_th,
                     unsigned char* out, cosy_stream_t stream);

/* ---- Proposal side of the detector: the RPN head's raw outputs -> proposals, and FPN features + boxes -> RoI features (torchvision 0.4.2's
 * AnchorGenerator, RegionProposalNetwork.filter_proposals, MultiScaleRoIAlign with Mask R-CNN's defaults) ----
 * DESIGN.md section 22 holds the arithmetic: float32, one rounding per operation.  The level tables are HOST structs, passed to the kernels by
 * value; every pointer inside them and every other pointer is DEVICE memory.  All functions check on the host before any launch (COSY_EINVAL,
 * cosy_last_error() names the argument); nothing is allocated.
 *
 * cosy_rpn_levels_t: level l has H[l] x W[l] cells of A anchors; objectness[l] (B,A,H,W) and deltas[l] (B,4A,H,W) are the head's NCHW float32
 * outputs, read in place; anchor i of a level = (y W + x) A + a has the box base[l][a] + (x stride_w[l], y stride_h[l]) on both corners; an
 * image's candidate index is i plus the anchors of the levels before l.  Limits: L <= 8, A <= 16, B <= 2047, at most 2^20 anchors per image,
 * pre_nms_top_n L <= cosy_nms_max_candidates().
 *
 * cosy_rpn_select: per image and level the k = min(pre_nms_top_n, present anchors) largest objectness LOGITS (no sigmoid; -0 counts as +0);
 * an anchor whose logit or any of its four deltas is NaN is absent.  sel_idx (B,L,pre_nms_top_n) int32 takes the anchors strictly above the
 * k-th value in ascending index order, then the lowest-index anchors AT it; sel_count (B,L) = k; rows past k are not written.  One launch.
 * cosy_rpn_decode: one slot of the arena (B cap; cap a multiple of 64 with pre_nms_top_n L <= cap <= cosy_nms_max_candidates()) per selected
 * anchor, slot = l pre_nms_top_n + rank: BoxCoder.decode with weights 1 and the log(1000/16) clamp, x clipped to [0, net_sizes[b][1]], y to
 * [0, net_sizes[b][0]] (net_sizes (B,2) float32 = height, width of the image itself), kept when both sides >= min_size.  A kept slot holds
 * cand_boxes, cand_scores (the logit), cand_level, cand_src (candidate index) and cand_keys (int64) = b << 52 | (0xffffffff - ordered score)
 * << 20 | cand_src; every other slot holds the key b << 52 | 2^52 - 1 only: sorting ALL B cap keys ascending lists every image's candidates by
 * descending score, equal scores by ascending candidate index.  counts (B) = kept slots, max_coord (B) = their largest coordinate (0 without
 * any): what cosy_nms_mask / cosy_nms_scan take as seg_count and max_coord with labels = cand_level.  Two memsets and one launch.
 * cosy_rpn_gather: kept / n_kept of cosy_nms_scan -> proposals (B max_keep,4), scores, levels, src (candidate index), padded with zeros
 * (level and src -1) past counts[b] = n_kept[b]. */
#define COSY_RPN_MAX_LEVELS 8
#define COSY_RPN_MAX_ANCHORS 16
typedef struct cosy_rpn_levels {
    const float* objectness[COSY_RPN_MAX_LEVELS];
    const float* deltas[COSY_RPN_MAX_LEVELS];
    int H[COSY_RPN_MAX_LEVELS], W[COSY_RPN_MAX_LEVELS];
    float stride_h[COSY_RPN_MAX_LEVELS], stride_w[COSY_RPN_MAX_LEVELS];
    float base[COSY_RPN_MAX_LEVELS][COSY_RPN_MAX_ANCHORS][4]; /* x1, y1, x2, y2 */
} cosy_rpn_levels_t;
int cosy_rpn_select(const cosy_rpn_levels_t* levels, int L, int A, int B, int pre_nms_top_n, int* sel_idx, int* sel_count, cosy_stream_t stream);
int cosy_rpn_decode(const cosy_rpn_levels_t* levels, int L, int A, int B, int pre_nms_top_n, const int* sel_idx, const int* sel_count,
                    const float* net_sizes, float min_size, int cap, float* cand_boxes, float* cand_scores, int* cand_level, int* cand_src,
                    long long* cand_keys, int* counts, float* max_coord, cosy_stream_t stream);
int cosy_rpn_gather(const int* kept, const int* n_kept, const float* cand_boxes, const float* cand_scores, const int* cand_level,
                    const int* cand_src, int B, int cap, int max_keep, float* proposals, float* scores, int* levels, int* src, int* counts,
                    cosy_stream_t stream);
/* MultiScaleRoIAlign in one launch: boxes (R,4) xyxy at the network's scale; row r belongs to image im_id[r] (R int32), or, with im_id null, to
 * image r / rows_per_image, and then counts (B int32, may be null) makes the rows r % rows_per_image >= counts[image] padding.  Level of a box
 * = clamp(floor(4 + log2(sqrt(area) / 224 + 1e-6)), k_min, k_max) - k_min (NaN: 0), which must index the L levels (k_max - k_min < L);
 * feat[l] is (B,C,H[l],W[l]) float32.  roi_align as torchvision 0.4.2 (no `aligned`): start x1 scale, size max(x2 scale - x1 scale, 1), P x P
 * bins of sampling_ratio^2 samples, a sample outside [-1, size] (or NaN) adds 0.  out (R,C,P,P) is written in full: a padding row, or one
 * whose image is outside [0, B), holds zeros and level -1.  levels_out (R int32) may be null.  P sampling_ratio <= 128, sampling_ratio >= 1. */
typedef struct cosy_msroi_levels {
    const float* feat[COSY_RPN_MAX_LEVELS];
    int H[COSY_RPN_MAX_LEVELS], W[COSY_RPN_MAX_LEVELS];
    float scale[COSY_RPN_MAX_LEVELS];
} cosy_msroi_levels_t;
int cosy_msroi_align(const cosy_msroi_levels_t* levels, int L, int B, int C, const float* boxes, const int* im_id, const int* counts,
                     int rows_per_image, int R, int P, int sampling_ratio, int k_min, int k_max, float* out, int* levels_out,
                     cosy_stream_t stream);
/* The adjoint of cosy_msroi_align with respect to the feature maps: grad_out (R,C,P,P) float32 -> grad_feat[l] (B,C,H[l],W[l]) float32 for
 * every level l < L whose pointer in the HOST array grad_feat is not null (a null level is skipped; levels->feat is not read).  boxes, im_id,
 * counts, rows_per_image, P, sampling_ratio, k_min, k_max as in the forward call: the same level, the same taps and weights, the same 1/g^2;
 * a row the forward writes as zeros adds nothing.  A gather: every cell of every requested level is written exactly once with a plain store
 * (+0 where nothing arrives: no memset needed), no floating-point atomic, equal bits on every call.  Per cell the terms fl(fl(wy wx) g) are
 * added in float32 by ascending row; inside a row by ascending y tap (of one tap the low cell's weight first), inside that by ascending x tap
 * (low first); the sum is divided by g^2 once.  row_ws: 8 R int32 of scratch.  Two launches.  Limits: the forward's,
 * R <= 2^30, C <= 32 x 65535, and B x (the 16 x 16 tiles of the requested levels) < 2^31. */
int cosy_msroi_align_backward(const cosy_msroi_levels_t* levels, float* const* grad_feat, int L, int B, int C, const float* grad_out,
                              const float* boxes, const int* im_id, const int* counts, int rows_per_image, int R, int P, int sampling_ratio,
                              int k_min, int k_max, int* row_ws, cosy_stream_t stream);

/* ---- Training side of the detector: the heads' raw outputs + targets -> Mask R-CNN's five losses and their gradients (torchvision 0.4.2's
 * Matcher, BalancedPositiveNegativeSampler, BoxCoder.encode, RPN compute_loss, select_training_samples, fastrcnn_loss, maskrcnn_loss) ----
 * DESIGN.md section 23 holds the arithmetic: float32, one rounding per operation; loss sums in float64 in a fixed order, rounded once.  Every
 * pointer is DEVICE memory except the level tables (host structs passed by value).  All functions check on the host before any launch
 * (COSY_EINVAL, cosy_last_error() names the argument); nothing is allocated; integer atomics only.
 * Ground truths of all images are concatenated: gt_boxes (G_total,4) xyxy, gt_off (B+1) int32 offsets, at most COSY_DT_MAX_GT per image.
 *
 * cosy_dt_match: Matcher(high, low, allow_low_quality) over box_iou(gt, candidates) for N candidates per image: anchors formed from their
 * index (cand_boxes null; levels as for cosy_rpn_select, the head pointers unused; N = the levels' anchors) or rows of cand_boxes (B N,4), of
 * which only the first cand_counts[b] (null: all) are candidates.  A NaN or negative IoU counts as 0; equal IoUs go to the lowest ground truth.
 * matched (B,N) int32: the ground truth's index, -1 below low, -2 between, -3 on a padding row; matched_iou (B,N); labels (B,N, may be null):
 * gt_labels[matched] (1 without gt_labels) / 0 for -1 / -1 otherwise.  best_ws: G_total uint32 of scratch for allow_low_quality.
 * cosy_dt_sample: BalancedPositiveNegativeSampler over labels (B,N) with int32 keys (B,N) read as unsigned: the min(max_positives, P) positives
 * (label >= 1) and the min(batch_size_per_image - that, N) negatives (label 0) with the smallest keys, equal keys lower index first.  samp_idx
 * (B, batch_size_per_image): all sampled indices ascending, samp_count (B); pos_idx (B, max_positives) / pos_count (B): the positives.  Rows past
 * the counts are not written.  One launch, one workgroup per image.
 * cosy_dt_encode: BoxCoder.encode_single(reference_boxes, boxes) with the four weights, n rows.
 * cosy_dt_rpn_loss: levels hold the head's outputs, grads (same layout) the gradient tensors, which the caller has ZEROED: the sampled anchors'
 * entries are written.  losses[0] = mean BCE-with-logits over the sampled anchors, losses[1] = sum |d - t| over the sampled positives / the
 * sampled.  terms_ws: 2 B batch_size_per_image doubles.
 * cosy_dt_roi_candidates: cand_boxes (B (rows_per_image + G_max), 4) = the first counts[b] proposals of image b, its ground truths, zeros;
 * cand_counts (B).
 * cosy_dt_roi_gather: the sampled rows of cosy_dt_sample over N candidates per image -> boxes, labels (-1: padding), the CLAMPED matched index
 * and the regression targets (B batch_size_per_image rows), and the positives' boxes, labels, matched index (B max_positives rows).
 * cosy_dt_fastrcnn_loss: rows with a label outside [0, C) are padding.  losses[0] = mean cross-entropy over the N real rows, losses[1] = sum of
 * smooth-L1(beta 1) over the rows with label > 0 / N; grad_logits (R,C) and grad_box (R,4C) are written in full.  n_real_ws: 1 int, terms_ws:
 * 2 R doubles.
 * cosy_dt_mask_loss: one positive RoI per row, B rows_per_image rows, of which image b's first pos_count[b] (null: all) are real.  mask_ptr (B)
 * int64 addresses of the images' uint8 masks (G,H,W), mask_dims (B,3) int32 = G, H, W with H W < 2^30 (a row whose image says otherwise, or whose
 * matched index lies outside [0, G), is written as zeros).  Targets: roi_align with the adaptive grid g =
 * min(ceil(max(extent, 1) / M), COSY_DT_MAX_GRID) per axis.  With mask_logits (R,C,M,M): loss = mean BCE-with-logits(mask_logits[r, labels[r]],
 * target) over the real rows, grad (R,C,M,M) written in full, partial_ws R doubles.  targets_out (R,M,M) may be null. */
#define COSY_DT_MAX_GT 1024
#define COSY_DT_MAX_BATCH 4096
#define COSY_DT_MAX_CLASSES 4096
#define COSY_DT_MAX_M 128
#define COSY_DT_MAX_GRID 4096
int cosy_dt_match(const cosy_rpn_levels_t* levels, int L, int A, const float* cand_boxes, const int* cand_counts, int N, int B, const float* gt_boxes,
                  const int* gt_off, const int* gt_labels, int G_max, int G_total, float high, float low, int allow_low_quality, unsigned* best_ws,
                  int* matched, float* matched_iou, int* labels, cosy_stream_t stream);
int cosy_dt_sample(const int* labels, const int* keys, int N, int B, int batch_size_per_image, int max_positives, int* samp_idx, int* samp_count,
                   int* pos_idx, int* pos_count, cosy_stream_t stream);
int cosy_dt_encode(const float* reference_boxes, const float* boxes, long n, float wx, float wy, float ww, float wh, float* out, cosy_stream_t stream);
int cosy_dt_rpn_loss(const cosy_rpn_levels_t* levels, const cosy_rpn_levels_t* grads, int L, int A, int B, int batch_size_per_image, const int* samp_idx,
                     const int* samp_count, const int* matched, const float* gt_boxes, const int* gt_off, double* terms_ws, float* losses,
                     cosy_stream_t stream);
int cosy_dt_roi_candidates(const float* proposals, const int* counts, int rows_per_image, const float* gt_boxes, const int* gt_off, int B, int G_max,
                           float* cand_boxes, int* cand_counts, cosy_stream_t stream);
int cosy_dt_roi_gather(const float* cand_boxes, int N, const int* matched, const int* labels, const int* samp_idx, const int* samp_count,
                       const int* pos_idx, const int* pos_count, const float* gt_boxes, const int* gt_off, int B, int batch_size_per_image,
                       int max_positives, float wx, float wy, float ww, float wh, float* boxes, int* out_labels, int* out_matched, float* targets,
                       float* pos_boxes, int* pos_labels, int* pos_matched, cosy_stream_t stream);
int cosy_dt_fastrcnn_loss(const float* class_logits, const float* box_regression, const int* labels, const float* regression_targets, int R, int C,
                          int* n_real_ws, double* terms_ws, float* grad_logits, float* grad_box, float* losses, cosy_stream_t stream);
int cosy_dt_mask_loss(const long long* mask_ptr, const int* mask_dims, int B, const float* boxes, const int* labels, const int* matched,
                      const int* pos_count, int rows_per_image, const float* mask_logits, int C, int M, double* partial_ws, float* grad, float* targets_out,
                      float* loss, cosy_stream_t stream);

/* ---- Input side of the detector: torchvision 0.4.2's GeneralizedRCNNTransform (normalise, resize, pad into one batch; boxes and masks
 * of the targets to the network's size) for uint8 frames ----
 * DESIGN.md section 25 holds the arithmetic: float32, one rounding per operation.  Everything that divides is computed by the CALLER and
 * handed over in `tables` (n_tables int32 of DEVICE memory, 16-byte aligned): at offset `lut` the bits of the 3 x 256 floats
 * p_c(u) = ((float32(u) / 255f) - mean_c) / std_c, channel-major; for an axis n_in -> n_out a tap table (n_out,4) = i0, i1, bits of l0,
 * bits of l1 (offset a multiple of 4 ints) and a nearest table (n_out) = source index, as cosy_resize_frames_u8 reads them; and at offset
 * `units` n_units pairs (item, mask plane), one per mask plane of the call.
 *
 * cosy_detector_input: n frames of any sizes in ONE launch.  Frame i is read in place: byte (c, y, x) lies at frame + c sc + y sy + x sx
 * (strides in bytes, >= 0; CHW, HWC and views of them alike).  out_images (n,3,Hp,Wp) float32: EVERY element is written exactly once;
 * inside (nh_i, nw_i) of image i
 *   top = fma(lx0, p00, lx1 * p01), bot = fma(lx0, p10, lx1 * p11), v = fma(ly0, top, ly1 * bot)      (xb / yb: the tap tables)
 * with every product rounded once, and outside it +0.0.  An item with COSY_DETIN_ONE_TAP set and nh == h, nw == w stores p00 and its tap
 * offsets are not read: the same bits where no table entry is -0.0, infinite or NaN, which is the caller's to know.  Where n_masks > 0,
 * masks (n_masks,h,w) uint8 contiguous go through nearest (xn / yn: the nearest tables) to masks_out (n_masks,nh,nw) uint8 contiguous, not
 * padded.  Where n_boxes > 0, boxes (n_boxes,4) float32 xyxy go to boxes_out as x * rw, y * rh, one product each.  Equal inputs give
 * equal bits.  out_images must be 4-byte aligned; rows that are 16-byte aligned are stored as 16-byte vectors.
 * Checked on the host before the launch (COSY_EINVAL, cosy_last_error() names the argument): 0 <= n, n_units >= 0, n + n_units <= 65535,
 * 1 <= Hp <= 524280, Wp >= 1, 3 Hp Wp < 2^31, lut + 768 <= n_tables, units + 2 n_units <= n_tables, non-null items_host / items / tables /
 * out_images and their alignment, and EVERY item of items_host -- the caller's host copy of the descriptors: a null frame, a size < 1,
 * nh > Hp or nw > Wp, a negative stride or count, a table offset outside [0, n_tables) or misaligned, or a null pointer beside a count > 0
 * refuses the whole call and nothing is written.  n = 0 returns COSY_OK at once.  The kernel reads the DEVICE copy `items` and applies
 * the same test again: an item that fails it there leaves its outputs UNTOUCHED and nothing is read through it; a unit whose item or plane
 * does not exist is skipped; a tap or nearest index outside its line is clamped into it.
 * Why two copies: the descriptors must be in device memory for the kernel, and the caller has just written them on the host to upload
 * them, so handing over that host copy lets a bad item refuse the call BEFORE anything is written, without a device-to-host copy or a
 * synchronisation.  Nothing is trusted because of it: the host test decides only the return value, and the kernel's own test of the bytes
 * it actually reads is what keeps an item that differs between the copies from reading or writing outside its buffers. */
enum { COSY_DETIN_ONE_TAP = 1 };
typedef struct cosy_detin_item {
    const unsigned char* frame;
    long long sc, sy, sx;           /* byte strides of channel, row, pixel */
    const unsigned char* masks;
    unsigned char* masks_out;
    const float* boxes;
    float* boxes_out;
    int h, w, nh, nw;
    int xb, yb, xn, yn;
    int n_masks, n_boxes;
    float rw, rh;
    int flags, reserved[3];         /* 128 bytes per item */
} cosy_detin_item_t;
int cosy_detector_input(const cosy_detin_item_t* items_host, const cosy_detin_item_t* items, int n, int Hp, int Wp, const int* tables,
                        long n_tables, int lut, int units, int n_units, float* out_images, cosy_stream_t stream);

/* ---- The detector's heads on the matrix pipe: every layer of Mask R-CNN's RPN head, box head + predictor and mask head + predictor as one
 * implicit GEMM (inference only) ----  DESIGN.md section 26 holds the contract and the summation order.
 * Activations are ROWS of the storage type `dtype`: M rows of c_in contiguous channels (NHWC; a linear layer's row is its input vector).
 * The rows of a call belong to n_levels groups of whole maps: level l owns rows [row_start[l], row_start[l+1]), which are B_l maps of
 * H[l] x W[l] cells, image-major, then y, then x; M = row_start[n_levels].  A 3x3 tap outside its map contributes nothing.
 * cosy_head_pack: contiguous NCHW float32 (B,C,HW) -> rows (B HW, C) of `dtype` (round to nearest even).  C a positive multiple of 8.
 * cosy_head_conv: out = act(W x + bias) of all M rows in one launch, accumulated in float32.
 *   ksize 3: 3x3 conv, pad 1, stride 1; ksize 1: 1x1 conv, or a linear layer with H = W = 1.  c_in is the channels of a row (a multiple of 8,
 *   anything else is refused), c_out the GEMM's columns.
 *   w: the weight (c_out, taps, c_in) in fragment order, NP = c_out rounded up to 64, KB = 16 (float32) or 32 (16-bit), KBn = ceil(c_in / KB):
 *     element [nt][tap][kb][lane][e], nt < NP / 16, lane < 64, e < KB / 4, holds w[16 nt + (lane & 15)][tap][KB kb + k] with
 *     k = (KB / 4) (lane >> 4) + e; zero where the row or the channel does not exist.
 *   bias: NP floats (zero past c_out).  relu: 1 = x < 0 ? 0 : x after the bias (a NaN stays NaN).
 *   store COSY_HEAD_STORE_ROWS: out = rows (M, c_out) of `dtype`, c_out a multiple of 8.
 *   store COSY_HEAD_STORE_NCHW: float32 NCHW.  Columns [0, n_split) go to `out`, the rest to `out1`; level l's maps start at element
 *     n_split row_start[l] of out as (B_l, n_split, H, W) and at (c_out - n_split) row_start[l] of out1 (two sibling layers as one GEMM).
 *     n_split = c_out: everything to out, out1 unused.
 *   store COSY_HEAD_STORE_DECONV_ROWS / _DECONV_NCHW: the layer is ConvTranspose2d(k=2, s=2): c_out = 4 C_o columns (o, dy, dx), bias
 *     repeated per column; column (o, dy, dx) of cell (y, x) is stored at (o, 2y+dy, 2x+dx) of a (2H, 2W) map, as rows of `dtype`
 *     (level l from row 4 row_start[l]; C_o a multiple of 8) or as float32 NCHW (level l from element 4 row_start[l] C_o).
 * Summation order of one output: accumulator +0.0; k-blocks of KB channels ascending; inside a block the taps (ky, kx) ascending; inside a
 *   tap, float32: the block's channels in the order 4 g + t, t = 0..3 outside, g = 0..3 inside (0, 4, 8, 12, 1, 5, ...), one fmaf each;
 *   16-bit: one MFMA over the block's 32 exact products.  Then one rounded bias add, ReLU, the conversion to the store's type.
 * Checked on the host before the launch (COSY_EINVAL, cosy_last_error() names the argument); M = 0 returns COSY_OK and launches nothing;
 * M <= 2^30, offsets are 64-bit.  x, w, out 16-byte aligned.  No atomics: equal inputs give equal bits.
 * cosy_head_big_rows(): M from which the launcher picks its large row tile; cosy_head_max_tile_rows(): rows of that tile. */
enum { COSY_HEAD_STORE_ROWS = 0, COSY_HEAD_STORE_NCHW = 1, COSY_HEAD_STORE_DECONV_ROWS = 2, COSY_HEAD_STORE_DECONV_NCHW = 3 };
typedef struct cosy_head_layer {
    const void* x;
    const void* w;
    const float* bias;
    void* out;
    void* out1;
    int dtype, ksize, c_in, c_out, relu, store, n_split, n_levels;
    int row_start[COSY_RPN_MAX_LEVELS + 1];
    int H[COSY_RPN_MAX_LEVELS], W[COSY_RPN_MAX_LEVELS];
} cosy_head_layer_t;
int cosy_head_big_rows(void);
int cosy_head_max_tile_rows(void);
int cosy_head_pack(const float* in, void* rows, int B, int C, int HW, int dtype, cosy_stream_t stream);
int cosy_head_conv(const cosy_head_layer_t* layer, cosy_stream_t stream);

/* ---- the detector's trunk on the matrix pipe: the ResNet body and the FPN as the heads' implicit GEMM (inference only) ----  DESIGN.md
 * section 27 holds the contract.  Rows, weights (fragment order), summation order, tiles and stores are those of cosy_head_conv.
 * cosy_trunk_conv: layer->H / W / row_start describe the INPUT maps; the output maps are Ho = (H - 1) / stride + 1, Wo likewise, and the launch
 *   owns the B Ho Wo output cells.  ksize 1 or 3 (pad ksize / 2), stride 1 or 2 (2: one level).  Output cell (y, x) reads the input cells
 *   (stride y + dy, stride x + dx); a tap outside the map feeds +0.0 and its address is never formed.
 *   Epilogue per output, in this order: v = fmaf(acc, scale[c], bias[c]) (scale NULL: acc + bias[c]; scale is padded like bias);
 *   residual != NULL: v = v + r, one rounded add; relu: x < 0 ? 0 : x (a NaN stays NaN); the conversion to the store's type.
 *   residual: rows of c_out channels of `dtype` on maps of res_H x res_W per image (one level, c_out a multiple of 8); output cell (y, x) takes
 *   the cell (min(floor(y sy), res_H - 1), min(floor(x sx), res_W - 1)) with sy = (float)res_H / Ho and the product in float32: torch's legacy
 *   mode='nearest' (res_H == Ho: the identity).
 *   store: COSY_HEAD_STORE_ROWS, or COSY_HEAD_STORE_NCHW with n_split == c_out; anything else is refused (COSY_EINVAL), as is what
 *   cosy_head_conv refuses.  M = 0 returns COSY_OK and launches nothing.  No atomics: equal inputs give equal bits.
 * cosy_trunk_stem_pack: images (B,3,H,W) contiguous float32 -> rows (B Ho Wo, 152) of `dtype` for the 7x7 stride-2 pad-3 stem: element
 *   (ky 7 + kx) 3 + c of output cell (y, x) is images[b, c, 2y - 3 + ky, 2x - 3 + kx], +0.0 outside the image; elements 147..151 are +0.0.
 * cosy_trunk_maxpool: rows (B H W, C) -> rows (B Ho Wo, C): max_pool2d(3, 2, 1), padding -inf, v > m || isnan(v) takes v.  C a multiple of 8. */
int cosy_trunk_conv(const cosy_head_layer_t* layer, int stride, const float* scale, const void* residual, int res_H, int res_W, cosy_stream_t stream);
int cosy_trunk_stem_pack(const float* images, void* rows, int B, int H, int W, int dtype, cosy_stream_t stream);
int cosy_trunk_maxpool(const void* x, void* out, int B, int H, int W, int C, int dtype, cosy_stream_t stream);

/* ---- the backward of the detector's heads on the matrix pipe, float32 only ----  DESIGN.md section 28 holds the contract.
 * A head layer is y = act(W x + b) as cosy_head_conv runs it; g is the gradient at its PRE-activation output, as float32 rows
 * (M, GP), GP = c_out rounded up to a multiple of 8, the pad columns +0.0.  ksize 1 / 3 as in cosy_head_conv; ksize 2 is
 * ConvTranspose2d(k=2, s=2): x rows (B H W, C), g rows (B 2H 2W, C_o) over the (2H, 2W) map, C_o a multiple of 8.
 * cosy_head_grad_pack: contiguous NCHW float32 (B, n0, HW) and (B, n1, HW) -> rows (B HW, GP), GP = (n0 + n1) rounded up to 8: the columns
 *   of g0, then those of g1, then +0.0.  A NULL g0 or g1 is a tensor of zeros.  B = 0 launches nothing.
 * cosy_head_dgrad: the data gradient dX[cell][c] = sum over (tap, o) of w[o][tap][c] g[cell - tap][o] as cosy_head_conv's GEMM, in its
 *   summation order, with no bias add.  layer->x = the rows g, c_in = GP (the reduction length, a multiple of 8), c_out = the layer's input
 *   channels (a multiple of 8), dtype COSY_F32, relu 0, bias unused, w = the transposed packing of cosy_head_weight_pack.
 *   ksize 2: H / W / row_start describe the maps of g, (2H, 2W), one level, as cosy_trunk_conv's stride 2 does; the launch owns the B H W cells;
 *   output cell (y, x) reads g at (2y + dy, 2x + dx), taps (dy, dx) ascending.
 *   store COSY_HEAD_STORE_ROWS: out = rows (M, c_out) float32; y != NULL: the rows the layer BELOW stored in forward, same shape: out = y <= 0 ?
 *   +0.0 : dX (torch's threshold_backward: a NaN y passes dX), i.e. the pre-activation gradient of that layer.
 *   store COSY_HEAD_STORE_NCHW: float32 NCHW as cosy_head_conv's, n_split == c_out, y NULL.
 * cosy_head_wgrad: dW[o][tap][c] = sum over cells of g[cell][o] x[cell + tap][c] (x = +0.0 outside its map, no address formed),
 *   db[o] = sum over cells of g[cell][o], on v_mfma_f32_16x16x4_f32 with the cells as the k dimension.  layer->x = the rows the layer read in
 *   forward, c_in, c_out (ksize 2: C_o), n_split, n_levels / row_start / H / W = the maps of x, dtype COSY_F32; w, bias, out, out1 unused.
 *   The M cells are cut into slabs of cosy_head_wgrad_slab_rows(M) cells (a function of M alone); every slab writes a partial tile to the
 *   workspace and a second pass adds the slabs in ascending order.  No atomics: equal inputs give equal bits.
 *   Results, float32, in torchvision's layout: ksize 1 / 3: (O, C, k, k) (a linear layer: (N, K)), outputs [0, n_split) to dw0 / db0 and the
 *   rest to dw1 / db1 (two sibling layers as one GEMM; n_split = c_out: dw1, db1 unused); ksize 2: dw0 (C, C_o, 2, 2), db0 (C_o).
 *   workspace: cosy_head_wgrad_workspace_bytes(M, ksize, c_in, c_out) bytes (0 for a shape the call refuses), allocated by the caller;
 *   a smaller workspace_bytes is refused, nothing is truncated.  M = 0 writes zeros to the results.
 * cosy_head_weight_pack: a parameter on the device in torchvision's layout -> fwd, the fragment order cosy_head_conv reads (float32; the
 *   bytes of the host packing), fwd_bias (c_out rounded up to 64 floats; ksize 2: 4 C_o, every bias four times) and bwd, the packing
 *   cosy_head_dgrad reads: rows c, reduction o rounded up to 16 with zeros, taps in reverse order (ksize 3) or (dy, dx) ascending (ksize 2).
 *   w0 / b0 (n0 outputs), then w1 / b1 (n1 outputs, n1 = 0: none) are the siblings of one GEMM.  One launch, no host round trip.
 * All: checked on the host before the launch (COSY_EINVAL, cosy_last_error() names the argument); M <= 2^30, 64-bit offsets; 1 to
 * COSY_RPN_MAX_LEVELS levels; pointers 16-byte aligned where cosy_head_conv asks for it. */
int cosy_head_wgrad_slab_rows(int M);
size_t cosy_head_wgrad_workspace_bytes(int M, int ksize, int c_in, int c_out);
int cosy_head_grad_pack(const float* g0, const float* g1, float* rows, int B, int n0, int n1, int HW, cosy_stream_t stream);
int cosy_head_weight_pack(const float* w0, const float* b0, const float* w1, const float* b1, int ksize, int c_in, int n0, int n1, float* fwd,
                          float* fwd_bias, float* bwd, cosy_stream_t stream);
int cosy_head_dgrad(const cosy_head_layer_t* layer, const float* y, cosy_stream_t stream);
int cosy_head_wgrad(const cosy_head_layer_t* layer, const float* g, float* dw0, float* db0, float* dw1, float* db1, void* workspace,
                    size_t workspace_bytes, cosy_stream_t stream);

/* ---- the backward of the detector's trunk on the matrix pipe, float32 only ----  DESIGN.md section 29 holds the contract.
 * A trunk layer is v = fmaf(conv_stride(x, W), scale, shift) [+ r], y = relu(v) as cosy_trunk_conv runs it; g is the gradient at v, float32
 * rows (B Ho Wo, c_out) on the layer's OUTPUT grid, Ho = (H - 1) / stride + 1; every channel count is a multiple of 8.
 * cosy_trunk_weight_pack: w (c_out, c_in, k, k) on the device in torchvision's layout, scale (c_out, or NULL: the FPN) and shift (c_out: the
 *   FrozenBatchNorm shift, or the FPN's bias) -> fwd, the fragment order cosy_trunk_conv reads (the bytes of the host packing), fwd_bias (shift,
 *   c_out rounded up to 64 floats, the pad +0.0) and bwd, the packing cosy_trunk_dgrad reads: ws = w scale[o] rounded ONCE to float32 (scale
 *   NULL: ws = w), rows c, reduction o rounded up to 16 with zeros, taps in reverse order.  Sizes as cosy_head_weight_pack's.  One launch.
 * cosy_trunk_dgrad: dX[(iy, ix)][c] = sum over o, (dy, dx) of ws[o][dy][dx][c] g[(y, x)][o] over the taps with iy = stride y + dy, ix =
 *   stride x + dx and (y, x) inside the output map, in cosy_head_dgrad's summation order (accumulator +0.0, blocks of 16 o ascending, the live
 *   taps in the packing's order inside a block, every term one fmaf).  layer->H / W / row_start describe the dX grid (the layer's INPUT maps),
 *   layer->x = g on the output grid, c_in = the layer's output channels (the reduction), c_out = its input channels, w = bwd, dtype COSY_F32,
 *   relu 0, bias unused.  stride 1 or 2 (2: one level, ksize 3: the four parity classes of (iy, ix) run as four row ranges, each with its 1,
 *   2, 2 or 4 live taps; a 1x1 at stride 2 is refused: run it at stride 1 on its output grid and hand the rows in as an EVEN operand).
 *   Store, per element, in this order: t = acc; for the operands add0, add1 with a rule other than COSY_TRUNK_ADD_NONE (rows of c_out float32
 *   channels, one level): SAME: t = t + rows[cell]; EVEN: the rows live on the ((H - 1) / 2 + 1, (W - 1) / 2 + 1) grid (addK_H, addK_W must say
 *   so), a cell with iy and ix even takes t = t + rows[(iy / 2, ix / 2)], every other cell is left untouched; NEAREST_T: the rows live on a finer
 *   addK_H x addK_W grid, t = t + rows[(fy, fx)] for every finer cell whose cosy_trunk_conv nearest source (sy = (float)H / addK_H) is this
 *   cell, (fy, fx) ascending; y != NULL: rows on the dX grid, t = y <= 0 ? +0.0 : t (a NaN y passes t); then COSY_HEAD_STORE_ROWS, or
 *   COSY_HEAD_STORE_NCHW with n_split == c_out.  Every + is one rounded float32 add.
 * cosy_trunk_wgrad: dw[o][c][tap] = scale[o] (sum over output cells of g[(y, x)][o] x[(stride y + dy, stride x + dx)][c]) in torchvision's
 *   (c_out, c_in, k, k), x = +0.0 outside its map; db[o] = sum of g[.][o] (db NULL: none).  layer->x = the rows the layer read, H / W /
 *   row_start their maps, c_in, c_out; the T = B Ho Wo output cells are cut into slabs of cosy_head_wgrad_slab_rows(T) and added in ascending
 *   order, then multiplied by scale[o] as one rounded product (scale NULL: none).  workspace: cosy_head_wgrad_workspace_bytes(T, ksize,
 *   c_in, c_out) bytes; a smaller one is refused.  T = 0 writes zeros.
 * All: checked on the host before any launch (COSY_EINVAL, the message starts with the function's name); at most 2^30 rows; 16-byte aligned
 * rows and packings.  No atomics: equal inputs give equal bits. */
enum { COSY_TRUNK_ADD_NONE = 0, COSY_TRUNK_ADD_SAME = 1, COSY_TRUNK_ADD_EVEN = 2, COSY_TRUNK_ADD_NEAREST_T = 3 };
int cosy_trunk_weight_pack(const float* w, const float* scale, const float* shift, int ksize, int c_in, int c_out, float* fwd, float* fwd_bias,
                           float* bwd, cosy_stream_t stream);
int cosy_trunk_dgrad(const cosy_head_layer_t* layer, int stride, const float* add0, int rule0, int add0_H, int add0_W, const float* add1,
                     int rule1, int add1_H, int add1_W, const float* y, cosy_stream_t stream);
int cosy_trunk_wgrad(const cosy_head_layer_t* layer, int stride, const float* g, const float* scale, float* dw, float* db, void* workspace,
                     size_t workspace_bytes, cosy_stream_t stream);

/* ---- the backward of the detector's trunk on bfloat16 rows, float32 master weights ----  DESIGN.md section 30 holds the contract.
 * The parameters, their gradients, scale, shift and every accumulation are float32; the rows (x, g, the add operands, y, dX) and both packed
 * weights are bfloat16, every conversion rounds to nearest even.  Layers, grids, strides, rules and limits are those of the float32 entries
 * above; dtype is COSY_BF16 (COSY_F32: the entries above; COSY_F16 is refused: float16 training needs a loss scaler, which is not built).
 * cosy_trunk_weight_pack16: w, scale (or NULL), shift float32 on the device -> fwd, the fragment order cosy_trunk_conv reads at COSY_BF16: the
 *   bytes of the host packing of w rounded to bfloat16; fwd_bias, float32 as cosy_trunk_weight_pack's; bwd, the packing cosy_trunk_dgrad16 reads:
 *   ws = bf16(fl32(w scale[o])) (ONE float32 product, then one rounding; scale NULL: ws = bf16(w)), rows c, reduction o in blocks of 32 (eight
 *   elements per lane, rounded up with zeros), taps in reverse order.  fwd: c_out rounded up to 64 x taps x c_in rounded up to 32 elements;
 *   bwd: c_in rounded up to 64 x taps x c_out rounded up to 32.  One launch.
 * cosy_trunk_grad_pack16: contiguous NCHW float32 (B, C, HW) -> bfloat16 rows (B HW, C), C a multiple of 8.  A NULL g is a tensor of zeros.
 * cosy_trunk_dgrad16: cosy_trunk_dgrad on bfloat16 rows: layer->x = g, w = bwd, out, add0, add1 and y are bfloat16.  Accumulator +0.0 float32,
 *   blocks of 32 o ascending, the live taps in the packing's order inside a block, one v_mfma_f32_16x16x32_bf16 per (block, tap): the products
 *   are exact in float32, the order of the 32 additions inside the instruction is the hardware's and the same on every call.  Store, per
 *   element: t = acc; t = t + (float)operand for add0, add1 under their rules (SAME, EVEN, NEAREST_T as above, an EVEN cell that takes nothing
 *   is left untouched), every + one rounded float32 add; y != NULL: t = y <= 0 ? +0.0 : t (a NaN y passes t); then ONE conversion to bfloat16.
 *   store: COSY_HEAD_STORE_ROWS only.
 * cosy_trunk_wgrad16: cosy_trunk_wgrad with layer->x and g bfloat16 rows; dw, db, scale and the workspace float32.  The cells are the k
 *   dimension of v_mfma_f32_16x16x32_bf16, 32 per instruction; a cell past its slab, a tap outside the map feed +0.0.  Slabs
 *   (cosy_head_wgrad_slab_rows), workspace (cosy_head_wgrad_workspace_bytes), the ascending second pass and the one scale[o] product are
 *   cosy_trunk_wgrad's.  x and g 16-byte aligned.
 * All: checked on the host before any launch (COSY_EINVAL, the message starts with the function's name).  No atomics: equal inputs give equal bits. */
int cosy_trunk_weight_pack16(const float* w, const float* scale, const float* shift, int ksize, int c_in, int c_out, void* fwd, float* fwd_bias,
                             void* bwd, cosy_stream_t stream);
int cosy_trunk_grad_pack16(const float* g, void* rows, int B, int C, int HW, cosy_stream_t stream);
int cosy_trunk_dgrad16(const cosy_head_layer_t* layer, int stride, const void* add0, int rule0, int add0_H, int add0_W, const void* add1,
                       int rule1, int add1_H, int add1_W, const void* y, cosy_stream_t stream);
int cosy_trunk_wgrad16(const cosy_head_layer_t* layer, int stride, const void* g, const float* scale, float* dw, float* db, void* workspace,
                       size_t workspace_bytes, cosy_stream_t stream);

/* ---- the backward of the detector's heads on bfloat16 rows, float32 master weights ----  DESIGN.md section 32 holds the contract.
 * The parameters, their gradients and every accumulation are float32; the rows (x, g, y, dX between two layers) and both packed weights are
 * bfloat16, every conversion rounds to nearest even.  Layers, maps, ksize (1, 3, or 2 for ConvTranspose2d(2, 2)), siblings and limits are those of
 * cosy_head_grad_pack .. cosy_head_wgrad above; dtype is COSY_BF16 (COSY_F32: the entries above; COSY_F16 is refused: no loss scaler is built).
 * cosy_head_weight_pack16: as cosy_head_weight_pack -> fwd, the bytes of the host packing of the weight rounded to bfloat16 in the 16-bit
 *   fragment order cosy_head_conv reads at COSY_BF16 (siblings: w0 then w1; ksize 2: the 4 C_o outputs (o, dy, dx)), c_out rounded up to 64 x
 *   taps x c_in rounded up to 32 elements; fwd_bias float32 as cosy_head_weight_pack's; bwd: bf16(w), rows c rounded up to 64, reduction o in
 *   blocks of 32 rounded up with zeros, taps in reverse order (ksize 3) or (dy, dx) ascending (ksize 2).  One launch.
 * cosy_head_grad_pack16: cosy_head_grad_pack with bfloat16 rows (B HW, GP): the columns of g0, then of g1, then +0.0; NULL is zeros.
 * cosy_head_dgrad16: cosy_head_dgrad on bfloat16 rows g, y and bwd: accumulator +0.0 float32, blocks of 32 o ascending, the taps in the
 *   packing's order inside a block, one v_mfma_f32_16x16x32_bf16 per (block, tap).  COSY_HEAD_STORE_ROWS: out bfloat16, t = y <= 0 ? +0.0 : acc
 *   (y NULL: acc), then ONE conversion.  COSY_HEAD_STORE_NCHW (ksize 1 / 3, y NULL, n_split == c_out): out float32 NCHW per level, the
 *   accumulator unrounded.
 * cosy_head_wgrad16: cosy_head_wgrad with layer->x and g bfloat16 rows (g: GP columns); dw, db and the workspace float32.  The cells are the k
 *   dimension of v_mfma_f32_16x16x32_bf16, 32 per instruction; ksize 2: the k dimension is the cells of x, the four taps read g at
 *   (2y + dy, 2x + dx), db is the sum over the four.  Slabs, workspace and the ascending second pass are cosy_head_wgrad's.
 * All: checked on the host before any launch (COSY_EINVAL, the message starts with the function's name).  No atomics: equal inputs give equal bits. */
int cosy_head_weight_pack16(const float* w0, const float* b0, const float* w1, const float* b1, int ksize, int c_in, int n0, int n1, void* fwd,
                            float* fwd_bias, void* bwd, cosy_stream_t stream);
int cosy_head_grad_pack16(const float* g0, const float* g1, void* rows, int B, int n0, int n1, int HW, cosy_stream_t stream);
int cosy_head_dgrad16(const cosy_head_layer_t* layer, const void* y, cosy_stream_t stream);
int cosy_head_wgrad16(const cosy_head_layer_t* layer, const void* g, float* dw0, float* db0, float* dw1, float* db1, void* workspace,
                      size_t workspace_bytes, cosy_stream_t stream);

/* ---- the detector's optimiser step on flat buffers, and the repack of all its layers in one launch ----  DESIGN.md section 33 holds the contract.
 * cosy_sgd_step: torch.optim.SGD(lr, momentum, weight_decay), dampening 0, no Nesterov, on flat float32 buffers of n elements.  lr, momentum and
 *   weight_decay are float32 (the caller rounds them); every product and every sum below is ONE rounded float32 operation, nothing is fused:
 *     d  = g + weight_decay w            (weight_decay == 0: d = g, no product is formed)
 *     m' = d when first_step != 0, else momentum m + d      (momentum == 0: m' = d and momentum_buf is neither read nor written; it may be NULL)
 *     w' = w - lr m'
 *   NaN and Inf propagate as these operations propagate them.  A streaming kernel: 16-byte loads and stores on the body (the three buffers must
 *   be 16-byte aligned), a scalar tail for n % 4, a grid of cosy_sgd_step_pass_elements() / 1024 workgroups (a function of the device's
 *   compute-unit count) that strides, 64-bit offsets, no atomics.  n = 0 launches nothing.
 * cosy_sgd_step_pass_elements: the elements one pass of that grid covers on the current device (tests size a buffer past it).
 * cosy_pack_table_build: the layers of a pack table, one row of 13 long long words each:
 *     [0] w0  [1] b0  [2] w1  [3] b1  [4] scale  [5] fwd  [6] fwd_bias  [7] bwd       device addresses (w1, b1, scale: 0 for none)
 *     [8] ksize  [9] c_in  [10] n0  [11] n1  [12] dtype (COSY_F32 or COSY_BF16: the type of fwd and bwd)
 *   A row means what cosy_head_weight_pack (COSY_F32) / cosy_head_weight_pack16 (COSY_BF16) mean by the same arguments, with one addition: scale
 *   (n0 floats, n1 = 0), the trunk's FrozenBatchNorm scale as cosy_trunk_weight_pack takes it (b0 is then the shift).  Every row is checked as those
 *   entries check their arguments, and fwd / bwd 16-byte, every other pointer 4-byte aligned (COSY_EINVAL, the message starts with
 *   "cosy_pack_table_build: layer <i>:"), before anything touches the device.  Then the table is written to `table` (device memory of
 *   cosy_pack_table_bytes(n_layers) bytes, 16-byte aligned, owned by the caller) and the call returns once it is there; *n_workgroups receives
 *   the grid of the run.  Layers start on workgroup boundaries: the table holds every layer's first workgroup.  1 <= n_layers <= 4096.
 * cosy_pack_table_run: ONE launch that writes fwd, fwd_bias and bwd of every layer of a built table from the parameters as they are now: the
 *   bytes the per-layer entries write (the packing rules exist once, csrc/detbwd_device.h).  A workgroup finds its layer by a search of the
 *   first-workgroup column, the same for all its threads.  It only launches: no validation of the table's contents, no copy.  table,
 *   n_layers and n_workgroups are those of the build. */
int cosy_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, float lr, float momentum, float weight_decay, int first_step,
                  cosy_stream_t stream);
long long cosy_sgd_step_pass_elements(void);
size_t cosy_pack_table_bytes(int n_layers);
int cosy_pack_table_build(const long long* rows, int n_layers, void* table, size_t table_bytes, long long* n_workgroups, cosy_stream_t stream);
int cosy_pack_table_run(const void* table, int n_layers, long long n_workgroups, cosy_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* COSYHIP_H */
