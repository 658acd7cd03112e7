/*
 * pave_hip.h -- C ABI of libpave_hip.so: the MI355X (gfx950) device side of the
 * PAVE-Net forward hot path.
 *
 * Every entry point takes plain device pointers + sizes + a hipStream_t passed
 * as void* (no torch / ATen types), returns 0 on success and a negative
 * PAVE_E_* code on failure (pave_last_error() has the message), launches on the
 * given stream and never synchronises or allocates.
 *
 * Reference interfaces these replace (paths relative to zgspose/PAVENet):
 *   [R1] third_party/mmcv/mmcv/ops/csrc/pytorch/pybind.cpp:160-173,737-748
 *        Tensor ms_deform_attn_forward(value, spatial_shapes, level_start_index,
 *                                      sampling_loc, attn_weight, im2col_step)
 *        -> third_party/mmcv/mmcv/ops/csrc/pytorch/cuda/ms_deform_attn_cuda.cu:209-277
 *        -> kernel third_party/mmcv/mmcv/ops/csrc/common/cuda/ms_deform_attn_cuda_kernel.cuh:200-254
 *   [R2] third_party/mmcv/mmcv/ops/multi_scale_deform_attn.py:305-412
 *        MultiScaleDeformableAttention.forward: softmax over L*P, loc = ref + off/(W,H),
 *        then [R1]  (encoder self-attention, hot loop #1)
 *   [R3] opera/models/utils/transformer.py:1644-1863 (T=3) / 2738-3117 (T=5)
 *        MulFramesMultiScaleDeformablePoseAttentionNumFrames{3,5}.forward: per-frame
 *        softmax + Z_t re-weighting (== joint softmax over T*L*K), pose-box scaled
 *        offsets, T x [R1]  (pose decoder, hot loop #2)
 *   [R4] third_party/mmcv/mmcv/ops/multi_scale_deform_attn.py:1388-1587 (T=3) / 1590-1981 (T=5)
 *        MulFramesMultiScaleDeformableAttentionNumFrames{3,5}.forward: same fusion with
 *        grid offsets, T x [R1]  (joint decoder, hot loop #3)
 */
#ifndef PAVE_HIP_H_
#define PAVE_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAVE_OK 0
#define PAVE_E_ARG (-1)     /* bad argument (null pointer, non-positive size, unsupported shape) */
#define PAVE_E_LAUNCH (-2)  /* hipLaunchKernel reported an error */
#define PAVE_E_STEP (-3)    /* batch %% im2col_step != 0, as the reference asserts */
#define PAVE_E_UNSUPPORTED (-4) /* valid arguments, but not a shape this entry point's kernel covers */

/* ABI version; bumped on any signature change (pavenet_amd/native.py checks it at load). */
#define PAVE_ABI_VERSION 21
int pave_abi_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* pave_last_error(void);

/*
 * [R1] Multi-scale deformable attention, forward, fp32 / fp64.
 *   value          [bs, S, M, D]
 *   spatial_shapes [L, 2] int64 (h, w), DEVICE memory   (as the reference tensor)
 *   level_start    [L]    int64,        DEVICE memory
 *   sampling_loc   [bs, Lq, M, L, P, 2] (x, y) normalised to [0,1]
 *   attn_weight    [bs, Lq, M, L, P]
 *   out            [bs, Lq, M*D]  (fully overwritten; need not be zeroed)
 * im2col_step only reproduces the reference's divisibility check
 * (ms_deform_attn_cuda.cu:242-245): min(bs, step) must divide bs.
 * Two kernels behind it: D %% 4 == 0 fp32 takes msda_fwd_vec_kernel (G lanes x 4 channels per (query, head),
 * float4 corner loads); every other case -- fp64, D not a multiple of 4 (the reference's gradcheck list has 30, 71
 * and 1025) -- takes msda_fwd_scalar_kernel, the COMPATIBILITY FALLBACK of this entry point: one thread per output
 * element, i.e. the reference kernel's own work decomposition (ms_deform_attn_cuda_kernel.cuh:200-254), kept for
 * coverage of the drop-in signature and not a CDNA4 design.  The PAVE-Net forward path never calls either: it runs
 * on the fused launches below (pave_enc_deform_attn_tile_f32, pave_deform_attn_*_fused_f32).
 */
int pave_ms_deform_attn_forward_f32(const float* value, const int64_t* spatial_shapes,
                                    const int64_t* level_start, const float* sampling_loc,
                                    const float* attn_weight, float* out, int bs, int S, int M,
                                    int D, int L, int Lq, int P, int im2col_step, void* stream);
int pave_ms_deform_attn_forward_f64(const double* value, const int64_t* spatial_shapes,
                                    const int64_t* level_start, const double* sampling_loc,
                                    const double* attn_weight, double* out, int bs, int S, int M,
                                    int D, int L, int Lq, int P, int im2col_step, void* stream);

/*
 * Fused T-frame deformable attention (M = 8 heads x D = 32 channels).
 *
 * One launch replaces, for all T frames: softmax / Z_t arithmetic, sampling
 * location arithmetic, T calls of [R1] and the cross-frame fusion.  The softmax
 * is the numerically stabilised joint softmax over all T*L*P logits of a
 * (unit, head), which is algebraically what [R3]/[R4] compute with an
 * un-stabilised exp.
 *
 * "unit" = one query row: encoder token (b, q) / pose query (b, q) / joint query (n, k).
 *
 *   value      [n_clips*T, S, 8, 32]  projected (and padding-masked) memory; frame t of
 *                                     clip c is slab c*T + t
 *   proj       [n_units, proj_stride] raw outputs of the offset / logit Linears for one unit:
 *                offsets at [t][m][l][p][2] starting at column 0,
 *                logits  at [t][m][l][p]    starting at column T*8*L*P*2
 *   unit_clip  [n_units] int32 clip index of each unit, or NULL => unit / units_per_clip
 *   order      [n_units] int32 permutation giving the processing order of units (XCD/L2
 *              locality), or NULL => identity
 *   frame_table [n_clips*T] int32, or NULL: the value slab of frame t of clip c is
 *              frame_table[c*T + t] instead of c*T + t -- `value` is then a per-frame cache
 *              [n_cached_frames, S, 8, 32] shared by overlapping clips (streaming windows of a video,
 *              opera/datasets/posetrack_video_pose.py:578-623: no per-window copy / re-projection).
 *              n_slabs = n_cached_frames (> 0 with a table; 0 or n_clips*T without): the entries are slab
 *              indices read on the device; every slab index is CLAMPED into [0, n_slabs) there, so a bad
 *              table reads a wrong frame of `value`, never memory outside it (a correct result still needs
 *              0 <= frame_table[i] < n_slabs: pavenet_amd/streaming.py checks the host list the table is
 *              made from, FrameSlabs.covers)
 *   out        [n_units, 256]
 *   stat_max, stat_sum  [n_units, 8] or NULL: per-head max logit and sum(exp(logit-max)) over the
 *              frames this call saw (for merging frame-sharded partial results)
 *
 * GRID form ([R2] with T = 1, [R4]): L = 4 levels x P = 4 points;
 *   ref [T, n_units, L, 2] (already multiplied by valid ratios);  loc = ref + off / (W_l, H_l)
 * POSE form ([R3]): L levels x P = K keypoints (K <= 24);
 *   ref [n_clips, T, Q, L, 2K] with n_units = n_clips*Q;  wh = clamp(max-min over K, 1e-4);
 *   loc = ref_k + off * wh * 0.5
 * ref_levels = L, or 1: ref is [T, n_units, 1, 2] / [n_clips, T, Q, 1, 2K] and every level reads the same
 *   row (un-padded batches: all valid ratios are 1, the reference broadcasts `reference_points[:, :, None]`
 *   over the levels, OT:6712-6720 / MT:845-856 -- no materialised copy).
 */
int pave_deform_attn_grid_fused_f32(const float* value, const int64_t* spatial_shapes,
                                    const int64_t* level_start, const float* proj,
                                    const float* ref, const int32_t* unit_clip,
                                    const int32_t* order, float* out, float* stat_max,
                                    float* stat_sum, int n_units, int units_per_clip, int n_clips,
                                    int T, int S, int L, int P, int proj_stride,
                                    const int32_t* frame_table, int n_slabs, int ref_levels, void* stream);

int pave_deform_attn_pose_fused_f32(const float* value, const int64_t* spatial_shapes,
                                    const int64_t* level_start, const float* proj,
                                    const float* ref, float* out, float* stat_max,
                                    float* stat_sum, int n_clips, int Q, int T, int S, int L,
                                    int K, int proj_stride, const int32_t* frame_table, int n_slabs,
                                    int ref_levels, void* stream);

/*
 * The encoder layer's merged projection (value_proj | sampling_offsets | attention_weights as ONE
 * N = 640 GEMM, third_party/mmcv/mmcv/ops/multi_scale_deform_attn.py:357-384) with the sampler's
 * per-(query, head) arithmetic done in the GEMM epilogue:
 *   a [M, K] fp32;  w_planes = the 3-plane split of the [640, K] row-concatenated weight;
 *   table [table_rows, 640]: row m adds table[m % table_rows] (bias + positional term);
 *   value_bias: NULL, or 256 floats added to the value columns INSTEAD of the table's first 256
 *     columns, which are then not read (value_proj has no positional term: its table columns are
 *     one bias row repeated);
 *   ref [M, 4, 2] reference points (normalised x, y per level);  levels_hw [4][2] (h, w), HOST memory
 *   -> value [M, 256];  samp [M, 384] = level PIXEL coordinates [8 heads][4 levels][4 points][x, y]
 *      ((ref + off / (w, h)) * (w, h) - 0.5), then softmaxed attention weights [8][16]
 * i.e. `proj` of pave_enc_deform_attn_tile_f32 in its prepared form (variant | 4): same bits as
 * feeding that kernel the raw projections (one definition of the arithmetic, csrc/pave_enc_math.h).
 * nplanes: 3 or PAVE_PLANES_FP16 (below).
 */
int pave_gemm_bf16x3_encproj_f32(const float* a, const void* w_planes, const float* table,
                                 long long table_rows, const float* value_bias, const float* ref,
                                 const int* levels_hw, float* value, float* samp, long long M, int K,
                                 int nplanes, void* stream);

/*
 * HRNet stem conv1 (third_party/mmdetection/mmdet/models/backbones/hrnet.py:549-556): 3x3 / stride 2
 * / pad 1 convolution of the NCHW image batch x [N, 3, H, W], 3 -> 64 channels, + bias (the folded
 * BatchNorm) + optional ReLU -> y [N, Ho, Wo, 64] NHWC, Ho = (H - 1) / 2 + 1.
 *   w_taps [27][64]: weight[co][c][ky][kx] at w_taps[(c * 3 + ky) * 3 + kx][co]
 */
int pave_conv3x3s2_c3_nchw_f32(const float* x, const float* w_taps, const float* bias, float* y, int N,
                               int H, int W, int relu, void* stream);

/*
 * Scaled-dot-product core of the decoders' self-attention (replaces what nn.MultiheadAttention
 * runs between its in- and out-projection, third_party/mmcv/mmcv/cnn/bricks/transformer.py:
 * 406-551 as the reference's decoder layers call it: no masks, no dropout, 32 channels per head).
 *   qkv [n_seq * L, ld]: row = (sequence, position); q at column 0, k at column H*32, v at 2*H*32
 *   out [n_seq * L, H*32] = softmax(q k^T / sqrt(32)) v per (sequence, head)
 * One head's K and V ([L, 32] each) are staged in LDS: L <= 568.
 */
int pave_mha_core_f32(const float* qkv, float* out, int n_seq, int L, int H, int ld, void* stream);

/*
 * Row-wise top-k in one launch: element (r, i) of x at x[r ld + i cs], i < n; k <= 1024,
 * n <= 32768 -> index [rows, k] int64 sorted by (value descending, index ascending), values
 * [rows, k] (may be NULL).  A NaN of either sign ranks above +inf (torch.topk's order), NaNs among
 * themselves by ascending index.  -0.0 and +0.0 are equal values: between them the lower index comes
 * first, also in the selection at the k-th value.  The values are read back from x, so they keep the
 * input's sign bits.  Replaces torch.topk for the
 * proposal selection (opera/models/utils/transformer.py:21383-21385) and the score selection
 * (opera/models/dense_heads/videopose_head_mul_frames.py:1416).
 */
int pave_topk_rows_f32(const float* x, float* values, long long* index, int rows, int n, int ld, int cs,
                       int k, void* stream);

/*
 * The N selected queries of every frame in one gather (videopose_head_mul_frames.py:1419-1427, 610):
 * poses [B, T*Q, C] (frame t at rows [t Q, (t+1) Q)), index [B, N] int64 (clamped to [0, Q))
 * -> out [T, B*N, C] frame-major.
 */
int pave_gather_frame_poses_f32(const float* poses, const long long* index, float* out, int B, int T,
                                int Q, int N, int C, void* stream);

/*
 * Post-processing of the refined poses in one launch (videopose_head_mul_frames.py:1440-1490,
 * get_p :1531-1535): pixels = clamp(kpt * (w, h), 0, (w, h)) [/ scale factor], bounding box =
 * min / max over the K key points, p = 0.7 (1 - exp(-0.2 / sigma_x)) (1 - exp(-0.2 / sigma_y)),
 * kpt <- kpt p^5 / (p^5 + 1e-10), key-point score = pose score * p.
 *   kpts, sigmas [B, N, K, 2]; scores [B, N]; wh, sf [B, 2] (sf only read when rescale != 0)
 *   sigma_ld: floats between consecutive (x, y) rows of sigmas (2 = dense; 4 = the sigma branch's output as its
 *   GEMM leaves it, padded to the 4-column grid)
 *   -> det_kpts [B, N, K, 3] (x, y, score), det_bboxes [B, N, 5] (x1, y1, x2, y2, score);  K <= 64
 */
int pave_pose_finalize_f32(const float* kpts, const float* sigmas, const float* scores, const float* wh,
                           const float* sf, float* det_kpts, float* det_bboxes, int B, int N, int K,
                           int rescale, int sigma_ld, void* stream);

/*
 * Reference-point update of the decoders read straight from the grouped per-frame MLP output
 * (opera/models/utils/transformer.py:6728-6735, mmdet/models/utils/transformer.py:861-866):
 *   y [R, T*op]: row r, frame t's o outputs at columns [t op, t op + o);  ref, out [R*T, o] with row
 *   (r / G) T G + t G + r % G  (G = queries per clip: frame-major inside a clip; G = R: frame-major
 *   over all rows);  out = sigmoid(y + inverse_sigmoid(ref)), eps as mmdet's inverse_sigmoid.
 */
int pave_ref_update_frames_f32(const float* y, const float* ref, float* out, int R, int T, int op, int o,
                               int G, float eps, void* stream);

/*
 * Two-stage query initialisation behind the proposal top-k (opera/models/utils/transformer.py:21386-21418), two
 * launches for the reference's gather / repeat / strided add / sigmoid sequence:
 *   pave_gather_rows_add_f32: rows[n, q, :] = src[n, index[n, q], :] (src [n, S, C] with a batch stride in elements,
 *     index [n, Q] int64: `tgt`, the selected rows of output_memory) and, when sum != NULL,
 *     sum[n, q, :] = rows[n, q, :] + add[q, :] (`query = tgt + query`; add [Q, C]).  C %% 4 == 0.
 *   pave_proposal_refs_f32: kpt [n*Q, ld] (its first K2 = 2 K columns; in place) += props[n, index[n, q], c & 1]
 *     (props [n, S, 2], batch stride in elements, 0 = one table for every clip; +inf marks an invalid proposal) and
 *     refs [n, T*Q, K2] = sigmoid(kpt) repeated for the T frames (`topk_kpts_unact.sigmoid().repeat(1, T, 1)`).
 * An index outside [0, S) is never dereferenced: the gathered row is zero, the proposal term is dropped.
 */
int pave_gather_rows_add_f32(const float* src, long long src_batch_stride, const long long* index, const float* add,
                             float* rows, float* sum, int n, int Q, int S, int C, void* stream);
int pave_proposal_refs_f32(float* kpt, int ld, const float* props, long long props_batch_stride,
                           const long long* index, float* refs, int n, int Q, int S, int K2, int T, void* stream);

/*
 * Greedy OKS-NMS, one launch for n_clips clips (replaces oks_nms / oks_iou,
 * opera/models/dense_heads/videopose_head_mul_frames.py:1624-1665, a NumPy loop behind a
 * device->host sync in the reference).
 *   kpts   [n_clips, N, K, 3] (x, y, score) pixels;  scores [n_clips, N];  sigmas [K] double, DEVICE
 *   keep   [n_clips, N] int32: 1 = kept;  order [n_clips, N] int32: indices by descending score
 * A pose is suppressed when its OKS with an earlier kept pose is > thresh.
 * Equal scores come out larger index first (the reverse of a stable ascending sort), and a NaN
 * score sorts as +inf, so `order` is a permutation of 0 .. N - 1 for any input.  N <= 4096.
 */
int pave_oks_nms_f32(const float* kpts, const float* scores, const double* sigmas, double thresh,
                     int32_t* keep, int32_t* order, int n_clips, int N, int K, void* stream);

/*
 * Fused row epilogues around the library GEMMs / convolutions (HBM-bound, one pass).
 *   bias_act_rows:      y[r,c] = act(x[r,c] + bias[c] + res[r,c]);  bias / res may be NULL,
 *                       y may alias x; relu != 0 applies max(.,0).  Replaces the separate
 *                       bias, residual-add and ReLU kernels behind conv / Linear
 *                       (mmdet resnet.py Bottleneck.forward, mmcv FFN).
 *   bias_add_layernorm: y[r,:] = LayerNorm(x[r,:] + bias + res[r,:]) * gamma + beta,
 *                       C % 4 == 0, C <= 3072 (the 'attn/ffn -> + identity -> norm' step of
 *                       mmcv BaseTransformerLayer.forward, bricks/transformer.py:1316-1353).
 */
/*
 * x[rows[i], 0:C] = values[0:C] (values == NULL: zeros) for i < n_rows; x [total_rows, ld] row-major, `rows`
 * int32 indices on the DEVICE (an index outside [0, total_rows) is skipped, never dereferenced).
 * The padding mask of the reference on a projected value matrix -- masked tokens are 0 when the mask follows
 * value_proj (third_party/mmcv/mmcv/ops/multi_scale_deform_attn.py:369-371) and value_proj.bias when it
 * precedes it (opera/models/utils/transformer.py:1706-1711, multi_scale_deform_attn.py:1454-1458) -- applied
 * to the listed rows only instead of a masked_fill pass over the whole memory (an 800 x 1333 image in an
 * 800 x 1344 batch masks ~1 % of the tokens).
 */
int pave_fill_rows_f32(float* x, long long ld, long long total_rows, const int* rows, long long n_rows,
                       const float* values, int C, void* stream);
int pave_bias_act_rows_f32(const float* x, const float* bias, const float* res, float* y,
                           long long rows, int C, int relu, void* stream);
/*
 * HRNet fuse layer (third_party/mmdetection/mmdet/models/backbones/hrnet.py:197-214:
 * `y = 0; for j: y += x[j] if i == j else fuse_layers[i][j](x[j])`, `relu(y)`), NHWC fp32, one pass:
 *   y[n, h, w, :] = act(s0[n, h >> sh0, w >> sh0, :] + s1[...] + s2[...] + s3[...])   (in this order)
 * source k is a [N, H >> sh_k, W >> sh_k, C] map -- the nearest-neighbour nn.Upsample(scale_factor =
 * 2^sh_k) that ends the coarser branches' fuse path is folded into the read; s1..s3 may be NULL.
 * y may alias a source with sh == 0.  C %% 4 == 0, 2^sh_k divides H and W.
 */
int pave_fuse_sum_nhwc_f32(const float* s0, int sh0, const float* s1, int sh1, const float* s2, int sh2,
                           const float* s3, int sh3, float* y, int N, int H, int W, int C, int relu,
                           void* stream);
int pave_bias_add_layernorm_f32(const float* x, const float* bias, const float* res,
                                const float* gamma, const float* beta, float* y, long long rows,
                                int C, float eps, void* stream);
/* As above, plus y_plus[r,:] = y[r,:] + pos[r %% pos_rows, :] in the same pass: the next
 * encoder layer's `query + query_pos` (mmcv multi_scale_deform_attn.py:353-354). */
int pave_bias_add_layernorm_pos_f32(const float* x, const float* bias, const float* res,
                                    const float* gamma, const float* beta, float* y,
                                    const float* pos, long long pos_rows, float* y_plus,
                                    long long rows, int C, float eps, void* stream);

/*
 * Encoder deformable attention ([R2]: mmcv MultiScaleDeformableAttention.forward, MO:373-404,
 * T = 1, M = 8, D = 32, L = 4, P = 4) with the value rows staged in LDS per 8 x 8-pixel image
 * tile and head (pavenet_amd/csrc/pave_enc_tile.hip).  Same inputs, outputs and results as
 * pave_deform_attn_grid_fused_f32 with T = 1 and no unit_clip / order; corners outside a tile's
 * LDS window are fetched from global memory, so results do not depend on the window size.
 *   value [n_frames, S, 8, 32]; proj [n_frames*S, proj_stride] (offsets [8][4][4][2], then
 *   logits [8][4][4]); ref [n_frames*S, 4, 2]; out [n_frames*S, 256]
 *   levels_hw   HOST array of 8 ints (h0, w0, ..., h3, w3), levels in flattening order
 *   variant     a bit mask: 0 = windows of -4 .. +3 px (3 workgroups per CU), 1 = -4 .. +4 px (1 per CU);
 *               | 4 = `proj` is PREPARED (pave_gemm_bf16x3_encproj_f32: pixel coordinates + attention weights;
 *               ref is not read; default windows only);  | 8 = `out` is fp16 [n_frames*S, 256] (fp16 operand
 *               mode: the rows only feed output_proj's MFMA, pave_gemm_fp16_act_f32 -- the same values at half
 *               the bytes).  Other bits / combinations: PAVE_E_ARG / PAVE_E_UNSUPPORTED before anything is enqueued
 *   window_shift  NULL, or a HOST array [8 heads][4 levels][2] of (dx, dy) in level pixels that
 *               moves the LDS window of (tile, head, level): a head's points sit around
 *               reference + its mean learnt offset (the reference initialises them on a ray 1..4 px
 *               out, MO:227-240), so centring the window there keeps them in LDS.  Speed only.
 * Returns PAVE_E_UNSUPPORTED (nothing launched) unless every level l satisfies
 * H_l <= (8 >> l) * ceil(H_0 / 8) and W_l likewise (a halving pyramid): callers then use
 * pave_deform_attn_grid_fused_f32.
 */
int pave_enc_deform_attn_tile_f32(const float* value, const float* proj, const float* ref,
                                  float* out, int n_frames, int S, const int* levels_hw,
                                  int proj_stride, int variant, const int* window_shift,
                                  void* stream);

/*
 * [R1] backward: void ms_deform_attn_backward(value, spatial_shapes, level_start_index,
 * sampling_loc, attn_weight, grad_output, grad_value, grad_sampling_loc, grad_attn_weight,
 * im2col_step)  (pybind.cpp:167-173, 743-748; ms_deform_attn_cuda.cu:279-351;
 * kernels ms_deform_attn_cuda_kernel.cuh:66-198, 256-801).
 *   grad_output [bs, Lq, M*D];  grad_value [bs, S, M, D] is ACCUMULATED into (caller zeroes it,
 *   as MO:72 does);  grad_sampling_loc [bs, Lq, M, L, P, 2] and grad_attn_weight
 *   [bs, Lq, M, L, P] are fully overwritten.
 */
int pave_ms_deform_attn_backward_f32(const float* value, const int64_t* spatial_shapes,
                                     const int64_t* level_start, const float* sampling_loc,
                                     const float* attn_weight, const float* grad_output,
                                     float* grad_value, float* grad_sampling_loc,
                                     float* grad_attn_weight, int bs, int S, int M, int D, int L,
                                     int Lq, int P, int im2col_step, void* stream);
int pave_ms_deform_attn_backward_f64(const double* value, const int64_t* spatial_shapes,
                                     const int64_t* level_start, const double* sampling_loc,
                                     const double* attn_weight, const double* grad_output,
                                     double* grad_value, double* grad_sampling_loc,
                                     double* grad_attn_weight, int bs, int S, int M, int D, int L,
                                     int Lq, int P, int im2col_step, void* stream);

/*
 * Device input pipeline for T frames of one clip (mmdet Resize(keep_ratio) -> Normalize(to_rgb)
 * -> Pad -> MulImageToTensor; configs/_base_/datasets/posetrack17_video_keypoint.py:71-84).
 *   src   [T, H0, W0, 3] HWC, BGR, uint8 (src_is_u8 = 1) or float32, DEVICE
 *   dst   [T, 3, Hp, Wp] float32: the (Hn, Wn) resized + normalised image top-left, zeros elsewhere
 *   mean, std  HOST float[3] (in the order of the channels AFTER the optional BGR->RGB swap)
 */
int pave_preprocess_frames(const void* src, int src_is_u8, float* dst, int T, int H0, int W0,
                           int Hn, int Wn, int Hp, int Wp, const float* mean, const float* std,
                           int to_rgb, void* stream);
/* The same, mirrored within the resized width: dst[.., x] for x < Wn is what pave_preprocess_frames writes at
 * Wn - 1 - x (bit for bit: the same arithmetic on the mirrored column); the padding stays zero on the right,
 * as mmdet's RandomFlip (after Resize, before Normalize / Pad) leaves it. */
int pave_preprocess_frames_flip(const void* src, int src_is_u8, float* dst, int T, int H0, int W0,
                                int Hn, int Wn, int Hp, int Wp, const float* mean, const float* std,
                                int to_rgb, void* stream);
/*
 * The same pipeline fed from NV12 surfaces, as hardware video decoders hand them out (pave_ingest.hip).
 *   src   T surfaces on the DEVICE, frame_stride bytes apart; a surface is H0 rows of `pitch` bytes of Y, then
 *         H0 / 2 rows of `pitch` bytes of interleaved U, V.  pitch >= W0; H0 and W0 even.
 *   csc   HOST float[6] = {yoff, cy, crv, cgu, cgv, cbu}.  Per source pixel, chroma from block (y >> 1, x >> 1):
 *           t = (Y - yoff) * cy;  B = t + (U - 128) * cbu;  G = (t + (U - 128) * cgu) + (V - 128) * cgv;
 *           R = t + (V - 128) * crv
 *         every product and sum rounded to fp32 on its own, then rintf (ties to even) and a clamp to [0, 255].
 * From that 8-bit BGR value on the arithmetic is pave_preprocess_frames's: dst equals, bit for bit, what
 * pave_preprocess_frames(src_is_u8 = 1) writes for the converted image.
 */
int pave_preprocess_frames_nv12(const void* src, long long frame_stride, int pitch, float* dst,
                                int T, int H0, int W0, int Hn, int Wn, int Hp, int Wp,
                                const float* csc, const float* mean, const float* std,
                                int to_rgb, void* stream);
/*
 * The same for n separately allocated surfaces in one launch (several cameras: each decoder hands out its own
 * allocation, pitch, matrix and range).  The plan is copied into the kernel's arguments (no host->device copy).
 *   src[i], pitch[i], csc[i]  surface i as above (one surface, no frame_stride); H0 x W0 is the same for all
 *   dst   [n, 3, Hp, Wp]: dst[i] equals, bit for bit, what pave_preprocess_frames_nv12 writes for surface i alone
 *         with csc[i] (both kernels run one per-pixel function)
 * 1 <= n <= PAVE_INGEST_MAX_SURFACES, every src[i] non-null, every pitch[i] >= W0; H0 and W0 even.
 */
#define PAVE_INGEST_MAX_SURFACES 32
typedef struct pave_ingest_plan {
  const void* src[PAVE_INGEST_MAX_SURFACES];    /* DEVICE: H0 rows of pitch[i] bytes of Y, then H0 / 2 rows of UV */
  int         pitch[PAVE_INGEST_MAX_SURFACES];
  float       csc[PAVE_INGEST_MAX_SURFACES][6]; /* yoff, cy, crv, cgu, cgv, cbu as in pave_preprocess_frames_nv12 */
  int n;
} pave_ingest_plan;
int pave_preprocess_surfaces_nv12(const pave_ingest_plan* plan, float* dst, int H0, int W0, int Hn, int Wn, int Hp,
                                  int Wp, const float* mean, const float* std, int to_rgb, void* stream);

/*
 * Row scatter of the live ring (pavenet_amd/live.py CameraRing): dst[t][row[i]] = src[t][i] for i < n and the first
 * k tensors, a plain copy in one launch.  The plan is a HOST struct copied into the kernel's arguments.
 *   src[t]  DEVICE [n, row_elems] fp32, dense;  dst[t]  DEVICE [dst_rows, row_elems] fp32, dense
 *   row[i]  the destination row of source row i
 * Refused with PAVE_E_ARG before any device call: a null pointer among the first k, n outside 1 .. 64, k outside
 * 1 .. 8, dst_rows or row_elems < 1, row_elems not a multiple of 4, a pointer that is not 16-byte aligned (the
 * kernel moves 16 bytes per lane), a row[i] outside [0, dst_rows), two equal row[i] (the result would depend on
 * block order).  A plan that passes cannot address memory outside its tensors.
 */
#define PAVE_SCATTER_MAX_ROWS 64
#define PAVE_SCATTER_MAX_TENSORS 8
typedef struct pave_scatter_plan {
  const void* src[PAVE_SCATTER_MAX_TENSORS];
  void*       dst[PAVE_SCATTER_MAX_TENSORS];
  int         row[PAVE_SCATTER_MAX_ROWS];
  int n, k, dst_rows;
  long long row_elems;
} pave_scatter_plan;
int pave_scatter_rows_f32(const pave_scatter_plan* plan, void* stream);

/*
 * Poses drawn into surfaces on the device (pavenet_amd/csrc/pave_draw.hip; the rule is DESIGN section 13), one launch
 * for n separately allocated surfaces of any sizes.  The plan is copied into the kernel's arguments.
 *   dst[i]     DEVICE, written in place.  _nv12: height[i] rows of pitch[i] bytes of Y, then height[i] / 2 rows of
 *              interleaved U, V (width and height even, pitch >= width).  _bgr: [height, width, 3] bytes, pitch[i]
 *              bytes per row (>= 3 width)
 *   kpts[i]    DEVICE [n_poses[i], K, 3] fp32 (x, y, score);  bboxes[i] [n_poses[i], 5] fp32 (x1, y1, x2, y2, score);
 *              keep[i] [n_poses[i]] int32 or NULL.  Both may be NULL where n_poses[i] == 0
 *   scale[i]   (sx, sy): a coordinate x becomes clamp((int)rintf((x / sx) * 4.f), 0, 32767) quarter pixels
 *   table[i]   which of the 4 colour tables surface i takes (NV12: one per matrix and range)
 *   color[t]   row 0: boxes; rows 1 .. 32: limbs; rows 33 .. 64: key points; 3 bytes each, stored as they are --
 *              (Y, U, V) for _nv12, (B, G, R) for _bgr
 *   edge[e]    limb e joins key points edge[e][0] and edge[e][1]
 * Pose p is drawn iff keep[p] != 0 (keep given), bboxes[p][4] > score_thr and its 2 K + 4 coordinates are finite;
 * key point k is visible iff its score > kpt_thr; a limb needs both ends.  Primitives of pose p in local order: 4 box
 * edges (draw_boxes != 0), E limbs (radius 2 thickness quarter pixels), K discs (radius 4 radius); a pixel takes the
 * colour of the covering primitive with the largest id p (4 + E + K) + local, an NV12 chroma sample the largest over
 * its 2 x 2 luma pixels.  No byte that nothing covers is written.
 * Refused with PAVE_E_ARG before any device call: a null plan, surface or pose tensor (n_poses > 0), n outside
 * 1 .. 32, width or height outside 1 .. 8192, odd NV12 sizes, a pitch below a row's bytes, n_poses outside 0 .. 4096,
 * K outside 1 .. 32, E outside 0 .. 32, an edge index >= K, thickness outside 1 .. 32, radius outside 0 .. 32, a scale
 * that is not positive and finite, a table index >= 4.  A plan that passes cannot address memory outside its
 * tensors, whatever the pose values are.
 */
#define PAVE_DRAW_MAX_SURFACES 32
#define PAVE_DRAW_MAX_K 32
#define PAVE_DRAW_MAX_E 32
#define PAVE_DRAW_MAX_TABLES 4
#define PAVE_DRAW_COLORS 65
#define PAVE_DRAW_MAX_POSES 4096
#define PAVE_DRAW_MAX_SIZE 8192
typedef struct pave_draw_plan {
  void*          dst[PAVE_DRAW_MAX_SURFACES];
  const float*   kpts[PAVE_DRAW_MAX_SURFACES];
  const float*   bboxes[PAVE_DRAW_MAX_SURFACES];
  const int32_t* keep[PAVE_DRAW_MAX_SURFACES];
  int            pitch[PAVE_DRAW_MAX_SURFACES];
  int            width[PAVE_DRAW_MAX_SURFACES];
  int            height[PAVE_DRAW_MAX_SURFACES];
  int            n_poses[PAVE_DRAW_MAX_SURFACES];
  float          scale[PAVE_DRAW_MAX_SURFACES][2];
  uint8_t        table[PAVE_DRAW_MAX_SURFACES];
  uint8_t        color[PAVE_DRAW_MAX_TABLES][PAVE_DRAW_COLORS][3];
  uint8_t        edge[PAVE_DRAW_MAX_E][2];
  int n, K, E, thickness, radius, draw_boxes;
  float score_thr, kpt_thr;
} pave_draw_plan;
int pave_draw_poses_nv12(const pave_draw_plan* plan, void* stream);
int pave_draw_poses_bgr(const pave_draw_plan* plan, void* stream);

/*
 * Poses drawn with their track ids (the same kernel source; DESIGN section 13, "Track ids in the picture"): a pose
 * whose id is >= 1 takes a colour chosen by the id and a plate with the id in decimal digits above its box.
 *   base       everything of pave_draw_plan, with the same meaning and the same refusals
 *   ids[i]     DEVICE [n_poses[i]] int32 (what pave_track_poses wrote) or NULL: surface i is drawn by base alone
 *   palette[t] rows 0 .. 31: the colour of id v is row (v - 1) % 32; row 32: the ink of the digits; 3 bytes each,
 *              stored as they are, one table per (matrix, range) pair as for color
 *   font[d]    the 5 x 7 face of digit d: 7 rows, bit 4 of a row is its left-most pixel
 *   label_scale  g in 0 .. 8: a font pixel is g x g picture pixels; 0: colours only, no labels
 *   untracked_skip  0: a pose with ids[i][p] <= 0 is drawn by base alone;  1: it is not drawn
 * A tracked pose's 4 box edges and E limbs take its palette row, its K discs keep base.color.  Its label, when
 * g >= 1, with n the number of decimal digits of the id and (X1, Y1, X2, Y2) its quantised box: ax = min(X1, X2) >> 2,
 * ay = max((min(Y1, Y2) >> 2) - 9 g, 0); the plate covers the g (6 n + 1) x 9 g pixels from (ax, ay), the ink the set
 * bits of the digits' faces, 6 g apart, from (ax + g, ay + g).  Primitive ids: plate n_poses (4 + E + K) + 2 p, ink
 * that + 1, so labels lie above every skeleton of their surface; the largest-id rule and the writes are base's.
 * Refused with PAVE_E_ARG before any device call: whatever pave_draw_poses_* refuses in base, a label_scale outside
 * 0 .. 8, an untracked_skip outside {0, 1}, a font row with bits above the low 5.  Id values need no check.
 */
#define PAVE_DRAW_PALETTE 32
typedef struct pave_draw_ids_plan {
  pave_draw_plan base;
  const int32_t* ids[PAVE_DRAW_MAX_SURFACES];
  uint8_t        palette[PAVE_DRAW_MAX_TABLES][PAVE_DRAW_PALETTE + 1][3];
  uint8_t        font[10][7];
  int label_scale, untracked_skip;
} pave_draw_ids_plan;
int pave_draw_tracks_nv12(const pave_draw_ids_plan* plan, void* stream);
int pave_draw_tracks_bgr(const pave_draw_ids_plan* plan, void* stream);

/*
 * People hidden in surfaces on the device (pavenet_amd/csrc/pave_anon.hip; the rule is DESIGN section 15,
 * integer-exact), one launch for n separately allocated surfaces of any sizes, in place.  The plan is copied into the
 * kernel's arguments.
 *   dst, kpts, bboxes, keep, pitch, width, height, n_poses, scale, table: as in pave_draw_plan, with the same
 *              quantisation and the same rule for which poses count and which key points are visible
 *   fill[t]    the 3 bytes mode 1 stores, as they are: (Y, U, V) for _nv12, (B, G, R) for _bgr
 *   head[h]    the n_head key points of the head
 *   region     0: the head (the bounding rectangle A of the visible head key points, e its larger side, grown by
 *              r = 4 margin + max((e head_scale) >> 4, (s head_min) >> 4) quarter pixels, s the larger side of the
 *              quantised box); 1: the person (A the box, r = 4 margin + ((s grow) >> 4))
 *   fallback_skip  a pose without a visible head key point under region 0 takes its person region (0) or none (1)
 *   cell       the picture is cut into cell x cell pixel cells from its origin; a cell is masked iff a region's A is
 *              within r of the rectangle of its pixels' points
 *   mode       0: every sample of a plane in a masked cell becomes (2 sum + n) / (2 n) over the cell's n original
 *              samples of that plane (NV12: Y over the pixels, U and V over the chroma samples; BGR: per channel);
 *              1: it becomes the fill colour
 * Only the bytes of masked cells are written.
 * Refused with PAVE_E_ARG before any device call: a null plan, surface or pose tensor (n_poses > 0), n outside
 * 1 .. 32, width or height outside 1 .. 8192, odd NV12 sizes, a pitch below a row's bytes, n_poses outside 0 .. 4096,
 * K outside 1 .. 32, n_head outside 0 .. 8 (0 with region 0), a head index >= K, a cell that is not 2, 4, 8, 16, 32 or
 * 64, margin outside 0 .. 64, grow, head_scale or head_min outside 0 .. 32, region, mode or fallback_skip outside
 * {0, 1}, a scale that is not positive and finite, a table index >= 4.  A plan that passes cannot address memory
 * outside its tensors, whatever the pose values are.
 */
#define PAVE_ANON_MAX_HEAD 8
#define PAVE_ANON_MAX_CELL 64
#define PAVE_ANON_MAX_MARGIN 64
#define PAVE_ANON_MAX_SIXTEENTHS 32
typedef struct pave_anon_plan {
  void*          dst[PAVE_DRAW_MAX_SURFACES];
  const float*   kpts[PAVE_DRAW_MAX_SURFACES];
  const float*   bboxes[PAVE_DRAW_MAX_SURFACES];
  const int32_t* keep[PAVE_DRAW_MAX_SURFACES];
  int            pitch[PAVE_DRAW_MAX_SURFACES];
  int            width[PAVE_DRAW_MAX_SURFACES];
  int            height[PAVE_DRAW_MAX_SURFACES];
  int            n_poses[PAVE_DRAW_MAX_SURFACES];
  float          scale[PAVE_DRAW_MAX_SURFACES][2];
  uint8_t        table[PAVE_DRAW_MAX_SURFACES];
  uint8_t        fill[PAVE_DRAW_MAX_TABLES][3];
  uint8_t        head[PAVE_ANON_MAX_HEAD];
  int n, K, n_head, region, mode, fallback_skip, cell, margin, grow, head_scale, head_min;
  float score_thr, kpt_thr;
} pave_anon_plan;
int pave_anonymize_nv12(const pave_anon_plan* plan, void* stream);
int pave_anonymize_bgr(const pave_anon_plan* plan, void* stream);

/*
 * Track ids: the poses of a frame linked to the poses of the frames before it (pavenet_amd/csrc/pave_track.hip; the
 * rule is DESIGN section 14, integer-exact), one launch for `entries` frames of any of `cameras` cameras.  The plan
 * is copied into the kernel's arguments.  One block per camera of the launch takes that camera's entries in plan
 * order: entries of one camera are in time order.
 *   kpts[i]    DEVICE [n[i], K, 3] fp32 (x, y, score);  bboxes[i] [n[i], 5] fp32;  keep[i] [n[i]] int32 or NULL
 *   ids[i]     DEVICE [n[i]] int32, out: the track id of every pose, 0 = not tracked.  kpts, bboxes and ids may be
 *              NULL where n[i] == 0 (the frame still counts: it advances the camera's clock and expires slots)
 *   camera[i]  whose state entry i reads and writes;  scale[i] (sx, sy) as in pave_draw_plan
 *   the state, DEVICE, read and written: track_id, track_last, track_area [cameras, M] int32, track_vis [cameras, M]
 *              (bit k: key point k visible), track_kpts [cameras, M, K, 2] int32 quarter pixels; frame, next_id,
 *              dropped [cameras] int32.  A slot with track_id 0 is free and its other fields are never read
 *   scratch    DEVICE, PAVE_TRACK_MAX_FRAMES x 128 x 128 int64 (4 MiB): the pair keys of every block
 *   C[k]       max(1, rint(ln(1 / match_thr) (2 sigma_k)^2 2^20)): key point k of a pair agrees iff
 *              (d2_k << 20) <= C[k] (area_d + area_t)
 * Refused with PAVE_E_ARG before any device call: a null plan, state tensor or scratch area, a null kpts, bboxes or
 * ids where n[i] > 0, entries outside 1 .. 32, n[i] outside 0 .. 128, K outside 1 .. 32, M outside 1 .. 128, cameras
 * outside 1 .. 4096, a camera index outside [0, cameras), a scale that is not positive and finite, a C[k] outside
 * [1, 2^24), min_kpts outside 1 .. K, max_age < 0.  Coordinates are clamped by the rule: a plan that passes cannot
 * address memory outside its tensors, whatever the pose values are.
 */
#define PAVE_TRACK_MAX_FRAMES 32
#define PAVE_TRACK_MAX_POSES 128
#define PAVE_TRACK_MAX_TRACKS 128
#define PAVE_TRACK_MAX_K 32
#define PAVE_TRACK_MAX_CAMERAS 4096
typedef struct pave_track_plan {
  const float*   kpts[PAVE_TRACK_MAX_FRAMES];
  const float*   bboxes[PAVE_TRACK_MAX_FRAMES];
  const int32_t* keep[PAVE_TRACK_MAX_FRAMES];
  int32_t*       ids[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  float          scale[PAVE_TRACK_MAX_FRAMES][2];
  int32_t*  track_id;
  int32_t*  track_last;
  int32_t*  track_kpts;
  uint32_t* track_vis;
  int32_t*  track_area;
  int32_t*  frame;
  int32_t*  next_id;
  int32_t*  dropped;
  long long* scratch;
  int   C[PAVE_TRACK_MAX_K];
  int entries, cameras, M, K, min_kpts, max_age;
  float score_thr, kpt_thr;
} pave_track_plan;
int pave_track_poses(const pave_track_plan* plan, void* stream);

/*
 * Track ids with a constant-velocity motion model (the same kernel source; DESIGN section 14, "Motion"): a slot is
 * compared where it is predicted to be, not where it was, and keeps a velocity that every match refreshes.
 *   base         everything of pave_track_plan, with the same meaning and the same refusals
 *   track_vel    DEVICE [cameras, M, 2] int32, read and written: (vx, vy) in 1/16 quarter pixel per frame
 *   track_hits   DEVICE [cameras, M] int32, read and written: the matches of the slot's track, its birth included
 *                (1: no velocity measured yet), saturating at 32767.  Neither is read in a free slot
 *   gain         1 .. 16, sixteenths: the weight of the newest measured velocity
 *   max_predict  0 .. 255: the most frames a slot is extrapolated over
 *   new_gate     1 .. 16: the factor on C[k] in the agreement test of a slot with hits == 1
 * With gap = frame - last and g = min(gap, max_predict) a live slot's point is P = clamp(kpts + ((vel g + 8) >> 4), 0,
 * 32767) and takes the place of kpts in the pair score; a match measures m = floor((32 S + n gap) / (2 n gap)), S the
 * sum of (detection - stored point) over the n key points visible in both, and stores vel = m when hits == 1, else
 * clamp((gain m + (16 - gain) vel + 8) >> 4, -32768, 32767); a birth stores vel = 0, hits = 1.
 * Refused with PAVE_E_ARG before any device call: whatever pave_track_poses refuses in base, a null track_vel or
 * track_hits, gain outside 1 .. 16, max_predict outside 0 .. 255, new_gate outside 1 .. 16.  Predictions are
 * clamped by the rule and velocities by their stores: a plan that passes cannot address memory outside its tensors,
 * whatever the pose values and the stored velocities are.
 */
typedef struct pave_track_motion_plan {
  pave_track_plan base;
  int32_t* track_vel;
  int32_t* track_hits;
  int gain, max_predict, new_gate;
} pave_track_motion_plan;
int pave_track_poses_motion(const pave_track_motion_plan* plan, void* stream);

/*
 * Steady poses: a per-track adaptive exponential filter on the key points and box corners of tracked poses
 * (pavenet_amd/csrc/pave_smooth.hip; the rule is DESIGN section 16, integer-exact), one launch for `entries` frames
 * of any of `cameras` cameras.  The plan is copied into the kernel's arguments.  One block per camera of the launch
 * takes that camera's entries in plan order: entries of one camera are in time order.
 *   kpts[i], bboxes[i], keep[i], n[i], camera[i], scale[i]   as in pave_track_plan
 *   ids[i]         DEVICE [n[i]] int32, in: the track id of every pose (what pave_track_poses wrote, or any ids);
 *                  a pose is filtered iff it is valid, its id is >= 1, no valid pose before it in the frame has the
 *                  same id, and a slot holds or can take the id
 *   out_kpts[i]    DEVICE [n[i], K, 3] fp32, out;  out_bboxes[i] [n[i], 5] fp32, out: the poses in ORIGINAL-IMAGE
 *                  pixels (scale (1, 1) downstream), coordinates multiples of 1/64: the filter's position of a
 *                  filtered pose, the quarter-pixel quantisation of any other pose with finite coordinates, the quiet
 *                  NaN 0x7fc00000 in a pose with a coordinate that is not finite; scores are copied bit for bit.
 *                  Neither may overlap an input.  All six may be NULL where n[i] == 0 (the frame still counts)
 *   the state, DEVICE, read and written: slot_id, slot_last [cameras, S] int32 (id 0: a free slot, its other fields
 *                  are never read), slot_pos, slot_vel [cameras, S, K + 2, 2] int32 (1/64 pixel, 1/64 pixel per
 *                  frame; the K key points, then the box corners; a point with pos x < 0 is uninitialised and its
 *                  other three values are never read); frame, dropped [cameras] int32
 *   alpha_min      1 .. 256: the filter's gain at rest, in 1/256
 *   beta           0 .. 4096: how fast the gain rises with a point's speed (1/16 per 1/1024 of the pose's size per
 *                  frame)
 *   velocity_gain  1 .. 16, sixteenths: the weight of the newest measured velocity of a point
 * Refused with PAVE_E_ARG before any device call: a null plan or state tensor, a null kpts, bboxes, ids, out_kpts or
 * out_bboxes where n[i] > 0, entries outside 1 .. 32, n[i] outside 0 .. 128, K outside 1 .. 32, S outside 1 .. 128,
 * cameras outside 1 .. 4096, a camera index outside [0, cameras), a scale that is not positive and finite, alpha_min,
 * beta or velocity_gain outside its range, max_age < 0.  Slot indices come from the plan's counts and the arithmetic
 * is 64-bit on whatever int32 the state holds: a plan that passes cannot address memory outside its tensors, whatever
 * the poses, the ids and the stored state are.
 */
typedef struct pave_smooth_plan {
  const float*   kpts[PAVE_TRACK_MAX_FRAMES];
  const float*   bboxes[PAVE_TRACK_MAX_FRAMES];
  const int32_t* keep[PAVE_TRACK_MAX_FRAMES];
  const int32_t* ids[PAVE_TRACK_MAX_FRAMES];
  float*         out_kpts[PAVE_TRACK_MAX_FRAMES];
  float*         out_bboxes[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  float          scale[PAVE_TRACK_MAX_FRAMES][2];
  int32_t* slot_id;
  int32_t* slot_last;
  int32_t* slot_pos;
  int32_t* slot_vel;
  int32_t* frame;
  int32_t* dropped;
  int entries, cameras, S, K, alpha_min, beta, velocity_gain, max_age;
  float score_thr, kpt_thr;
} pave_smooth_plan;
int pave_smooth_poses(const pave_smooth_plan* plan, void* stream);

/*
 * Zones and counting lines: which tracks are inside which polygon, for how long, and which directed line a track
 * crossed (pavenet_amd/csrc/pave_zones.hip; the rule is DESIGN section 17, integer-exact), one launch for `entries`
 * frames of any of `cameras` cameras.  The plan is copied into the kernel's arguments.  One block per camera of the
 * launch takes that camera's entries in plan order: entries of one camera are in time order.
 *   kpts[i], bboxes[i], keep[i], n[i], camera[i], scale[i]   as in pave_track_plan;  ids[i] as in pave_smooth_plan
 *   out_zones[i]     DEVICE [n[i]] int32, out: bit z set iff the pose's track is inside zone z (0: takes no part)
 *   out_dwell[i]     DEVICE [n[i], 8] int32, out: frames the track has been inside zone z, 0 where it is not
 *   out_events[i]    DEVICE [max_events, 5] int32, out: the frame's events (kind, index, id, pose, frame) in the
 *                    rule's fixed order, the first max_events of them; rows past the count are zero
 *   out_n_events[i]  DEVICE [1] int32, out: ALL events of the frame (it may exceed max_events)
 *                    out_zones and out_dwell may be NULL where n[i] == 0 (the frame still counts)
 *   the state, DEVICE int32, read and written: slot_id, slot_last, slot_inside, slot_alerted [cameras, S] (id 0: a
 *                    free slot, its other fields are never read), slot_pos [cameras, S, 2] (1/8 pixel), slot_streak,
 *                    slot_since [cameras, S, 8]; frame, dropped [cameras];
 *                    counters [cameras, PAVE_ZONE_COUNTER_WORDS]: occupancy, entered, exited, appeared, vanished
 *                    [8] at PAVE_ZONE_CNT_*, crossed [8, 2] (forward, backward) at PAVE_ZONE_CNT_CROSSED
 *   geometry         DEVICE [cameras, PAVE_ZONE_GEOM_WORDS] int32, read only: the number of zones and of lines, the
 *                    vertex count and dwell_frames of every zone, the zones' vertices [8, 16, 2] and the lines' ends
 *                    [8, 2, 2] (A, B), in 1/8 pixel, at PAVE_ZONE_GEOM_*.  Counts are clamped to 0 .. 8 and 0 .. 16
 *                    as they are read
 *   anchor           PAVE_ZONE_ANCHOR_FEET | _BOX | _CENTRE;  anchor_kpt[0 .. n_anchor): the key points of 'feet'
 *   min_frames       1 .. 255: the frames a raw inside test must disagree before the bit flips
 * Refused with PAVE_E_ARG before any device call: whatever pave_smooth_poses refuses in the fields of the same name
 * (a null plan or state tensor, a null kpts, bboxes or ids where n[i] > 0, entries outside 1 .. 32, n[i] outside
 * 0 .. 128, K outside 1 .. 32, S outside 1 .. 128, cameras outside 1 .. 4096, a camera index outside [0, cameras), a
 * scale that is not positive and finite, max_age < 0), a null counters or geometry tensor, a null out_zones or
 * out_dwell where n[i] > 0, a null out_events or out_n_events, min_frames outside 1 .. 255, max_events outside
 * 1 .. 4096, an anchor outside 0 .. 2, n_anchor outside 0 .. 4, an anchor_kpt outside [0, K).  Every loop bound is
 * from the plan or the maxima below: a plan that passes cannot address memory outside its tensors, whatever the
 * poses, the ids, the stored state and the geometry hold.
 */
#define PAVE_ZONE_MAX_ZONES 8
#define PAVE_ZONE_MAX_LINES 8
#define PAVE_ZONE_MAX_VERTICES 16
#define PAVE_ZONE_MAX_ANCHOR_KPTS 4
#define PAVE_ZONE_MAX_EVENTS 4096
#define PAVE_ZONE_EVENT_WORDS 5
#define PAVE_ZONE_ENTER 1
#define PAVE_ZONE_EXIT 2
#define PAVE_ZONE_DWELL 3
#define PAVE_ZONE_APPEAR 4
#define PAVE_ZONE_VANISH 5
#define PAVE_ZONE_CROSS_FWD 6
#define PAVE_ZONE_CROSS_BACK 7
#define PAVE_ZONE_ANCHOR_FEET 0
#define PAVE_ZONE_ANCHOR_BOX 1
#define PAVE_ZONE_ANCHOR_CENTRE 2
#define PAVE_ZONE_CNT_OCCUPANCY 0
#define PAVE_ZONE_CNT_ENTERED 8
#define PAVE_ZONE_CNT_EXITED 16
#define PAVE_ZONE_CNT_APPEARED 24
#define PAVE_ZONE_CNT_VANISHED 32
#define PAVE_ZONE_CNT_CROSSED 40
#define PAVE_ZONE_COUNTER_WORDS 56
#define PAVE_ZONE_GEOM_NZONES 0
#define PAVE_ZONE_GEOM_NLINES 1
#define PAVE_ZONE_GEOM_NVERT 2
#define PAVE_ZONE_GEOM_DWELL 10
#define PAVE_ZONE_GEOM_ZONES 18
#define PAVE_ZONE_GEOM_LINES 274
#define PAVE_ZONE_GEOM_WORDS 306
typedef struct pave_zone_plan {
  const float*   kpts[PAVE_TRACK_MAX_FRAMES];
  const float*   bboxes[PAVE_TRACK_MAX_FRAMES];
  const int32_t* keep[PAVE_TRACK_MAX_FRAMES];
  const int32_t* ids[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_zones[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_dwell[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_events[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_n_events[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  float          scale[PAVE_TRACK_MAX_FRAMES][2];
  int32_t* slot_id;
  int32_t* slot_last;
  int32_t* slot_pos;
  int32_t* slot_inside;
  int32_t* slot_alerted;
  int32_t* slot_streak;
  int32_t* slot_since;
  int32_t* frame;
  int32_t* dropped;
  int32_t* counters;
  const int32_t* geometry;
  int anchor_kpt[PAVE_ZONE_MAX_ANCHOR_KPTS];
  int entries, cameras, S, K, anchor, n_anchor, min_frames, max_events, max_age;
  float score_thr, kpt_thr;
} pave_zone_plan;
int pave_zone_events(const pave_zone_plan* plan, void* stream);

/*
 * Zones, counting lines and their live counts drawn into surfaces on the device (pavenet_amd/csrc/pave_overlay.hip;
 * the rule is DESIGN section 19, integer-exact), one launch for n separately allocated surfaces of any sizes, in
 * place.  The plan is copied into the kernel's arguments.  The monitor's tensors are only read.
 *   dst, pitch, width, height, table: as in pave_draw_plan;  camera[i]: the camera whose geometry surface i shows
 *   geometry, counters, slot_id, slot_alerted, slot_inside: DEVICE, the tensors of the same names of pave_zone_plan
 *              ([cameras, PAVE_ZONE_GEOM_WORDS], [cameras, PAVE_ZONE_COUNTER_WORDS] and three [cameras, S]).  Counts
 *              are clamped to 0 .. 8 and 0 .. 16 and vertex words to 0 .. 65535 as they are read; a zone without
 *              vertices is not drawn
 *   color[t]   rows 0 .. 7: the zones; 8 .. 15: the lines; 16: an alerted zone; 17: the labels' ink; 3 bytes each,
 *              stored or blended as they are -- (Y, U, V) for _nv12, (B, G, R) for _bgr
 *   alpha, alpha_occupied, alpha_alert: 0 .. 256, the weight of a zone's colour in its fill by the zone's state
 *   outline    0 .. 32 px: a zone's edges as capsules of radius 2 outline quarter pixels (0: none)
 *   thickness  1 .. 32 px: a line's capsule, radius 2 thickness;  arrow 0 .. 255 px: the length of its direction stem
 *   label_scale  g in 0 .. 8: a font pixel is g x g picture pixels; 0: no labels
 *   zone_label PAVE_ZONE_LABEL_NONE | _OCCUPANCY | _ENTERED;  line_label PAVE_LINE_LABEL_NONE | _NET | _FORWARD | _BACKWARD
 *   font[d]    the 5 x 7 faces of the digits 0 .. 9 and, d = 10, of the minus sign: 7 rows, bit 4 the left-most pixel
 * Pixel (px, py) is tinted by zone z iff the point (8 px, 8 py) is inside it by pave_zone_events' own test:
 * out = (src (256 - a) + col a + 128) >> 8 per byte, zones in ascending index; an NV12 chroma sample once per zone
 * with a_c = (a n + 2) >> 2 for its n luma pixels inside.  Over the fills lie opaque primitives, the largest id
 * winning as in pave_draw_plan, on quarter-pixel vertices Q = G >> 1: zone edges (id 16 z + e), lines (128 + l),
 * stems (136 + l), zone plates and their ink (144 + 2 z, + 1), line plates and their ink (160 + 2 l, + 1).  No byte
 * that neither a fill with a positive alpha nor a primitive covers is written.
 * Refused with PAVE_E_ARG before any device call: a null plan, surface or monitor tensor, n outside 1 .. 32, width or
 * height outside 1 .. 8192, odd NV12 sizes, a pitch below a row's bytes, a table index >= 4, cameras outside
 * 1 .. 4096, a camera outside [0, cameras), S outside 1 .. 128, an alpha outside 0 .. 256, outline outside 0 .. 32,
 * thickness outside 1 .. 32, arrow outside 0 .. 255, label_scale outside 0 .. 8, zone_label outside 0 .. 2, line_label
 * outside 0 .. 3, a font row with bits above the low 5.  A plan that passes cannot address memory outside its
 * tensors, whatever the geometry, the counters and the state hold.
 */
#define PAVE_ZONE_DRAW_COLORS 18
#define PAVE_ZONE_DRAW_ALERT 16
#define PAVE_ZONE_DRAW_INK 17
#define PAVE_ZONE_DRAW_FACES 11
#define PAVE_ZONE_LABEL_NONE 0
#define PAVE_ZONE_LABEL_OCCUPANCY 1
#define PAVE_ZONE_LABEL_ENTERED 2
#define PAVE_LINE_LABEL_NONE 0
#define PAVE_LINE_LABEL_NET 1
#define PAVE_LINE_LABEL_FORWARD 2
#define PAVE_LINE_LABEL_BACKWARD 3
typedef struct pave_zone_draw_plan {
  void*          dst[PAVE_DRAW_MAX_SURFACES];
  int            pitch[PAVE_DRAW_MAX_SURFACES];
  int            width[PAVE_DRAW_MAX_SURFACES];
  int            height[PAVE_DRAW_MAX_SURFACES];
  int            camera[PAVE_DRAW_MAX_SURFACES];
  uint8_t        table[PAVE_DRAW_MAX_SURFACES];
  const int32_t* geometry;
  const int32_t* counters;
  const int32_t* slot_id;
  const int32_t* slot_alerted;
  const int32_t* slot_inside;
  uint8_t        color[PAVE_DRAW_MAX_TABLES][PAVE_ZONE_DRAW_COLORS][3];
  uint8_t        font[PAVE_ZONE_DRAW_FACES][7];
  int n, cameras, S, alpha, alpha_occupied, alpha_alert, outline, thickness, arrow, label_scale, zone_label, line_label;
} pave_zone_draw_plan;
int pave_draw_zones_nv12(const pave_zone_draw_plan* plan, void* stream);
int pave_draw_zones_bgr(const pave_zone_draw_plan* plan, void* stream);

/*
 * The same person again: a colour descriptor per pose read from the pixels under it, and a gallery per camera that
 * maps track ids to person ids which survive a gap (pavenet_amd/csrc/pave_reid.hip; the rule is DESIGN section 18,
 * integer-exact).  The plans are copied into the kernels' arguments; the surfaces are read only.
 *
 * pave_reid_describe_nv12 / _bgr: one launch, one workgroup per (entry, pose, region); region 0 the torso, 1 the legs.
 *   src[i]     DEVICE uint8, read only: an NV12 surface [height * 3 / 2, pitch] whose first `width` columns are the
 *              picture, or a BGR picture [height, width, 3] with pitch = 3 width
 *   kpts[i], bboxes[i], keep[i], n[i], scale[i]   as in pave_track_plan
 *   hist[i]    DEVICE [n[i], 2, 256] int32, out: the normalised descriptor (h[b] * 128) / count of every region, bin
 *              (y * 8 + u) * 8 + v; zero where the region is invalid
 *   count[i]   DEVICE [n[i], 2] int32, out: the samples of the region, 0 where it is invalid (a pose without keep,
 *              with a box score <= score_thr or a coordinate that is not finite; no visible key point of one of its
 *              two parts and no fallback; wholly off the picture; fewer than PAVE_REID_MIN_SAMPLES samples)
 *   part[r][h][0 .. n_part[r][h])   the key points of region r: h = 0 its upper part (torso: shoulders, legs: hips),
 *              h = 1 its lower part (hips, knees)
 * pave_reid_update_nv12 / _bgr: two launches, that one into hist and count (here scratch areas of the caller), then
 * one workgroup per camera of the launch, which takes that camera's entries in plan order: entries of one camera are
 * in time order.
 *   ids[i]     DEVICE [n[i]] int32, in: the track id of every pose;  camera[i] whose gallery entry i reads and writes
 *   out_ids[i] DEVICE [n[i]] int32, out: the person id of every pose, 0 where it takes no part or was dropped
 *   out_sim[i] DEVICE [n[i]] int32, out: the score at which the pose was re-identified in this frame, else 0
 *   the gallery, DEVICE int32, read and written: person, track, last [cameras, S] (person 0: a free slot, its other
 *              fields are never read), hits [cameras, S, 2], hist [cameras, S, 2, 256]; frame, next, dropped [cameras]
 *   pairs      DEVICE, PAVE_TRACK_MAX_FRAMES x 128 x 128 int32 (2 MiB): the pair scores of every block
 *   match_thr  0 .. PAVE_REID_NEVER (which no score reaches);  min_hits 1 .. PAVE_REID_MAX_HITS;  gain 1 .. 16
 * Refused with PAVE_E_ARG before any device call: a null plan, a null surface, hist or count, a null kpts or bboxes
 * where n[i] > 0, entries outside 1 .. 32, n[i] outside 0 .. 128, K outside 1 .. 32, width or height outside
 * 1 .. 8192, odd NV12 sizes, a pitch below a row's bytes (BGR: other than 3 width), a scale that is not positive and
 * finite, an n_part outside 0 .. 4, a part index outside [0, K); by the update entries also a null ids, out_ids or
 * out_sim where n[i] > 0, a null gallery tensor or pairs area, S outside 1 .. 128, cameras outside 1 .. 4096, a
 * camera index outside [0, cameras), max_lost < 0, match_thr, min_hits or gain outside its range.  Sample addresses
 * are clipped to the picture and slot indices are loop counters of the plan's counts: a plan that passes cannot
 * address memory outside its tensors, whatever the poses, ids, state and pixels hold.
 */
#define PAVE_REID_BINS 256
#define PAVE_REID_CAP 1024
#define PAVE_REID_MIN_SAMPLES 16
#define PAVE_REID_MAX_PART 4
#define PAVE_REID_MAX_HITS 32767
#define PAVE_REID_NEVER 65537
typedef struct pave_reid_describe_plan {
  const uint8_t* src[PAVE_TRACK_MAX_FRAMES];
  const float*   kpts[PAVE_TRACK_MAX_FRAMES];
  const float*   bboxes[PAVE_TRACK_MAX_FRAMES];
  const int32_t* keep[PAVE_TRACK_MAX_FRAMES];
  int32_t*       hist[PAVE_TRACK_MAX_FRAMES];
  int32_t*       count[PAVE_TRACK_MAX_FRAMES];
  int            pitch[PAVE_TRACK_MAX_FRAMES];
  int            width[PAVE_TRACK_MAX_FRAMES];
  int            height[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  float          scale[PAVE_TRACK_MAX_FRAMES][2];
  int part[2][2][PAVE_REID_MAX_PART];
  int n_part[2][2];
  int entries, K;
  float score_thr, kpt_thr;
} pave_reid_describe_plan;
typedef struct pave_reid_plan {
  pave_reid_describe_plan d;
  const int32_t* ids[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_ids[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_sim[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  int32_t* person;
  int32_t* track;
  int32_t* last;
  int32_t* hits;
  int32_t* hist;
  int32_t* frame;
  int32_t* next;
  int32_t* dropped;
  int32_t* pairs;
  int cameras, S, max_lost, match_thr, min_hits, gain;
} pave_reid_plan;
int pave_reid_describe_nv12(const pave_reid_describe_plan* plan, void* stream);
int pave_reid_describe_bgr(const pave_reid_describe_plan* plan, void* stream);
int pave_reid_update_nv12(const pave_reid_plan* plan, void* stream);
int pave_reid_update_bgr(const pave_reid_plan* plan, void* stream);

/*
 * Postures and falls: the class of every tracked pose from its trunk and legs, debounced per track id, with the
 * posture changes, falls, people who stay down and raised hands of the frame (pavenet_amd/csrc/pave_posture.hip; the
 * rule is DESIGN section 20, integer-exact), one launch for `entries` frames of any of `cameras` cameras.  The plan is
 * copied into the kernel's arguments.  One block per camera of the launch takes that camera's entries in plan order:
 * entries of one camera are in time order.
 *   kpts[i], bboxes[i], keep[i], n[i], camera[i], scale[i]   as in pave_track_plan;  ids[i] as in pave_smooth_plan
 *   out_posture[i]   DEVICE [n[i]] int32, out: the debounced posture of the pose's track, PAVE_POSTURE_UNKNOWN ..
 *                    _LYING, or -1 where the pose takes no part
 *   out_raw[i]       DEVICE [n[i]] int32, out: the class of this frame alone, or -1
 *   out_hands[i]     DEVICE [n[i]] int32, out: bit w set iff wrist w of the part `wrists` is raised in this frame
 *   out_since[i]     DEVICE [n[i]] int32, out: the frames the track has spent in its posture (0: takes no part)
 *   out_events[i]    DEVICE [max_events, 5] int32, out: the frame's events (kind, index, id, pose, frame) in the
 *                    rule's fixed order, the first max_events of them; rows past the count are zero.  index: the new
 *                    class (POSTURE), frame - upright (FALL), the frames lying (DOWN), the raw wrist mask (HANDS_*)
 *   out_n_events[i]  DEVICE [1] int32, out: ALL events of the frame (it may exceed max_events)
 *                    out_posture, out_raw, out_hands and out_since may be NULL where n[i] == 0 (the frame still counts)
 *   the state, DEVICE int32, read and written: slot_id, slot_last, slot_posture, slot_since, slot_upright (the last
 *                    frame the slot was seen UPRIGHT, 0: never), slot_streak, slot_alerted, slot_hands (0 | 1),
 *                    slot_hand_streak [cameras, S] (id 0: a free slot, its other fields are never read); frame,
 *                    dropped [cameras]; counters [cameras, PAVE_POSTURE_COUNTER_WORDS]: the live slots per posture
 *                    [5] at PAVE_POSTURE_CNT_NOW, the live slots with a raised hand, and the running totals of falls
 *                    and of DOWN events
 *   part[p][0 .. n_part[p])   the key points of part p = PAVE_POSTURE_PART_SHOULDERS | _HIPS | _ANKLES | _WRISTS.
 *                    n_part is clamped to 0 .. 4 and an index to [0, K) as they are read
 *   min_frames       1 .. 255: the frames a raw class (a raw hand bit) must disagree before the posture (the bit) follows
 *   lean, flat       1 .. 255, sixteenths of a slope: UPRIGHT up to |dx| / dy = lean / 16, LYING up to |dy| / |dx| = flat / 16
 *   squat            0 .. 255, sixteenths of the trunk's height: LOW iff the ankles are less than that below the hips
 *                    (0: no LOW)
 *   hand_up          PAVE_POSTURE_HANDS_OFF, or 0 .. 255, sixteenths of the trunk's height a wrist is above the shoulders
 *   fall_window      0 .. 2^30: LYING within so many frames of UPRIGHT is a FALL
 *   down_frames      0 .. 2^30: the frames lying after which DOWN is reported once (0: never)
 * Refused with PAVE_E_ARG before any device call: whatever pave_zone_events refuses in the fields of the same name (a
 * null plan or state tensor, a null kpts, bboxes or ids where n[i] > 0, entries outside 1 .. 32, n[i] outside
 * 0 .. 128, K outside 1 .. 32, S outside 1 .. 128, cameras outside 1 .. 4096, a camera index outside [0, cameras), a
 * scale that is not positive and finite, max_age < 0, a null counters tensor, a null out_events or out_n_events,
 * min_frames outside 1 .. 255, max_events outside 1 .. 4096), a null out_posture, out_raw, out_hands or out_since
 * where n[i] > 0, lean or flat outside 1 .. 255, squat outside 0 .. 255, hand_up outside -1 .. 255, fall_window or
 * down_frames outside 0 .. 2^30, an n_part outside 0 .. 4, a part index outside [0, K).  Every loop bound is from the
 * plan or the maxima below: a plan that passes cannot address memory outside its tensors, whatever the poses, the ids
 * and the stored state hold.
 */
#define PAVE_POSTURE_UNKNOWN 0
#define PAVE_POSTURE_UPRIGHT 1
#define PAVE_POSTURE_LOW 2
#define PAVE_POSTURE_LEANING 3
#define PAVE_POSTURE_LYING 4
#define PAVE_POSTURE_CLASSES 5
#define PAVE_POSTURE_EV_POSTURE 1
#define PAVE_POSTURE_EV_FALL 2
#define PAVE_POSTURE_EV_DOWN 3
#define PAVE_POSTURE_EV_HANDS_UP 4
#define PAVE_POSTURE_EV_HANDS_DOWN 5
#define PAVE_POSTURE_PART_SHOULDERS 0
#define PAVE_POSTURE_PART_HIPS 1
#define PAVE_POSTURE_PART_ANKLES 2
#define PAVE_POSTURE_PART_WRISTS 3
#define PAVE_POSTURE_PARTS 4
#define PAVE_POSTURE_MAX_PART 4
#define PAVE_POSTURE_MAX_EVENTS 4096
#define PAVE_POSTURE_EVENT_WORDS 5
#define PAVE_POSTURE_MAX_SLOPE 255
#define PAVE_POSTURE_MAX_WAIT 1073741824
#define PAVE_POSTURE_HANDS_OFF (-1)
#define PAVE_POSTURE_CNT_NOW 0
#define PAVE_POSTURE_CNT_HANDS_UP 5
#define PAVE_POSTURE_CNT_FALLS 6
#define PAVE_POSTURE_CNT_DOWNS 7
#define PAVE_POSTURE_COUNTER_WORDS 8
typedef struct pave_posture_plan {
  const float*   kpts[PAVE_TRACK_MAX_FRAMES];
  const float*   bboxes[PAVE_TRACK_MAX_FRAMES];
  const int32_t* keep[PAVE_TRACK_MAX_FRAMES];
  const int32_t* ids[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_posture[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_raw[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_hands[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_since[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_events[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_n_events[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  float          scale[PAVE_TRACK_MAX_FRAMES][2];
  int32_t* slot_id;
  int32_t* slot_last;
  int32_t* slot_posture;
  int32_t* slot_since;
  int32_t* slot_upright;
  int32_t* slot_streak;
  int32_t* slot_alerted;
  int32_t* slot_hands;
  int32_t* slot_hand_streak;
  int32_t* frame;
  int32_t* dropped;
  int32_t* counters;
  int part[PAVE_POSTURE_PARTS][PAVE_POSTURE_MAX_PART];
  int n_part[PAVE_POSTURE_PARTS];
  int entries, cameras, S, K, min_frames, lean, flat, squat, hand_up, fall_window, down_frames, max_events, max_age;
  float score_thr, kpt_thr;
} pave_posture_plan;
int pave_posture_events(const pave_posture_plan* plan, void* stream);

/*
 * Footfall heat maps: where tracked people stood and walked, accumulated per camera on a grid of cells, and the map
 * as a colour overlay (pavenet_amd/csrc/pave_heat.hip; the rules are DESIGN section 21, integer-exact).  The plans are
 * copied into the kernels' arguments.
 *
 * pave_heat_update: one launch for `entries` frames of any of `cameras` cameras; one block per camera of the launch
 * takes that camera's entries in plan order, as pave_zone_events does: entries of one camera are in time order.
 *   kpts[i], bboxes[i], keep[i], ids[i], n[i], camera[i], scale[i], anchor, anchor_kpt, n_anchor, S, K, max_age,
 *   score_thr, kpt_thr   as in pave_zone_plan: the same poses take part and stand on the same 1/8-pixel anchor
 *   out_cell[i]      DEVICE [n[i]] int32, out: the pose's cell gy Gw + gx, -1 if it takes no part or is off the map
 *   out_dwell[i], out_visits[i]   DEVICE [n[i]] int32, out: the two maps at that cell after the frame, else 0
 *                    (all three may be NULL where n[i] == 0: the frame still counts)
 *   the state, DEVICE int32, read and written: slot_id, slot_last, slot_cell [cameras, S] (id 0: a free slot, its
 *                    other fields are never read; cell -1: off the map); frame, dropped [cameras]; peak [cameras, 2]
 *                    (the maxima of dwell and visits); dwell, visits [cameras, Gh, Gw], Gw = ceil(width / cell),
 *                    Gh = ceil(height / cell)
 *   width, height    the map's size in original-image pixels, 1 .. 8192; cell 4 | 8 | 16 | 32 | 64; Gw, Gh <= 512
 *   radius           0 .. 3: a pose adds (r + 1 - |dx|)(r + 1 - |dy|) to the cells within r of its own
 *   half_life        0 .. 2^18: every half_life frames both maps and peak are halved (0: never)
 * Refused with PAVE_E_ARG before any device call: whatever pave_zone_events refuses in the fields of the same name, a
 * null map, peak or output tensor, width or height outside 1 .. 8192, a cell that is not one of the five, a grid above
 * 512 cells a side, radius outside 0 .. 3, half_life outside 0 .. 2^18.
 *
 * pave_draw_heat_nv12 / _bgr: one launch for n separately allocated surfaces, in place; the maps are only read.
 *   dst, pitch, width, height, table, camera: as in pave_zone_draw_plan
 *   map        DEVICE [cameras, Gh, Gw] int32: the map that is drawn;  peak: DEVICE [cameras, 2] int32;  source:
 *              PAVE_HEAT_DWELL | PAVE_HEAT_VISITS, the word of peak that belongs to map
 *   palette    DEVICE [tables, 256, 3] bytes, stored or blended as they are: (Y, U, V) for _nv12, (B, G, R) for _bgr
 *   map_width, map_height, cell: the map's size and cell as in pave_heat_plan
 *   full_scale 1 .. 2^31 - 1, or 0: max(peak[camera][source], 1), read by the kernel
 *   alpha_max  0 .. 256;  floor 0 .. 255;  smooth 0 | 1
 * level = min(255, 255 max(v, 0) / scale) per cell (int64), taken from the pixel's own cell or (smooth) bilinear
 * between cell centres; a = level < floor ? 0 : (alpha_max level + 128) >> 8; out = (src (256 - a) + palette[level] a
 * + 128) >> 8 per byte; an NV12 chroma sample once, from the level at its block's centre.  A byte with a == 0, a pixel
 * at or beyond the map's size and padding are never written.
 * Refused with PAVE_E_ARG before any device call: a null plan, surface, map, peak or palette, n outside 1 .. 32, width
 * or height outside 1 .. 8192, odd NV12 sizes, a pitch below a row's bytes, tables outside 1 .. 8, a table index >=
 * tables, cameras outside 1 .. 4096, a camera outside [0, cameras), a map size, cell or grid as above, source outside
 * 0 .. 1, full_scale < 0, alpha_max outside 0 .. 256, floor outside 0 .. 255, smooth outside 0 .. 1.
 * Every cell index is clamped to the grid where it is formed and peak is clamped to >= 1 where it is read: a plan that
 * passes cannot address memory outside its tensors, whatever the poses, the state and the maps hold.
 */
#define PAVE_HEAT_MAX_GRID 512
#define PAVE_HEAT_MAX_RADIUS 3
#define PAVE_HEAT_MAX_HALF_LIFE 262144
#define PAVE_HEAT_MAX_TABLES 8
#define PAVE_HEAT_DWELL 0
#define PAVE_HEAT_VISITS 1
typedef struct pave_heat_plan {
  const float*   kpts[PAVE_TRACK_MAX_FRAMES];
  const float*   bboxes[PAVE_TRACK_MAX_FRAMES];
  const int32_t* keep[PAVE_TRACK_MAX_FRAMES];
  const int32_t* ids[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_cell[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_dwell[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_visits[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  float          scale[PAVE_TRACK_MAX_FRAMES][2];
  int32_t* slot_id;
  int32_t* slot_last;
  int32_t* slot_cell;
  int32_t* frame;
  int32_t* dropped;
  int32_t* peak;
  int32_t* dwell;
  int32_t* visits;
  int anchor_kpt[PAVE_ZONE_MAX_ANCHOR_KPTS];
  int entries, cameras, S, K, anchor, n_anchor, width, height, cell, radius, half_life, max_age;
  float score_thr, kpt_thr;
} pave_heat_plan;
int pave_heat_update(const pave_heat_plan* plan, void* stream);

typedef struct pave_heat_draw_plan {
  void*          dst[PAVE_DRAW_MAX_SURFACES];
  int            pitch[PAVE_DRAW_MAX_SURFACES];
  int            width[PAVE_DRAW_MAX_SURFACES];
  int            height[PAVE_DRAW_MAX_SURFACES];
  int            camera[PAVE_DRAW_MAX_SURFACES];
  uint8_t        table[PAVE_DRAW_MAX_SURFACES];
  const int32_t* map;
  const int32_t* peak;
  const uint8_t* palette;
  int n, cameras, tables, map_width, map_height, cell, source, full_scale, alpha_max, floor, smooth;
} pave_heat_draw_plan;
int pave_draw_heat_nv12(const pave_heat_draw_plan* plan, void* stream);
int pave_draw_heat_bgr(const pave_heat_draw_plan* plan, void* stream);

/*
 * Track trails: the recent path of every tracked person, kept per camera in a ring of points per slot, and the paths
 * as tapered lines in the picture (pavenet_amd/csrc/pave_trails.hip; the rules are DESIGN section 22, integer-exact).
 * The plans are copied into the kernels' arguments.
 *
 * pave_trail_update: one launch for `entries` frames of any of `cameras` cameras; one block per camera of the launch
 * takes that camera's entries in plan order, as pave_zone_events does: entries of one camera are in time order.
 *   kpts[i], bboxes[i], keep[i], ids[i], n[i], camera[i], scale[i], anchor, anchor_kpt, n_anchor, S, K, max_age,
 *   score_thr, kpt_thr   as in pave_zone_plan: the same poses take part and stand on the same 1/8-pixel anchor
 *   out_count[i], out_span[i], out_dist[i], out_path[i]   DEVICE [n[i]] int32, out: the committed points of the pose's
 *                    slot, the frames since the oldest of them, floor |pos - oldest| and the length along the points
 *                    to pos (1/8 pixel); 0 for a pose that takes no part (all four may be NULL where n[i] == 0)
 *   the state, DEVICE int32, read and written: slot_id, slot_last, slot_head, slot_count [cameras, S] (id 0: a free
 *                    slot, its other fields are never read), slot_pos [cameras, S, 2], slot_box [cameras, S, 4] (x0,
 *                    y0, x1, y1 over the committed points and pos), pts [cameras, S, L, 2], when [cameras, S, L] (the
 *                    ring: point `head` is the newest, `count` of them are committed); frame, dropped [cameras]
 *   L                1 .. PAVE_TRAIL_MAX_POINTS: points of a ring
 *   stride           1 .. 255: frames between two commits at the least
 *   min_step         0 .. 65535: 1/8 pixels (Chebyshev) between two committed points at the least
 * Refused with PAVE_E_ARG before any device call: whatever pave_zone_events refuses in the fields of the same name, a
 * null state or output tensor, L outside 1 .. 64, stride outside 1 .. 255, min_step outside 0 .. 65535.
 * slot_head is reduced to (unsigned)head % L and slot_count clamped to 1 .. L wherever they index the ring, and a
 * slot index is a loop counter: a plan that passes cannot address memory outside its tensors, whatever the poses and
 * the state hold.
 *
 * pave_draw_trails_nv12 / _bgr: one launch for n separately allocated surfaces, in place; the state is only read.
 *   dst, pitch, width, height, table, camera: as in pave_zone_draw_plan
 *   slot_id .. frame: the tensors of pave_trail_plan, for every camera;  S, L: their sizes
 *   palette    the bytes stored, per table: (Y, U, V) for _nv12, (B, G, R) for _bgr; a slot takes row (id - 1) % 32
 *   thickness, thickness_tail   1 .. 32 pixels at the newest and the oldest end, thickness_tail <= thickness
 *   head_radius  0 .. 32 pixels: a disc at pos (0: none)
 *   tail_frames  0 (every segment) or 1 .. 2^30: a segment whose older point was committed more than this many
 *                frames ago is not drawn
 *   linger     -1 (every live slot) or 0 .. 2^30: only slots seen within the last `linger` frames
 * A point in quarter pixels is Q = clamp(p >> 1, 0, 32767).  With n = count and p_0 .. p_{n-1} the committed points,
 * oldest first, p_n = pos: capsule j = 0 .. n - 1 from Q(p_j) to Q(p_{j+1}) of radius 2 thickness_tail + floor(2
 * (thickness - thickness_tail)(j + 1) / n) quarter pixels, and (head_radius > 0) the disc j = n at Q(pos) of radius 4
 * head_radius; covered as in pave_draw_plan.  A pixel takes the colour of the covering primitive with the largest
 * (id, j); an NV12 chroma sample the largest over its 2 x 2 luma pixels.  A byte no primitive covers and padding are
 * never written.
 * Refused with PAVE_E_ARG before any device call: a null plan, surface or state tensor, n outside 1 .. 32, width or
 * height outside 1 .. 8192, odd NV12 sizes, a pitch below a row's bytes, a table index >= 4, cameras outside 1 ..
 * 4096, a camera outside [0, cameras), S outside 1 .. 128, L outside 1 .. 64, thickness or thickness_tail outside 1 ..
 * 32 or thickness_tail > thickness, head_radius outside 0 .. 32, tail_frames outside 0 .. 2^30, linger outside -1 ..
 * 2^30.  head and count are reduced as in the update before they index the ring.
 */
#define PAVE_TRAIL_MAX_POINTS 64
#define PAVE_TRAIL_MAX_STRIDE 255
#define PAVE_TRAIL_MAX_STEP 65535
#define PAVE_TRAIL_MAX_THICKNESS 32
#define PAVE_TRAIL_MAX_RADIUS 32
#define PAVE_TRAIL_MAX_FRAMES 1073741824
typedef struct pave_trail_plan {
  const float*   kpts[PAVE_TRACK_MAX_FRAMES];
  const float*   bboxes[PAVE_TRACK_MAX_FRAMES];
  const int32_t* keep[PAVE_TRACK_MAX_FRAMES];
  const int32_t* ids[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_count[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_span[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_dist[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_path[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  float          scale[PAVE_TRACK_MAX_FRAMES][2];
  int32_t* slot_id;
  int32_t* slot_last;
  int32_t* slot_pos;
  int32_t* slot_head;
  int32_t* slot_count;
  int32_t* slot_box;
  int32_t* pts;
  int32_t* when;
  int32_t* frame;
  int32_t* dropped;
  int anchor_kpt[PAVE_ZONE_MAX_ANCHOR_KPTS];
  int entries, cameras, S, K, L, anchor, n_anchor, stride, min_step, max_age;
  float score_thr, kpt_thr;
} pave_trail_plan;
int pave_trail_update(const pave_trail_plan* plan, void* stream);

typedef struct pave_trail_draw_plan {
  void*          dst[PAVE_DRAW_MAX_SURFACES];
  int            pitch[PAVE_DRAW_MAX_SURFACES];
  int            width[PAVE_DRAW_MAX_SURFACES];
  int            height[PAVE_DRAW_MAX_SURFACES];
  int            camera[PAVE_DRAW_MAX_SURFACES];
  uint8_t        table[PAVE_DRAW_MAX_SURFACES];
  const int32_t* slot_id;
  const int32_t* slot_last;
  const int32_t* slot_pos;
  const int32_t* slot_head;
  const int32_t* slot_count;
  const int32_t* slot_box;
  const int32_t* pts;
  const int32_t* when;
  const int32_t* frame;
  uint8_t        palette[PAVE_DRAW_MAX_TABLES][PAVE_DRAW_PALETTE][3];
  int n, cameras, S, L, thickness, thickness_tail, head_radius, tail_frames, linger;
} pave_trail_draw_plan;
int pave_draw_trails_nv12(const pave_trail_draw_plan* plan, void* stream);
int pave_draw_trails_bgr(const pave_trail_draw_plan* plan, void* stream);

/*
 * The ground plane: every pose's position on the floor in millimetres through a calibrated homography, its track's
 * speed and distance walked, its nearest neighbour, and the poses restated in floor units for the anchor-based
 * consumers (pavenet_amd/csrc/pave_floor.hip; the rule is DESIGN section 23, integer-exact).  The plan is copied
 * into the kernel's arguments.
 *
 * pave_floor_update: one launch for `entries` frames of any of `cameras` cameras; one block per camera of the launch
 * takes that camera's entries in plan order, as pave_zone_events does: entries of one camera are in time order.
 *   kpts[i], bboxes[i], keep[i], ids[i], n[i], camera[i], scale[i], anchor, anchor_kpt, n_anchor, S, K, max_age,
 *   score_thr, kpt_thr   as in pave_zone_plan: the same 1/8-pixel anchor (ax, ay)
 *   calib            DEVICE [cameras, PAVE_FLOOR_CALIB_WORDS] int64, read: words 0 .. 8 the matrix G row by row (1/8
 *                    pixel -> floor, times a power of two; every row has (|g0| + |g1|) 65535 + |g2| < 2^61), words 9 ..
 *                    12 the bounds x0, y0, x1, y1 in mm (read clamped to +-PAVE_FLOOR_MAX_MM), word 13 != 0: the
 *                    camera is calibrated.  With n = G (ax, ay, 1): on the floor iff n2 > 0 and X = floor((2 n0 + n2)
 *                    / (2 n2)), Y likewise lie in the bounds, ends included
 *   out[i]           DEVICE [PAVE_FLOOR_OUT_WORDS * n[i]] int32, out: on [n], xy [n, 2] (mm), vel [n, 2], speed [n]
 *                    (1/256 mm per frame), travel [n] (mm), nearest [n] (a pose index or -1), gap [n] (mm or -1), near
 *                    [n], one after the other
 *   out_floor[i]     DEVICE [n[i] * K * 3 + n[i] * 5] float, out: the key points, then the boxes, of the result in
 *                    floor units: with P = floor(4 (X - origin) / unit) per axis in 0 .. 32767 every x and y is P / 4,
 *                    else NaN; the scores are copied (both may be NULL where n[i] == 0)
 *   the state, DEVICE int32, read and written: slot_id, slot_last, slot_hits, slot_travel [cameras, S] (id 0: a free
 *                    slot, its other fields are never read), slot_pos (mm), slot_vel (1/256 mm per frame) [cameras,
 *                    S, 2]; frame, dropped [cameras]
 *   velocity_gain    1 .. 16: sixteenths of the newest move that go into the velocity
 *   near             0 .. 2^20 mm: neighbours at most this far are counted
 *   unit             1 .. 1000 mm per floor pixel;  origin_x, origin_y: +-PAVE_FLOOR_MAX_MM, the plan's corner in mm
 * Refused with PAVE_E_ARG before any device call: whatever pave_zone_events refuses in the fields of the same name, a
 * null state, calibration or output tensor, velocity_gain outside 1 .. 16, near outside 0 .. 2^20, unit outside 1 ..
 * 1000, an origin outside +-(2^20 - 1).  A slot index is a loop counter and a pose index is below n[i]: a plan that
 * passes cannot address memory outside its tensors, whatever the poses, the state and the calibration hold.
 */
#define PAVE_FLOOR_CALIB_WORDS 16
#define PAVE_FLOOR_CALIB_BOUNDS 9
#define PAVE_FLOOR_CALIB_VALID 13
#define PAVE_FLOOR_OUT_WORDS 10
#define PAVE_FLOOR_MAX_MM 1048575
#define PAVE_FLOOR_MAX_NEAR 1048576
#define PAVE_FLOOR_MAX_UNIT 1000
#define PAVE_FLOOR_MAX_GAIN 16
#define PAVE_FLOOR_MAX_HITS 1073741824
typedef struct pave_floor_plan {
  const float*   kpts[PAVE_TRACK_MAX_FRAMES];
  const float*   bboxes[PAVE_TRACK_MAX_FRAMES];
  const int32_t* keep[PAVE_TRACK_MAX_FRAMES];
  const int32_t* ids[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out[PAVE_TRACK_MAX_FRAMES];
  float*         out_floor[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  float          scale[PAVE_TRACK_MAX_FRAMES][2];
  int32_t* slot_id;
  int32_t* slot_last;
  int32_t* slot_hits;
  int32_t* slot_pos;
  int32_t* slot_vel;
  int32_t* slot_travel;
  int32_t* frame;
  int32_t* dropped;
  const int64_t* calib;
  int anchor_kpt[PAVE_ZONE_MAX_ANCHOR_KPTS];
  int entries, cameras, S, K, anchor, n_anchor, velocity_gain, near, unit, origin_x, origin_y, max_age;
  float score_thr, kpt_thr;
} pave_floor_plan;
int pave_floor_update(const pave_floor_plan* plan, void* stream);

/*
 * Contacts and groups on the floor: which tracks stand within a radius of each other, debounced with hysteresis, for
 * how long, which parties they form (the connected components of the contact graph), and the MEET / PART / LONG
 * events of the frame (pavenet_amd/csrc/pave_contacts.hip; the rule is DESIGN section 24, integer-exact).  It takes
 * what pave_floor_update wrote: the `on` and `xy` sections of its output.  The plan is copied into the kernel's
 * arguments.
 *
 * pave_contact_update: one launch for `entries` frames of any of `cameras` cameras; one block per camera of the launch
 * takes that camera's entries in plan order, as pave_floor_update does: entries of one camera are in time order.
 *   on[i]            DEVICE [n[i]] int32, read: != 0: the pose is placed on the floor
 *   xy[i]            DEVICE [n[i], 2] int32, read: its floor position in mm (read clamped to +-PAVE_FLOOR_MAX_MM, so a
 *                    squared distance is below 2^44)
 *   ids[i]           DEVICE [n[i]] int32, read: the track ids of the frame; a pose takes part iff on, id >= 1 and no
 *                    pose before it that passes both tests has its id (all three may be NULL where n[i] == 0)
 *   n[i]             0 .. PAVE_TRACK_MAX_POSES;  camera[i] in [0, cameras)
 *   out[i]           DEVICE [PAVE_CONTACT_OUT_WORDS * n[i]] int32, out: group [n] (the smallest track id of the pose's
 *                    component), size [n] (its slots), contacts [n] (the pose's degree), partner [n] (the id of its
 *                    contact of the smallest since, the lower slot on a tie, or 0), together [n] (frames since that
 *                    contact began, or 0), one after the other; all 0 for a pose without a slot (may be NULL where n[i]
 *                    == 0)
 *   out_events[i]    DEVICE [max_events, PAVE_CONTACT_EVENT_WORDS] int32, out: rows (kind, a, b, frames, pose_a, pose_b,
 *                    frame), a < b the two track ids, pose_* their rows in this frame or -1: first the PARTs of the
 *                    slots that expired, in ascending (s, t) of the slot pair, then the MEET, PART and LONG of the
 *                    pairs of live slots in ascending (s, t); zero past the count
 *   out_n_events[i]  DEVICE [1] int32, out: all events of the frame, stored or not
 *   the state, DEVICE int32, read and written: slot_id, slot_last [cameras, S] (id 0: a free slot, its other fields
 *                    are never read), slot_pos [cameras, S, 2] (mm); link, since [cameras, S, S]: the words of the slot
 *                    pair s < t at [s, t] (link bit 0: in contact, bits 8 ..: the frames in a row the distance test has
 *                    disagreed with it; since: the frame the contact began, 0 without one), read only while both slots
 *                    are live, zeroed when either is born; frame, dropped [cameras]; counters [cameras,
 *                    PAVE_CONTACT_COUNTER_WORDS]: PAVE_CONTACT_CNT_*
 *   radius           0 .. 2^20 mm: two tracks not in contact are near iff dx^2 + dy^2 <= radius^2
 *   release          radius .. 2^21 mm: two tracks in contact are near iff dx^2 + dy^2 <= release^2
 *   min_frames       1 .. 255: the contact bit flips once near has disagreed with it this many frames in a row
 *   long_frames      0 .. 2^30: a contact of exactly this many frames is reported once (0: never)
 *   max_events       1 .. 4096 rows of out_events[i];  max_age >= 0: a slot unseen for more frames is freed
 * Refused with PAVE_E_ARG before any device call: a null plan, entries outside 1 .. 32, S outside 1 .. 128, cameras
 * outside 1 .. 4096, a null state or output tensor, a null input where n[i] > 0, n[i] outside 0 .. 128, a camera index
 * outside [0, cameras), radius, release, min_frames, long_frames or max_events outside their ranges, max_age < 0.  A
 * slot index is a loop counter below S and a pose index is below n[i]: a plan that passes cannot address memory
 * outside its tensors, whatever the inputs and the state hold.
 */
#define PAVE_CONTACT_MEET 1
#define PAVE_CONTACT_PART 2
#define PAVE_CONTACT_LONG 3
#define PAVE_CONTACT_OUT_WORDS 5
#define PAVE_CONTACT_EVENT_WORDS 7
#define PAVE_CONTACT_COUNTER_WORDS 8
#define PAVE_CONTACT_CNT_CONTACTS 0
#define PAVE_CONTACT_CNT_MEETS 1
#define PAVE_CONTACT_CNT_PARTS 2
#define PAVE_CONTACT_CNT_LONGS 3
#define PAVE_CONTACT_CNT_GROUPS 4
#define PAVE_CONTACT_CNT_GROUPED 5
#define PAVE_CONTACT_CNT_LARGEST 6
#define PAVE_CONTACT_MAX_RADIUS 1048576
#define PAVE_CONTACT_MAX_RELEASE 2097152
#define PAVE_CONTACT_MAX_LONG 1073741824
#define PAVE_CONTACT_MAX_EVENTS 4096
typedef struct pave_contact_plan {
  const int32_t* on[PAVE_TRACK_MAX_FRAMES];
  const int32_t* xy[PAVE_TRACK_MAX_FRAMES];
  const int32_t* ids[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_events[PAVE_TRACK_MAX_FRAMES];
  int32_t*       out_n_events[PAVE_TRACK_MAX_FRAMES];
  int            n[PAVE_TRACK_MAX_FRAMES];
  int            camera[PAVE_TRACK_MAX_FRAMES];
  int32_t* slot_id;
  int32_t* slot_last;
  int32_t* slot_pos;
  int32_t* link;
  int32_t* since;
  int32_t* frame;
  int32_t* dropped;
  int32_t* counters;
  int entries, cameras, S, radius, release, min_frames, long_frames, max_events, max_age;
} pave_contact_plan;
int pave_contact_update(const pave_contact_plan* plan, void* stream);

/*
 * 3x3 convolution, NHWC fp32, pad 1, stride 1 or 2, bias (+ReLU) fused: implicit GEMM on the
 * exact-fp32 MFMA.  Used for the ResNet / HRNet 3x3 convolutions with BatchNorm folded in
 * (mmdet resnet.py Bottleneck.conv2 / BasicBlock, hrnet.py).
 *   x [N, H, W, Cin];  w [3, 3, Cin, Cout] (tap-major, Cout innermost);  bias [Cout] or NULL;
 *   y [N, Ho, Wo, Cout], Ho = (H - 1)/stride + 1.  Cin %% 32 == 0, Cout %% 64 == 0.
 */
int pave_conv3x3_nhwc_f32(const float* x, const float* w, const float* bias, float* y, int N,
                          int H, int W, int Cin, int Cout, int stride, int relu, void* stream);

/*
 * Row GEMM with the whole Bottleneck tail in its prologue / epilogue (fp32 MFMA, exact fp32):
 *   A1 = a_bias ? relu(a[M, K] + a_bias[K]) : a            (conv2's folded bn2 + ReLU on load)
 *   out[M, N] = act([A1 | a2[M, K2]] * w[K + K2, N] + bias[N] + residual[M, N])
 * = mmdet resnet.py:264-283 `bn2 -> relu -> conv3 -> bn3 -> (+ downsample(x) | + identity) ->
 * relu` on the NHWC map (BatchNorm folded into w / bias; the downsample 1x1 convolution is the
 * second K range, w = [W3; Wd]).  a_bias, a2 (with K2 = 0), bias, residual may be NULL;
 * `residual` may alias `out` (every element is read before it is written by the same lane).
 * K %% 32 == 0, K2 %% 32 == 0, N %% 64 == 0, M < 2^31.
 */
int pave_rows_gemm_bias_res_act_f32(const float* a, const float* a_bias, const float* a2,
                                    const float* w, const float* bias, const float* residual,
                                    float* out, long long M, int K, int K2, int N, int relu,
                                    void* stream);

/*
 * ResNet stem tail in one pass (resnet.py:640-645 `norm1 -> relu -> maxpool` with BN folded):
 *   y[N, Ho, Wo, C] = maxpool3x3/s2/p1(relu(x[N, H, W, C] + bias[C])),  Ho = (H - 1)/2 + 1.
 */
int pave_bias_relu_maxpool_nhwc_f32(const float* x, const float* bias, float* y, int N, int H,
                                    int W, int C, void* stream);

/*
 * fp32 row GEMM on the bf16 matrix cores by operand splitting into `nplanes` bf16 terms:
 *   nplanes = 3: exact split, 6 bf16 MFMAs per product tile, error <= 2^-23 relative per product
 *                (fp32-level);  2: 3 MFMAs, ~2^-16;  1: plain bf16 operands;  PAVE_PLANES_FP16:
 *                plain fp16 operands (BASELINE config 5's "fp16 MFMA projections") -- always
 *                with fp32 accumulation and fp32 in/out.
 *   out[M, N] = act(A'[M, K] * W[N, K]^T + bias[N] + residual[M, N]),
 *   A' = a_bias ? relu(a + a_bias[K]) : a;  act: relu = 0 none | 1 ReLU | 2 exact GELU x Phi(x) (nn.GELU, the
 *   activation of the Swin block's FFN, third_party/mmdetection/mmdet/models/backbones/swin.py:330-341) |
 *   3 sigmoid 1 / (1 + exp(-x)) (the heads' sigma branches, videopose_head_mul_frames.py:533, 652);  2 and 3:
 *   3 planes / fp16 only
 * = nn.Linear (mmcv FFN / projections, bricks/transformer.py:1046-1120) with the residual and
 * activation of its caller in the epilogue.  `w_planes` = the weight [N, K] split once by
 * pave_split_bf16x3_f32 into `nplanes` bf16 planes and re-laid slab-major [K/16][nplanes][N][16]
 * (one 16-wide K slab of a column tile contiguous; pavenet_amd.ops.split_weight_bf16x3).
 * residual may alias out.  M < 2^31.
 *   3 planes: K %% 32 == 0 (K >= 64), N %% 4 == 0; for N %% 64 != 0 the weight planes carry
 *   roundup(N, 64) rows (zero rows beyond N) while out / bias / residual have N columns.
 *   PAVE_PLANES_FP16: the same kernels and shape rules as 3 planes (one fp16 plane [K/16][1][N][16], the
 *   fp32 activation rows converted to fp16, round to nearest even, where the 3-plane form splits them;
 *   one v_mfma_f32_32x32x16_f16 per tile and 16-wide K slab).
 *   1 / 2 bf16 planes: K %% 64 == 0, N %% 128 == 0 (first-generation kernels).
 * Every entry point below that takes `nplanes` accepts 3 or PAVE_PLANES_FP16 (pave_gemm_bf16x3_f32,
 * _ex_f32 and pave_conv3x3_split_f32 also 1 and 2).
 */
#define PAVE_PLANES_FP16 16 /* nplanes value: ONE plane of fp16 (not bf16) operands */
int pave_gemm_bf16x3_f32(const float* a, const float* a_bias, const void* w_planes,
                         const float* bias, const float* residual, float* out, long long M, int K,
                         int N, int relu, int nplanes, void* stream);

/*
 * fp16 operand mode with fp16 ACTIVATIONS around a launch (BASELINE configs[4]; wide tile forms, N %% 256 == 0):
 * a tensor that is only ever a GEMM operand -- the hidden activation between the two Linears of an FFN
 * (third_party/mmcv/mmcv/cnn/bricks/transformer.py:1046-1120) -- is stored as the fp16 values the next launch's
 * MFMA consumes anyway: the same results as fp32 storage (the consumer would round it to fp16 at operand fetch),
 * half the bytes on an HBM-bound chain.
 *   a [M, K] fp32, or fp16 when a_is_f16;  w_plane = ONE fp16 plane [K/16][1][N][16] (PAVE_PLANES_FP16);
 *   gamma == NULL:  out[M, N] = act(a W^T + bias), fp32 or (out_is_f16) fp16;  relu as pave_gemm_bf16x3_f32;
 *   gamma != NULL:  out[M, 256] = LayerNorm(a W^T + bias + residual) * gamma + beta, fp32 (N == 256; residual fp32,
 *                   may be NULL or alias out).
 */
int pave_gemm_fp16_act_f32(const void* a, int a_is_f16, const void* w_plane, const float* bias,
                           const float* residual, const float* gamma, const float* beta, float eps, void* out,
                           int out_is_f16, long long M, int K, int N, int relu, void* stream);

/*
 * Same GEMM with two epilogue options (the encoder layer's `value_proj | sampling_offsets |
 * attention_weights` Linears of third_party/mmcv/mmcv/ops/multi_scale_deform_attn.py:355-379 run
 * as ONE launch over the layer input):
 *   residual_rows > 0: `residual` is a [residual_rows, N] table and row m adds residual[m %
 *     residual_rows] -- a per-token term shared by all frames (e.g. (query_pos @ W^T + b) when the
 *     positional encoding is the same for every frame); 0: residual is [M, N] as above.
 *   out2 != NULL: the product is cut at column n_split (n_split %% 128 == 0) into two dense
 *     matrices, out [M, n_split] and out2 [M, N - n_split].
 */
int pave_gemm_bf16x3_ex_f32(const float* a, const float* a_bias, const void* w_planes,
                            const float* bias, const float* residual, long long residual_rows,
                            float* out, float* out2, int n_split, long long M, int K, int N,
                            int relu, int nplanes, void* stream);

/*
 * out[i] = sigmoid(tmp[i] + inverse_sigmoid(ref[i])), inverse_sigmoid(x) = log(max(clamp(x, 0, 1),
 * eps) / max(1 - clamp(x, 0, 1), eps)): the per-layer reference-point update of the pose / joint
 * decoders (opera/models/utils/transformer.py:6733-6735,
 * third_party/mmdetection/mmdet/models/utils/transformer.py:865-866) as one launch.
 */
int pave_ref_update_f32(const float* tmp, const float* ref, float* out, long long n, float eps,
                        void* stream);

/*
 * GroupNorm of an NHWC map x [N, HW, C] (G groups of C/G consecutive channels), y = GN(x) * gamma +
 * beta written to y + n * y_batch_stride + (hw * C + c): the destination may be a slice of a larger
 * [N, S, C] token buffer (the neck's conv -> GN levels land directly in the transformer's flattened
 * multi-level feature, third_party/mmdetection/mmdet/models/necks/channel_mapper.py:90-100 +
 * opera/models/utils/transformer.py:21312-21331).  Statistics are accumulated in fp64 in a fixed
 * order (bit-reproducible).  Scratch supplied by the caller: partial [N * nchunks * G * 2] doubles
 * (nchunks = number of row chunks the statistics pass is cut into), ab [N * 2 * C] floats.
 * C %% 4 == 0, (C / G) %% 4 == 0, C / 4 divides 256.
 */
int pave_groupnorm_nhwc_f32(const float* x, const float* gamma, const float* beta, float* y,
                            long long y_batch_stride, int N, int HW, int C, int G, float eps,
                            double* partial, int nchunks, float* ab, void* stream);

/*
 * The same GroupNorm over up to four maps of one N, C and G at once -- the levels of the neck
 * (necks/channel_mapper.py:90-100: one ConvModule per level, each with its own GroupNorm(32)) -- as THREE launches
 * instead of three per level; per level the values are those of pave_groupnorm_nhwc_f32 with the same nchunks,
 * bit for bit.  Scratch: partial [N * G * 2 * sum(nchunks)] doubles, ab [nlev * N * 2 * C] floats.
 */
typedef struct pave_gn_level {
  const float* x;              /* [N, HW, C] dense */
  const float* gamma;          /* [C] */
  const float* beta;           /* [C] */
  float* y;                    /* row n at y + n * y_batch_stride */
  long long y_batch_stride;    /* floats, >= HW * C */
  int HW;
  int nchunks;                 /* row chunks of the statistics pass */
  float eps;
} pave_gn_level;
int pave_groupnorm_levels_nhwc_f32(const pave_gn_level* levels, int nlev, int N, int C, int G, double* partial,
                                   float* ab, void* stream);

/*
 * out[M, N] = act([a | a2] @ W^T + bias + residual): two row matrices a [M, K1] and a2 [M, K - K1]
 * share one K axis and one accumulator (3 bf16 planes) -- the ResNet Bottleneck tail with a
 * stride-1 downsample, relu(conv3(y) + downsample(x)) = relu([y | x] @ [W3 | Wd]^T + b3 + bd)
 * (third_party/mmdetection/mmdet/models/backbones/resnet.py:264-283), in ONE launch with no
 * concatenation copy.  w_planes = the planes of the [N, K] row-concatenated weight.
 * K %% 32 == 0, N %% 64 == 0, 0 < K1 < K, K1 %% 16 == 0.  residual may be NULL or alias out.
 */
int pave_gemm_bf16x3_cat_f32(const float* a, long long K1, const float* a2, const void* w_planes,
                             const float* bias, const float* residual, float* out, long long M, int K,
                             int N, int relu, int nplanes, void* stream);

/*
 * Grouped row GEMM (3 bf16 planes): the N axis is cut into N / group_n groups; group i computes
 *   out[:, i group_n : (i + 1) group_n] = act(a[:, i K : (i + 1) K] @ W_i^T + bias_i),
 * a [M, lda] row-major (lda >= groups * K), W_i [group_n, K]; w_planes = the planes of the [N, K]
 * row-concatenation of the W_i.  One launch for the T per-frame Linears of one layer of the
 * reference's per-frame key-point / regression branches (pre_pre_ / pre_ / "" / next_ / next_next_
 * kpt_branches, opera/models/utils/transformer.py:6728-6740;
 * third_party/mmdetection/mmdet/models/utils/transformer.py:860-875).
 * K %% 32 == 0, group_n %% 64 == 0, lda %% 4 == 0.
 */
int pave_gemm_bf16x3_grouped_f32(const float* a, long long lda, const void* w_planes, const float* bias,
                                 float* out, long long M, int K, int N, int group_n, int relu,
                                 int nplanes, void* stream);

/*
 * out[M, 256] = LayerNorm(a @ W^T + bias + residual) * gamma + beta  (3 bf16 planes, N == 256): the
 * attention / FFN output Linear, its residual add and the post-norm of a BaseTransformerLayer
 * (third_party/mmcv/mmcv/cnn/bricks/transformer.py:1316-1353) in ONE launch -- a 128 x 256 block
 * tile owns whole rows, the row statistics are completed across its waves through LDS (two-pass
 * mean / centred variance).  residual may be NULL or alias out.  K %% 64 == 0.
 */
int pave_gemm_bf16x3_ln_f32(const float* a, const void* w_planes, const float* bias,
                            const float* residual, const float* gamma, const float* beta, float eps,
                            float* out, long long M, int K, int N, int nplanes, void* stream);

/*
 * 3x3 / pad 1 / stride 1|2 convolution, NHWC fp32 in and out, as an implicit GEMM through the same
 * split-operand kernel (K axis = (ky, kx, cin)), bias (+ReLU) in the epilogue:
 *   x [N, H, W, Cin];  w_planes = the weight [Cout, 3, 3, Cin] (i.e. [Cout, 9*Cin] rows) split and
 *   re-laid like pave_gemm_bf16x3_f32's operand;  y [N, Ho, Wo, Cout], Ho = (H - 1)/stride + 1.
 * Replaces a ResNet / HRNet 3x3 nn.Conv2d + folded BatchNorm (+ identity) (+ReLU)
 * (third_party/mmdetection/mmdet/models/backbones/resnet.py:53-98 BasicBlock, hrnet.py:183-260)
 * in the split / 16-bit GEMM modes.
 *   3 planes: Cin %% 16 == 0, Cout %% 4 == 0; the weight planes are ZERO-PADDED to
 *   roundup(9 Cin, 32) columns and roundup(Cout, 64) rows (HRNet's 48- / 96-channel branches);
 *   residual [N, Ho, Wo, Cout] (may be NULL or alias y) is added before the ReLU.
 *   PAVE_PLANES_FP16: as 3 planes.  1 / 2 bf16 planes: Cin %% 64 == 0, Cout %% 64 == 0, residual == NULL.
 */
int pave_conv3x3_split_f32(const float* x, const void* w_planes, const float* bias,
                           const float* residual, float* y, int N, int H, int W, int Cin, int Cout,
                           int stride, int relu, int nplanes, void* stream);

/*
 * The same convolution (3 planes) with the K axis cut into parts -- for maps with FEW output pixels
 * and many input channels, where the 128-row tiles alone leave most of the chip idle (the
 * ChannelMapper's extra level: 3x3 / stride 2, 2048 -> 256 on the C5 map,
 * third_party/mmdetection/mmdet/models/necks/channel_mapper.py:84-97).  Each part is computed by
 * its own workgroups into `workspace` ([parts][N Ho Wo][Cout] fp32), a second launch adds the
 * parts IN ORDER (deterministic), then bias, residual and ReLU.
 *   pave_conv3x3_splitk_workspace_bytes: the workspace the shape needs; 0 = the shape has no
 *   split-K plan (enough tiles or a short K): call pave_conv3x3_split_f32.
 *   pave_conv3x3_splitk_f32: workspace_bytes >= that value; the workspace is free for reuse in
 *   stream order after the call.
 */
long long pave_conv3x3_splitk_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride);
int pave_conv3x3_splitk_f32(const float* x, const void* w_planes, const float* bias,
                            const float* residual, float* y, int N, int H, int W, int Cin, int Cout,
                            int stride, int relu, void* workspace, long long workspace_bytes,
                            int nplanes, void* stream);

/*
 * The same split-K plan for the plain row GEMM out[M, N] = act(a[M, K] W^T + bias + residual) (relu = 0 | 1): few
 * row tiles and K >= 2048 -- ResNet layer4's 1x1 reductions (resnet.py:264-271) and the ChannelMapper's C5 lateral
 * on a one-clip batch.  pave_gemm_splitk_workspace_bytes = 0: the shape has no plan, use pave_gemm_bf16x3_f32.
 */
long long pave_gemm_splitk_workspace_bytes(long long M, int K, int N);
int pave_gemm_bf16x3_splitk_f32(const float* a, const void* w_planes, const float* bias, const float* residual,
                                float* out, long long M, int K, int N, int relu, int nplanes, void* workspace,
                                long long workspace_bytes, void* stream);

/*
 * Form policy (per host thread): which kernel forms the GEMM / convolution dispatchers of this thread may pick.
 * Several of them choose a form by the row count M -- split-K parts of the 3x3, strided 1x1 and long-K row GEMMs,
 * the K-split small-row form, the LayerNorm pass instead of the fused LayerNorm epilogue -- and M comes from the
 * batch, so a clip's last bits depended on what shared its batch.
 *   0  today's selection, by row / tile count (the default);
 *   1  "tile order": only forms bit-identical to the 128-row tile kernels (small-row one-wave, narrow, wide,
 *      8-wave, two row tiles per wave); no split-K parts, no K-split small-row form, the fused LayerNorm epilogue
 *      in its wide form (gemm_w_ln_kernel) at every M;
 *   2  "K-split order": gemm_sk_kernel's order at every M for the plain row GEMM / LayerNorm GEMM where it
 *      applies (K >= 512, or K >= 256 with N <= 512; the LayerNorm GEMM then takes its separate pass), order 1
 *      everywhere else.
 * Under 1 and 2 every decision is a function of (K, N, planes, kind, policy) only: an output row is a function of
 * its own input row, whatever the batch.  pave_set_form_policy: PAVE_E_ARG outside 0 .. 2.
 */
int pave_set_form_policy(int policy);
int pave_get_form_policy(void);

/*
 * The summation order a launch takes, as the dispatchers decide it (a pure host function: no device, no state but
 * the diag build's form override).  kind: PAVE_FORM_*; K = the GEMM's reduction length (9 Cin for the 3x3, Cin
 * for the strided 1x1), N = its output columns (padded as the entries pad them); nplanes 3 or PAVE_PLANES_FP16.
 *   *order: PAVE_ORDER_*; it names the order, not the kernel -- forms proven bit-identical share one;
 *   *ksplit: the split-K parts of PAVE_ORDER_SPLITK (their count changes the order), else 1.
 */
#define PAVE_FORM_ROWS 0          /* pave_gemm_bf16x3_f32, _ex (one output, no a_bias), _grouped */
#define PAVE_FORM_ROWS_SPLITK 1   /* the same launch where a caller takes pave_gemm_bf16x3_splitk_f32 when it has a plan */
#define PAVE_FORM_ROWS_TILE 2     /* a_bias, two outputs or two A sources (_ex, _cat): tile forms at every M */
#define PAVE_FORM_LN 3            /* pave_gemm_bf16x3_ln_f32 */
#define PAVE_FORM_CONV3X3 4       /* pave_conv3x3_split_f32 / pave_conv3x3_splitk_f32 */
#define PAVE_FORM_CONV1X1S 5      /* pave_conv1x1_strided_split_f32 */
#define PAVE_FORM_ENCPROJ 6       /* pave_gemm_bf16x3_encproj_f32 */
#define PAVE_ORDER_TILE 0         /* the 128-row tile kernels' order (LN: the wide form's fused LayerNorm epilogue) */
#define PAVE_ORDER_KSPLIT 1       /* gemm_sk_kernel's: K quarters over four waves, added ((p0 + p1) + p2) + p3 */
#define PAVE_ORDER_SPLITK 2       /* split-K parts (*ksplit of them), added in order by a second launch */
#define PAVE_ORDER_TILE_LNPASS 3  /* LN: tile-order GEMM, then the separate LayerNorm pass */
#define PAVE_ORDER_KSPLIT_LNPASS 4 /* LN: K-split-order GEMM, then the separate LayerNorm pass */
#define PAVE_ORDER_TILE_LN8 5     /* LN: the 8-wave block's fused LayerNorm (row statistics summed across 8 waves) */
int pave_form_plan(long long M, int K, int N, int kind, int nplanes, int policy, int* order, int* ksplit);

/*
 * ResNet Bottleneck of the 64-channel stage from its 3x3 convolution on, CHAINED with the next
 * block's conv1, in ONE launch (third_party/mmdetection/mmdet/models/backbones/resnet.py:263-300
 * Bottleneck.forward: conv2 + bn2 + relu -> conv3 + bn3 -> + identity | downsample(x) -> relu; then
 * the following block's conv1 + bn1 + relu), BatchNorms folded, NHWC fp32, M = N H W pixels:
 *   c2  = relu(conv3x3_pad1(c1 [N, H, W, 64]; w2_planes) + b2)            -> c2  [M, 64] (scratch)
 *         c1 == NULL and w2_planes == NULL: the launch starts at conv3 and c2 [M, 64] is its INPUT
 *         (the 3x3 -- pave_conv3x3_split_f32 -- was a launch of its own)
 *   out = relu([c2 | a2] @ W3^T + b3 + residual)                          -> out [M, 256]
 *         a2 [M, k2] (k2 %% 32 == 0): the block input of a stride-1 downsample block, W3 = the
 *         [256, 64 + k2] row-concatenated conv3 | downsample weight, b3 = both biases; else
 *         residual [M, 256] = the block input (may alias out), a2 == NULL, k2 == 0
 *   c1n = relu(out @ W1n^T + b1n)                                         -> c1n [M, cn], cn = 64 | 128
 *         (w1n_planes == NULL, cn == 0: the launch stops after `out`)
 * w2_planes as pave_conv3x3_split_f32's (3 planes), w3_planes / w1n_planes as
 * pave_gemm_bf16x3_f32's (3 planes).  Every value equals what pave_conv3x3_split_f32,
 * pave_gemm_bf16x3_cat_f32 / pave_gemm_bf16x3_f32 give launched one after the other (same
 * kernels bodies, same tiles) -- the chain exists for time: a workgroup carries one 128-pixel tile
 * through the three GEMMs, so the HBM-bound conv3 + identity phase of one workgroup overlaps the
 * MFMA-bound phases of its neighbours and conv1 reads `out` back from L2.
 */
int pave_bottleneck_chain_f32(const float* c1, const void* w2_planes, const float* b2, float* c2,
                              const void* w3_planes, const float* b3, const float* residual,
                              const float* a2, int k2, float* out, const void* w1n_planes,
                              const float* b1n, float* c1n, int cn, int N, int H, int W, int nplanes,
                              void* stream);

/*
 * 1x1 convolution with a stride on an NHWC map (the ResNet downsample branch,
 * third_party/mmdetection/mmdet/models/backbones/resnet.py:258-262 `self.downsample(x)`): the row
 * GEMM pave_gemm_bf16x3_f32 (3 planes) whose A row m is the input pixel (oy * stride, ox * stride)
 * of image n -- no strided-slice copy.  x [N, H, W, Cin], y [N, Ho, Wo, Cout], Ho = (H - 1)/stride + 1.
 */
int pave_conv1x1_strided_split_f32(const float* x, const void* w_planes, const float* bias, float* y,
                                   int N, int H, int W, int Cin, int Cout, int stride, int relu,
                                   int nplanes, void* stream);

/*
 * The ResNet / HRNet stem convolution (7x7, stride 2, pad 3, 3 -> 64 channels; folded BatchNorm as
 * `bias`; third_party/mmdetection/mmdet/models/backbones/resnet.py:632-640) read straight from the
 * NCHW fp32 image batch x [N, 3, H, W], as an implicit GEMM on the 3-plane split scheme.
 * w_planes = 23 K-slabs [23][3][64][16] bf16 holding the SAME weights in two K layouts:
 *   slabs 0..11:  K = (c, ky, kx) with kx padded 7 -> 8 and (c, ky) padded 21 -> 24 rows (192) --
 *                 the per-lane window-load kernel (any W);
 *   slabs 12..22: K = (c, ky, kx') with kx' = kx + 1 (tap 0 unused) and (c, ky) padded 21 -> 22 rows
 *                 (176) -- the kernel that stages the block's input window in LDS by LDS-DMA,
 *                 taken when W %% 4 == 0 and x is 16-byte aligned.
 * y [N, Ho, Wo, 64] NHWC, Ho = (H - 1) / 2 + 1.
 * nplanes = PAVE_PLANES_FP16: w_planes = [23][1][64][16] fp16 (the same two layouts, one plane); only the
 * LDS-window kernel exists for it (W %% 4 == 0, x 16-byte aligned; PAVE_E_UNSUPPORTED otherwise).
 * row_pitch (ABI 19): elements between two image rows (0 or W: dense rows).  row_pitch > W is the layout
 * pave_repitch_rows_f32 writes: row_pitch %% 4 == 0, x 16-byte aligned, columns W .. row_pitch - 1 of every row
 * ZERO (they are the convolution's right-hand zero padding) -- an image of ANY width, e.g. the 750 x 1333 frames
 * of the reference's PoseTrack test pipeline (configs/_base_/datasets/posetrack17_video_keypoint.py:68-81,
 * size_divisor = 1), then takes the LDS-window kernel; Wo = (W - 1) / 2 + 1 is that of the real width.
 */
int pave_conv7x7s2_nchw_split_f32(const float* x, const void* w_planes, const float* bias, float* y,
                                  int N, int H, int W, int row_pitch, int Cout, int relu, int nplanes,
                                  void* stream);

/*
 * dst[r, 0:W] = src[r, 0:W], dst[r, W:pitch] = 0 for r < rows: dense fp32 rows re-laid at a row pitch that is a
 * multiple of 4 elements (16-byte aligned rows for the LDS-DMA stem above).  pitch %% 4 == 0, pitch >= W, dst
 * 16-byte aligned, src any alignment; one pass, ~2 x the image bytes.
 */
int pave_repitch_rows_f32(const float* src, float* dst, long long rows, int W, int pitch, void* stream);

/*
 * The (shifted-)window multi-head self-attention core of a Swin block -- ShiftWindowMSA.forward around
 * WindowMSA.forward, third_party/mmdetection/mmdet/models/backbones/swin.py:22-126, 128-286 -- on the
 * UN-partitioned token map (pad to a multiple of the window, roll by -shift, window partition, relative-position
 * bias, the -100 mask between roll regions, softmax, PV, window reverse, reverse roll and crop are all index
 * arithmetic inside the kernel; no copy of the map, no mask tensor):
 *   qkv [B, H, W, 3 C] fp32 = the block's qkv Linear per token (q | k | v, each [heads][32]);
 *   bias_t [heads, ws^2 (key j), ws^2 (query i)] = relative_position_bias_table[relative_position_index],
 *     TRANSPOSED per head (lanes = queries read consecutive addresses);
 *   pad_qkv [3 C] = the qkv Linear's bias: what a zero pad token projects to (the reference pads BEFORE qkv);
 *   out [B, H, W, C]: the attention output at every real pixel, the input of `proj`.
 * scale = head_dim^-0.5 (or qk_scale).  Built for window 7, head dim 32 (C == heads * 32): every Swin variant
 * of the reference's configs.
 */
int pave_swin_window_attn_f32(const float* qkv, const float* bias_t, const float* pad_qkv, float* out, int B,
                              int H, int W, int C, int heads, int window, int shift, float scale, void* stream);

/*
 * Exact merge of G partial attention rows of a frame-sharded T-frame attention (pavenet_amd/dist.py; SURVEY
 * 8e: "all-gather of pose-query logits"): parts [G, U, C + 2 H] = per rank the softmax-weighted row over its
 * frames (normalised by its own sum) followed by the per-head max logit and sum(exp(logit - max)) the fused
 * kernels emit (stat_max, stat_sum) -> out [U, C], the row of ONE softmax over all ranks' logits.  A rank
 * with sum = 0 (no frames) drops out.  C / H channels per head (a multiple of 4).
 */
int pave_merge_softmax_partials_f32(const float* parts, float* out, int G, int U, int C, int H, void* stream);

/* x[n] fp32 -> planes[nplanes][n] bf16.  nplanes = 3: every term rounded to nearest even, x = p0 + p1 + p2
 * exactly (the terms' signs are independent of x's: with the activations' truncation split on the other side the
 * products a kernel leaves out average to zero);  2: a truncation term, then the remainder rounded;  1: x rounded. */
int pave_split_bf16x3_f32(const float* x, void* planes, long long n, int nplanes, void* stream);

/*
 * Test-time augmentation merge (opera/models/detectors/petr.py:118-187 aug_test / merge_aug_results ->
 * mmdet multiclass_nms(return_inds=True) -> mmcv batched_nms -> nms_cpu / softnms_cpu), one launch, one
 * workgroup per image.  The plan is copied into the kernel's arguments (no host->device copy).
 *   bboxes[a] [B, N, 5] (x1, y1, x2, y2, score) and kpts[a] [B, N, K, 3] DEVICE: augmentation a's head results
 *   keep[a]   [B, N] int32 DEVICE or NULL: rows with keep = 0 do not enter the merge (results_to_list's mask)
 *   flip[a], img_w[a * B + b], scale_factor[a * B + b][4]: the augmentation's meta (horizontal flip only)
 *   flip_perm [K]: the left/right permutation applied to flipped key points (out[k] = in[flip_perm[k]])
 * Rows are concatenated augmentation-major, mapped back (flip, then / scale_factor), filtered by
 * score > score_thr, and suppressed by method 0 = nms (ovr > iou_thr, descending score, equal scores: lower
 * merged index first), 1 = soft naive, 2 = soft linear, 3 = soft gaussian (ovr >= iou_thr; sigma, min_score).
 * Outputs, M = min(max_num, A N) (A N if max_num <= 0):
 *   dets [B, M, 5] (soft-NMS: decayed scores), labels [B, M] int64 (0), kpts [B, M, K, 3] (score 1),
 *   inds [B, M] int64 (rows of the concatenation, -1 past the end), keep [B, M] int32, count [B] int32.
 * A N <= 4096 (the boxes live in LDS), A <= 16, A B <= 128, K <= 64.
 */
#define PAVE_AUG_MAX_AUGS 16
#define PAVE_AUG_MAX_SLOTS 128
#define PAVE_AUG_MAX_K 64
typedef struct pave_aug_plan {
  const float* bboxes[PAVE_AUG_MAX_AUGS];
  const float* kpts[PAVE_AUG_MAX_AUGS];
  const int32_t* keep[PAVE_AUG_MAX_AUGS];
  int32_t flip[PAVE_AUG_MAX_AUGS];
  float img_w[PAVE_AUG_MAX_SLOTS];
  float scale_factor[PAVE_AUG_MAX_SLOTS][4];
  int32_t flip_perm[PAVE_AUG_MAX_K];
  int32_t n_aug, B, N, K;
} pave_aug_plan;
int pave_aug_merge_nms_f32(const pave_aug_plan* plan, float score_thr, int max_num, int method, float iou_thr,
                           float sigma, float min_score, int offset, float* dets, int64_t* labels, float* kpts,
                           int64_t* inds, int32_t* keep, int32_t* count, void* stream);

/* Horizontal flip of preprocessed canvases x [n, C, Hp, Wp] -> y (out of place): columns [0, w) mirrored
 * within themselves, w = valid_w[i] (DEVICE int32 [n]) or valid_w_all when valid_w is NULL; the columns
 * from w on are copied unchanged. */
int pave_hflip_canvas_f32(const float* x, float* y, const int32_t* valid_w, int valid_w_all, int n, int C, int Hp,
                          int Wp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PAVE_HIP_H_ */
