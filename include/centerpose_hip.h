/*
 * centerpose_hip.h — C ABI of libcenterpose_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the CenterPose inference hot path.  Every entry point takes plain
 * pointers and sizes (no torch / ATen types), returns 0 on success or a negative CP_ERR_* code
 * (never prints-and-continues like the reference's launchers, dcn_v2_im2col_cuda.cu:346-350),
 * launches on the caller's stream and never synchronises.  Unless stated otherwise pointers are
 * DEVICE pointers to float32.  Paths below are relative to the reference tree
 * (/root/reference/src/lib/...).
 *
 * Threading: stateless entry points (cp_dcnv2_forward, cp_conv2d_nhwc, cp_decode, cp_postprocess, cp_pnp_solve,
 * cp_preprocess, cp_render_gaussians) may be called concurrently on different streams.  A cp_model is not re-entrant:
 * one forward / detect at a time per model (its workspace, profile records and hipGraph cache are per model).
 * cp_last_error() is per calling thread (the message of that thread's last failing call); cp_set_default_precision() is
 * process-global.  The kernel-selection hooks the test-suite uses are NOT part of this header: centerpose_hip_testing.h.
 */
#ifndef CENTERPOSE_HIP_H
#define CENTERPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cp_stream_t; /* hipStream_t */
typedef struct cp_model cp_model;

#define CP_OK 0
#define CP_ERR_INVALID (-1)
#define CP_ERR_LAUNCH (-2)
#define CP_ERR_ALLOC (-3)
#define CP_ERR_STATE (-4)

/* Library / device info.  cp_version() returns a static string.
 * CP_ABI_VERSION counts incompatible changes of this header; cp_abi_version() returns the value the library was built
 * with, so a caller compiled against another revision can refuse to run instead of passing arguments with a stale
 * meaning.  History: 1 = round-1 header; 2 = cp_preprocess takes the FORWARD 2x3 affine as double[6] and inverts it
 * itself (round 1: the inverse as float[6]); 3 = cp_dcnv2_forward accepts every shape of the reference op (generic
 * kernel), cp_num_kernel_variants() / cp_num_roles() size the profile buffers; 4 = cp_track_* added; 5 = cp_track_status, list truncation instead of reset on overflow;
 * 6 = cp_preprocess_batch, cp_linear_assignment, CP_NUM_KERNEL_VARIANTS 43, cp_set_debug moved out of this header (centerpose_hip_testing.h);
 * 7 = cp_decode_tiled / cp_decode_tiled_workspace_bytes, cp_model_detect decodes output grids above 32768 pixels;
 *     later additions without a version change: cp_box_iou, cp_box_eval, cp_pose_loss_workspace_bytes,
 *     cp_pose_loss_forward, cp_pose_loss_backward, cp_pose_targets_workspace_bytes, cp_pose_targets,
 *     cp_pose_targets_track_workspace_bytes, cp_pose_targets_track,
 *     cp_model_lean_supported, cp_model_detect_lean(_workspace_bytes), cp_model_dense_heads, cp_model_heads_at(_workspace_bytes),
 *     cp_decode_peaks(_workspace_bytes), cp_decode_gathered; CP_NUM_KERNEL_VARIANTS 46;
 *     cp_pose_heads_forward / _backward (+ _workspace_bytes, cp_pose_heads_chunk_images), cp_model_features;
 *     cp_groupnorm_workspace_bytes, cp_groupnorm_forward_nhwc / _backward_nhwc, cp_gru_gate_forward / _backward;
 *     cp_train_inputs_workspace_bytes, cp_train_inputs;
 *     cp_pose_targets_track_det_workspace_bytes, cp_pose_targets_track_det;
 *     cp_adam_table_bytes, cp_adam_table_build, cp_adam_state_bytes, cp_adam_workspace_bytes, cp_adam_step;
 *     cp_grad_flat_elems, cp_grad_flat_offsets, cp_grad_pack_table_bytes, cp_grad_pack_table_build, cp_grad_pack;
 *     cp_dcnv2_backward_prec_workspace_bytes, cp_dcnv2_backward_prec, cp_dcnv2_backward_prec_mask;
 *     cp_draw_workspace_bytes, cp_draw_primitives, cp_draw_detections, cp_draw_tracks. */
#define CP_ABI_VERSION 7
const char* cp_version(void);
int cp_abi_version(void);
const char* cp_last_error(void);

/* ------------------------------------------------------------------------------------------
 * DCNv2 forward — replaces `_ext.dcn_v2_forward`
 *   models/networks/DCNv2/src/vision.cpp:5, dcn_v2.h:9-46, cuda/dcn_v2_cuda.cu:42-172 and its
 *   raw-pointer launcher `modulated_deformable_im2col_cuda` (cuda/dcn_v2_im2col_cuda.h:67-79).
 * Same tensor layouts as the reference (all contiguous NCHW float32):
 *   input [B,C,H,W], weight [Co,C,kh,kw], bias [Co], offset [B,dg*2*kh*kw,Ho,Wo] ((dh,dw)
 *   interleaved per tap), mask [B,dg*kh*kw,Ho,Wo], output [B,Co,Ho,Wo].
 * Ho = (H + 2*ph - (dh*(kh-1)+1)) / sh + 1 (Wo likewise), as dcn_v2_cuda.cu:75-76.
 * Every shape the reference op accepts is accepted (C % deformable_group == 0).  Two paths, same results:
 *   - what CenterPose uses (pose_dla_dcn.py:384: kh=kw=3, stride 1, pad 1, dilation 1, deformable_group 1,
 *     C % 16 == 0, Co > 32): the fused gather + matrix-core kernels (dcn16p.hip / dcn16.hip / igemm.hip);
 *   - anything else (the reference's own self-checks: DCNv2/testcpu.py:32-67 with 2 channels, :169-180 with
 *     deformable_group 2; other kernel sizes / strides / dilations): a generic float32 kernel (dcn_generic.hip),
 *     correct but not tuned.
 * `workspace` must hold cp_dcnv2_workspace_bytes(...) bytes (NHWC staging + packed weights; the generic path does not
 * touch it).
 * ------------------------------------------------------------------------------------------ */
size_t cp_dcnv2_workspace_bytes(int B, int C, int H, int W, int Co);
int cp_dcnv2_forward(cp_stream_t stream, const float* input, const float* weight, const float* bias,
                     const float* offset, const float* mask, float* output, int B, int C, int H, int W, int Co,
                     int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int deformable_group,
                     void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * DCNv2 backward — replaces `_ext.dcn_v2_backward`
 *   models/networks/DCNv2/src/vision.cpp:6, dcn_v2.h:38-80, cuda/dcn_v2_cuda.cu:206-340 (cpu/dcn_v2_cpu.cpp:109-238)
 *   and its launchers modulated_deformable_col2im{,_coord}_cuda (cuda/dcn_v2_im2col_cuda.cu:197-327).
 * Layouts and shape arguments are those of cp_dcnv2_forward (NCHW float32, offset channels (dh, dw) interleaved per
 * tap); grad_output [B,Co,Ho,Wo].  Outputs, all written (not accumulated), all required (no NULL):
 *   grad_input [B,C,H,W], grad_offset / grad_mask as offset / mask, grad_weight [Co,C,kh,kw], grad_bias [Co].
 * Semantics of the reference's op, quirks included:
 *   - a sample outside (-1, H) x (-1, W) contributes to no gradient; only in-image corners are read or written;
 *   - grad_input uses pad_h for BOTH axes, as the reference's col2im launchers do (dcn_v2_im2col_cuda.cu:368,
 *     dcn_v2_im2col_cpu.cpp:364); grad_offset / grad_mask / grad_weight use (pad_h, pad_w).  Only matters when
 *     pad_h != pad_w (never in CenterPose);
 *   - grad_offset is multiplied by the mask; grad_mask = sum_c grad_col * bilinear(input).
 * Arithmetic is exact float32 (v_mfma_f32_32x32x2_f32 contractions, float32 VALU elsewhere) whatever
 * cp_set_default_precision says: the precision mode governs the forward only.
 * Reproducibility: grad_offset, grad_mask, grad_weight and grad_bias are bitwise reproducible run to run; grad_input
 * is summed with float atomics and may differ in the last bits.
 * Two paths, same semantics: 3x3 / stride 1 / pad 1 / dilation 1 / deformable_group 1 / C % 16 == 0 (every CenterPose
 * and resdcn DCN layer) stages the input NHWC and scatters through an LDS halo tile; everything else runs a generic
 * kernel.  Shapes are checked as the forward checks them, and every tensor must have fewer than 2^31 elements;
 * CP_ERR_INVALID before any launch otherwise, or when workspace_bytes is below the query.  Launches on `stream` and
 * never synchronises.
 * ------------------------------------------------------------------------------------------ */
size_t cp_dcnv2_backward_workspace_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph,
                                         int pw, int dh, int dw, int deformable_group);
int cp_dcnv2_backward(cp_stream_t stream, const float* input, const float* weight, const float* offset,
                      const float* mask, const float* grad_output, float* grad_input, float* grad_offset,
                      float* grad_mask, float* grad_weight, float* grad_bias, int B, int C, int H, int W, int Co,
                      int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int deformable_group,
                      void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * DCNv2 backward, deterministic — the same five gradients as cp_dcnv2_backward with the same arguments and
 * semantics, every one of them bitwise reproducible run to run: grad_input is summed without any float atomic.
 * Covers the fast geometry only: 3x3 / stride 1 / pad 1 / dilation 1 / deformable_group 1 / C % 16 == 0.  Any other
 * geometry is refused before any launch (the query returns 0, the call CP_ERR_INVALID with the geometry in
 * cp_last_error), as are the shapes, NULL pointers and short workspaces cp_dcnv2_backward refuses.
 * The summation order of grad_input is contract:
 *   - for destination cell (b, y, x) and channel c the contributions  w_q * (grad_col * mask)  are added in ascending
 *     order of the entry id ((pix * 9 + tap) * 4 + q), pix = ho * Wo + wo the output pixel, q the bilinear corner
 *     (0: (y0, x0), 1: (y0, x0 + 1), 2: (y0 + 1, x0), 3: (y0 + 1, x0 + 1));
 *   - corners outside the image and samples outside (-1, H) x (-1, W) contribute nothing;
 *   - a list of more than 512 entries is cut, in list order, into consecutive chunks of 512; each chunk is summed
 *     serially from zero and the partial sums are added in chunk order.  A list of at most 512 entries is one serial sum.
 * The result for one image is therefore a function of that image's tensors alone: not of its position in the batch, of
 * the batch size, of how the call chunks the batch, or of the grid.  grad_offset / grad_mask sum the channels in
 * ascending order in one lane, grad_weight / grad_bias as in cp_dcnv2_backward.
 * The workspace is larger than cp_dcnv2_backward's (a sorted index of 16 bytes per (pixel, tap, corner) of a chunk of
 * images); nothing is read back to the host, the call is stream-ordered and can be captured in a graph.
 * ------------------------------------------------------------------------------------------ */
size_t cp_dcnv2_backward_det_workspace_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph,
                                             int pw, int dh, int dw, int deformable_group);
int cp_dcnv2_backward_det(cp_stream_t stream, const float* input, const float* weight, const float* offset,
                          const float* mask, const float* grad_output, float* grad_input, float* grad_offset,
                          float* grad_mask, float* grad_weight, float* grad_bias, int B, int C, int H, int W, int Co,
                          int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int deformable_group,
                          void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * DCNv2 backward with a precision argument — cp_dcnv2_backward (deterministic == 0) or cp_dcnv2_backward_det
 * (deterministic != 0) with `precision` (CP_PREC_*).  CP_PREC_F32 IS the call without it, for either `deterministic`
 * value: same kernels, same bits, same workspace size.  CP_PREC_F16X3 runs the two contractions of the fast geometry
 * (3x3 / stride 1 / pad 1 / dilation 1 / deformable_group 1 / C % 16 == 0) on v_mfma_f32_32x32x16_f16 with the
 * split-binary16 arithmetic of cp_conv2d_backward_prec_nhwc (hi*hi + hi*lo + lo*hi, float32 accumulation, exact
 * power-of-two pre-scales):
 *   - the modulated deformable columns of a chunk of images are materialised once, pixel-major, as split dwords (the
 *     float32 value the float32 weight gradient builds, times 2^e of the bound |max input| * |max mask|: a column is a
 *     convex combination of input values times one mask value, so the scaled column stays below 2^15 (1 + 2^-20) for any
 *     mask, sigmoid output or not), and grad_weight is the weight gradient of the 1x1 convolution 9C -> Co over them;
 *   - grad_col is the data gradient of that 1x1 convolution (weight scaled per column k = tap * C + c), pixel-major.
 * Everything else is the float32 code of the two calls: staging, the scatter or the deterministic index, grad_bias, the
 * copy-out.  grad_bias is therefore bit-identical between the modes; grad_offset, grad_mask and grad_input are computed
 * from an f16x3 grad_col and differ from the float32 mode's in the last bits (relative error of a product below 2^-20).
 * The generic geometry runs float32 in either mode.  cp_dcnv2_backward_prec_mask (host arithmetic) reports what a shape
 * gets: bit 0 = the weight gradient, bit 1 = grad_col runs in f16x3 (grad_col stays float32 for a chunk the f16x3
 * convolution kernels cannot address); 0 for CP_PREC_F32 and for the generic geometry; CP_ERR_INVALID (with a text)
 * for a refused shape or an unknown precision ("unknown precision" in cp_last_error), which the other two calls refuse
 * likewise before any launch.  A deterministic request outside the fast geometry is refused as cp_dcnv2_backward_det
 * refuses it.
 * Reproducibility in f16x3: the only new atomics are order-free |max| commits, so on the deterministic path all five
 * gradients stay bitwise reproducible run to run, and on the default path all but grad_input do.  The |max| slots are per
 * CALL (over the whole batch), so cp_dcnv2_backward_det's clause "the result for one image is a function of that image's
 * tensors alone" holds in this mode to the mode's tolerance, not to the bit: a pre-scale that differs by a power of two
 * between two batches can move the last bit of a `lo` half that falls into binary16's subnormals.  Results are
 * equivariant, bit for bit, under power-of-two scalings of input, weight, mask and grad_output (short of overflow and
 * underflow).  The contract of cp_dcnv2_backward_det itself is unchanged.
 * Workspace: grad_col and the split columns of a chunk EACH follow the 256 MiB rule (at most 256 MiB, or one image), so the
 * chunks are the float32 mode's; the mode adds that column buffer, one |max| slot block, the split copy of grad_output
 * (padded, like the float32 copy, to a multiple of 32 channels) and the binary16 weight pack, and is never smaller than the
 * float32 workspace; the query is exact and a shorter buffer is refused before any launch.
 * ------------------------------------------------------------------------------------------ */
size_t cp_dcnv2_backward_prec_workspace_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph,
                                              int pw, int dh, int dw, int deformable_group, int deterministic,
                                              int precision);
int cp_dcnv2_backward_prec(cp_stream_t stream, const float* input, const float* weight, const float* offset,
                           const float* mask, const float* grad_output, float* grad_input, float* grad_offset,
                           float* grad_mask, float* grad_weight, float* grad_bias, int B, int C, int H, int W, int Co,
                           int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int deformable_group,
                           int deterministic, int precision, void* workspace, size_t workspace_bytes);
int cp_dcnv2_backward_prec_mask(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                int dw, int deformable_group, int deterministic, int precision);

/* ------------------------------------------------------------------------------------------
 * Prediction-head block, forward and backward — replaces the per-head loop
 *   `for head in self.heads: z[head] = self.__getattr__(head)(y[-1])` and its autograd graph
 *   (models/networks/pose_dla_dcn.py:491-521 builds the Sequentials, :537-539 runs them; resnet_dcn.py likewise):
 *   head i = Conv2d(Cin, hid, 3, padding=1) -> ReLU -> Conv2d(hid, classes_i, 1), all n heads on one feature map.
 * feat [B,H,W,Cin] NHWC (the engine's layout; a channels_last torch tensor [B,Cin,H,W] is this memory).  The pointer
 * arrays are HOST arrays of n device pointers: w0[i] [hid,Cin,3,3], b0[i] [hid], w1[i] [classes_i,hid,1,1],
 * b1[i] [classes_i] in PyTorch layout; classes[i] in 1..64 (host ints); hid shared by the heads.
 *   forward   out[i] [B,classes_i,H,W] NCHW raw logits (what cp_model_forward returns).  Built from the library's
 *             convolution kernels; the 3x3 layer follows cp_set_default_precision like cp_conv2d_nhwc, the 1x1 is float32.
 *   backward  grad_out[i] [B,classes_i,H,W] NCHW, or NULL for a head the loss does not use: it contributes nothing
 *             and its four parameter gradients are written as zeros.  Outputs, written (not accumulated):
 *             grad_w0[i], grad_b0[i], grad_w1[i], grad_b1[i] in the parameters' layouts, and grad_feat [B,H,W,Cin] NHWC
 *             = the sum over the heads, or NULL (frozen backbone): the data-gradient contraction is then not launched.
 * Semantics are autograd's for the block; the ReLU gate is `hidden > 0` on the hidden value the backward recomputes.
 * Backward arithmetic is exact float32 (v_mfma_f32_32x32x2_f32 contractions, float32 VALU elsewhere) whatever
 * cp_set_default_precision says (that switch governs the forward only).  Nothing is kept between forward and backward: the backward recomputes a head's hidden
 * layer for cp_pose_heads_chunk_images(B, H, W, hid) images at a time (at most 256 MiB, or one image) inside `workspace`
 * and drops it; the hidden maps of all heads never exist together.
 * Reproducibility: every gradient, grad_feat included, is bitwise reproducible run to run (weight and bias gradients are
 * summed over pixel slabs in slab order, grad_feat over the heads in index order; no atomics).
 * Accepted: Cin % 32 == 0, hid % 32 == 0, any B, H, W >= 1, every tensor (and one image's hidden map) below 2^31
 * elements; anything else, a NULL pointer other than those named above or a workspace below the query returns
 * CP_ERR_INVALID with a cp_last_error() text before any launch (the queries return 0).  Launches on `stream`, never
 * synchronises.
 * cp_pose_heads_backward_prec_* are the backward's calls with a `precision` argument (CP_PREC_*), for the same block
 * (pose_dla_dcn.py:491-521, :537-539).  CP_PREC_F32 IS the calls without it: same kernels, same bits, same workspace
 * size.  CP_PREC_F16X3 runs the three wide contractions of a head on v_mfma_f32_32x32x16_f16 with the split-binary16
 * arithmetic of cp_conv2d_backward_prec_nhwc (hi*hi + hi*lo + lo*hi, float32 accumulation, exact power-of-two pre-scales):
 * the recomputed hidden layer on the kernel and operands an f16x3 cp_pose_heads_forward uses, so the gate is the one that
 * forward's ReLU applied; the 3x3 weight gradient; the data gradient.  The gate, grad_w1, grad_b0 and grad_b1 stay float32
 * sums in the float32 mode's orders.  The only atomics are order-free |max| commits, so every gradient stays bitwise
 * reproducible run to run, and is equivariant, bit for bit, under power-of-two scalings of grad_out.  The f16x3 workspace
 * is larger: a split copy of the whole feature map (made once per call, B H W Cin x 4 bytes), one of the hidden chunk, the
 * binary16 weight packs and two |max| slot blocks.  cp_pose_heads_backward_prec_mask (host arithmetic) reports what a shape
 * gets: bit 0 = the weight gradient, bit 1 = the data gradient, bit 2 = the recomputed hidden layer runs in f16x3 (the last
 * two stay float32 for a chunk of 0xf0000000 bytes or more); 0 for CP_PREC_F32; CP_ERR_INVALID (with a text) for a refused
 * shape or an unknown precision, which the other two calls refuse likewise before any launch, as they do everything
 * cp_pose_heads_backward refuses.
 * ------------------------------------------------------------------------------------------ */
int cp_pose_heads_chunk_images(int B, int H, int W, int hid);
size_t cp_pose_heads_forward_workspace_bytes(int B, int H, int W, int Cin, int hid, int n, const int* classes);
int cp_pose_heads_forward(cp_stream_t stream, const float* feat, int n, const float* const* w0, const float* const* b0,
                          const float* const* w1, const float* const* b1, const int* classes, float* const* out, int B,
                          int H, int W, int Cin, int hid, void* workspace, size_t workspace_bytes);
size_t cp_pose_heads_backward_workspace_bytes(int B, int H, int W, int Cin, int hid, int n, const int* classes);
int cp_pose_heads_backward(cp_stream_t stream, const float* feat, int n, const float* const* w0, const float* const* b0,
                           const float* const* w1, const float* const* b1, const int* classes,
                           const float* const* grad_out, float* const* grad_w0, float* const* grad_b0,
                           float* const* grad_w1, float* const* grad_b1, float* grad_feat, int B, int H, int W, int Cin,
                           int hid, void* workspace, size_t workspace_bytes);
size_t cp_pose_heads_backward_prec_workspace_bytes(int B, int H, int W, int Cin, int hid, int n, const int* classes,
                                                   int precision);
int cp_pose_heads_backward_prec(cp_stream_t stream, const float* feat, int n, const float* const* w0,
                                const float* const* b0, const float* const* w1, const float* const* b1, const int* classes,
                                const float* const* grad_out, float* const* grad_w0, float* const* grad_b0,
                                float* const* grad_w1, float* const* grad_b1, float* grad_feat, int B, int H, int W, int Cin,
                                int hid, int precision, void* workspace, size_t workspace_bytes);
int cp_pose_heads_backward_prec_mask(int B, int H, int W, int Cin, int hid, int precision);

/* ------------------------------------------------------------------------------------------
 * Backbone + heads — replaces `create_model` / `load_model` / `model(images, pre_images,
 *   pre_hms, pre_hm_hp)[-1]`  (models/model.py:26-87, models/networks/pose_dla_dcn.py:457-570,
 *   detectors/object_pose.py:135-138).
 *
 * arch: "dla_34" (DLA-34 + DCNv2 up-sampling) or "dlav1_34" (+ ConvGRU + GroupNorm heads).
 *       "resdcn_18|34|50|101|152": ResNet + three DCNv2 / ConvTranspose2d up-sampling stages (resnet_dcn.py), single frame.
 * heads: names/classes in the order of `opt.heads` (opts.py:394-426).
 * Parameters are fed one tensor at a time under the reference's state_dict names (HOST float32
 * pointers; `module.` prefixes are the caller's business as in model.py:43-48); finalize folds
 * eval-mode BatchNorm into per-channel scale/shift, re-packs every convolution as [tap][ci][co]
 * and uploads.  Unknown names are ignored (CP_OK) like load_model's "Drop parameter" branch;
 * finalize fails with CP_ERR_STATE if a required tensor is missing.
 * ------------------------------------------------------------------------------------------ */
int cp_model_create(const char* arch, int tracking_task, int num_heads, const char* const* head_names,
                    const int* head_classes, int head_conv, cp_model** out);
int cp_model_set_param(cp_model* m, const char* name, const float* host_data, int64_t numel);
int cp_model_finalize(cp_model* m);
void cp_model_destroy(cp_model* m);

/* Bytes of device scratch needed by cp_model_forward for a batch of B images of H x W -- under the model's precision and the
 * kernel-selection switches as they stand now: ask again after changing either.  cp_model_forward, cp_model_forward_tap and
 * cp_model_features refuse a smaller workspace_bytes with CP_ERR_INVALID before their first launch. */
size_t cp_model_workspace_bytes(cp_model* m, int B, int H, int W);
/* Bytes of that scratch the last pass over m reached (a forward / detect call, or the last dry pass of the query above); 0 before
 * the first.  The launch sequence depends on taps and switches; whatever it was, this is at most what the query returned. */
size_t cp_model_workspace_used(const cp_model* m);
/* Stand-alone 2x2 max-pool launches (DLA's Tree.downsample) of that same last pass.  An entry whose input's producer wrote the
 * pooled copy itself launches none: the count says which form the pass took at each of the four stride-2 entries. */
int cp_model_maxpool_launches(const cp_model* m);

/* images [B,3,H,W] NCHW (H, W multiples of 32).  pre_img [B,3,H,W], pre_hm [B,1,H,W],
 * pre_hm_hp [B,8,H,W] may each be NULL (pose_dla_dcn.py:312-318).  head_out[i] receives head i
 * as [B,classes_i,H/4,W/4] NCHW — raw logits, except that with sigmoid_hm != 0 the 'hm' and
 * 'hm_hp' heads are returned post-sigmoid (object_pose.py:136-138 fused into the epilogue). */
int cp_model_forward(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images,
                     const float* pre_img, const float* pre_hm, const float* pre_hm_hp, float* const* head_out,
                     int sigmoid_hm, void* workspace, size_t workspace_bytes);

/* The forward pass up to the tensor the heads read (pose_dla_dcn.py:531-536 `y[-1]`; resnet_dcn.py: the output of
 * deconv_layers), written to feat_out as [B,H/4,W/4,Cin] NHWC; no head is launched.  Arguments and workspace
 * (cp_model_workspace_bytes) as cp_model_forward.  Bit-identical to the "feat" tap (resdcn: "deconv_layers.17") up to the
 * layout.  For models whose head block has the plain conv3x3 -> ReLU -> conv1x1 form: dla_34 and resdcn_*; dlav1_34
 * (ConvGRU + GroupNorm heads) and hourglass (two stacks) return CP_ERR_STATE.  Feeds cp_pose_heads_forward / _backward. */
int cp_model_features(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                      const float* pre_hm, const float* pre_hm_hp, float* feat_out, void* workspace,
                      size_t workspace_bytes);

/* One frame batch end to end on the device: backbone + heads + sigmoid(hm, hm_hp) + decode — what
 * `ObjectPoseDetector.process` does (detectors/object_pose.py:131-165) — in ONE call.  Arguments as in
 * cp_model_forward and cp_decode; head_out[] receives the head tensors (hm / hm_hp post-sigmoid), det the
 * [B,K,118] records.  With use_graph != 0 the launch sequence is captured into a hipGraph on first use (keyed
 * by every pointer / size argument, so buffers must be reused) and replayed afterwards: a frame costs one graph
 * launch instead of ~120 kernel launches.  Needs a non-default stream; ignored while profiling is armed.
 * Output grids (H/4) x (W/4) above 32768 pixels are decoded by cp_decode_tiled's kernels (its size limits apply, and
 * the workspace grows with the grid); up to 32768 pixels the launches and workspace are cp_decode's.
 * Every head is computed on every output pixel, although the decode reads only hm and hm_hp everywhere and the regression
 * heads at the decoded peaks: the dense regression maps are a by-product.  A caller that wants the records asks
 * cp_model_detect_lean below and gets the maps on request (cp_model_dense_heads) at their old cost. */
size_t cp_model_detect_workspace_bytes(cp_model* m, int B, int H, int W, int K);
int cp_model_detect(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                    const float* pre_hm, const float* pre_hm_hp, float* const* head_out, int K, int rep_mode,
                    int fit_gaussian, float balance, int legacy_bool_mask, float* det, void* workspace,
                    size_t workspace_bytes, int use_graph);

/* cp_model_detect without the dense regression maps.  Sequence, on one stream: backbone -> hm and hm_hp densely (sigmoided) ->
 * peaks (NMS + top-K of the 1 + 8 maps) -> every other head evaluated ONLY at the pixels the decode reads it at (hp_offset at
 * the K peaks of each joint map, the rest at the K centre peaks: the fused 3x3 + ReLU + 1x1 head as an implicit GEMM over a
 * pixel list, same operands and pre-scale as the dense launch) -> records.  Per image 4 heads at K pixels and one at 8 K instead
 * of 5 heads at (H/4)(W/4).
 *   cp_model_lean_supported  1 when the model, shape, precision and switch setting take this path: f16x3, no ConvGRU, the
 *                            grouped fused-head form (dla_34, hourglass).  Otherwise 0, and the entries below return
 *                            CP_ERR_STATE / 0 bytes: call cp_model_detect.
 *   head_out[i]   hm, hm_hp: [B,classes,H/4,W/4] as cp_model_detect; other entries are not read.
 *   table_out[i]  every other head: its compact table.  Centre-indexed heads [B,classes,K]: entry k = the head at
 *                 pk_ind[b][0][k]; hp_offset [B,8,2,K]: entry k of joint j = the head at pk_ind[b][j + 1][k].
 *   pk_score, pk_ind  [B,9,K] float32 / int32: the peaks (score desc; index = y * (W/4) + x), map 0 = hm, 1..8 = hm_hp.
 *   det           as cp_model_detect.  Against it: score and cls are bit-equal; a gathered entry differs from the dense map's
 *                 by float32 summation order and last bits of the second product's pre-scale (<= 2e-5 * max(1, max|head|)).
 * The feature map the heads read stays in `workspace` until the next call that uses the model or the workspace:
 *   cp_model_dense_heads  writes the dense [B,classes,H/4,W/4] maps of every head other than hm / hm_hp from it (head_out
 *                         indexed like the model's heads; hm / hm_hp entries ignored), bit-identical to cp_model_forward's;
 *   cp_model_heads_at     evaluates those heads at a caller's pixel list index[B][n] (y * (W/4) + x, values outside the map
 *                         are clamped into it; duplicates allowed) into table_out[i] = [B,classes,n].
 * Both return CP_ERR_STATE when no feature map is kept. */
int cp_model_lean_supported(cp_model* m, int B, int H, int W);
size_t cp_model_detect_lean_workspace_bytes(cp_model* m, int B, int H, int W, int K);
int cp_model_detect_lean(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                         const float* pre_hm, const float* pre_hm_hp, float* const* head_out, float* const* table_out,
                         float* pk_score, int* pk_ind, int K, int rep_mode, int fit_gaussian, float balance,
                         int legacy_bool_mask, float* det, void* workspace, size_t workspace_bytes, int use_graph);
int cp_model_dense_heads(cp_model* m, cp_stream_t stream, float* const* head_out);
size_t cp_model_heads_at_workspace_bytes(cp_model* m, int B, int n);
int cp_model_heads_at(cp_model* m, cp_stream_t stream, const int* index, int n, float* const* table_out, void* workspace,
                      size_t workspace_bytes);

/* Debug/parity aid: same as cp_model_forward but additionally copies the named intermediate
 * activation (names follow the reference module paths, e.g. "base.level3", "dla_up.ida_2.node_3",
 * "feat", "convGRU.step1") to tap_out as NCHW.  tap_dims receives {C,H,W}. */
int cp_model_forward_tap(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images,
                         const float* pre_img, const float* pre_hm, const float* pre_hm_hp, float* const* head_out,
                         int sigmoid_hm, void* workspace, size_t workspace_bytes, const char* tap_name,
                         float* tap_out, int* tap_dims);

/* Arithmetic of the convolution / DCNv2 contractions (activations, weights at the boundary, accumulation and
 * epilogues are float32 in both modes):
 *   CP_PREC_F32   (0) exact float32 matrix instructions (v_mfma_f32_32x32x2_f32), 157 TFLOP/s ceiling
 *   CP_PREC_F16X3 (1) every float32 operand split into two binary16 numbers, products evaluated as
 *                     hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with float32 accumulation (relative product
 *                     error < 2^-20), 833 TFLOP/s ceiling; layers whose channel counts are not multiples of 32
 *                     (the 16-channel stem levels, final 1x1 heads) stay on the exact path.
 * cp_set_default_precision affects models created afterwards and the stand-alone cp_conv2d_nhwc / cp_dcnv2_forward. */
#define CP_PREC_F32 0
#define CP_PREC_F16X3 1
int cp_set_default_precision(int precision);
int cp_model_set_precision(cp_model* m, int precision);

/* Per-launch timing of the implicit-GEMM kernels with HIP events recorded on the launch stream
 * (replaces the reference's wall-clock `torch.cuda.synchronize()` fences, base_detector.py:466-498).
 * cp_model_profile(m, 1) arms it; every conv / DCN launch of later forwards is bracketed by an event
 * pair.  cp_model_profile_read drains them: out[v*4 + 0..3] = {launches, total milliseconds, total
 * algorithmic FLOPs (2*M*Cout*KH*KW*Cin), total algorithmic bytes (input + output + weights
 * [+ offsets/mask] [+ residual], float32)} per kernel variant v in [0, CP_NUM_KERNEL_VARIANTS). */
#define CP_NUM_KERNEL_VARIANTS 46
int cp_num_kernel_variants(void); /* the value the LIBRARY was built with: size cp_model_profile_read's buffer from it */
int cp_model_profile(cp_model* m, int enable);
int cp_model_profile_read(cp_model* m, double* out, int num_variants);
const char* cp_kernel_variant_name(int v);
/* The same launches grouped by what they compute (the figures BASELINE.json's north_star names: DCNv2 traffic, 1x1
 * convolution MFMA rate, decode time).  Valid after cp_model_profile_read: out[r*4 + 0..3] = {launches, milliseconds,
 * algorithmic FLOPs, algorithmic bytes} of role r since the previous read. */
#define CP_ROLE_CONV 0        /* 3x3 / 7x7 convolutions of the base network and the hourglass */
#define CP_ROLE_CONV1X1 1     /* 1x1 projections, Root nodes, hourglass skips */
#define CP_ROLE_DCN 2         /* DCNv2 gather + contraction (pose_dla_dcn.py:386-389) */
#define CP_ROLE_DCN_OFFSET 3  /* conv_offset_mask Cin->27 (dcn_v2.py:105-111) */
#define CP_ROLE_HEAD 4        /* 3x3 of a prediction head (fused heads: 3x3 + 1x1) */
#define CP_ROLE_HEAD_FINAL 5  /* final 1x1 of an un-fused head */
#define CP_ROLE_GRU 6         /* ConvGRU convolutions (convGRU.py:32-39) */
#define CP_ROLE_LOWC 7        /* stem / level0 / level1 direct kernels (f16x3 mode) */
#define CP_ROLE_DECODE 8      /* cp_model_detect's decode launch (both kernels) */
#define CP_ROLE_DECONV 9      /* dense ConvTranspose2d(k=4, s=2) + BatchNorm + ReLU of the resdcn up-sampling */
#define CP_NUM_ROLES 10
int cp_num_roles(void);
int cp_model_profile_roles(cp_model* m, double* out, int num_roles);
const char* cp_role_name(int role);

/* ------------------------------------------------------------------------------------------
 * Generic NHWC convolution (exposed for unit tests of the implicit-GEMM kernel).
 *   x [B,H,W,Cin] NHWC, w [Cout,Cin,KH,KW] (reference/PyTorch layout, DEVICE), scale/shift/
 *   residual may be NULL.  out [B,Ho,Wo,Cout] NHWC.  act: 0 none, 1 relu, 2 sigmoid.
 *   Any Cout is accepted with scale / shift ([Cout] each): the call copies them into zero-padded regions of the
 *   workspace, which the kernels read up to their N tile.  The N tile follows the Cout passed in (16 up to 16, 32 up to
 *   32, 128 for multiples of 128, else 64), so a caller that used to pad the weight, scale and shift by hand to the tile
 *   gets the same kernel for every width but 65..127: those, padded to 128 before, now run on the 64-wide tile.
 *   One more case under the f16x3 precision: the row-streaming kernel of 64 -> (<= 32) channel 3x3 layers stores 16
 *   bytes at a time and needs an output row of Cout % 4 == 0 floats, so such a layer with 27 true channels, padded to 32
 *   by hand before, now runs on the halo kernel of the same 32-wide tile.
 * ------------------------------------------------------------------------------------------ */
size_t cp_conv2d_workspace_bytes(int Cin, int Cout, int KH, int KW);
int cp_conv2d_nhwc(cp_stream_t stream, const float* x, const float* w, const float* scale, const float* shift,
                   const float* residual, float* out, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                   int stride, int pad, int act, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * Conv2d backward — replaces torch.nn.Conv2d's backward in models/networks/pose_dla_dcn.py:48-62 (BasicBlock's 3x3
 *   pairs), the Root / project 1x1 layers, ResNet's 1x1 stride-2 down-samples and DCNv2/dcn_v2.py:118-128
 *   (conv_offset_mask): autograd's gradients of out = conv2d(x, w) + bias with dilation 1 and groups 1.
 * Layouts are cp_conv2d_nhwc's: x [B,H,W,Cin] NHWC, w [Cout,Cin,KH,KW] (PyTorch layout), grad_out [B,Ho,Wo,Cout] NHWC with
 * Ho = (H + 2 pad - KH) / stride + 1 (Wo likewise).  Outputs, written (not accumulated): grad_w [Cout,Cin,KH,KW],
 * grad_bias [Cout] (sums of grad_out over images and pixels) and grad_x [B,H,W,Cin] NHWC.  A NULL grad_x or grad_bias is
 * not computed and not touched.  y (the ACTIVATED forward output, [B,Ho,Wo,Cout]) or NULL: when given, the layer was
 * relu(conv + bias) and grad_out is gated by y > 0 wherever it is read.  BatchNorm scale / shift and residual inputs of the
 * forward are not part of this operator: callers compose them.
 * Arithmetic is float32 whatever cp_set_default_precision says (that switch governs the forward only); every sum has a
 * fixed order and there are no atomics, so all outputs are bitwise reproducible call to call.
 * cp_conv2d_backward_prec_* are the same three calls with a `precision` argument (CP_PREC_*).  CP_PREC_F32 IS the calls
 * without it: same kernels, same bits, same workspace size.  CP_PREC_F16X3 runs the two contractions of the MFMA path --
 * the weight gradient and the data gradient, both strides -- on v_mfma_f32_32x32x16_f16: grad_out (gated and padded), x
 * and w are pre-scaled by exact powers of two (grad_out and x per tensor from one |max| pass each, w per input channel),
 * split into two binary16 numbers hi + lo, and every product block is hi*hi + hi*lo + lo*hi with float32 accumulation;
 * the scales are undone by exact power-of-two multiplies.  The relative error of a product is below 2^-20, so accuracy
 * stays float32-class; the gate, the pad lanes and grad_bias are float32, every sum still has a fixed order and the
 * gradients are bitwise reproducible call to call; results are equivariant, bit for bit, under power-of-two scalings of
 * x, w and grad_out.  The low-channel and the generic path are float32 in either mode.  The f16x3 workspace is larger (the
 * split copies of grad_out and x).  cp_conv2d_backward_prec_mask (host arithmetic) reports what a geometry gets: bit 0 =
 * the weight gradient, bit 1 = the data gradient runs in f16x3; 0 for CP_PREC_F32 and off the MFMA path; CP_ERR_INVALID
 * (with a text) for a refused geometry or an unknown precision, which the other two calls refuse likewise before any launch.
 * MFMA path (v_mfma_f32_32x32x2_f32): KH == KW in {1, 3}, stride in {1, 2}, pad == KH / 2, Cin % 32 == 0, any H, W >= 1 and
 * any Cout (grad_out is staged once into the workspace, zero-padded to a multiple of 32 channels: 27 is the case that
 * matters).  Low-channel path (v_mfma_f32_16x16x4_f32): KH == KW == 3, pad == 1, stride in {1, 2}, Cin == 16, Cout in
 * {16, 32} and B * Ho * Wo >= 4096 output pixels, any H, W (dla_34's level0 / level1 layers).  Everything else with KH, KW in
 * 1..7, stride in 1..4, 0 <= pad < min(KH, KW), Cin % 4 == 0 takes plain deterministic kernels that are correct, not fast.
 * cp_conv2d_backward_path reports which of the three (CP_CONV_BWD_*) cp_conv2d_backward_nhwc takes for a geometry, or
 * CP_ERR_INVALID (with a cp_last_error() text) for one the operator refuses; host arithmetic.
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch (the query returns 0): a NULL pointer other
 * than those named above, a workspace below the query, B / H / W / Cout < 1, Cin % 4 != 0, another geometry, an empty output
 * grid, a tensor of 2^31 elements or more.  The query is host arithmetic; need_grad_x == 0 leaves out the data gradient's
 * operands.  Launches on `stream`, never synchronises.
 * ------------------------------------------------------------------------------------------ */
#define CP_CONV_BWD_GENERIC 0
#define CP_CONV_BWD_MFMA 1
#define CP_CONV_BWD_LOWC 2
int cp_conv2d_backward_path(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
size_t cp_conv2d_backward_workspace_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                          int need_grad_x);
int cp_conv2d_backward_nhwc(cp_stream_t stream, const float* x, const float* w, const float* y_or_null,
                            const float* grad_out, float* grad_x_or_null, float* grad_w, float* grad_bias_or_null, int B,
                            int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, void* workspace,
                            size_t workspace_bytes);
size_t cp_conv2d_backward_prec_workspace_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                               int need_grad_x, int precision);
int cp_conv2d_backward_prec_nhwc(cp_stream_t stream, const float* x, const float* w, const float* y_or_null,
                                 const float* grad_out, float* grad_x_or_null, float* grad_w, float* grad_bias_or_null,
                                 int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                 int precision, void* workspace, size_t workspace_bytes);
int cp_conv2d_backward_prec_mask(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                 int precision);

/* ------------------------------------------------------------------------------------------
 * BatchNorm2d for training, fused with the residual add and the ReLU — replaces the nn.BatchNorm2d(momentum=0.1) ->
 *   `out += residual` -> ReLU chains of models/networks/pose_dla_dcn.py:40-62 (BasicBlock), pose_dla_dcn.py:150-168 (Root),
 *   pose_dla_dcn.py:381 (the DCN's actf) and resnet_dcn.py, forward and backward:
 *     y = act((x - mean) * invstd * gamma + beta [+ residual]),  act: 0 none, 1 relu.
 * All tensors float32; x, residual, y, grad_out, grad_x, grad_residual [B,H,W,C] NHWC; gamma, beta, the statistics and their
 * gradients [C].  C % 4 == 0, 4 <= C <= 4096; every pointer 16-byte aligned.  NULL gamma / beta mean 1 / 0 (affine=False).
 * Forward, training != 0: mean and the biased variance of the batch (over B*H*W values per channel, at least 2) are
 * computed without forming E[x^2] - mean^2 (pivoted sums merged by Chan's rule); save_mean = mean, save_invstd =
 * 1 / sqrt(var + eps); running_mean / running_var, when given, become (1 - momentum) * r + momentum * stat, the variance
 * unbiased by n / (n - 1).  Forward, training == 0: the running pair (required) gives save_mean and save_invstd and is left
 * alone.  y must not alias x.
 * Backward: g = grad_out, gated by y > 0 when y (the forward's ACTIVATED output) is given; xhat = (x - save_mean) * save_invstd;
 * grad_beta = sum g, grad_gamma = sum g * xhat; grad_x = gamma * invstd * (g - grad_beta / n - xhat * grad_gamma / n) in
 * training, gamma * invstd * g in evaluation; grad_residual = g.  Outputs are written, not accumulated; a NULL output is not
 * computed and not touched.  (With y == NULL grad_residual is grad_out itself: callers pass NULL and reuse grad_out.)
 * No atomics; every sum has a fixed order that depends on the shape alone: all outputs are bitwise reproducible call to call.
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch (the query returns 0 for the shape ones): a NULL
 * pointer other than those named *_or_null, a workspace below the query, B / H / W < 1, C % 4 != 0 or outside 4..4096,
 * training with B*H*W < 2, evaluation without the running pair, act outside {0, 1}, eps < 0, a tensor of 2^31 elements or
 * more.  The query is host arithmetic, serves both calls and is monotone in B.  Launches on `stream`, never synchronises.
 * ------------------------------------------------------------------------------------------ */
size_t cp_batchnorm_workspace_bytes(int B, int H, int W, int C);
int cp_batchnorm_forward_nhwc(cp_stream_t stream, const float* x, const float* gamma_or_null, const float* beta_or_null,
                              const float* residual_or_null, float* running_mean_or_null, float* running_var_or_null,
                              float* y, float* save_mean, float* save_invstd, int B, int H, int W, int C, int training,
                              float momentum, float eps, int act, void* workspace, size_t workspace_bytes);
int cp_batchnorm_backward_nhwc(cp_stream_t stream, const float* x, const float* y_or_null, const float* grad_out,
                               const float* gamma_or_null, const float* save_mean, const float* save_invstd,
                               float* grad_x_or_null, float* grad_residual_or_null, float* grad_gamma_or_null,
                               float* grad_beta_or_null, int B, int H, int W, int C, int training, void* workspace,
                               size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * SyncBatchNorm — the training BatchNorm above with the statistics of the GLOBAL batch of a process group (one process per
 *   GPU, the batch sharded by images), and the gradients that go with them.  The library holds no communicator: each pass is
 *   two calls with one all-gather of the caller's between them, and every rank calls them with the same `world` and C.
 * Tensors, layouts, NULL conventions and constraints are cp_batchnorm_*'s; the workspace is cp_batchnorm_workspace_bytes'.
 * Forward, phase A, cp_batchnorm_sync_stats_nhwc: this rank's record = mean[C] | M2[C] | count, M2 = sum (x - mean)^2 over
 *   the rank's B*H*W values per channel (one value is allowed: M2 = 0).  A record is cp_batchnorm_sync_record_floats(C) =
 *   2 C + 4 floats (0 for a refused C); the count is carried exactly, as a 32-bit integer's bit pattern in the first word of
 *   the last 16-byte slot (the other three words zero), so the records must be moved as bits (an all-gather), never summed.
 * Forward, phase B, cp_batchnorm_sync_forward_nhwc: records = [world][record_floats] in rank order.  The ranks are merged by
 *   Chan's many-way rule in rank order about rank 0's mean, with the expressions that merge a tensor's slabs in
 *   cp_batchnorm_forward_nhwc: n = sum n_r, mean = m_0 + sum n_r (m_r - m_0) / n, M2 = sum M2_r + n_r (m_r - mean)^2,
 *   save_invstd = 1 / sqrt(M2 / n + eps); running_mean / running_var are updated as above, the variance unbiased by the
 *   global n / (n - 1).  Every rank therefore computes bit-identical save_mean, save_invstd and running statistics.
 *   *save_count (one float on the device) = n; the backward reads it there.  Then y as above.  Every record's count must be
 *   at least 1 (not checked: the records are on the device).
 * Backward, phase A, cp_batchnorm_sync_backward_reduce_nhwc: with the global save_mean / save_invstd, sums = [2][C]: sum g
 *   and invstd * sum g (x - mean) over this rank's values (g gated by y > 0 as above); grad_beta / grad_gamma, when given, are
 *   copies: the LOCAL sums, which a data-parallel gradient reduction averages like every other parameter gradient.
 * Backward, phase B, cp_batchnorm_sync_backward_apply_nhwc: sums_all = [world][2][C] in rank order is added in rank order
 *   (S1, S2), then grad_x = gamma * invstd * (g - S1 / n - xhat * S2 / n) with n = *save_count; grad_residual = g.
 * With world == 1 every output is bitwise that of cp_batchnorm_forward_nhwc / _backward_nhwc (training).  No atomics; all
 * outputs are bitwise reproducible call to call.
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch: what cp_batchnorm_* refuses for the shape, NULL
 * pointers, alignment and the workspace; world outside 1..1024; a global count below 2 (world == 1 with B*H*W < 2).  Launch
 * on `stream`, never synchronise.
 * ------------------------------------------------------------------------------------------ */
int cp_batchnorm_sync_record_floats(int C);
int cp_batchnorm_sync_stats_nhwc(cp_stream_t stream, const float* x, float* record, int B, int H, int W, int C, void* workspace,
                                 size_t workspace_bytes);
int cp_batchnorm_sync_forward_nhwc(cp_stream_t stream, const float* x, const float* gamma_or_null, const float* beta_or_null,
                                   const float* residual_or_null, float* running_mean_or_null, float* running_var_or_null,
                                   float* y, float* save_mean, float* save_invstd, float* save_count, const float* records,
                                   int world, int B, int H, int W, int C, float momentum, float eps, int act, void* workspace,
                                   size_t workspace_bytes);
int cp_batchnorm_sync_backward_reduce_nhwc(cp_stream_t stream, const float* x, const float* y_or_null, const float* grad_out,
                                           const float* save_mean, const float* save_invstd, float* sums,
                                           float* grad_gamma_or_null, float* grad_beta_or_null, int B, int H, int W, int C,
                                           void* workspace, size_t workspace_bytes);
int cp_batchnorm_sync_backward_apply_nhwc(cp_stream_t stream, const float* x, const float* y_or_null, const float* grad_out,
                                          const float* gamma_or_null, const float* save_mean, const float* save_invstd,
                                          const float* sums_all, int world, const float* save_count, float* grad_x_or_null,
                                          float* grad_residual_or_null, int B, int H, int W, int C, void* workspace,
                                          size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * GroupNorm for training, fused with the ReLU — nn.GroupNorm(G, C) and the ReLU behind it in the dlav1_34 heads of
 *   models/networks/pose_dla_dcn.py:491-521 (groups by models/networks/GN.py), forward and backward:
 *     y = act(xhat * gamma + beta),  xhat = (x - mean) * invstd,  act: 0 none, 1 relu.
 * All tensors float32; x, y, grad_out, grad_x [B,H,W,C] NHWC; gamma, beta and their gradients [C]; save_mean, save_invstd
 * [B][G].  NULL gamma / beta mean 1 / 0 (affine=False).  The statistics are per (image, group) over n = (C / G) H W values,
 * the variance biased, never formed as E[x^2] - mean^2 (pivoted sums merged by Chan's rule).  y must not alias x.
 * Backward: g = grad_out, gated by y > 0 when y (the forward's ACTIVATED output) is given; grad_beta[c] = sum g and
 * grad_gamma[c] = sum g * xhat over images and pixels; grad_x = invstd * (g * gamma - s1 / n - xhat * s2 / n) with s1 = sum g *
 * gamma and s2 = sum g * gamma * xhat over the (image, group).  Outputs are written, not accumulated; a NULL output is not
 * computed and not touched.
 * No atomics; every sum has a fixed order that depends on the shape alone: all outputs are bitwise reproducible call to call.
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch (the query returns 0 for the shape ones): a NULL
 * pointer other than those named *_or_null, a workspace below the query, B / H / W < 1, C % 4 != 0 or outside 4..4096, G < 1
 * or C % G != 0, C / G neither 1, 2 nor a multiple of 4 (a 16-byte lane must not straddle a group boundary unevenly: 48
 * channels in 16 groups), act outside {0, 1}, eps < 0, a tensor of 2^31 elements or more, a pointer that is not 16-byte
 * aligned.  The query is host arithmetic, serves both calls and is monotone in B.  Launches on `stream`, never synchronises.
 * ------------------------------------------------------------------------------------------ */
size_t cp_groupnorm_workspace_bytes(int B, int H, int W, int C, int G);
int cp_groupnorm_forward_nhwc(cp_stream_t stream, const float* x, const float* gamma_or_null, const float* beta_or_null,
                              float* y, float* save_mean, float* save_invstd, int B, int H, int W, int C, int G, float eps,
                              int act, void* workspace, size_t workspace_bytes);
int cp_groupnorm_backward_nhwc(cp_stream_t stream, const float* x, const float* y_or_null, const float* grad_out,
                               const float* gamma_or_null, const float* save_mean, const float* save_invstd,
                               float* grad_x_or_null, float* grad_gamma_or_null, float* grad_beta_or_null, int B, int H, int W,
                               int C, int G, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * The ConvGRU's gate arithmetic for training — ConvGRUCell.forward of models/networks/convGRU.py:32-39 behind its six
 *   convolutions, forward and backward, float32, one pass each, no workspace:
 *     x3 = [Wir x + b | Wiz x + b | Win x + b] and h3 = [Whr h | Whz h | Whn h] as [M][3 Ch] (M = B H W pixel rows of NHWC
 *     tensors); hprev, hout, grad_hout, grad_hprev [M][Ch]; grad_x3, grad_h3 [M][3 Ch].
 *     r = sigmoid(x3r + h3r), z = sigmoid(x3z + h3z), n = tanh(x3n + r * h3n), hout = (1 - z) * n + z * hprev.
 * h3 == NULL is step 0 of every forward: h = 0 and h3 = 0 (the hidden-side convolutions have no bias and are not run);
 * hprev and the two hidden-side gradients must then be NULL too.
 * Backward: r, z and n are recomputed from the inputs (no gate tensor is kept).  With g = grad_hout: da_n = g (1 - z) (1 - n^2),
 * grad_x3n = da_n, grad_h3n = da_n r, grad_x3r = grad_h3r = da_n h3n r (1 - r), grad_x3z = grad_h3z = g (hprev - n) z (1 - z),
 * grad_hprev = g z.  grad_x3 is always written; a NULL grad_h3 / grad_hprev is not computed.  Bitwise reproducible.
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch: a NULL pointer other than those named *_or_null,
 * h3 without hprev or the reverse, a hidden-side gradient at step 0, M < 1, Ch % 4 != 0 or outside 4..1024, a tensor of 2^31
 * elements or more, a pointer that is not 16-byte aligned.  Launches on `stream`, never synchronises.
 * ------------------------------------------------------------------------------------------ */
int cp_gru_gate_forward(cp_stream_t stream, const float* x3, const float* h3_or_null, const float* hprev_or_null, float* hout,
                        int M, int Ch);
int cp_gru_gate_backward(cp_stream_t stream, const float* x3, const float* h3_or_null, const float* hprev_or_null,
                         const float* grad_hout, float* grad_x3, float* grad_h3_or_null, float* grad_hprev_or_null, int M,
                         int Ch);

/* Dense ConvTranspose2d(Cin, Cout, kernel 4, stride 2, padding 1, bias=False) followed by an optional per-channel affine
 * and ReLU (resnet_dcn.py's deconv `up` layers with their BatchNorm): x [B,H,W,Cin] NHWC, w [Cin,Cout,4,4] (PyTorch
 * layout, DEVICE), scale/shift [Cout] or NULL, out [B,2H,2W,Cout] NHWC.  act: 0 none, 1 relu.  Cin % 32 == 0.
 * Precision follows cp_set_default_precision (exact f32 or f16x3 with range-safe scaling). */
size_t cp_conv_transpose2d_workspace_bytes(int Cin, int Cout);
int cp_conv_transpose2d_nhwc(cp_stream_t stream, const float* x, const float* w, const float* scale, const float* shift,
                             float* out, int B, int H, int W, int Cin, int Cout, int act, void* workspace,
                             size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * ConvTranspose2d for training — the up-sampling layers of both backbone families, float32 NHWC:
 *   depth-wise  IDAUp's `up` of models/networks/pose_dla_dcn.py:402-417: ConvTranspose2d(C, C, K = 2 f, stride f, padding f / 2,
 *               groups C, bias=False), w [C,1,K,K] (PyTorch layout), x [B,H,W,C] -> [B,fH,fW,C].
 *   dense       the deconv layers of models/networks/resnet_dcn.py:232-240: ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1,
 *               bias=False), w [Cin,Cout,4,4], x [B,H,W,Cin] -> [B,2H,2W,Cout] (forward: cp_conv_transpose2d_nhwc above).
 * cp_conv_transpose2d_dw_nhwc is the depth-wise forward, out = add_or_null + up(x): the kernel the engine's IDAUp runs, with
 * the `layers[i] + layers[i - 1]` of the following node fused (add and out [B,fH,fW,C]; NULL: no addend).  No workspace.
 * cp_conv_transpose2d_backward_nhwc: autograd's gradients of either layer from grad_out [B, stride H, stride W, Cout]:
 * grad_w in w's layout and grad_x [B,H,W,Cin], written, not accumulated; a NULL grad_x is not computed and not touched.
 * Arithmetic is float32 whatever cp_set_default_precision says (the _prec calls below take their own); every sum has a fixed order and there are no atomics, so all
 * outputs are bitwise reproducible call to call.
 * Accepted geometries:
 *   depth-wise  groups == Cin == Cout, stride in {2, 4}, K == 2 stride, pad == stride / 2, C % 4 == 0, and the [K K][C] float
 *               weight table within the 60 KiB of LDS the kernels stage it in: C <= 960 at stride 2, C <= 240 at stride 4
 *               (the forward call takes the same set); tensors below 2^30 elements (32-bit byte offsets)
 *   dense       groups == 1, K == 4, stride == 2, pad == 1, Cin % 32 == 0, Cout % 32 == 0
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch (the query returns 0): a NULL pointer other than
 * those named *_or_null, a workspace below the query, B / H / W < 1, another geometry, a tensor of 2^31 elements or more, a
 * pointer that is not 16-byte aligned.  The query is host arithmetic and monotone in B; need_grad_x == 0 leaves out the data
 * gradient's operands.  Launches on `stream`, never synchronises.
 *
 * cp_conv_transpose2d_backward_prec_* are the same calls with a `precision` argument (CP_PREC_*).  CP_PREC_F32 IS the calls
 * above: the same kernels, bits and workspace size.  CP_PREC_F16X3 runs the dense layer's two contractions in the
 * split-binary16 arithmetic of cp_conv2d_backward_prec_nhwc (hi*hi + hi*lo + lo*hi, float32 accumulation, exact power-of-two
 * pre-scales from |max| slots): the weight gradient on that operator's slab kernel with grad_out as the input and x as the
 * output gradient (16 taps, stride 2, pad 1), the data gradient as the 4x4 / stride-2 convolution of grad_out on the forward's
 * f16x3 implicit GEMM, w packed with a power-of-two scale per row.  A data gradient no f16x3 kernel takes (a tensor of
 * 0xf0000000 bytes or more) stays float32.  The depth-wise layers have no matrix product: they are the float32 call bit for
 * bit.  Fixed summation order, no atomics but the |max| slots': bitwise reproducible call to call.  The workspace is larger
 * (the |max| slots, the split copies of grad_out and x, the packed weight).  cp_conv_transpose2d_backward_prec_mask (host
 * arithmetic) reports what a geometry gets: bit 0 = the weight gradient, bit 1 = the data gradient runs in f16x3; 0 for
 * CP_PREC_F32 and for depth-wise layers; CP_ERR_INVALID for a refused geometry.  Any other `precision` is refused.
 * ------------------------------------------------------------------------------------------ */
int cp_conv_transpose2d_dw_nhwc(cp_stream_t stream, const float* x, const float* w, const float* add_or_null, float* out,
                                int B, int H, int W, int C, int f);
size_t cp_conv_transpose2d_backward_workspace_bytes(int B, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                                                    int groups, int need_grad_x);
int cp_conv_transpose2d_backward_nhwc(cp_stream_t stream, const float* x, const float* w, const float* grad_out,
                                      float* grad_x_or_null, float* grad_w, int B, int H, int W, int Cin, int Cout, int K,
                                      int stride, int pad, int groups, void* workspace, size_t workspace_bytes);
size_t cp_conv_transpose2d_backward_prec_workspace_bytes(int B, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                                                         int groups, int need_grad_x, int precision);
int cp_conv_transpose2d_backward_prec_nhwc(cp_stream_t stream, const float* x, const float* w, const float* grad_out,
                                           float* grad_x_or_null, float* grad_w, int B, int H, int W, int Cin, int Cout, int K,
                                           int stride, int pad, int groups, int precision, void* workspace,
                                           size_t workspace_bytes);
int cp_conv_transpose2d_backward_prec_mask(int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int groups,
                                           int precision);

/* ------------------------------------------------------------------------------------------
 * MaxPool2d for training — Tree.downsample of models/networks/pose_dla_dcn.py:211-224 (kernel 2, stride 2, padding 0; it floors,
 *   so an odd last row / column belongs to no window) and the maxpool of models/networks/resnet_dcn.py (kernel 3, stride 2,
 *   padding 1; padding counts as -inf), forward and backward, float32 NHWC:
 *   x, grad_x [B,H,W,C]; out, grad_out [B,Ho,Wo,C], Ho = (H + 2 pad - kernel) / 2 + 1 (Wo likewise).
 * The winner of a window is torch's in both calls: the taps inside the image are scanned in row-major order and a tap replaces
 * the current one only if it is strictly greater (or a NaN), so a window of equal values (the zeros a ReLU leaves) selects its
 * first tap.  The forward copies the winners, so it is bitwise torch's.  The backward keeps no index tensor: every grad_x
 * element recomputes, from x, the winner of each window that covers it (one at kernel 2, up to four at kernel 3) and adds that
 * window's grad_out where it is the winner itself, windows in (row, column) order; elements that no window covers or that never
 * win are exact zeros.  grad_x is written, not accumulated.  No atomics; bitwise reproducible call to call.
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch: a NULL pointer, another (kernel, stride, pad),
 * B / H / W < 1, C % 4 != 0, an empty output (H or W below the window), a pointer that is not 16-byte aligned, a tensor of
 * 2^31 elements or more.  No workspace.  Launches on `stream`, never synchronises.
 * ------------------------------------------------------------------------------------------ */
int cp_maxpool2d_forward_nhwc(cp_stream_t stream, const float* x, float* out, int B, int H, int W, int C, int kernel, int stride,
                              int pad);
int cp_maxpool2d_backward_nhwc(cp_stream_t stream, const float* x, const float* grad_out, float* grad_x, int B, int H, int W,
                               int C, int kernel, int stride, int pad);

/* ------------------------------------------------------------------------------------------
 * Weight and bias gradient of the image stems — Conv2d(Cin, Cout, kernel 7, stride 1 | 2, padding 3) with Cin in 1..3, the
 *   layers cp_conv2d_backward_nhwc refuses: base_layer, pre_img_layer and pre_hm_layer of models/networks/pose_dla_dcn.py:247-271
 *   and conv1 of models/networks/resnet_dcn.py.
 * x_nchw [B,Cin,H,W] is the caller's image as a data loader hands it over (planes, NOT NHWC); grad_out_nhwc and y [B,Ho,Wo,Cout]
 * NHWC with Ho = (H - 1) / stride + 1 (Wo likewise).  Outputs, written (not accumulated): grad_w [Cout,Cin,7,7] (PyTorch layout)
 * and grad_bias [Cout] (NULL: not stored).  y (the ACTIVATED forward output) or NULL: when given, grad_out is gated by y > 0.
 * There is no data gradient: the input is an image.  Cout in {16, 32, 48, 64}.
 * Float32 on v_mfma_f32_16x16x4_f32 whatever cp_set_default_precision says; partial sums per workgroup go to the workspace and
 * are added in a fixed order; no atomics: bitwise reproducible call to call.
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch (the query returns 0): a NULL pointer other than
 * those named *_or_null, a workspace below the query, B / H / W < 1, another Cin / Cout / stride, a tensor of 2^31 elements or
 * more.  The query is host arithmetic.  Launches on `stream`, never synchronises.
 * ------------------------------------------------------------------------------------------ */
size_t cp_conv2d_stem_backward_workspace_bytes(int B, int H, int W, int Cin, int Cout, int stride);
int cp_conv2d_stem_backward(cp_stream_t stream, const float* x_nchw, const float* grad_out_nhwc, const float* y_or_null,
                            float* grad_w, float* grad_bias_or_null, void* workspace, size_t workspace_bytes, int B, int H,
                            int W, int Cin, int Cout, int stride);
/* The same operator for Cout in multiples of 16 from 16 to 128 — convolution(7, 3, 128, stride=2), the first layer of
 * models/networks/large_hourglass.py:209-212.  The kernels are the ones above, run over channel blocks of at most 64, so up to
 * 64 channels the two pairs give the same bits; same arguments, same workspace rule, same refusals but for the range of Cout.
 * (A pair of its own: cp_conv2d_stem_backward keeps refusing what it has always refused.) */
size_t cp_conv2d_stem_wide_backward_workspace_bytes(int B, int H, int W, int Cin, int Cout, int stride);
int cp_conv2d_stem_wide_backward(cp_stream_t stream, const float* x_nchw, const float* grad_out_nhwc, const float* y_or_null,
                                 float* grad_w, float* grad_bias_or_null, void* workspace, size_t workspace_bytes, int B, int H,
                                 int W, int Cin, int Cout, int stride);

/* ------------------------------------------------------------------------------------------
 * The kp_module merge of the stacked hourglass for training — models/networks/large_hourglass.py:95-112 (MergeUp,
 *   make_unpool_layer) as kp_module.forward uses them (:176-187): out = up1 + Upsample(scale_factor=2)(low), nearest neighbour,
 *   forward and backward, float32 NHWC: low, grad_low [B,H,W,C]; up1, out, grad_out [B,2H,2W,C].
 * Backward: grad_low[b,y,x,c] = (g[2y,2x] + g[2y,2x+1]) + (g[2y+1,2x] + g[2y+1,2x+1]), g = grad_out, in exactly that order:
 * bitwise reproducible, and exact on dyadic data.  grad_low is written, not accumulated.  The gradient with respect to up1 is
 * grad_out itself: there is no kernel and no copy for it.  No atomics, no workspace.
 * Refused with CP_ERR_INVALID and a cp_last_error() text before any launch: a NULL pointer, B / H / W < 1, C < 4 or C % 4 != 0,
 * a pointer that is not 16-byte aligned, a tensor of 2^31 elements or more.  Launches on `stream`, never synchronises.
 * ------------------------------------------------------------------------------------------ */
int cp_upsample2_add_nhwc(cp_stream_t stream, const float* up1, const float* low, float* out, int B, int H, int W, int C);
int cp_upsample2_add_backward_nhwc(cp_stream_t stream, const float* grad_out, float* grad_low, int B, int H, int W, int C);

/* ------------------------------------------------------------------------------------------
 * Heat-map decode — replaces `object_pose_decode(..., Inference=True)` (models/decode.py:72-375,
 *   models/utils.py:43-47; called from detectors/object_pose.py:154-161) including the 13
 *   device->host copies and the per-point Python loop (decode.py:191-252).
 * Inputs are the head tensors, NCHW float32 on the device, H x W = output grid (<= 32768 pixels, W % 4 == 0),
 * one category, 8 joints: hm [B,1,H,W], hps [B,16,H,W], wh [B,2,H,W], hm_hp [B,8,H,W] are
 * required (the detector's Inference configuration); hps_uncertainty [B,16], scale [B,3],
 * scale_uncertainty [B,3], reg [B,2], hp_offset [B,2], tracking [B,2], tracking_hp [B,16] may be
 * NULL (decode.py:304-345 zero-fill / +0.5 rules).  hm and hm_hp must already be sigmoided unless
 * apply_sigmoid != 0, in which case they hold logits and are overwritten with their sigmoid
 * (object_pose.py:136-138).
 *   K                 opt.K (<= 128)                      rep_mode   opt.rep_mode (0..4)
 *   fit_gaussian      opt.tracking_task || opt.refined_Kalman || rep_mode == 2 (decode.py:222)
 *   balance           opt.balance_coefficient[opt.c] (decode.py:309)
 *   legacy_bool_mask  0: `mask_2 == 7` is the AND of its 7 conditions (torch <= 1.1, what the
 *                     published models were used with); 1: reproduce torch >= 1.2, where the sum of
 *                     bool tensors can never equal 7 and every kps_heatmap_* stays -10000.
 * Output det [B,K,118]: bboxes[0:4] score[4] kps[5:21] cls[21] obj_scale[22:25]
 *   obj_scale_uncertainty[25:28] tracking[28:30] tracking_hp[30:46] kps_displacement_mean[46:62]
 *   kps_displacement_std[62:78] kps_heatmap_mean[78:94] kps_heatmap_std[94:110]
 *   kps_heatmap_height[110:118]  — the 13 keys of decode.py:347-361, output-grid units.
 * Ordering: (score desc, pixel index asc); torch.topk's order among exactly equal scores is
 * implementation-defined, so parity is defined on distinct scores.
 *
 * cp_decode_tiled: the same arguments, outputs and ordering as cp_decode (bit-identical wherever both accept a shape)
 * for output grids of any size: 1 <= K <= 128, K <= H*W <= 1048576 (a 4096 x 4096 network input), W % 4 == 0 and
 * W <= 4096; anything else returns CP_ERR_INVALID.  The peaks are found per band of whole rows and merged per map, so
 * the workspace grows with H*W: cp_decode_tiled_workspace_bytes(B, H, W, K) (0 for an unsupported shape); it must be
 * 16-byte aligned.  cp_model_detect takes this path for output grids above 32768 pixels.
 * ------------------------------------------------------------------------------------------ */
#define CP_DET_STRIDE 118
size_t cp_decode_workspace_bytes(int B, int K);
int cp_decode(cp_stream_t stream, int B, int H, int W, float* hm, const float* hps, const float* wh,
              const float* hps_uncertainty, const float* scale, const float* scale_uncertainty, const float* reg,
              float* hm_hp, const float* hp_offset, const float* tracking, const float* tracking_hp, int K,
              int rep_mode, int fit_gaussian, float balance, int legacy_bool_mask, int apply_sigmoid, float* det,
              void* workspace, size_t workspace_bytes);
size_t cp_decode_tiled_workspace_bytes(int B, int H, int W, int K);
int cp_decode_tiled(cp_stream_t stream, int B, int H, int W, float* hm, const float* hps, const float* wh,
                    const float* hps_uncertainty, const float* scale, const float* scale_uncertainty, const float* reg,
                    float* hm_hp, const float* hp_offset, const float* tracking, const float* tracking_hp, int K,
                    int rep_mode, int fit_gaussian, float balance, int legacy_bool_mask, int apply_sigmoid, float* det,
                    void* workspace, size_t workspace_bytes);

/* The decode in its two halves (cp_decode and cp_decode_tiled are the two called in sequence), for callers that evaluate the
 * regression heads at the peaks only (cp_model_detect_lean does exactly this):
 *   cp_decode_peaks     hm [B,1,H,W], hm_hp [B,8,H,W] (apply_sigmoid as cp_decode) -> pk_score / pk_ind [B,9,K]: the K peaks
 *                       of each map after the 3x3 NMS, score descending, index = y * W + x; map 0 = hm, 1..8 = hm_hp.
 *                       Any shape cp_decode or cp_decode_tiled accepts; workspace: cp_decode_peaks_workspace_bytes (0 =
 *                       unsupported shape), 16-byte aligned.
 *   cp_decode_gathered  the records from the peaks and COMPACT tables holding each regression head at the peaks: hps
 *                       [B,16,K], wh [B,2,K] and the optional hps_uncertainty [B,16,K], scale [B,3,K], scale_uncertainty
 *                       [B,3,K], reg [B,2,K], tracking [B,2,K], tracking_hp [B,16,K] (entry k = the head at pk_ind[b][0][k]),
 *                       hp_offset [B,8,2,K] (entry k of joint j = the head at pk_ind[b][j+1][k]); hm_hp is the dense map.
 *                       Same float expressions as cp_decode: tables copied out of dense maps give bit-identical records. */
size_t cp_decode_peaks_workspace_bytes(int B, int H, int W, int K);
int cp_decode_peaks(cp_stream_t stream, int B, int H, int W, float* hm, float* hm_hp, int K, int apply_sigmoid, float* pk_score,
                    int* pk_ind, void* workspace, size_t workspace_bytes);
int cp_decode_gathered(cp_stream_t stream, int B, int H, int W, const float* hm_hp, const float* hps, const float* wh,
                       const float* hps_uncertainty, const float* scale, const float* scale_uncertainty, const float* reg,
                       const float* hp_offset, const float* tracking, const float* tracking_hp, const float* pk_score,
                       const int* pk_ind, int K, int rep_mode, int fit_gaussian, float balance, int legacy_bool_mask, float* det);

/* ------------------------------------------------------------------------------------------
 * Pre-process — replaces `BaseDetector.pre_process`'s image work
 *   (detectors/base_detector.py:127-134: cv2.resize when scale != 1, cv2.warpAffine(..., INTER_LINEAR), then
 *    (x/255 - mean)/std, HWC->CHW).
 * image_hwc_bgr: DEVICE uint8 [H,W,3] (BGR as cv2.imread gives); trans6: HOST double[6], the row-major 2x3 FORWARD
 * matrix `trans_input` (source -> network input), inverted inside exactly as cv::invertAffineTransform does;
 * mean3/std3: HOST float[3] (opts.py:436-437); out_chw: DEVICE float32 [3,out_h,out_w].
 * Both kernels follow OpenCV's fixed-point arithmetic (5-bit bilinear weights for the warp, 11-bit coefficients for the
 * resize; oracle/cv_emul.py restates it), so the network input is built from the same rounded 8-bit values as the
 * reference's.  cp_resize_u8: in / out DEVICE uint8 [H,W,C] -> [out_h,out_w,C].
 * ------------------------------------------------------------------------------------------ */
int cp_preprocess(cp_stream_t stream, const unsigned char* image_hwc_bgr, int H, int W, const double* trans6,
                  const float* mean3, const float* std3, float* out_chw, int out_h, int out_w);
/* The same warp + normalise for B frames of one size that share the transform (fix_res batches, run_batch): images DEVICE
 * uint8 [B,H,W,3] contiguous -> out DEVICE float32 [B,3,out_h,out_w]; one launch. */
int cp_preprocess_batch(cp_stream_t stream, const unsigned char* images_bhwc_bgr, int B, int H, int W, const double* trans6,
                        const float* mean3, const float* std3, float* out_bchw, int out_h, int out_w);
int cp_resize_u8(cp_stream_t stream, const unsigned char* image_hwc, int H, int W, int C, unsigned char* out_hwc,
                 int out_h, int out_w);

/* ------------------------------------------------------------------------------------------
 * Post-process + soft-NMS — replaces `ObjectPoseDetector.post_process` + `merge_outputs`
 *   (detectors/object_pose.py:167-197 -> utils/post_process.py:12-68 `object_pose_post_process`,
 *    utils/image.py:23-32 `transform_preds`, object_pose.py:27-124 `soft_nms_nvidia` with Nt=0.5, method=2,
 *    threshold=vis_thresh).
 * det:   DEVICE float32 [B,K,118] from cp_decode.
 * meta:  DEVICE float64 [B,8]: 0..5 = get_affine_transform(c, s, 0, (out_w,out_h), inv=1) row-major (image.py:35-68),
 *        6 = s / max(out_w, out_h), 7 unused.
 * out:   DEVICE float64 [B,K,CP_POST_STRIDE]; image b's kept detections, in the reference's final order, are
 *        out[b][0 .. count[b]) with fields: score 0 | cls 1 | obj_scale 2 | obj_scale_uncertainty 5 |
 *        kps_displacement_std 8 | bbox 24 | ct 28 | kps 30 | tracking 46 | tracking_hp 48 | kps_displacement_mean 64 |
 *        kps_heatmap_mean 80 | kps_heatmap_std 96 | kps_heatmap_height 112.
 * count: DEVICE int32 [B].   nms: 0 = threshold filter only (opt.nms False), 1 = Gaussian soft-NMS.
 * vis_thresh is a double because the reference compares float64 scores with the Python float opt.vis_thresh.
 * div_scale: the `scale` of multi-scale testing (object_pose.py:171-176), 1 for the demo configuration.
 * workspace: cp_postprocess_workspace_bytes(B, K) bytes.
 * ------------------------------------------------------------------------------------------ */
#define CP_POST_STRIDE 120
size_t cp_postprocess_workspace_bytes(int B, int K);
int cp_postprocess(cp_stream_t stream, const float* det, int B, int K, const double* meta, double vis_thresh, int nms,
                   float div_scale, double* out, int* count, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * Tracking-input render — the drawing half of `BaseDetector._get_additional_inputs`
 *   (detectors/base_detector.py:150-388 -> utils/image.py:135-150 `draw_umich_gaussian`, :126-132 `gaussian2D`).
 * recs: DEVICE float64 [N,5] = (channel, x, y, radius, k) per Gaussian (x, y, radius integral; k = peak value);
 * out:  DEVICE float32 [C,H,W] (pre_hm: C=1, pre_hm_hp: C=8, or both stacked); cleared first when clear != 0.
 * Each record is drawn clipped to the map and merged with max(), exactly as the reference's in-place np.maximum.
 * ------------------------------------------------------------------------------------------ */
int cp_render_gaussians(cp_stream_t stream, const double* recs, int N, float* out, int C, int H, int W, int clear);

/* ------------------------------------------------------------------------------------------
 * Batched cuboid PnP — replaces the per-detection loop `pnp_shell` -> `CuboidPNPSolver.solve_pnp`
 *   -> `cv2.solvePnPGeneric(SOLVEPNP_ITERATIVE | SOLVEPNP_EPNP)` + `cv2.projectPoints`
 *   (utils/pnp/cuboid_pnp_shell.py:11-24, utils/pnp/cuboid_pnp_solver.py:141-239,
 *   detectors/base_detector.py:547-654).
 *   pts   [N, npts, 2] float32 image points (the reference hands cv2 float64 values, cuboid_pnp_solver.py:153; the
 *         float32 boundary perturbs a coordinate of a few hundred pixels by <= 3e-5 px, far inside the 1 degree / 1 %
 *         pose tolerance; all arithmetic after the load is float64), npts = 8 (rep_mode 0/3/4: `kps`) or 16 (rep_mode 1:
 *         displacement/heat-map pairs interleaved per vertex, base_detector.py:558-566); a point
 *         with x or y < -5000 is invalid (cuboid_pnp_solver.py:145)
 *   scale [N, 3] float32 relative cuboid size (divided by its y component inside, shell :12)
 *   cam   [N, 4] float64 (fx, fy, cx, cy) of each detection's image
 *   out   [N, 40] float64:
 *     [0] status: 1 solved, 2 solved but t_z < 0 (reference drops it, solver :207-220), -1 < 4 valid points,
 *                 0 failure (degenerate correspondences, e.g. 4-5 coplanar points handed to EPnP)
 *                 Branches as the reference selects them (solver :157-171): >= 6 valid non-planar points
 *                 SOLVEPNP_ITERATIVE (DLT + LM), coplanar model points its homography initialisation + LM,
 *                 4-5 valid points SOLVEPNP_EPNP (no refinement; approximate for exactly 4 points, as published)
 *     [1:4] rvec  [4:7] tvec (OpenCV frame)  [7] RMS reprojection error
 *     [8:24] the 8 cuboid vertices projected with (rvec, tvec), pixels
 *     [24:28] quaternion xyzw (OpenCV frame)   [28:31] location, [31:35] quaternion xyzw in the
 *     OpenGL frame the evaluation uses (solver :179-196)   [35] valid points  [36] LM iterations
 * ------------------------------------------------------------------------------------------ */
#define CP_PNP_STRIDE 40
size_t cp_pnp_workspace_bytes(int N);
int cp_pnp_solve(cp_stream_t stream, const float* pts, const float* scale, const double* cam, int N, int npts,
                 double* out, void* workspace, size_t workspace_bytes);

/* PnP of every post-processed detection of a batch without leaving the device -- replaces the per-detection loop of
 *   `BaseDetector.run` (detectors/base_detector.py:547-566 point assembly by rep_mode, :652 `pnp_shell`) between
 *   `merge_outputs` and the packaging of `cuboid_pnp_shell.py:26-91`.
 *   post / count: outputs of cp_postprocess ([B,K,CP_POST_STRIDE] float64, [B] int32).
 *   rep_mode: 0 / 3 / 4 -> 8 points from `kps`; 1 -> 16 points, (kps_displacement_mean, kps_heatmap_mean) per vertex.
 *   cam: DEVICE float64 [B,4] (fx, fy, cx, cy) per image.
 *   The assembly casts the float64 record fields to cp_pnp_solve's float32 `pts` / `scale` inputs (same rounding as the
 *   host path, which builds float32 arrays from the same float64 values): row (b,k) is bit-identical to cp_pnp_solve on
 *   points assembled on the host by the reference rule (tests/test_gpu_pose_chain.py).
 *   out: DEVICE float64 [B,K,CP_PNP_STRIDE]; row (b,k) as cp_pnp_solve for k < count[b], status -1 beyond.
 * No host synchronisation and no host-visible count: the whole chain backbone -> decode -> post-process -> PnP is a
 * fixed launch sequence. */
size_t cp_pnp_from_post_workspace_bytes(int B, int K);
int cp_pnp_from_post(cp_stream_t stream, const double* post, const int* count, int B, int K, int rep_mode,
                     const double* cam, double* out, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * CenterPoseTrack bookkeeping for B concurrent videos, on the device -- replaces, per frame, the host-side Python of
 *   `BaseDetector.run` between `merge_outputs` and the next frame's inputs (detectors/base_detector.py:501-544 Gaussian
 *   fusion, :547-654 `boxes`, :660-665 `self.tracker.step`, :150-388 which Gaussians `_get_additional_inputs` draws;
 *   utils/tracker.py:112-302 `Tracker.step`: greedy association, 32-state Kalman filter per track, scale pool, filtered
 *   PnP; utils/pnp/cuboid_pnp_shell.py:26-91 packaging and visibility rejects).
 * Supported configuration = the demo's (src/demo.py:117-129): `tracking_task` with `kalman` and / or `scale_pool`,
 * greedy or Hungarian association (`hungarian`), `Tracker` or -- `baseline`, the reference's `--refined_Kalman` --
 * `Tracker_baseline` (utils/tracker_baseline.py:14-310); lists seeded from annotations and ground-truth previous-frame
 * maps through cp_track_seed (below); anything else stays on the host mirror (centerpose_amd/lib/utils/tracker.py).  Per
 * video the state holds at most `cap` (<= CP_TRACK_CAP) tracks.
 *
 *   params        HOST struct (opt fields; cat_rule: 0 camera / bottle / cup, 1 book / chair / cereal_box, 2 bike / laptop /
 *                 shoe -- the visibility reject of cuboid_pnp_shell.py:70-84; K = slots per image of post / det_pnp)
 *   vmeta         DEVICE float64 [B,16] per video: trans_input 2x3 row-major | width height inp_width inp_height |
 *                 fx fy cx cy | 2 pad  (the `meta` of base_detector.py:142-147)
 *   post, count   outputs of cp_postprocess ([B,K,CP_POST_STRIDE] float64, [B] int32)
 *   det_pnp       DEVICE float64 [B,K,CP_PNP_STRIDE] from cp_pnp_from_post, or NULL when params->use_pnp == 0
 *   state         DEVICE, cp_track_state_bytes(B, cap) bytes, zeroed by cp_track_reset:
 *                   int32 hdr[4 + 4 B]: hdr[0] = which half holds the current lists; per video b at hdr[4 + 4 b]:
 *                   n tracks, last id given out, sticky count of list entries DROPPED because a frame needed more than cap
 *                   tracks (the list then keeps its first cap entries in the reference's order -- matched, new by score,
 *                   coasting -- and no id is spent on a dropped detection: read it with cp_track_status), scratch;  then (256-byte aligned) float64 tracks[2][B][cap][CP_TRACK_STRIDE]
 *                 track record (doubles): 0 tracking_id | 1 age | 2 active | 3 flags (bit 0 location / quaternion /
 *                   projected_cuboid / kps_3d_cam / kps_pnp valid, 1 kps_pnp_kf / kps_3d_cam_kf / kps_ori_kf valid, 2 in
 *                   this frame's `boxes`, 3 kps_ori valid, 4 filter state valid) | 4 the CP_POST_STRIDE detection fields |
 *                   124 kps_fusion_mean[16] | 140 kps_fusion_std[16] | 156 location[3] | 159 quaternion_xyzw[4] |
 *                   163 projected_cuboid[16] | 179 kps_pnp[18] | 197 kps_3d_cam[27] | 224 kps_ori[18] | 242 kf.x[32] |
 *                   274 kf.P as 8 blocks of 4x4 | 402 scale-pool sums[7] | 409 kps_mean_kf[16] | 425 kps_std_kf[16] |
 *                   441 obj_scale_kf[3] | 444 obj_scale_uncertainty_kf[3] | 447 vertex confidences[8] | 455 kps_pnp_kf[18] |
 *                   473 kps_3d_cam_kf[27] | 500 kps_ori_kf[18]
 *   render_recs   DEVICE float64 [B,cap,9,5]: next frame's Gaussians as (plane, x, y, radius, k) records for
 *                 cp_render_gaussians(recs, B*cap*9, out, C = 9 B, ...): plane b = pre_hm of video b, plane B + 8 b + j =
 *                 pre_hm_hp[j] of video b; plane -1 = nothing to draw
 * No host synchronisation; five kernel launches + the batched PnP of the filtered vertices.
 * ------------------------------------------------------------------------------------------ */
#define CP_TRACK_STRIDE 520
#define CP_TRACK_CAP 128
typedef struct cp_track_params {
    double new_thresh, pre_thresh, R, conf_lo, conf_hi;
    int max_age, kalman, scale_pool, use_pnp, hps_uncertainty, show_axes, cat_rule, render_hm_mode, render_hmhp_mode, pre_hm,
        pre_hm_hp, K, cap;
    int hungarian; /* != 0: optimal assignment (tracker.py:154-170) instead of the greedy walk.
                    *   1 = the solver the reference calls (tracker.py:6,157): sklearn.utils.linear_assignment_ of the pinned
                    *       scikit-learn 0.22.2, i.e. the Kuhn-Munkres state machine, restated operation for operation
                    *       (csrc/track_common.h: trk_munkres; the module no longer exists in scikit-learn >= 0.23);
                    *   2 = scipy.optimize.linear_sum_assignment's rectangular shortest-augmenting-path solver, restated
                    *       operation for operation (trk_lsap) -- what a host with a current scipy / scikit-learn would run, and
                    *       the faster of the two (O(n^2 m) against the state machine's O(n^3 m) worst case on one lane).
                    * Both are optimal; with many 1e18 "forbidden" entries the optimum is degenerate and the two can undo
                    * different forbidden pairs: same matching cost, possibly another order of the left-over detections and
                    * hence of new tracking ids / coasting tracks.  Goldens exist for both (tests/golden/tracker_ref.json). */
    int baseline;  /* 1: Tracker_baseline (--refined_Kalman, utils/tracker_baseline.py:14-310): only (x, y) of a vertex observed,
                      plain scale average, association on raw centres against velocity-advanced track centres */
} cp_track_params;
size_t cp_track_state_bytes(int B, int cap);
size_t cp_track_workspace_bytes(int B, int K, int cap);
int cp_track_reset(cp_stream_t stream, void* state, int B, int cap);
int cp_track_step(cp_stream_t stream, const cp_track_params* params, const double* vmeta, const double* post, const int* count,
                  const double* det_pnp, int B, void* state, double* render_recs, void* workspace, size_t workspace_bytes);
/* dropped_out: HOST int32 [B], the sticky overflow counters above.  Copies 16 + 16 B bytes and synchronises `stream`. */
int cp_track_status(cp_stream_t stream, const void* state, int B, int* dropped_out);

/* Seeding from annotations, between two frames (added without an ABI change: a new entry point only) -- replaces
 *   `Tracker.init_track(meta)` / `Tracker_baseline.init_track(meta)` with meta['pre_dets'] (utils/tracker.py:21-49,
 *   utils/tracker_baseline.py:21-49: reset, then every seed with score > new_thresh becomes a track with the next id, age 1,
 *   active 1, `init_kf` of the tracker class, a scale pool of one sample) and the ground-truth branch of
 *   `_get_additional_inputs` (detectors/base_detector.py:167-209, --gt_pre_hm_hmhp / --gt_pre_hm_hmhp_first).
 *   seeds         DEVICE float64 [B, S, CP_SEED_STRIDE], one record per seed (tools/objectron_eval/eval_video_official.py:
 *                 430-449), 1 <= S <= CP_TRACK_CAP:
 *                   0 the track record's [4, 156): the CP_POST_STRIDE detection fields (score, cls, obj_scale,
 *                     obj_scale_uncertainty, kps_displacement_std, bbox, ct, kps, tracking, tracking_hp, kps_displacement_mean,
 *                     kps_heatmap_mean, kps_heatmap_std, kps_heatmap_height), kps_fusion_mean[16], kps_fusion_std[16] |
 *                   152 the track record's [179, 242): kps_pnp[18], kps_3d_cam[27], kps_ori[18] | 215 kps_gt[18] (centre
 *                     first, normalised) | 233 presence bits: 1 ct given (else the bbox centre is taken), 2 kps_gt given,
 *                     4 kps_pnp / kps_3d_cam given, 8 kps_ori given
 *   seed_count    DEVICE int32 [B]: seeds of video b (values above S count as S).  NEGATIVE: video b is left bitwise
 *                 untouched -- list, id counter, overflow counter and its rows of render_recs; 0: reset to an empty list.
 *   gt_render     DEVICE int32 [B] or NULL: != 0 -> the rows of render_recs of video b hold the ground-truth Gaussians of
 *                 its new tracks (centre from bbox when pre_hm, the eight vertices of kps_gt when pre_hm_hp, k = 1, no
 *                 pre_thresh / visibility / bounds test: a blob may be centred outside the input and cp_render_gaussians
 *                 clips it; a coordinate that is not finite or does not fit int32 withdraws its record, as does a missing
 *                 kps_gt); else what cp_track_step would write for these tracks -- where that would re-draw kps_pnp_kf /
 *                 kps_mean_kf, which a seeded track does not have yet (the reference raises), no vertex is drawn.
 *   state         as cp_track_step; the CURRENT lists are replaced (call it between two frames, on the frames' stream).
 *                 Beyond params->cap the first cap accepted seeds are kept and the rest is counted into the overflow counter.
 *   render_recs   as cp_track_step: all cap rows of a seeded video are written (plane -1 beyond its list).
 * Reads new_thresh, pre_thresh, R, kalman, scale_pool, baseline, use_pnp, the render modes, pre_hm, pre_hm_hp, hps_uncertainty,
 * the confidence borders and cap of `params`.  One kernel launch, no host synchronisation. */
#define CP_SEED_STRIDE 234
int cp_track_seed(cp_stream_t stream, const cp_track_params* params, const double* vmeta, const double* seeds,
                  const int* seed_count, const int* gt_render, int B, int S, void* state, double* render_recs);

/* The tracker's assignment on the HOST (no device work, no stream): replaces `linear_assignment(dist)` of tracker.py:157 for the
 * host tracker (centerpose_amd/lib/utils/tracker.py) with the very routine the device tracker runs.
 *   cost       HOST float64 [n_rows, n_cols] row-major (detections x tracks)
 *   solver     1 = scikit-learn 0.22.2's Munkres, 2 = scipy's rectangular LSAP (cp_track_params.hungarian)
 *   match_out  HOST int32 [n_rows]: column of each row, -1 for rows left out (min(n_rows, n_cols) rows get one)
 * Every entry of `cost` must be finite (a forbidden pair is 1e18, as in the tracker, never inf): a NaN or infinite entry is
 * refused with CP_ERR_INVALID before any work, and cp_last_error names the first offending row and column.  CP_ERR_INVALID is
 * also returned when the solver cannot finish -- Munkres met one of its iteration bounds, or the LSAP found the problem
 * infeasible -- which only finite costs whose differences overflow float64 (entries near +-1e308) can cause; match_out then
 * holds a valid partial matching (possibly empty).  Neither solver can loop for ever, whatever the input. */
int cp_linear_assignment(const double* cost, int n_rows, int n_cols, int solver, int* match_out);

/* Objectron box metrics, float64 (added without an ABI change: new entry points only).  Boxes are the evaluator's 9 x 3
 * vertex sets (centre + 8 corners in objectron/dataset/box.py order).  All pointers are DEVICE memory owned by the caller;
 * both calls only enqueue on `stream`.
 *
 * cp_box_iou: IoU3D.IoU(Box(a[i]), Box(b[i])).iou() (objectron/dataset/iou.py:22-37) for i < n -> iou [n].  Same fit,
 *   transforms and Sutherland-Hodgman clipping as the reference; the intersection volume is the divergence theorem over
 *   the clipped faces instead of qhull (agrees to ~1e-13, to ~1e-6 where vertices lie within the 1e-6 plane epsilon).
 *
 * cp_box_eval: for each of n matched pairs, Evaluator.evaluate_3d and evaluate_2d (eval_image_official.py:673-793) with
 *   eval_num_symmetry = num_symmetry >= 1:
 *   pred3d [n,9,3] the (scaled) predicted box, gt3d [n,9,3] the annotation, pred2d [n,9,2] the predicted projection,
 *   mo2c [n,4,4] and proj [n,4,4] the annotation's object-to-camera and projection matrices, single_rotation [n] int32:
 *   nonzero evaluates rotation index 0 only in both sweeps (eval_mug_symmetric False on a mug).
 *   out [n, CP_BOX_EVAL_STRIDE]:
 *     [0] IoU of the best rotation (first index of the maximum; 0 when no rotation has IoU > 0)
 *     [1] ADD  [2] ADD-S  [3] azimuth error  [4] polar error (degrees) of that rotation; with no IoU > 0,
 *         ADD = ADD-S = 1.0 (_MAX_DISTANCE) and the viewpoint errors of the unrotated prediction
 *     [5] 2D error: the minimum mean reprojection distance over the 2D sweep (first index on ties)
 *     [6] best 3D rotation index (-1: none)  [7] best 2D index  [8] CP_BOX_FLAG_* bits:
 *         SINGULAR_RAY  a 4 x 4 ray solve of compute_ray met an exactly zero pivot (numpy's inv raises and the
 *                       reference falls back to pinv): the viewpoint errors are NaN
 *         SINGULAR_MO2C mo2c is singular (the reference raises): the 2D error is NaN
 *         CLIP_OVERFLOW a clipped polygon exceeded its 10-vertex capacity (not expected for boxes) */
#define CP_BOX_EVAL_STRIDE 9
#define CP_BOX_FLAG_SINGULAR_RAY 1
#define CP_BOX_FLAG_SINGULAR_MO2C 2
#define CP_BOX_FLAG_CLIP_OVERFLOW 4
int cp_box_iou(cp_stream_t stream, const double* a, const double* b, int n, double* iou);
int cp_box_eval(cp_stream_t stream, const double* pred3d, const double* gt3d, const double* pred2d, const double* mo2c,
                const double* proj, const int* single_rotation, int n, int num_symmetry, double* out);

/* ------------------------------------------------------------------------------------------
 * Training loss — replaces `ObjectPoseLoss.forward` and the autograd backward of its graph
 *   trains/object_pose.py:22-205 with models/losses.py:47-75 (_neg_loss / FocalLoss), :143-226 (RegL1Loss,
 *   RegKLDScaleLoss, RegKLDKeyLoss), :243-254 (RegWeightedL1Loss), models/utils.py:9-50 (_sigmoid,
 *   _transpose_and_gather_feat).
 * Every term is computed per (image b, symmetry variant s), giving [B,S] matrices; summed over the stacks (each / num_stacks)
 * and weighted, the per-variant total picks choice[b] = argmin over s of total*valid + inf*(!valid), valid = sum_k ind > 0,
 * with torch.argmin's rules (first minimum; first NaN if any).  loss and the stats are the means over b of the chosen
 * entries.  The backward differentiates the chosen entries only, as the reference's graph does.
 *
 * Layouts (all contiguous; the binding converts the dataset's uint8 / int64 masks to float32 and the indices to int32):
 *   heads  [B, ch, H, W] float32, one set per stack:  hm ch = num_classes, hm_hp J, hps / hps_uncertainty / tracking_hp 2J,
 *          wh / reg / hp_offset / tracking 2, scale / scale_uncertainty 3 (J = num_joints)
 *   gt     hm [B,S,num_classes,H,W], hm_hp [B,S,J,H,W], ind [B,S,K] int32, reg_mask [B,S,K], hps / hps_mask [B,S,K,2J],
 *          wh / reg / tracking [B,S,K,2], scale [B,S,K,3], hp_ind [B,S,K*J] int32, hp_mask [B,S,K*J],
 *          hp_offset [B,S,K*J,2], tracking_mask [B,S,K], tracking_hp / tracking_hp_mask [B,S,K,2J]
 * Terms (CP_PL_T_*, the order of the weighted sum at object_pose.py:163-168):
 *   hm, hm_hp  focal loss; the forward overwrites the head's logits with sigmoid(logit) in place (_sigmoid's sigmoid_)
 *              and writes clamp(sigmoid, 1e-4, 1-1e-4) to `clamped`; the backward reads that in-place sigmoid back
 *   hp         RegWeightedL1Loss on hps, or RegKLDKeyLoss with hps_uncertainty (CP_PL_HPS_UNCERTAINTY, train phase)
 *   wh, off    RegL1Loss with reg_mask;  hp_offset RegL1Loss with hp_ind / hp_mask;  tracking RegL1Loss, tracking_mask
 *   obj_scale  train: RegL1Loss (exp(pred) * dimension_ref with CP_PL_RESIDUAL) or RegKLDScaleLoss with
 *              scale_uncertainty (CP_PL_SCALE_UNCERTAINTY); val (CP_PL_VAL): RegL1Loss's relative form, numerator
 *              1*mask - pred*mask, target zeros replaced by 1e-6
 *   tracking_hp RegWeightedL1Loss with tracking_hp_mask
 *   The L1 denominators add 1e-4, the KLD ones 1e-6, as the reference.  A term whose bit of `terms` is clear counts 0.
 * Outputs of the forward (device): loss [1]; stats [10] in the reference's key order: loss, hm, hp, hm_hp, hp_offset, wh,
 *   off, obj_scale, tracking, tracking_hp (a term that is off gives 0); choice [B] int64; optional terms_out
 *   [CP_PL_NUM_TERMS, B, S] (each term's [B,S] matrix, summed over the stacks); clamped heat maps per stack.
 * Backward: dloss is a device pointer to dL/dloss (one float, read on the device).  dmaps (host array [num_stacks * 2],
 *   may be NULL, as may each entry) gives dL/d(in-place sigmoid) of hm [st*2] / hm_hp [st*2+1] from graphs built on the
 *   overwritten logits tensor; it is chained through the sigmoid (dmaps * y (1 - y), sigmoid_'s backward) and added to the
 *   loss' gradient.  grad[st * CP_PL_NUM_HEADS + h] receives dL/d(head h of stack st) (written, not accumulated) and must
 *   be non-NULL for every head a counted term uses, and for a heat map with a dmaps entry; the others are ignored.
 *   `workspace` must be the one the forward wrote, unchanged.
 * Reproducibility: no float atomics; per-workgroup partials are summed in a fixed order that does not depend on s, and
 *   repeated indices are accumulated serially per image, so every output is bitwise reproducible run to run and identical
 *   variants give identical terms.
 * Limits: 1 <= num_stacks <= CP_PL_MAX_STACKS, 1 <= S <= CP_PL_MAX_S, 1 <= K <= CP_PL_MAX_K, K*J <= CP_PL_MAX_K * 32,
 *   1 <= J <= 32, num_classes >= 1, (H*W) % 4 == 0, every head and ground-truth tensor below 2^31 elements; the hm / hm_hp
 *   heads, their clamped maps, gt_hm, gt_hm_hp, their gradients and dmaps 16-byte aligned (float4 lines); NULL pointers
 *   that a counted term needs, a misaligned heat-map pointer or a workspace below the query return CP_ERR_INVALID before
 *   any launch.  An index outside
 *   [0, H*W) is read at 0 and counts as masked (the binding refuses such batches before calling).  Launches on `stream`,
 *   never allocates, never synchronises.
 * ------------------------------------------------------------------------------------------ */
#define CP_PL_MAX_STACKS 4
#define CP_PL_MAX_S 64
#define CP_PL_MAX_K 256
#define CP_PL_NUM_TERMS 9
#define CP_PL_T_HM 0
#define CP_PL_T_WH 1
#define CP_PL_T_OFF 2
#define CP_PL_T_HP 3
#define CP_PL_T_HM_HP 4
#define CP_PL_T_HP_OFFSET 5
#define CP_PL_T_SCALE 6
#define CP_PL_T_TRACKING 7
#define CP_PL_T_TRACKING_HP 8
#define CP_PL_NUM_HEADS 11
#define CP_PL_H_HM 0
#define CP_PL_H_HM_HP 1
#define CP_PL_H_HPS 2
#define CP_PL_H_HPS_UNC 3
#define CP_PL_H_WH 4
#define CP_PL_H_REG 5
#define CP_PL_H_SCALE 6
#define CP_PL_H_SCALE_UNC 7
#define CP_PL_H_HP_OFFSET 8
#define CP_PL_H_TRACKING 9
#define CP_PL_H_TRACKING_HP 10
#define CP_PL_VAL 1                /* phase == 'val' */
#define CP_PL_RESIDUAL 2           /* opt.use_residual */
#define CP_PL_HPS_UNCERTAINTY 4    /* opt.hps_uncertainty */
#define CP_PL_SCALE_UNCERTAINTY 8  /* opt.obj_scale_uncertainty */
#define CP_PL_HM_HP_MAPS 16        /* opt.hm_hp: the hm_hp heads get the sigmoid side effect even when the term is off */
#define CP_PL_NUM_STATS 10
typedef struct cp_pose_loss_desc {
    int B, S, K, H, W, num_classes, num_joints, num_stacks;
    int terms; /* bit CP_PL_T_*: the term counts */
    int flags; /* CP_PL_VAL | CP_PL_RESIDUAL | ... */
    float weight[CP_PL_NUM_TERMS]; /* opt.*_weight per term (off and hp_offset both take off_weight) */
    float kl_kps, kl_scale;        /* opt.KL_kps_uncertainty, opt.KL_scale_uncertainty */
    float dimension_ref[3];        /* opt.dimension_ref (CP_PL_RESIDUAL) */
    /* ground truth (batch[...]) */
    const float *gt_hm, *gt_hm_hp;
    const int* ind;
    const float *reg_mask, *gt_hps, *hps_mask, *gt_wh, *gt_reg, *gt_scale;
    const int* hp_ind;
    const float *hp_mask, *gt_hp_offset, *gt_tracking, *tracking_mask, *gt_tracking_hp, *tracking_hp_mask;
    /* heads: head[st][CP_PL_H_*]; hm / hm_hp are overwritten in place by the forward */
    float* head[CP_PL_MAX_STACKS][CP_PL_NUM_HEADS];
    float* clamped[CP_PL_MAX_STACKS][2]; /* clamp(sigmoid) of hm [0] and hm_hp [1] */
} cp_pose_loss_desc;
size_t cp_pose_loss_workspace_bytes(const cp_pose_loss_desc* d);
int cp_pose_loss_forward(cp_stream_t stream, const cp_pose_loss_desc* d, float* loss, float* stats, long long* choice,
                         float* terms_out, void* workspace, size_t workspace_bytes);
int cp_pose_loss_backward(cp_stream_t stream, const cp_pose_loss_desc* d, const float* dloss, const float* const* dmaps,
                          float* const* grad, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * ObjectPose training targets — replaces the current-frame part of ObjectPoseDataset.__getitem__
 *   datasets/dataset_combined.py:957-1130 (+ the arrays of :368-393), for a batch, already collated to [B,S,...].
 * The host keeps image decoding, the augmentation draws and the output affine trans_output_rot (:354); the records below
 * carry them (centerpose_amd/pose_targets.py pack_annotations writes them).  S = the category's variant count
 * (:357-366), R = opt.output_res, K = max_objs (10 in the reference, :128), num_joints = 8.
 * Records (HOST pointers, float64; staged into the workspace with hipMemcpyAsync on `stream`, so pageable memory may be
 * reused when the call returns):
 *   images [B][CP_PT_IMG_STRIDE]
 *     0..5   trans_output_rot, the 2x3 output affine, row-major (:354)
 *     6, 7   width, height of the decoded image (:317)
 *     8      flipped, 0 or 1 (:324-326)
 *     9      rot, the augmentation angle in degrees; only rot != 0 is read (:1043)
 *     10     num_objs = min(len(anns['objects']), max_objs) (:300)
 *     11..26 anns['camera_data']['camera_projection_matrix'], 4x4 row-major (:957)
 *   objects [B][K][CP_PT_OBJ_STRIDE] (slots k >= num_objs are not read)
 *     0      the object's variant count, 1 <= n <= S: 4 or 1 from ann['symmetric'], or the value carried over from the
 *            previous object when the key is missing (:962-966)
 *     1..18  ann['projected_cuboid'], 9 x (x, y), centre first (:974)
 *     19..22 ann['quaternion_xyzw'] (:986)
 *     23..25 ann['location'] (:987)
 *     26..52 ann['keypoints_3d'], 9 x (x, y, z) (:988)
 *     53..55 ann['scale'] (:1058-1062)
 * Outputs (DEVICE pointers), the collated `ret` entries, every element written (no pre-clear needed):
 *   out_hm [B,S,1,R,R] f32, out_hm_hp [B,S,8,R,R] f32 (hm_hp), out_reg_mask [B,S,K] u8, out_ind [B,S,K] i64,
 *   out_hps [B,S,K,16] f32, out_hps_mask [B,S,K,16] u8, out_hps_uncertainty [B,S,K,16] f32 (hps_uncertainty),
 *   out_scale [B,S,K,3] f32 (obj_scale), out_hp_offset [B,S,K*8,2] f32, out_hp_ind / out_hp_mask [B,S,K*8] i64
 *   (reg_hp_offset); out_wh / out_reg [B,S,K,2] f32 and out_scale_uncertainty [B,S,K,3] f32 (all zeros) are written
 *   when non-NULL.  An output its option turns off is ignored and may be NULL; one it turns on must not be.
 * Semantics are the reference's, integer behaviour included: variant projection in float64 truncated with int(),
 *   corners truncated toward zero into int64 after the visibility test, the joints' affine assigned into int64 (so
 *   hp_offset is always 0), max(0, int(gaussian_radius)), hm / hm_hp = the max over the covering Gaussians of
 *   float32(exp(-(dx^2+dy^2) / (2 sigma^2))), sigma = (2r+1)/6.  Bitwise deterministic (no atomics).
 * Refused with CP_ERR_INVALID before any device work: NULL pointers as above, B, S, R < 1, R > 46340, K outside
 *   [1, CP_PT_MAX_OBJS], num_joints != 8, hm / hm_hp not 16-byte aligned, num_objs outside [0, K], a variant count outside
 *   [1, S], a workspace below the query.  Launches on `stream`, never allocates, never synchronises.
 * ------------------------------------------------------------------------------------------ */
#define CP_PT_MAX_OBJS 64
#define CP_PT_IMG_STRIDE 32
#define CP_PT_IMG_TRANS 0
#define CP_PT_IMG_WIDTH 6
#define CP_PT_IMG_HEIGHT 7
#define CP_PT_IMG_FLIPPED 8
#define CP_PT_IMG_ROT 9
#define CP_PT_IMG_NUM_OBJS 10
#define CP_PT_IMG_PROJ 11
#define CP_PT_OBJ_STRIDE 64
#define CP_PT_OBJ_NSYM 0
#define CP_PT_OBJ_CUBOID 1
#define CP_PT_OBJ_QUAT 19
#define CP_PT_OBJ_LOC 23
#define CP_PT_OBJ_KPS3D 26
#define CP_PT_OBJ_SCALE 53
typedef struct cp_pose_targets_desc {
    int B, S, R, max_objs, num_joints;
    /* opt.center_3D, opt.use_absolute_scale, opt.obj_scale, opt.hps_uncertainty, opt.reg_hp_offset, opt.hm_hp (0 / 1) */
    int center_3D, use_absolute_scale, obj_scale, hps_uncertainty, reg_hp_offset, hm_hp;
    const double *images, *objects; /* host records, layouts above */
    float *out_hm, *out_hm_hp;
    unsigned char* out_reg_mask;
    long long* out_ind;
    float* out_hps;
    unsigned char* out_hps_mask;
    float *out_hps_uncertainty, *out_wh, *out_reg, *out_scale, *out_scale_uncertainty, *out_hp_offset;
    long long *out_hp_ind, *out_hp_mask;
} cp_pose_targets_desc;
size_t cp_pose_targets_workspace_bytes(const cp_pose_targets_desc* d); /* 0: shape refused */
int cp_pose_targets(cp_stream_t stream, const cp_pose_targets_desc* d, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * ObjectPose training targets of the tracking task (CenterPoseTrack) — replaces Step 1 of ObjectPoseDataset.__getitem__
 *   in its noise-simulation mode, datasets/dataset_combined.py:555-937 with data_generation_mode == 0 (the detector-in-
 *   the-loop lines 468-550, 644-693, 752-763, 890-911, 939-952 are cp_pose_targets_track_det's, below), and the three
 *   places where Step 2 reads its results: the cup / mug skip (:968-972), the variant filter (:983-987), tracking /
 *   tracking_hp (:1106-1117, :1129-1137).  `cur` is cp_pose_targets' descriptor for the current frame, unchanged in meaning; every output of
 *   cp_pose_targets is written too.  The host keeps the choice of the previous frame (:415-425), both frames' images and
 *   JSON, the augmentation draws, the affines trans_input_pre (:438-449) and trans_output_rot, and ALL random draws: a
 *   fixed set per previous object, filled whether or not the object ends up using them
 *   (centerpose_amd/pose_targets_track.py draw_track_noise / pack_track_annotations write the records).
 * Geometry and options: input_w, input_h (opt.input_w / input_h), down_ratio, max_pre_objs = Kp in [1, CP_PT_MAX_OBJS];
 *   hm_disturb, lost_disturb, fp_disturb, hm_hp_disturb, hp_lost_disturb, hp_fp_disturb (double); hm_heat_random,
 *   hm_hp_heat_random, tracking_label_mode, and pre_hm, pre_hm_hp, tracking, tracking_hp (0 / 1).
 * Records (HOST pointers, float64, staged like cp_pose_targets'):
 *   track_images [B][CP_PTK_IMG_STRIDE]
 *     0..5   trans_input_pre, the 2x3 input affine of the previous frame, row-major (:439, :448)
 *     6      the number of previous-frame objects, len(anns_pre['objects']) <= Kp
 *     7..22  anns_pre['camera_data']['camera_projection_matrix'], 4x4 row-major (:555)
 *   pre_objects [B][Kp][CP_PTK_PRE_STRIDE] (slots past the count are not read)
 *     0..52  as objects[] of cp_pose_targets: the variant count with the reference's carry-over (:561-565),
 *            projected_cuboid, quaternion_xyzw, location, keypoints_3d of ann_pre
 *     56     skip, 0 or 1: the cup / mug filter (:567-571), resolved on the host
 *     57     id_symmetry_pre, the host's np.random.choice(num_symmetry) (:578)
 *     58     the integer track-id code of opt.c + ann_pre['name'].split('_')[1] (:765), unique per image
 *     64..71 the centre's draws: 2 truncated normals (:715), the lost uniform (:730), the heat uniform (:733), the
 *            false-positive uniform (:929), its 2 normals (:932-933), its peak, uniform(0, 0.4) (:937)
 *     72 + 7 j .. 78 + 7 j  joint j's draws: 2 truncated normals (:808), the lost uniform (:814), the false-positive
 *            uniform (:878), its 2 normals (:881-882), its peak, uniform(0, 0.3) (:888)
 *   cur_objects [B][K][CP_PTK_CUR_STRIDE]
 *     0      the integer track-id code of opt.c + ann['name'].split('_')[1] (:1108, :1131)
 *     1      skip, 0 or 1: the cup quirk of :968-972, which reads the LAST previous object's 'mug'
 * Outputs (DEVICE pointers), every element written (no pre-clear needed), S / R / K of `cur`:
 *   out_pre_hm [B,1,input_h,input_w] f32 (pre_hm), out_pre_hm_hp [B,8,input_h,input_w] f32 (pre_hm_hp),
 *   out_tracking [B,S,K,2] f32 and out_tracking_mask [B,S,K] u8 (tracking), out_tracking_hp [B,S,K,16] f32 and
 *   out_tracking_hp_mask [B,S,K,16] u8 (tracking_hp).  An output its option turns off is ignored and may be NULL.
 * Semantics are the reference's, rounding points included: points through float32 in affine_transform, ct float32 by
 *   box and float64 under center_3D, astype(int32) truncation, floats assigned into the int64 pts_pre / pt2,
 *   pts_single_pre in float32 and / down_ratio, np.maximum(1 - 2 ** (sqrt(nx^2 + ny^2) - 4.5), 0) in float64; the maps
 *   are the max over the covering draws of float32(k * exp(-(dx^2+dy^2) / (2 sigma^2))), the product in float64, a
 *   draw clipped to the map as draw_umich_gaussian clips it (utils/image.py:135-150).  Bitwise deterministic.
 * Refused with CP_ERR_INVALID before any device work: whatever cp_pose_targets refuses in `cur`, NULL pointers for
 *   records or for outputs that are turned on, pre_hm / pre_hm_hp not 16-byte aligned, input_w / input_h < 1 or their
 *   product above 2^31 - 1, down_ratio < 1, Kp outside [1, CP_PT_MAX_OBJS], a previous-object count outside [0, Kp], a
 *   variant count or id_symmetry_pre outside its range, a workspace below the query.  Launches on `stream`, never
 *   allocates, never synchronises.
 * ------------------------------------------------------------------------------------------ */
#define CP_PTK_IMG_STRIDE 32
#define CP_PTK_IMG_TRANS 0
#define CP_PTK_IMG_NUM_PRE 6
#define CP_PTK_IMG_PROJ 7
#define CP_PTK_PRE_STRIDE 128
#define CP_PTK_PRE_SKIP 56
#define CP_PTK_PRE_IDSYM 57
#define CP_PTK_PRE_ID 58
#define CP_PTK_PRE_DRAWS 64
#define CP_PTK_DRAW_CT_NOISE 0
#define CP_PTK_DRAW_CT_LOST 2
#define CP_PTK_DRAW_CT_HEAT 3
#define CP_PTK_DRAW_CT_FP 4
#define CP_PTK_DRAW_CT_FP_NOISE 5
#define CP_PTK_DRAW_CT_FP_PEAK 7
#define CP_PTK_DRAW_JOINTS 8
#define CP_PTK_DRAW_JOINT_STRIDE 7
#define CP_PTK_DRAW_J_NOISE 0
#define CP_PTK_DRAW_J_LOST 2
#define CP_PTK_DRAW_J_FP 3
#define CP_PTK_DRAW_J_FP_NOISE 4
#define CP_PTK_DRAW_J_FP_PEAK 6
#define CP_PTK_CUR_STRIDE 2
#define CP_PTK_CUR_ID 0
#define CP_PTK_CUR_SKIP 1
typedef struct cp_pose_targets_track_desc {
    cp_pose_targets_desc cur;
    int input_w, input_h, down_ratio, max_pre_objs;
    int hm_heat_random, hm_hp_heat_random, tracking_label_mode, pre_hm, pre_hm_hp, tracking, tracking_hp, reserved;
    double hm_disturb, lost_disturb, fp_disturb, hm_hp_disturb, hp_lost_disturb, hp_fp_disturb;
    const double *track_images, *pre_objects, *cur_objects; /* host records, layouts above */
    float *out_pre_hm, *out_pre_hm_hp, *out_tracking;
    unsigned char* out_tracking_mask;
    float* out_tracking_hp;
    unsigned char* out_tracking_hp_mask;
} cp_pose_targets_track_desc;
size_t cp_pose_targets_track_workspace_bytes(const cp_pose_targets_track_desc* d); /* 0: shape refused */
int cp_pose_targets_track(cp_stream_t stream, const cp_pose_targets_track_desc* d, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * The same targets with the detector in the loop — adds data_generation_mode == 1 of ObjectPoseDataset.__getitem__
 *   (datasets/dataset_combined.py:464-550 the matching, :644-693, :752-763, :792-794, :851-867, :890-911, :939-952 the
 *   per-object branches) for the images whose record asks for it; the other images of the batch are computed exactly as
 *   cp_pose_targets_track computes them (bit for bit).  The detector's answer arrives as the DEVICE records of
 *   cp_postprocess and cp_pnp_from_post on the previous frame's input image; what BaseDetector.run and pnp_shell do
 *   between them and `boxes` (base_detector.py:547-654, cuboid_pnp_shell.py:24-91) happens here.
 * `track` is cp_pose_targets_track's descriptor, unchanged in meaning.  Added:
 *   det_post  DEVICE float64 [B, K_det, CP_POST_STRIDE], det_count DEVICE int32 [B] (cp_postprocess with the meta of
 *             get_affine_transform(c, s, 0, (output_res, output_res), inv=1), :479-489), det_pnp DEVICE float64
 *             [B, K_det, CP_PNP_STRIDE] (cp_pnp_from_post with the camera of :469-473); K_det in [1, 128]
 *   render_hm_mode 0 / 1, render_hmhp_mode 0..3 (opt.render_hm_mode, opt.render_hmhp_mode)
 *   cat_rule  pnp_shell's reject by category: 0 camera / bottle / cup (3 points), 1 book / chair / cereal_box (6 points),
 *             2 bike / laptop / shoe (none)
 *   gen       HOST float64 [B][CP_PTKD_GEN_STRIDE]: 0 data_generation_mode of the image (0 / 1, the draw of :465, made by
 *             the host), 1 the radius scale: aug_s when same_aug_pre and frame_dist != 0, else aug_s_pre (:681-690)
 * Per image in mode 1 (one wavefront per image, two launches for the batch):
 *   1. slot k < det_count[b] is a box when its PnP status is 1 and pnp_shell's rejects pass on the 9 normalised points
 *      (the centroid of the 8 reprojected vertices, then the vertices, / width, / height in float64).
 *   2. instances_2d of every previous object (:506-532): the projected_cuboid in float32; when flipped, x = width - x - 1
 *      in float32 and the row swaps (0,4), (2,6), (1,5), (3,7) of the NINE-row array (the reference applies flip_idx - 1
 *      to it, so the centre row trades places with row 4); / width, / height in float32; nine points of -10000 when row 0
 *      is not strictly inside (0, 1).
 *   3. per box the Frobenius norms of rows 1..8 against every object, summed in float64 in row order, and the first
 *      minimum (:542-543); per object the only box whose minimum it is, whatever its distance, or among several the
 *      nearest (lowest slot on exact ties), dropped when its norm exceeds 1000 (:646-661).
 *   4. the matched object reads of its box: ct (:665), kps_ori rows 1..8 (render_hmhp_mode 0 / 1) or the reprojected
 *      rows 1..8 (2 / 3), kps_heatmap_std and kps_heatmap_height rounded to float32 (the detector returns float32 arrays),
 *      and a score.  The score is the one of the image's LAST box, not of the matched one: :949-951 read the loop variable
 *      `result_ori` that the matching loop of :539-540 leaves behind.
 *   Rounding points: ct_detector and pts_detector go through float32 into affine_transform, its products in float64;
 *   pts_detector * (width, height) in float64; the tracking label of a matched object under tracking_label_mode 1 is
 *   ct_detector / down_ratio in float64 and float32(pts_detector) / down_ratio in float32; the in-bounds test of :893-896
 *   is on the float64 point and the draw at its truncation; radius_detector[j, 0] = int32(float64(float32 std[2 j]) *
 *   scale); the peaks are float64(float32 height[j]), 1, or the score.  The noise draws of :715, :808, :814 are read as in
 *   mode 0; the test of :725-727 does not apply, so an object whose noisy centre left the input stays in the lists.
 * Refused with CP_ERR_INVALID before any device work: whatever cp_pose_targets_track refuses in `track`, NULL det_post /
 *   det_count / det_pnp / gen, det_post / det_pnp not 8-byte or det_count not 4-byte aligned, K_det outside [1, 128], a
 *   mode other than 0 / 1, a radius scale that is not finite, render_hm_mode outside 0..1, render_hmhp_mode outside 0..3,
 *   cat_rule outside 0..2, a workspace below the query.  Launches on `stream`, never allocates, never synchronises.
 * ------------------------------------------------------------------------------------------ */
#define CP_PTKD_GEN_STRIDE 4
#define CP_PTKD_GEN_MODE 0
#define CP_PTKD_GEN_RADIUS_SCALE 1
#define CP_PTKD_MAX_K 128
typedef struct cp_pose_targets_track_det_desc {
    cp_pose_targets_track_desc track;
    const double* det_post; /* device */
    const int* det_count;   /* device */
    const double* det_pnp;  /* device */
    int K_det, render_hm_mode, render_hmhp_mode, cat_rule;
    const double* gen; /* host */
} cp_pose_targets_track_det_desc;
size_t cp_pose_targets_track_det_workspace_bytes(const cp_pose_targets_track_det_desc* d); /* 0: shape refused */
int cp_pose_targets_track_det(cp_stream_t stream, const cp_pose_targets_track_det_desc* d, void* workspace,
                              size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * Training input images — replaces ObjectPoseDataset._get_input (datasets/dataset_combined.py:278-288, called at :348 for
 *   the current frame and at :456 for the tracking task's previous frame) together with the horizontal flip of the
 *   decoded frame (:335-339, :433-435) and color_aug (utils/image.py:239-277), for N images in one call.
 * The host keeps image decoding and every random draw; a record per image carries the draws (centerpose_amd/
 * train_inputs.py pack_input / draw_color_aug write it).
 * frames   DEVICE pointer: the decoded 8-bit HWC BGR frames in one buffer of `frames_bytes` bytes; record n names its
 *          frame by byte offset, height and width, so the frames of one call may differ in size.
 * records  HOST pointer, float64 [N][CP_TI_STRIDE]; staged into the workspace with hipMemcpyAsync on `stream`, so
 *          pageable memory may be reused when the call returns:
 *     0      byte offset of the frame in `frames`
 *     1, 2   height, width of the frame (img.shape[0], img.shape[1], :322)
 *     3..8   trans_input, the FORWARD 2x3 input affine, row-major (:344); inverted on the device exactly as
 *            cv::invertAffineTransform / cp_preprocess do, a singular matrix giving the zero matrix (every output pixel
 *            is then what source pixel (0, 0) gives)
 *     9      flipped, 0 or 1: source column x is read at W - 1 - x, i.e. the warp of img[:, ::-1, :] (:337); c[0] is
 *            mirrored in trans_input by the caller (:339)
 *     10     colour flag, 0 or 1: split == 'train' and not opt.no_color_aug (:284)
 *     11     order of brightness (b), contrast (c), saturation (s) after random.shuffle (utils/image.py:270-271):
 *            0 = bcs, 1 = bsc, 2 = cbs, 3 = csb, 4 = sbc, 5 = scb
 *     12..14 alpha = 1 + uniform(-0.4, 0.4) of the first, second and third operation RUN (:255, :260, :265)
 *     15..17 the lighting shift per B, G, R channel, np.dot(eigvec, eigval * alpha) of lighting_ (:243-245)
 * out      DEVICE float32 [N, 3, out_h, out_w] (opt.input_res twice), every element written.
 * Per image, in the reference's order and precision:
 *   1. cv2.warpAffine(INTER_LINEAR, constant 0 border) in OpenCV's fixed-point arithmetic, as cp_preprocess: the same
 *      8-bit levels;
 *   2. float32(v8) / 255 in float32 (:283);
 *   3. with the colour flag: gs = 0.114 B + 0.587 G + 0.299 R in float32 (BGR2GRAY on a float image), gs_mean its mean
 *      over the whole warped image, both taken before any operation; the three operations in the record's order in
 *      float32, a = float32(alpha), 1 - a = float32(1.0 - alpha): brightness v *= a, contrast v = v a + gs_mean (1 - a),
 *      saturation v = v a + gs (1 - a), every product and sum rounded on its own; then the lighting shift
 *      v = float32(double(v) + shift[c]) (a float64 array added into the float32 image);
 *   4. (v - mean3[c]) / std3[c] in float32 (:286; NOT cp_preprocess's float64 form), written NCHW (:287).
 *   gs_mean is float32(sum / (out_h out_w)) of a float64 sum reduced in a fixed order without atomics: results are
 *   bitwise reproducible, and an image's result does not depend on the other images of the call.  It differs from
 *   numpy's pairwise float32 mean in the last bits.
 * Images whose colour flag is clear take no grey pass; a call without a colour image is one kernel launch.
 * Workspace: cp_train_inputs_workspace_bytes(N, out_h, out_w) bytes (0: refused).  After the call the float32 gs_mean
 *   of every image (0 where the colour flag is clear) is at byte offset CP_TI_WS_MEANS(N) of the workspace.
 * Refused with CP_ERR_INVALID before any device work: NULL pointers, N < 1, out_h / out_w < 1 (or a grid beyond 2^31 - 1
 *   workgroups), a non-finite record value, a frame whose height or width is no integer >= 1, an order code outside
 *   0..5, a frame extent [offset, offset + 3 H W) beyond frames_bytes, `out` not 16-byte aligned, a workspace below the
 *   query.  A singular trans_input is not refused.  Launches on `stream`, never allocates, never synchronises.
 * ------------------------------------------------------------------------------------------ */
#define CP_TI_STRIDE 24
#define CP_TI_OFFSET 0
#define CP_TI_HEIGHT 1
#define CP_TI_WIDTH 2
#define CP_TI_TRANS 3
#define CP_TI_FLIPPED 9
#define CP_TI_COLOR 10
#define CP_TI_ORDER 11
#define CP_TI_ALPHA 12
#define CP_TI_SHIFT 15
#define CP_TI_WS_MEANS(N) ((((size_t)(N) * CP_TI_STRIDE * sizeof(double) + 255) / 256) * 256)
size_t cp_train_inputs_workspace_bytes(int N, int out_h, int out_w); /* 0: shape refused */
int cp_train_inputs(cp_stream_t stream, const unsigned char* frames, size_t frames_bytes, const double* records, int N,
                    const float* mean3, const float* std3, float* out, int out_h, int out_w, void* workspace,
                    size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * cp_adam_*: gradient-norm clipping and the Adam update of all tensors of a param group -- the update of the reference's
 *   training step, trains/base_trainer.py:91-99 (`clip_grad_norm_(model.parameters(), 100.)`, `optimizer.step()`) with
 *   the optimizer of test.py:41 (`torch.optim.Adam(model.parameters(), opt.lr)`; amsgrad=False, maximize=False).
 * At most three launches per call whatever n_tensors is, no float atomics, no host synchronisation, bitwise reproducible.
 * All tensors are float32 and dense: tensor i is `lengths[i]` consecutive floats at p[i] (parameter), g[i] (gradient),
 * m[i] (exp_avg) and v[i] (exp_avg_sq), each 4-byte aligned; a tensor whose four pointers are all 16-byte aligned moves
 * 16 bytes per lane, any other goes element by element.
 *
 * The table (one definition of the layout; cp_adam_table_build writes it into HOST memory, the caller copies it to the
 * device as it is): n_tensors tensor records of CP_ADAM_TENSOR_BYTES, then n_chunks chunk records of
 * CP_ADAM_CHUNK_BYTES.
 *   tensor record  bytes 0/8/16/24: p, g, m, v (device addresses); 32: int64 length; 40: int32 active (0 or 1); 44: 0
 *   chunk record   bytes 0: int32 tensor index; 4: uint32 first element within the tensor; 8: int32 element count
 *                  (1..CP_ADAM_CHUNK); 12: int32 flags (CP_ADAM_VEC: all four pointers of the tensor are 16-byte aligned)
 * Chunks are in tensor order and, within a tensor, ascending; a tensor of n elements takes ceil(n / CP_ADAM_CHUNK) chunks
 * that start at multiples of CP_ADAM_CHUNK, so a chunk never straddles two tensors, a tensor of length 0 takes none, and
 * a tensor that takes no part in the step (active_or_null[i] == 0: a parameter without a gradient) takes none either:
 * its pointers are not read, its step counter and its memory do not move.
 *
 * The state block, DEVICE memory of cp_adam_state_bytes(n_tensors) bytes that the caller zeroes once and keeps between
 * steps (8-byte aligned):
 *   CP_ADAM_STATE_NORM     float32 total_norm of the last call: sqrt(sum g^2) over the active tensors, the chunk sums and
 *                          their sum in float64 in table order; NaN when the call did not measure it (no clipping and no
 *                          CP_ADAM_SKIP_NONFINITE)
 *   CP_ADAM_STATE_COEF     float32 clip coefficient, torch's: min(1, max_norm / (total_norm + 1e-6)) in float32 (NaN for
 *                          a NaN norm); 1 without clipping
 *   CP_ADAM_STATE_SKIPPED  int32 1: the call changed nothing (see flags), else 0
 *   CP_ADAM_STATE_STEPS    float32 [n_tensors] step counters (torch's `step`), advanced by 1 for every active tensor
 *   CP_ADAM_STATE_BC(n)    float64 [2][n_tensors] bias corrections 1 - beta1^step and 1 - beta2^step, computed in float64
 *                          from the double betas (in float32 1 - 0.999f alone is off by 6e-5 relative)
 * cp_adam_step, per element of every chunk, torch's Adam as its float32 kernels round it:
 *   g' = coef g + weight_decay p;  m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * p, m and v are written; g is NOT (clip_grad_norm_ scales .grad in place, this call leaves it as it was).
 *   max_norm <= 0: no clipping (coef = 1; the sum-of-squares launch is dropped unless the flag below needs the norm).
 *   flags & CP_ADAM_SKIP_NONFINITE: when total_norm is inf or NaN the call raises CP_ADAM_STATE_SKIPPED and changes
 *   neither p, m, v nor any step counter.  Without the flag a non-finite norm goes through the arithmetic as in torch
 *   (coef 0 or NaN).
 * Refused with CP_ERR_INVALID and a cp_last_error text before any launch (cp_adam_table_bytes: returns 0): NULL pointers,
 *   n_tensors < 1, a length < 0, more than 2^31 elements in the active tensors together, an active non-empty tensor with
 *   a NULL or not 4-byte aligned address, a table buffer below cp_adam_table_bytes, n_chunks < 0, a table or state block
 *   not 8-byte aligned, lr < 0, a beta outside [0, 1), eps < 0, weight_decay < 0, any non-finite hyper-parameter, a
 *   workspace below cp_adam_workspace_bytes(n_chunks).  cp_adam_step cannot see the table's content (device memory): it
 *   trusts n_tensors / n_chunks to be those of the cp_adam_table_build call that made it.
 * ------------------------------------------------------------------------------------------ */
#define CP_ADAM_CHUNK 4096
#define CP_ADAM_TENSOR_BYTES 48
#define CP_ADAM_CHUNK_BYTES 16
#define CP_ADAM_VEC 1
#define CP_ADAM_SKIP_NONFINITE 1
#define CP_ADAM_STATE_NORM 0
#define CP_ADAM_STATE_COEF 4
#define CP_ADAM_STATE_SKIPPED 8
#define CP_ADAM_STATE_STEPS 16
#define CP_ADAM_STATE_BC(n) (16 + (((size_t)(n) * 4 + 7) / 8) * 8)
/* HOST: bytes of the table of these lengths (0: refused) and, through n_chunks, its number of chunks */
size_t cp_adam_table_bytes(int n_tensors, const int64_t* lengths, const int* active_or_null, int* n_chunks);
/* HOST: writes the table into `table` (host memory of table_bytes) from host arrays of device addresses */
int cp_adam_table_build(void* table, size_t table_bytes, int n_tensors, const void* const* p, const void* const* g,
                        const void* const* m, const void* const* v, const int64_t* lengths, const int* active_or_null,
                        int* n_chunks);
size_t cp_adam_state_bytes(int n_tensors);  /* 0: n_tensors < 1 */
size_t cp_adam_workspace_bytes(int n_chunks); /* 0: n_chunks < 0 */
int cp_adam_step(cp_stream_t stream, const void* table, int n_tensors, int n_chunks, double lr, double beta1, double beta2,
                 double eps, double weight_decay, double max_norm, int flags, void* state, void* workspace,
                 size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * cp_grad_*: the gradient pack of data-parallel training -- every gradient of a model into one flat float32 buffer,
 *   scaled, in one launch whatever n_tensors is; one all-reduce then runs over the buffer and cp_adam_step reads its
 *   gradients from it (the reference: torch's DataParallel, trains/base_trainer.py:42-48, and loss.mean() over the
 *   replicas, base_trainer.py:89).  No atomics, no host synchronisation, never allocates.
 *
 * The flat layout is decided by the lengths alone, so it is the same on every rank: tensor i takes lengths[i] floats at
 *   offsets[i], a multiple of 4 floats (16 bytes), offsets ascending in tensor order (a tensor of length 0 takes no
 *   space); behind the last tensor, at offsets[n_tensors] (a multiple of 4 as well), come n_tensors float flags, padded to
 *   a multiple of 4.  cp_grad_flat_elems is the length of all of it, cp_grad_flat_offsets writes the n_tensors + 1 offsets.
 *   Refused (cp_grad_flat_elems and cp_grad_pack_table_bytes: return 0; the others: CP_ERR_INVALID) with a cp_last_error
 *   text: n_tensors < 1, a length < 0, more than 2^31 - 1 elements in all.
 *
 * The table (cp_grad_pack_table_build writes it into HOST memory, the caller copies it to the device as it is):
 *   n_tensors + 1 tensor records of CP_GRAD_TENSOR_BYTES, then n_chunks chunk records of CP_GRAD_CHUNK_BYTES.
 *   tensor record  bytes 0: source (device address; NULL: the tensor has no gradient); 8: int64 offset in the flat buffer.
 *                  Record n_tensors has a NULL source and the offset of the flags.
 *   chunk record   bytes 0: int32 tensor index; 4: uint32 first element within the tensor; 8: int32 element count
 *                  (1..CP_ADAM_CHUNK); 12: int32 flags (CP_GRAD_VEC: the source is 16-byte aligned; CP_GRAD_ZERO: no source)
 *   Chunks are in tensor order and, within a tensor, ascending; a tensor of n elements takes ceil(n / CP_ADAM_CHUNK) chunks
 *   that start at multiples of CP_ADAM_CHUNK, whether it has a source or not: a chunk never straddles two tensors, and
 *   n_chunks depends on the lengths alone.  `offsets` must be the n_tensors + 1 values of cp_grad_flat_offsets.
 *
 * cp_grad_pack, one launch: for a tensor with a source flat[offsets[i] + k] = scale * src_i[k] (one float32 multiply;
 *   scale == 1 is a plain copy); for a tensor without, the region is set to 0; flat[offsets[n_tensors] + i] = 1.0 where
 *   tensor i has a source, else 0.0.  The padding floats between the tensors and behind the flags are never written (the
 *   caller zeroes the buffer once), nor is anything at or past flat_elems.  A source that IS its destination
 *   (src_i == flat + offsets[i]) is allowed and scales in place; any other overlap of a source with the flat buffer is NOT
 *   checked and gives undefined values.  A source that is 16-byte aligned moves 16 bytes per lane, any other goes element by
 *   element (the destination is always 16-byte aligned).
 *   Refused with CP_ERR_INVALID before any launch: a NULL table or flat, n_tensors < 1, n_chunks < 0, a table not 8-byte or a
 *   flat not 16-byte aligned, a source not 4-byte aligned (at cp_grad_pack_table_build), a non-finite scale, a flat_elems
 *   below what a table of n_tensors tensors and n_chunks chunks can describe.  cp_grad_pack cannot see the table's content
 *   (device memory): it trusts n_tensors / n_chunks to be those of the cp_grad_pack_table_build call that made it.
 * ------------------------------------------------------------------------------------------ */
#define CP_GRAD_TENSOR_BYTES 16
#define CP_GRAD_CHUNK_BYTES 16
#define CP_GRAD_VEC 1
#define CP_GRAD_ZERO 2
/* HOST: floats of the flat buffer of these lengths (0: refused) */
size_t cp_grad_flat_elems(int n_tensors, const int64_t* lengths);
/* HOST: writes offsets[0 .. n_tensors] */
int cp_grad_flat_offsets(int n_tensors, const int64_t* lengths, int64_t* offsets);
/* HOST: bytes of the table of these lengths (0: refused) and, through n_chunks, its number of chunks */
size_t cp_grad_pack_table_bytes(int n_tensors, const int64_t* lengths, int* n_chunks);
/* HOST: writes the table into `table` (host memory of table_bytes) from a host array of device addresses */
int cp_grad_pack_table_build(void* table, size_t table_bytes, int n_tensors, const void* const* src, const int64_t* lengths,
                             const int64_t* offsets, int* n_chunks);
int cp_grad_pack(cp_stream_t stream, const void* table, int n_tensors, int n_chunks, float* flat, int64_t flat_elems,
                 float scale);

/* ------------------------------------------------------------------------------------------
 * Overlay: the detections drawn into the 8-bit frames on the device -- what the reference's `out_img_pred` shows
 *   (detectors/object_pose.py:357-392 `save_results` through utils/debugger.py:131-162 `add_coco_bbox`, :214-296
 *   `add_coco_hp`, :299-320 `add_axes`), without a read-back of the records.  Added without an ABI change (new entry points).
 *
 * A primitive is 8 x int32: kind, x0, y0, x1, y1, size, colour (B | G << 8 | R << 16), aux.  Pixel Q is covered by
 *   CP_DRAW_SEGMENT  size = thickness t in 1..16: 4 dist^2(Q, segment P0P1) <= t^2, in exact integers (a capsule)
 *   CP_DRAW_DISC     size = radius r in 0..64: |Q - P0|^2 <= r^2
 *   CP_DRAW_RECT     size = thickness t: the union of the four segments between (x0,y0) (x1,y0) (x1,y1) (x0,y1)
 *   CP_DRAW_FILL     the rectangle with both corners inclusive, corners in any order
 *   CP_DRAW_GLYPH    aux = ASCII code, (x0, y0) = top-left of the cell, size = integer scale s in 1..8: each set bit of the
 *                    library's own 5 x 7 font is an s x s block (cell pitch 6 s); the digits, ' ', '.', ':', '/', '-' and the
 *                    letters of "op", "ID:", "Pred:", "Frame", "GT", "PnP" exist, any other code draws nothing
 *   kind 0 or unknown: nothing.
 * Coordinates lie in [CP_DRAW_COORD_MIN, CP_DRAW_COORD_MAX]; a primitive with a coordinate or a size outside its range is
 * skipped whole, never clamped (csrc/draw_common.h states the rule and its int64 bounds; cv2's rasteriser is not reproduced:
 * no anti-aliasing, not its thick-line polygons, not its Hershey font).
 * Painter's order: a pixel takes the colour of the highest-indexed primitive of its image that covers it.  Pixels no
 * primitive covers, and the pad bytes of a pitched row, are not written.
 *
 * cp_draw_primitives: frames DEVICE uint8 [B, H, pitch_bytes] (rows of W BGR pixels), drawn in place; prims DEVICE int32
 *   [B, P, 8], P slots per image, unused slots kind 0 (the capacity is known to the host, the occupancy is not: device-built
 *   lists need no read-back).  Two launches on `stream` (per-image compaction of the slots that draw, then one workgroup per
 *   64 x 16 pixel tile), no allocation, no synchronisation, no atomics: deterministic and capturable.
 *   workspace: cp_draw_workspace_bytes(B, P) bytes (0: B or P refused), 16-byte aligned.
 *   Refused with CP_ERR_INVALID before any device work: NULL pointers, B < 1, P outside 1..CP_DRAW_MAX_P, H or W outside
 *   1..CP_DRAW_MAX_DIM, pitch_bytes < 3 W, a workspace below the query or not 16-byte aligned.
 *
 * cp_draw_detections / cp_draw_tracks: the list builders, one thread per record.  Record (b, k) owns the CP_DRAW_SLOTS
 *   slots [k CP_DRAW_SLOTS, (k + 1) CP_DRAW_SLOTS) of image b in prims [B, K CP_DRAW_SLOTS, 8] (K = cap for the tracks) and
 *   leaves all-zero slots where it draws nothing: slot CP_DRAW_SLOT_BOX the box, CP_DRAW_SLOT_LABEL the label's rectangle and
 *   its CP_DRAW_LABEL_CHARS glyphs ("ID:<n>"; the score and `Pred:` lines need Python's decimal formatting and are drawn by
 *   the host path only), CP_DRAW_SLOT_DISCS the 8 vertices, CP_DRAW_SLOT_EDGES the 12 edges, CP_DRAW_SLOT_CROSS the crosses
 *   (front, top, top, front, top, top: the reference's nested loop as it runs), CP_DRAW_SLOT_AXES the 3 axes.
 *   Only records with score > vis_thresh; float64 coordinates are truncated towards zero as np.int32 / int() do, and one that
 *   is not finite or leaves the coordinate range withdraws its primitive; the box is clipped to [0, width] x [0, height].
 *   cp_draw_detections: post / count from cp_postprocess, det_pnp from cp_pnp_from_post or NULL (no cuboids), cam DEVICE
 *   float64 [B,4] (fx, fy, cx, cy) or NULL (no axes); the axes' camera-frame box is rebuilt from the solve as
 *   `finish_detection` does (OpenCV frame with show_axes, the evaluation's otherwise).
 *   cp_draw_tracks: `state` of cp_track_step; draws the tracks in this frame's `boxes` (flags bit 2) with projected_cuboid
 *   (bit 0) and the axes of kps_3d_cam_kf (bit 1).
 * cp_draw_params: HOST struct.  theme: 0 'black', 1 'white' (opt.debugger_theme); labels: draw "ID:<n>" (with tracking_task);
 *   width, height: the frame size the boxes are clipped to.
 * ------------------------------------------------------------------------------------------ */
#define CP_DRAW_SEGMENT 1
#define CP_DRAW_DISC 2
#define CP_DRAW_RECT 3
#define CP_DRAW_FILL 4
#define CP_DRAW_GLYPH 5
#define CP_DRAW_COORD_MIN (-8192)
#define CP_DRAW_COORD_MAX 8191
#define CP_DRAW_MAX_DIM 8192
#define CP_DRAW_MAX_P 65536
#define CP_DRAW_SLOTS 44
#define CP_DRAW_SLOT_BOX 0
#define CP_DRAW_SLOT_LABEL 1   /* the label's filled rectangle, then CP_DRAW_LABEL_CHARS glyphs */
#define CP_DRAW_LABEL_CHARS 13 /* "ID:" + at most 10 digits */
#define CP_DRAW_SLOT_DISCS 15  /* 8 vertices */
#define CP_DRAW_SLOT_EDGES 23  /* 12 edges */
#define CP_DRAW_SLOT_CROSS 35  /* front, top, top, front, top, top: the reference's nested loop as it runs */
#define CP_DRAW_SLOT_AXES 41   /* y, z, x */
typedef struct cp_draw_params {
    double vis_thresh;
    int reg_bbox, show_axes, paper_display, tracking_task, theme, labels, width, height;
} cp_draw_params;
size_t cp_draw_workspace_bytes(int B, int P);
int cp_draw_primitives(cp_stream_t stream, unsigned char* frames_bhwc_bgr, int B, int H, int W, size_t pitch_bytes,
                       const int* prims, int P, void* workspace, size_t workspace_bytes);
int cp_draw_detections(cp_stream_t stream, const double* post, const int* count, const double* det_pnp, const double* cam, int B,
                       int K, const cp_draw_params* params, int* prims);
int cp_draw_tracks(cp_stream_t stream, const void* state, int B, int cap, const double* cam, const cp_draw_params* params,
                   int* prims);

#ifdef __cplusplus
}
#endif
#endif /* CENTERPOSE_HIP_H */
