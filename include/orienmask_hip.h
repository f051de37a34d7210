/* orienmask_hip.h -- C ABI of the MI355X (gfx950) OrienMask inference hot path.
 *
 * One shared library, liborienmask_hip.so, plain pointers and sizes only (no torch types).
 * Every device buffer is allocated by the caller (the Python host passes
 * torch-ROCm tensor.data_ptr()); the library never allocates device memory on the hot path
 * and launches only on the stream it is handed.  All functions return 0 on success or a
 * negative OM_E* code; om_last_error() holds the message (thread-local).  No exceptions
 * cross this boundary; the library has no mutable global state besides that thread-local message, the process-wide
 * kernel-choice switches (om_set_*_variant, om_set_stem_fusion: A/B runs and tests) and the unit-test entries at the end, which
 * own a hipMalloc'ed tile-queue word each.
 * Threading: forwards of one om_model may be enqueued from several host threads when every thread uses its own stream and its
 * own workspace.  WORKSPACES: a `workspace` / `scratch` / `partials` argument is memory the entry may use as it likes for the
 * duration of the call and whose CONTENTS ARE UNDEFINED ON ENTRY: every entry clears, writes or masks what it later reads, on the
 * stream it is handed, and its outputs do not depend on what the memory held (old activations, NaNs, stale tickets and counts:
 * tests/test_workspace_contract.py fills it with 0x00 / 0xFF / 0x7C / 0x01 and compares the outputs bit for bit).  The same holds
 * for every output buffer: an entry never reads an output element before writing it.  The ONLY words a caller must initialise are
 * named where they are declared: om_sgd_clip_step's valid_since and clip state, om_sgd_clip_ema_step's EMA state (zeroed once),
 * om_recover_masks_rle_strings' str_cursor (zeroed per call), om_conv2d_split*'s optional status_dev, and om_loss_accumulate's
 * counter block.  The caller serialises (a) stream captures of one model (they share one second stream), (b) om_profile_* and
 * (c) more than 64 caller streams with an attached postprocess at once.  The reference's plugin surface is single-threaded
 * under the GIL and never leaves this contract.
 *
 * What each entry point replaces in the reference (/root/reference):
 *   om_model_* / om_forward        OrienMaskYOLOFPNPlus.__init__/forward
 *                                  model/orienmask_yolo_fpnplus.py:9-90 (+ model/base.py:104-137,
 *                                  model/backbone/darknet.py:6-54), i.e. what trainer/tester.py:39-40
 *                                  and infer.py:154-155 call as `model(image)`
 *   om_postprocess                 OrienMaskYOLOPostProcess.apply
 *                                  eval/orienmask_yolo_postprocess.py:66-166, called at
 *                                  trainer/tester.py:43-44 and infer.py:156
 *   om_nms                         the pybind export `nms(dets[n,5], threshold) -> keep`
 *                                  eval/src/nms_cpu.cpp:65-75 / eval/src/nms_cuda.cpp:8-17, called
 *                                  from eval/function.py:69-72,98-101
 *   om_conv2d                      one ConvBNRelu (model/base.py:104-137); exported so parity tests
 *                                  can check a single layer against torch
 */
#ifndef ORIENMASK_HIP_H
#define ORIENMASK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OM_VERSION 140          /* 0.1.4: forward status word (om_forward_status_offset, OM_STATUS_*), no process-wide switches */

#define OM_OK 0
#define OM_EINVAL (-1)          /* bad argument (null pointer, shape not supported) */
#define OM_ESTATE (-2)          /* call order (forward before load_weights, ...) */
#define OM_ENOMEM (-3)          /* caller-provided workspace too small */
#define OM_EHIP (-4)            /* a HIP runtime call failed; see om_last_error() */

#define OM_MAX_SCALES 3
#define OM_MAX_ANCHORS 9

typedef struct om_model om_model;
typedef void* om_stream;        /* a hipStream_t (torch.cuda.current_stream().cuda_stream) */

/* Layout of one convolution inside the packed weight blob (all offsets in floats).
 * weights: [cout_pad][ksize*ksize][cin] (OHWI, rows >= cout zero);  scale/shift: [cout_pad]
 * y = conv(x) * scale + shift, then LeakyReLU(0.1) if leaky (BatchNorm folded by the host). */
typedef struct om_layer_info {
    char name[64];              /* reference module prefix, e.g. "backbone.conv4.3.conv.1" */
    int32_t cin, cout, cout_pad, ksize, stride;
    int32_t has_bn;             /* 1: conv(bias=False)+BN+leaky;  0: conv(bias=True) only */
    int32_t leaky;
    int32_t wino_planes;        /* 0: no Winograd weights; 16: F(2x2,3x3); 24: F(2x4,3x3) (2 rows x 4 columns per tile) */
    int64_t w_off, scale_off, shift_off;
    int64_t wino_off;           /* >= 0: Winograd weights U = G_y g G_x^T, [wino_planes][cout_pad][cin], plane index
                                   = 4 i + j (16) or 6 i + j (24), for the stride-1 3x3 layers; -1: none */
    int64_t wino_alt_off;       /* wino_planes == 24 only: the layer's F(2x2,3x3) weights [16][cout_pad][cin] as well, used when
                                   the batch is too small for the 2 x 4 tiling to fill the chip; -1 otherwise */
    int64_t w16_off;            /* fp16 path: offset IN HALFS into the fp16 weight blob (om_model_load_weights_f16):
                                   [cout_pad][ksize*ksize][cin] fp16 (rows >= cout zero); -1: the stem (always fp32) */
    int64_t wsplit_off;         /* split-operand mode (om_model_set_precision(m, 1)): offset in 4-BYTE WORDS into the split blob
                                   (om_model_load_weights_split) of the layer's weights as hi/lo fp16 pairs of
                                   x = weight * 2^e[cout]  (hi = fp16(x), lo = fp16(x - hi)):
                                   wino_planes == 24: the F(2x4,3x3) planes, [24][cout_pad][cin / 16][2][16] halfs -- per row and
                                     group of 16 input channels the 16 hi halfs, then the 16 lo halfs;
                                   otherwise: the direct weights, [cout_pad][ksize*ksize][cin / 16][4][8] halfs -- per group of
                                     16 input channels hi of channels {0-3, 8-11}, hi of {4-7, 12-15}, lo of {0-3, 8-11}, lo of
                                     {4-7, 12-15} (the order in which a lane half reads fp32 activations from LDS);
                                   -1: the stem (always fp32 operands) */
    int64_t wsplit_scale_off;   /* offset in 4-byte words into the split blob of [cout_pad] floats scale * 2^-e[cout] (the
                                   power of two is exact, so the epilogue rounds as with the unscaled weights) */
    int64_t wsplit_direct_off;  /* wino_planes == 24 only (else -1): the same layer's DIRECT 3x3 weights in the "otherwise" layout
                                   of wsplit_off, with exponents of their own, for the latency mode (om_model_set_latency_cells) */
    int64_t wsplit_direct_scale_off;   /* ... and their [cout_pad] floats scale * 2^-e[cout] */
} om_layer_info;

/* Constants of OrienMaskYOLOPostProcess.__init__ (eval/orienmask_yolo_postprocess.py:9-37). */
typedef struct om_post_cfg {
    int32_t num_scales;                         /* 3 */
    int32_t grid_h[OM_MAX_SCALES], grid_w[OM_MAX_SCALES];   /* coarse -> fine, e.g. 17,34,68 */
    int32_t image_h, image_w;                   /* 544, 544; orientation maps are image/4 */
    int32_t anchors_per_scale;                  /* 3 */
    float anchor_w[OM_MAX_ANCHORS], anchor_h[OM_MAX_ANCHORS];    /* pixels, index = anchor id */
    int32_t anchor_mask[OM_MAX_SCALES][3];      /* anchor ids used by each scale */
    int32_t num_classes;                        /* 80 */
    float conf_thresh;                          /* 0.005 */
    float nms_thresh;                           /* 0.5, suppress when IoU >= thresh */
    int32_t nms_pre, nms_post;                  /* 400, 100 */
    float orien_thresh;                         /* 0.3 */
    int32_t bbox_pix_stride;                    /* floats between pixels of the NHWC bbox heads
                                                   (256 for om_forward's outputs) */
    int32_t nms_semantics;                      /* which of the reference's two NMS backends (eval/function.py:98-101) the
                                                   suppression follows:
                                                   0 = nms_cpu (eval/src/nms_cpu.cpp:4-63): areas (x2-x1)*(y2-y1), suppress
                                                       when IoU >= nms_thresh, survivors in ascending candidate order;
                                                   1 = nms_cuda (eval/src/nms_kernel.cu:13-140): areas w*h, suppress when
                                                       IoU > nms_thresh, survivors in score-descending order */
    int32_t nms_normalized;                     /* batched_nms(normalized=...), eval/function.py:91-92: 1 = class offset
                                                   cls * 2.0; 0 = cls * (max(x, y) + max(w, h) / 2 + 0.5) over the image's
                                                   candidates */
    int32_t anchors_of_scale[OM_MAX_SCALES];    /* anchors of each scale where they differ (len(anchor_mask[i]),
                                                   postprocess.py:17-27), 1..3; 0 = anchors_per_scale.  num_scales may be 1..3:
                                                   the heads of unused scales are not read (pass NULL) */
} om_post_cfg;

int om_version(void);
const char* om_last_error(void);

/* ---- model ------------------------------------------------------------------------------- */
int om_model_create(om_model** out, int num_anchors, int num_classes);    /* OrienMaskYOLOFPNPlus */
/* variant 0: OrienMaskYOLOFPNPlus (model/orienmask_yolo_fpnplus.py:9-90);
 * variant 1: OrienMaskYOLO (model/orienmask_yolo.py:8-86: one route8 into a 192-channel neck4, no skips). */
int om_model_create_variant(om_model** out, int variant, int num_anchors, int num_classes);
void om_model_destroy(om_model* m);
int om_model_num_layers(const om_model* m);
int om_model_layer_info(const om_model* m, int index, om_layer_info* info);
size_t om_model_weight_floats(const om_model* m);
/* packed_dev: device pointer to the blob described by om_model_layer_info; it must stay alive
 * (and unchanged) for as long as om_forward is called.  dtype: 0 = float32. */
int om_model_load_weights(om_model* m, const void* packed_dev, size_t bytes, int dtype);

/* ---- precision of om_forward's convolutions (no counterpart in the reference, whose convolutions are whatever cuDNN /
 * MKLDNN run) -----------------------------------------------------------------------------------------------------------
 * 0: operands fp32 on v_mfma_f32_32x32x2_f32 (products exact, fp32 accumulate).
 * 1: SPLIT operands, in EVERY convolution: the fused F(4,3) kernel of the stride-1 3x3 layers (conv_wino14.hip), the implicit
 *    GEMM of the 1x1 / stride-2 / head layers (conv_igemm_split.hip), and backbone.conv1 + backbone.conv2.0, which om_forward
 *    runs as ONE kernel (conv_stem2.hip: conv1's 27-term products on the matrix pipe with hi/lo operands too; equal to
 *    om_conv2d_stem followed by om_conv2d_split within 2e-6 of the tensor's scale, not bit for bit).  That fusion is off
 *    while om_model_keep_activations is on, so om_layer_output_view then shows conv1 / conv2.0 from the two-kernel path
 *    (conv1 with fp32 operands); tests/test_hip_parity.py::test_stem2_split_matches_two_kernels compares the two.  Every fp32 operand x
 *    is carried as hi = fp16(x), lo = fp16(x - hi) and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with
 *    fp32 accumulation (the lo*lo term, <= 2^-22 of the product, is dropped): 5.3x the matrix rate at the same bytes per
 *    element.  Representation error <= 2^-22 |x| for |x| >= 2^-14 * 2^11 and 2^-25 absolute below (measured end to end in
 *    DESIGN.md 3.5).  Weights are pre-scaled per output channel by the packer; activations are split as they are, so a
 *    layer input must stay below fp16's 65504 in magnitude -- for a stride-1 3x3 layer its TRANSFORMED input, up to 10x
 *    the activation in the fused F(4,3) kernel om_forward runs (20x in om_conv2d_winograd24_split).  An operand beyond that range turns the layer's outputs into NaN, and every split-operand kernel
 *    raises OM_STATUS_SPLIT_RANGE in the forward's status word when it stores a non-finite output (below): the caller
 *    re-runs that batch with mode 0 (orienmask_amd/model.py does).  Needs om_model_load_weights_split; activations between
 *    layers stay fp32.  In this mode the stride-1 3x3 layers run the fused F(4,3)-along-the-rows kernel (conv_wino14.hip:
 *    the transformed input never leaves the CU) at EVERY size (mode 0 switches between F(2x4,3x3) and F(2x2,3x3) at 1700
 *    1/32-scale cells per batch), so an image's outputs do not depend on the batch it is in. */
size_t om_model_weight_split_words(const om_model* m);
int om_model_load_weights_split(om_model* m, const void* packed_split_dev, size_t bytes);
int om_model_set_precision(om_model* m, int mode);
/* Latency mode of precision 1 (no counterpart in the reference, whose published figure is bs = 1 FPS: README.md:5,
 * infer.py:143-172).  cells > 0: a forward whose batch has fewer than `cells` 1/32-scale cells (B * H/32 * W/32; one 544 x 544
 * image has 289) runs its stride-1 3x3 layers as DIRECT convolutions with split operands in the implicit GEMM -- small tiles,
 * one short round -- instead of the fused F(4,3) kernel, whose 128 x 64 tiles leave most of the chip idle at a few images.
 * Same layer, other summation: heads agree with the fused form to ~1e-6 of scale, not bit for bit, so an image's outputs then
 * depend on which side of the switch its batch is.  0 (default): off -- outputs independent of the batch size. */
int om_model_set_latency_cells(om_model* m, long long cells);
/* Latency mode only: the implicit GEMM's launches of few tiles (<= 256 tiles of 64 x 64 / 128 x 64: one image's 1/16- and
 * 1/32-scale layers are 40 .. 152) cut every tile's k loop into up to `max_parts` parts (default 8; as many as two workgroups per
 * CU take in one round, sixteen k-steps each at least), one workgroup per part; the parts' raw accumulators meet in the
 * workspace's partial-tile area and the part that arrives last sums them IN PART ORDER and stores the tile -- no spinning, and
 * the same bits whichever part is last.  At bs = 1 these layers stream their weights (19 MB for a 512 -> 1024 3x3 layer) and
 * the number of CUs that request decides the rate.  1: whole tiles. */
int om_model_set_latency_ksplit(om_model* m, int max_parts);
int om_model_get_precision(const om_model* m);
/* Precision mode 1 only: 1 (default) = the routes and skips (the 1x1 layers whose output the reference up-samples and concatenates,
 * orienmask_yolo_fpnplus.py:78-86) store ONE copy at their own resolution and the 1x1 layer behind the concat reads them
 * up-sampled (om_conv2d_split_gather); 0 = they store their output replicated into the concat buffer, as modes 0 / fp16 do.
 * Same values bit for bit; changes om_forward_workspace_bytes (call it again).  Not active while om_model_keep_activations
 * is on (om_layer_output_view reports the concat slices). */
int om_model_set_upsample_on_read(om_model* m, int enable);

size_t om_forward_workspace_bytes(const om_model* m, int B, int H, int W);
/* workspace: om_forward_workspace_bytes bytes, 256-byte aligned, contents undefined on entry -- activations and Winograd scratch
 * (shared by live range), the partial-tile area of the stream-K / split-K forms, one block of queue / flag / arrival words per
 * layer and the status word; om_forward clears the words on `stream` before its first layer and nothing else needs clearing.
 * x: [B,3,H,W] float32 NCHW, H and W multiples of 32.
 * bbox32/16/8: [B, H/s, W/s, 256] float32 NHWC, channels [0, A*(5+C)) valid  (the caller views
 *              them as [B, A*(5+C), H/s, W/s] with strides)
 * oriens:      [B, 6*A, H/4, W/4] float32 NCHW contiguous */
int om_forward(om_model* m, const float* x, int B, int H, int W, float* bbox32, float* bbox16, float* bbox8,
               float* oriens, void* workspace, size_t ws_bytes, om_stream stream);
/* The forward's STATUS WORD: one int32 inside the workspace handed to om_forward, om_forward_status_offset() bytes from its
 * start, cleared when a forward starts and OR-ed by its kernels (om_forward_f16 has no conditions to report).  The caller reads it with whatever device-to-host copy it does anyway after the step
 * (orienmask_amd/eval.py reads it together with the detection counts).  0 = the outputs are valid. */
#define OM_STATUS_SPLIT_RANGE 1 /* precision mode 1: a split-operand layer stored a non-finite output -- an operand left the
                                   fp16 range of the hi/lo representation (or the fp32 result itself is non-finite): re-run
                                   the batch with om_model_set_precision(m, 0) */
#define OM_STATUS_SK_TIMEOUT 2  /* a stream-K finisher gave up waiting for its partner workgroup's partial tile (bounded spin
                                   so that a fault cannot hang the device): the outputs are invalid */
size_t om_forward_status_offset(const om_model* m, int B, int H, int W);

/* ---- fp16 activations, fp32 accumulate (BASELINE.json configs[4]; no reduced-precision path exists in the
 * reference -- the arithmetic is defined by oracle/orienmask_ref.py:forward_f16) -------------------------------
 * Activations between layers and the convolution weights are IEEE fp16; sums, BatchNorm scale/shift, LeakyReLU and the
 * residual add are fp32, rounded once per layer at the store; the stem reads the fp32 image; the four head tensors are
 * written fp32 exactly as om_forward writes them.  Needs BOTH blobs: om_model_load_weights (scale/shift, stem) and
 * om_model_load_weights_f16 (the fp16 weights laid out per om_layer_info.w16_off, om_model_weight_halfs() halfs). */
size_t om_model_weight_halfs(const om_model* m);
int om_model_load_weights_f16(om_model* m, const void* packed_f16_dev, size_t bytes);
size_t om_forward_f16_workspace_bytes(const om_model* m, int B, int H, int W);      /* contents undefined on entry, as om_forward's */
int om_forward_f16(om_model* m, const float* x, int B, int H, int W, float* bbox32, float* bbox16, float* bbox8,
                   float* oriens, void* workspace, size_t ws_bytes, om_stream stream);
/* kernel that runs layer `index` in the fp16 configuration (6 = conv3x3_f16_tall_kernel<512,128>, 7 = conv_stem2_f16_kernel: the first
 * two layers in one launch, 8 = a layer computed inside the previous layer's kernel): algo 0 = conv_stem_kernel<f16>, 1 = conv_igemm_f16_kernel<bm,bn>,
 * 4 = conv3x3_f16_kernel<bm,bn> (stride-1 3x3: the three taps of a kernel row share one LDS copy of the input rows) */
int om_layer_tile_f16(const om_model* m, int index, int B, int H, int W, int* bm, int* bn, int* algo);

/* ---- intermediate activations (tests / debugging; BASELINE configs[1] checks the DarkNet-53 features) -------------------
 * Where layer `index`'s output lives inside the workspace of the last om_forward (f16 = 0) / om_forward_f16 (f16 = 1) call
 * at this problem size: an NHWC view [B, H/div, W/div, channels] starting byte_offset bytes into the workspace, pixel
 * stride pix_stride ELEMENTS (a concat buffer's slice has pix_stride > channels).  The four head layers write
 * caller-owned tensors and are rejected; so is a model without om_model_keep_activations(m, 1). */
int om_layer_output_view(const om_model* m, int index, int B, int H, int W, int f16, size_t* byte_offset, int* channels,
                         int* pix_stride, int* div);
/* The forward's activations (and the Winograd scratch) share workspace memory by live range: a tensor's slab is reused once its
 * last consumer has run.  keep = 1 gives every tensor its own slab again (larger om_forward_workspace_bytes) so that
 * om_layer_output_view can be read after the forward; it must be set before the workspace is sized. */
int om_model_keep_activations(om_model* m, int keep);

/* ---- measurement: per-layer durations with HIP events on the stream om_forward launches on
 * (the reference measures with torch.cuda.Event pairs, utils/timer.py:70-82).  While enabled, every
 * om_forward records events around every kernel of every layer; om_profile_read synchronises on them and
 * returns, per layer (graph order of om_model_layer_info) and summed over the recorded forwards, the
 * milliseconds of the layer's main kernel (layer_ms) and of its pre-pass (layer_pre_ms: the Winograd input
 * transform; 0 for single-kernel layers), plus the number of forwards. */
/* Tile shape (rows x channels per workgroup) of the conv kernel instantiation that runs layer `index` at
 * this problem size; 0 x 0 for the stem kernel.  Lets a profile be grouped by kernel.  algo: 0 conv_stem_kernel, 1 conv_igemm_f32,
 * 2 / 3 Winograd F(2x2) GEMM / fused, 5 / 6 F(2x4) GEMM with fp32 / split operands, 7 conv_igemm_split, 8 wino14_split (fused
 * F(4,3)), 9 conv_stem2_split_kernel (precision mode 1: backbone.conv1 + backbone.conv2.0 in one kernel, reported for conv1),
 * 10 "part of the previous layer's kernel" (reported for conv2.0 then: om_forward launches nothing for it), 11 conv_igemm_split in
 * its GATHER form (precision mode 1: the 1x1 layer behind an up-sample + concat reads the low-resolution slices where their
 * producers stored them, om_conv2d_split_gather). */
int om_layer_tile(const om_model* m, int index, int B, int H, int W, int* bm, int* bn, int* algo);
/* algo: 0 = conv_stem_kernel, 1 = conv_igemm_f32_kernel<bm,bn>, 2 = wino_input_kernel + wino_gemm_kernel<bm,bn>,
 *       3 = wino_fused_kernel<bn> (input transform fused into the GEMM's loader),
 *       5 = wino24_input_kernel + wino24_gemm_kernel (Winograd F(2x4,3x3), 64x64 tile) */
int om_profile_enable(om_model* m, int enable);
/* record events only around the layers with layer_mask[i] != 0 (an event pair costs a few microseconds of GPU time, so a
 * timed region that only needs one kernel's durations should not pay for all ~90 layers); om_profile_read then returns 0
 * for the other layers */
int om_profile_enable_layers(om_model* m, const unsigned char* layer_mask, int n_layers);
int om_profile_read(om_model* m, float* layer_ms, float* layer_pre_ms, int n_layers, int* n_forwards);

/* ---- one convolution (unit-test entries) ---------------------------------------------------
 * These entries exist so that parity tests can check single layers; unlike the hot path they own a few device words (the
 * tile-queue ticket, hipMalloc'ed on first use and never freed), which om_forward carves from the caller's workspace. */
/* in: [B,H,W,cin] NHWC (pixel stride in_pix_stride floats); w/scale/shift as in om_layer_info;
 * res: optional [B,Ho,Wo,cout] NHWC added after the activation; out: [B,Ho,Wo,cout] NHWC. */
int om_conv2d(const float* in, int B, int H, int W, int cin, int in_pix_stride, const float* w,
              const float* scale, const float* shift, int cout, int ksize, int stride, int leaky,
              const float* res, int res_pix_stride, float* out, int out_pix_stride, om_stream stream);
/* The same with the output layouts om_forward uses: out_mode 0 = NHWC; 1 = NHWC with every output pixel replicated up x up
 * (NearestUpsample fused into the producer, model/base.py:95-101: out is [B, Ho*up, Wo*up, ...]); 2 = NCHW contiguous
 * [B, cout, Ho, Wo] (the orientation head). */
int om_conv2d_mode(const float* in, int B, int H, int W, int cin, int in_pix_stride, const float* w,
                   const float* scale, const float* shift, int cout, int ksize, int stride, int leaky,
                   const float* res, int res_pix_stride, float* out, int out_pix_stride, int out_mode, int up,
                   om_stream stream);
/* The same layer through Winograd F(2x2,3x3) (3x3, stride 1): u = G g G^T as [16][cout_pad][cin];
 * scratch: om_conv2d_winograd_scratch_bytes(B,H,W,cin) bytes of device memory for the transformed input. */
size_t om_conv2d_winograd_scratch_bytes(int B, int H, int W, int cin);
int om_conv2d_winograd(const float* in, int B, int H, int W, int cin, int in_pix_stride, const float* u,
                       const float* scale, const float* shift, int cout, int leaky, const float* res,
                       int res_pix_stride, float* out, int out_pix_stride, void* scratch, size_t scratch_bytes,
                       om_stream stream);
/* fp16 layer (unit-test entry): in/res/w fp16 (w laid out as om_layer_info.w16_off describes), scale/shift fp32,
 * out fp16 NHWC, or fp32 NHWC when out_f32 = 1; pixel strides in elements of the respective type. */
int om_conv2d_f16(const void* in, int B, int H, int W, int cin, int in_pix_stride, const void* w, const float* scale,
                  const float* shift, int cout, int ksize, int stride, int leaky, const void* res, int res_pix_stride,
                  void* out, int out_pix_stride, int out_f32, om_stream stream);
int om_conv2d_stem_f16(const float* in, int B, int H, int W, const float* w, const float* scale, const float* shift,
                       int cout, void* out, om_stream stream);
/* The same layer through Winograd F(2x4,3x3): u = G_y g G_x^T as [24][cout_pad][cin], cout_pad = cout rounded up to 64. */
size_t om_conv2d_winograd24_scratch_bytes(int B, int H, int W, int cin);
int om_conv2d_winograd24(const float* in, int B, int H, int W, int cin, int in_pix_stride, const float* u,
                         const float* scale, const float* shift, int cout, int leaky, const float* res,
                         int res_pix_stride, float* out, int out_pix_stride, void* scratch, size_t scratch_bytes,
                         om_stream stream);
/* one ConvBNRelu with split operands (conv_igemm_split.hip): w_split / scale_split as om_layer_info.wsplit_off /
 * wsplit_scale_off describe for a layer without F(2x4) form; other arguments as om_conv2d_mode.  tile_bm x tile_bn: 0, 0 =
 * the tile shape om_forward would pick, else one of the built shapes 256x128, 128x128, 128x64, 64x64, 128x32 with tile_bn
 * dividing cout_pad (per call: tile sweeps and tests of every instantiation).  status_dev: optional device int32 that the
 * kernel ORs OM_STATUS_* bits into (the caller clears it), NULL = not reported. */
int om_conv2d_split(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* w_split,
                    const float* scale_split, const float* shift, int cout, int ksize, int stride, int leaky, const float* res,
                    int res_pix_stride, float* out, int out_pix_stride, int out_mode, int up, int tile_bm, int tile_bn,
                    int32_t* status_dev, om_stream stream);
/* om_conv2d_split with a tile's k loop cut into up to max_parts (1 .. 8) parts, as the latency mode's small launches run
 * (om_model_set_latency_ksplit: fewer where the tile count or the k loop's length caps it).  Takes effect for the 128x64 and
 * 64x64 shapes of at most 256 tiles; anything else runs as om_conv2d_split.  The partial tiles live in library-owned memory
 * (unit-test entry; om_forward uses the caller's workspace). */
int om_conv2d_split_k(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* w_split,
                      const float* scale_split, const float* shift, int cout, int ksize, int stride, int leaky, const float* res,
                      int res_pix_stride, float* out, int out_pix_stride, int out_mode, int up, int tile_bm, int tile_bn,
                      int max_parts, int32_t* status_dev, om_stream stream);
/* The 1x1 layer behind an up-sample + concat, as om_forward runs neck16.0 / neck8.0 / neck4.0 in precision mode 1
 * (conv_igemm_split.hip, GATHER form): the input channels are the concatenation of nseg (1..4) NHWC tensors, segment g with
 * seg_channels[g] channels (a multiple of 32) stored at [B, H/seg_up[g], W/seg_up[g], seg_pix_stride[g]] (seg_up a power of two
 * dividing H and W) and read nearest-up-sampled; cout_pad must be a multiple of 128.  Bit-identical to om_conv2d_split over
 * the materialised concat.  Replaces F.interpolate(scale_factor, 'nearest') + torch.cat + the following 1x1 Conv-BN-LeakyReLU
 * of /root/reference/model/orienmask_yolo_fpnplus.py:78-86 (forward: route / skip concatenations). */
int om_conv2d_split_gather(int nseg, const float* const* seg_ptr, const int* seg_channels, const int* seg_pix_stride,
                           const int* seg_up, int B, int H, int W, const void* w_split, const float* scale_split, const float* shift,
                           int cout, int leaky, float* out, int out_pix_stride, int32_t* status_dev, om_stream stream);
/* ... with split operands (om_model_set_precision mode 1): u_split as om_layer_info.wsplit_off describes, scale_split =
 * scale * 2^-e per output channel; scratch as for om_conv2d_winograd24; status_dev as for om_conv2d_split. */
int om_conv2d_winograd24_split(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* u_split,
                               const float* scale_split, const float* shift, int cout, int leaky, const float* res,
                               int res_pix_stride, float* out, int out_pix_stride, void* scratch, size_t scratch_bytes,
                               int32_t* status_dev, om_stream stream);
/* The stride-1 3x3 layer in the fused split-operand form om_forward runs in precision mode 1 (conv_wino14.hip: Winograd F(4,3)
 * along the rows, the input transform inside the kernel, no scratch): u14_split = the packed weights
 * [cout_pad/64][cin/16][6][3][64][32 halfs] (orienmask_amd/pack.py: winograd14_weights_split), cout_pad = cout rounded up to 64,
 * cin a multiple of 16; scale_split = scale * 2^-e; status_dev as for om_conv2d_split. */
int om_conv2d_wino14_split(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* u14_split,
                           const float* scale_split, const float* shift, int cout, int leaky, const float* res,
                           int res_pix_stride, float* out, int out_pix_stride, int32_t* status_dev, om_stream stream);
/* Host only: how that kernel cuts a B x H x W layer into blocks.  Returns the number n <= 2 of classes of column blocks and fills
 * classes[5 k ..] = {first tile column, tile columns per block, blocks, padded rows per block, row blocks} for k < n (a tile column
 * is four pixels from x = 0; a class's blocks are side by side).  The padded row space is G = b * row_pitch + y + 1, G = 0 ..
 * B * row_pitch (row_pitch = H + 1: neighbouring images share a zero row); *m_tiles = sum of blocks x row blocks. */
int om_conv2d_wino14_blocks(int B, int H, int W, int* classes, int* row_pitch, long long* m_tiles);
/* The same layer as TWO kernels with a 128 x 128 tile (round 6; conv_wino14.hip: wino14_v_kernel writes the transformed input
 * V = [cin/16][6][B (H + 2)][ceil(W / 4)] entries of 64 bytes into `scratch`, wino14_wide_kernel reads it by LDS-DMA: eight waves of
 * 64 entries x 32 channels x six planes, the fused kernel's epilogue): the same products in the same order, BIT-IDENTICAL outputs.
 * cout_pad must be a multiple of 128 and cout of 4, the views 16-byte aligned.  om_forward (precision mode 1) runs the layers with
 * at least 512 input channels this way -- where 2.5 x the input through HBM for the pre-pass is small next to the layer's work --
 * unless om_set_wino14_wide(0) / OM_NO_W14_WIDE=1 (process-wide A/B switch; default on). */
size_t om_conv2d_wino14_wide_scratch_bytes(int B, int H, int W, int cin);
int om_conv2d_wino14_wide(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* u14_split,
                          const float* scale_split, const float* shift, int cout, int leaky, const float* res,
                          int res_pix_stride, float* out, int out_pix_stride, void* scratch, size_t scratch_bytes,
                          int32_t* status_dev, om_stream stream);
int om_set_wino14_wide(int on);
int om_get_wino14_wide(void);
/* A/B switches of the two first-layers fusions (process-wide; default on; OM_NO_STEM3=1 / OM_NO_STEM2_F16=1 in the environment
 * turn them off before the first use): which = 0 the third layer (backbone.conv2.1.conv.0) inside the split-operand
 * first-two-layers kernel, which = 1 the fp16 first-two-layers kernel.  Off -> the separate kernels: bit-identical results for
 * which = 0; for which = 1 conv1's fp32 sums are formed in another order before their one rounding to fp16 (a few per cent of the
 * activations move by one fp16 step: inside the fp16 configuration's tolerance, not bit-identical).  For a
 * view the fused launcher cannot take (alignment, pixel stride, descriptor size) the forward plans the separate kernels ahead. */
int om_set_stem_fusion(int which, int on);
int om_get_stem_fusion(int which);      /* 1 on, 0 off, -1 bad argument */
/* Which kernel runs the stride-1 3x3 layers of the fp16 configuration (process-wide; the results are the same sums in the same
 * order, bit-identical): 0 the 256 x 128 / 128 x 128 / 128 x 64 shared-patch kernel everywhere (rounds 1-4); 1 (default;
 * environment OM_C3_TALL) the tall-patch kernel of round 5 (conv3x3_f16.hip: 512 raster pixels x 128 channels per eight-wave
 * workgroup, one input patch per 32-channel chunk for all nine taps) where the tile chooser picks it; 2 wherever it can run
 * (cout_pad a multiple of 128, rows of at most 191 pixels). */
int om_set_conv3x3_f16_variant(int mode);
int om_get_conv3x3_f16_variant(void);
/* first layer: in [B,3,H,W] NCHW -> out [B,H,W,cout] NHWC, 3x3 stride 1. */
int om_conv2d_stem(const float* in, int B, int H, int W, const float* w, const float* scale,
                   const float* shift, int cout, float* out, om_stream stream);
/* The first TWO layers as om_forward runs them in precision mode 1 (conv_stem2.hip): backbone.conv1 (3 -> 32, 3x3, BN, LeakyReLU;
 * w1 [32][27], scale1 / shift1 [32] as for om_conv2d_stem) and backbone.conv2.0 (32 -> 64, 3x3 stride 2, BN, LeakyReLU when
 * leaky2; w2_split / scale2_split as om_layer_info.wsplit_off / wsplit_scale_off describe, shift2 [64]) in one kernel:
 * in [B,3,H,W] NCHW (H, W even) -> out [B,H/2,W/2,out_pix_stride] NHWC.  conv1's products run on the matrix pipe with split
 * operands here (fp32 multiply-adds in om_conv2d_stem): the same values as om_conv2d_stem followed by om_conv2d_split to 2e-6 of
 * the tensor's scale, not bit for bit.  status_dev as for om_conv2d_split.
 * Replaces /root/reference/model/backbone/darknet.py:20-22 (conv1, conv2's first block) as called from model/base.py:104-137. */
int om_conv2d_stem2_split(const float* in, int B, int H, int W, const float* w1, const float* scale1, const float* shift1,
                          const void* w2_split, const float* scale2_split, const float* shift2, int cout2, int leaky2, float* out,
                          int out_pix_stride, int32_t* status_dev, om_stream stream);
/* ... with the layer behind them in the same launch (round 5): backbone.conv2.1.conv.0, the 64 -> 32 1x1 convolution of the first
 * residual block (/root/reference/model/backbone/darknet.py:9-13), computed on each tile's conv2.0 outputs while they are in the
 * workgroup: `out` is written as by om_conv2d_stem2_split (the block's residual reads it), `out3` [B,H/2,W/2,out3_pix_stride] gets
 * what om_conv2d_split would compute from it -- the same split8 / three-instruction arithmetic per 16 channels, bit for bit.
 * w3_split / scale3_split: conv_weights_split rows [32][4][4][8] halfs and scale * 2^-e; cout3 = 32. */
int om_conv2d_stem3_split(const float* in, int B, int H, int W, const float* w1, const float* scale1, const float* shift1,
                          const void* w2_split, const float* scale2_split, const float* shift2, int cout2, int leaky2, float* out,
                          int out_pix_stride, const void* w3_split, const float* scale3_split, const float* shift3, int cout3, int leaky3,
                          float* out3, int out3_pix_stride, int32_t* status_dev, om_stream stream);
/* The same two layers as om_forward_f16 runs them (conv_stem2.hip: conv_stem2_f16_kernel; round 5): conv1 from the fp32 image with
 * fp32 weights (fp32-level sums, one rounding to fp16 -- the activation om_conv2d_stem_f16 stores, never written here), conv2.0 on
 * fp16 operands: w2_f16 = its fp16 rows [64][9 * 32] (om_layer_info.w16_off), scale2 / shift2 [64] fp32; out [B,H/2,W/2,out_pix_stride]
 * fp16 NHWC, 8-byte aligned.  Equal to om_conv2d_stem_f16 followed by om_conv2d_f16 up to conv1's rounding ties. */
int om_conv2d_stem2_f16(const float* in, int B, int H, int W, const float* w1, const float* scale1, const float* shift1,
                        const void* w2_f16, const float* scale2, const float* shift2, int cout2, int leaky2, void* out,
                        int out_pix_stride, om_stream stream);

/* ---- preprocess: FastCOCOTransform.__call__ + pad, fused ------------------------------
 * Replaces /root/reference/data/transform.py:444-510 (permute, Resize = F.interpolate bilinear
 * align_corners=False, Normalize = (x - mean) / std) and /root/reference/infer.py:21-32 (zero padding to a
 * multiple of 32).  in: [N,h,w,3] float32 HWC; the image is resized to resize_h x resize_w, normalised and
 * placed at (pad_top, pad_left) of the [N,3,out_h,out_w] NCHW output; everything else is pad_value. */
int om_preprocess(const float* in_nhwc, int N, int h, int w, int resize_h, int resize_w, const float* mean3,
                  const float* std3, int pad_top, int pad_left, int out_h, int out_w, float pad_value, float* out_nchw,
                  om_stream stream);
/* The same for n images of their OWN sizes and element types in one call: what an inference loop has after decoding a
 * directory of photos (uint8, BGR from cv2).  One launch per OM_PRE_BATCH images; the table reaches the kernel by value, so the
 * entry allocates nothing, copies nothing and does not synchronise.
 *   images  HOST array of n DEVICE pointers, each to a dense [h,w,3] HWC image: uint8 at any byte address (images staged back
 *           to back need no padding between or behind them: no byte outside [image, image + h*w*3*elem) is read), float32
 *           4-byte aligned
 *   geom    HOST int32 [n][8], row i = { h, w, resize_h, resize_w, pad_top, pad_left, flags, 0 } of image i:
 *           flags = OM_PRE_U8 (the image is uint8; otherwise float32) | OM_PRE_BGR (output channel c reads source channel
 *           2 - c; mean3 / std3 are indexed by the OUTPUT channel); the last element is reserved and must be 0
 *   out     [n,3,out_h,out_w] float32: image i resized to resize_h x resize_w, normalised and placed at (pad_top, pad_left) of
 *           plane set i, everything else of the plane set pad_value.  16-byte stores when out_w is a multiple of 4 and
 *           out_nchw 16-byte aligned, 4-byte stores otherwise
 * Every plane set has the bits om_preprocess writes for float32(image) in RGB order with the same geometry (uint8 -> float32
 * is exact).  A null pointer, n <= 0, a row whose resized image does not fit the output or has an empty side, and unknown flag
 * bits are refused before anything is launched, with a message naming the image index. */
#define OM_PRE_BATCH 16         /* images per launch */
#define OM_PRE_U8 1
#define OM_PRE_BGR 2
int om_preprocess_batch(const void* const* images, const int32_t* geom, int n, const float* mean3, const float* std3,
                        int out_h, int out_w, float pad_value, float* out_nchw, om_stream stream);
/* pad() alone on an NCHW tensor of `planes` = N*C planes. */
int om_pad_nchw(const float* in, long long planes, int h, int w, int pad_top, int pad_left, int out_h, int out_w,
                float pad_value, float* out, om_stream stream);

/* ---- JPEG decoding ---------------------------------------------------------------------------
 * Baseline JPEG in two halves: the host parses the stream and undoes the Huffman coding (csrc/om_jpeg.cpp: plain C++, no HIP
 * call, nothing that initialises the GPU -- a loader worker may call it), the device does the arithmetic (csrc/jpeg.hip:
 * dequantise, accurate-integer IDCT, chroma up-sampling, YCbCr -> RGB).  The result is, bit for bit, what libjpeg(-turbo) gives
 * with its defaults (ISLOW IDCT, fancy up-sampling): PIL's Image.open(...).convert('RGB').
 *
 * SUPPORTED: SOF0, 8-bit samples, 8-bit quantisation tables, Huffman coding, 1 component (sampling 1x1) or 3 components with
 * ids 1,2,3, luma sampling 1x1, 2x1 or 2x2 with chroma 1x1 (4:4:4, 4:2:2, 4:2:0), one interleaved scan, restart intervals, any
 * legal layout of the DQT / DHT / APPn / COM segments.  UNSUPPORTED (status OM_OK, supported = 0 and a reason OM_JPEG_R_*; the
 * caller gives the bytes to a host reader): every other process, precision, component set or sampling, 16-bit quantisation
 * tables, an Adobe APP14 segment, several scans, DNL or a height of 0, an Exif orientation other than 1 (host readers disagree
 * on whether to rotate), an image of 2^31 / 3 pixels or more, and a dequantised coefficient beyond OM_JPEG_COEF_BOUND.  REJECTED
 * (status OM_EINVAL and a message): a stream that is truncated, runs past its buffer, carries an undefined Huffman code or table
 * reference, has a run past coefficient 63, a bad restart sequence, no EOI behind the scan, or a DC predictor that leaves int16.
 * No byte outside [bytes, bytes + len) is read and none outside the given buffers written, for any byte string whatever.
 *
 * info: int32 [OM_JPEG_INFO_WORDS], written by both host entries:
 *   [OM_JPEG_I_WIDTH] [OM_JPEG_I_HEIGHT] [OM_JPEG_I_NCOMP] [OM_JPEG_I_HMAX] [OM_JPEG_I_VMAX] [OM_JPEG_I_RESTART]
 *   [OM_JPEG_I_SUPPORTED] 1 / 0, [OM_JPEG_I_REASON] OM_JPEG_R_*; and, for a supported stream,
 *   [OM_JPEG_I_BLOCKS] 8x8 blocks of all components: the coefficient buffer is 128 bytes times this;
 *   [OM_JPEG_I_COMP + OM_JPEG_COMP_WORDS * c + ...] of component c: 0 h, 1 v (sampling factors), 2 blocks per row and 3 block
 *   rows of its plane (padded to whole MCUs), 4 real width ceil(W * h / hmax) and 5 real height ceil(H * v / vmax) in samples.
 * OM_JPEG_COEF_BOUND: the device IDCT works in int32, libjpeg's C code in 64-bit long.  With every |coefficient * quantiser| at
 * most this, every intermediate of both IDCT passes fits int32 (derivation: csrc/om_jpeg.cpp; proof by interval arithmetic:
 * tests/test_jpeg_cpu.py), so the two agree.  An 8-bit image's own coefficients stay below 1024 + 127. */
#define OM_JPEG_BATCH 16        /* images per launch set of om_jpeg_decode_batch */
#define OM_JPEG_COEF_BOUND 1170
#define OM_JPEG_INFO_WORDS 32
#define OM_JPEG_I_WIDTH 0
#define OM_JPEG_I_HEIGHT 1
#define OM_JPEG_I_NCOMP 2
#define OM_JPEG_I_SUPPORTED 3
#define OM_JPEG_I_REASON 4
#define OM_JPEG_I_HMAX 5
#define OM_JPEG_I_VMAX 6
#define OM_JPEG_I_RESTART 7
#define OM_JPEG_I_BLOCKS 8
#define OM_JPEG_I_COMP 10
#define OM_JPEG_COMP_WORDS 6
#define OM_JPEG_R_NONE 0
#define OM_JPEG_R_PROGRESSIVE 1
#define OM_JPEG_R_ARITHMETIC 2
#define OM_JPEG_R_LOSSLESS 3
#define OM_JPEG_R_PRECISION 4   /* 12- or 16-bit samples */
#define OM_JPEG_R_FRAME 5       /* another frame type (extended sequential, differential) or sample precision */
#define OM_JPEG_R_QUANT16 6
#define OM_JPEG_R_COMPONENTS 7  /* 4 components, or ids other than 1,2,3 */
#define OM_JPEG_R_ADOBE 8
#define OM_JPEG_R_SAMPLING 9
#define OM_JPEG_R_SCANS 10
#define OM_JPEG_R_DNL 11
#define OM_JPEG_R_ORIENTATION 12
#define OM_JPEG_R_SIZE 13
#define OM_JPEG_R_RANGE 14      /* a |coefficient * quantiser| beyond OM_JPEG_COEF_BOUND (found by om_jpeg_entropy_decode only) */
#define OM_JPEG_DESC_WORDS 8
/* The headers alone: geometry, supported or not and why.  Host only. */
int om_jpeg_info(const uint8_t* bytes, size_t len, int32_t* info);
/* Host only.  coef (cap_bytes >= 128 * info[OM_JPEG_I_BLOCKS], else OM_ENOMEM) receives the UNDEQUANTISED coefficients,
 * de-zigzagged, [block][64] int16, component after component, each component's blocks in raster order of its padded plane;
 * quant receives [ncomp][64] uint16, the quantisation table of each component in natural order.  info is written as by
 * om_jpeg_info; of an unsupported stream nothing else is written.  A stream this entry finds to be unsupported only while
 * decoding (OM_JPEG_R_RANGE, OM_JPEG_R_SCANS behind the first scan) has supported = 0 on return as well. */
int om_jpeg_entropy_decode(const uint8_t* bytes, size_t len, int16_t* coef, size_t cap_bytes, uint16_t* quant, int32_t* info);
/* Device side.  desc: HOST int64 [n][OM_JPEG_DESC_WORDS], row i = { width, height, ncomp, hmax, vmax, coef_off, quant_off,
 * out_off } of image i: the geometry om_jpeg_info reported and where the image's data lie -- coef_off in int16 elements into
 * coef (a multiple of 64), quant_off in uint16 elements into quant (a multiple of 64), out_off in bytes into out (a multiple of
 * 16).  coef, quant, out and workspace are DEVICE memory, 16-byte aligned; coef and quant hold what om_jpeg_entropy_decode wrote.
 * out receives, at out_off, the dense [height,width,3] uint8 RGB image (a grey stream replicated to three channels); no other
 * byte of out is written.  Images of one call may differ in size and sampling; two launches per OM_JPEG_BATCH images
 * (IDCT into component planes in the workspace, then up-sampling + colour), asynchronous on `stream`, no allocation, no
 * synchronisation, no atomics.  workspace: om_jpeg_workspace_bytes(desc, n) bytes, contents undefined on entry, as out's.
 * Every row is checked against coef_elems, quant_elems, out_bytes and ws_bytes before anything is launched.  The streams must
 * be ones the host SUPPORTS: nothing here looks at a coefficient's value. */
size_t om_jpeg_workspace_bytes(const int64_t* desc, int n);      /* 0: a bad row, see om_last_error */
int om_jpeg_decode_batch(const int64_t* desc, int n, const int16_t* coef, size_t coef_elems, const uint16_t* quant,
                         size_t quant_elems, void* workspace, size_t ws_bytes, uint8_t* out, size_t out_bytes, om_stream stream);

/* ---- postprocess --------------------------------------------------------------------------
 * workspace (every om_postprocess* entry and the buffer handed to om_model_attach_postprocess): om_postprocess_workspace_bytes
 * bytes, 256-byte aligned, contents undefined on entry -- candidate keys, per-tile counts, the radix histograms and the list
 * counter (cleared by the entry), the compacted candidate list, the detections' mask constants and, for nms_pre > 512, the
 * suppression bit matrix.  om_postprocess_assemble reads what om_postprocess_detect left there; om_postprocess_masks nothing. */
size_t om_postprocess_workspace_bytes(const om_post_cfg* cfg, int B);
/* Limits of the fused path (the reference has none): nms_pre <= 1024; 1..3 scales of 1..3 anchors; conf_thresh >= 0 (the
 * decode skips a candidate whose sigmoid(objectness) is not above it before reading its class logits); num_classes such that
 * (2047 / C + 2) * max(C & ~31, C & 31) + 63 <= 6144 -- every C < 2048 (a decode thread's visits per sweep are unrolled: 10 of
 * them cover C <= 251, a second instantiation with 24 the rest, e.g. LVIS's 1203; csrc/post.hip DEC_VISITS / DEC_VISITS_MANY);
 * larger class counts return OM_EINVAL with that message.
 * out_bbox [B,nms_post,5] (cx,cy,w,h normalised, score); out_cls [B,nms_post] int64;
 * out_mask [B,nms_post,image_h,image_w] uint8 0/1 (rows >= out_count[b] are left untouched);
 * out_count [B] int32; out_keep [B,nms_post] int32 position of each detection in the
 * pre-NMS candidate list, may be NULL.  oriens as written by om_forward. */
int om_postprocess(const om_post_cfg* cfg, const float* bbox32, const float* bbox16, const float* bbox8,
                   const float* oriens, int B, float* out_bbox, int64_t* out_cls, uint8_t* out_mask,
                   int32_t* out_count, int32_t* out_keep, void* workspace, size_t ws_bytes, om_stream stream);
/* om_postprocess in its two halves (it IS detect followed by assemble on one stream).  detect: decode, threshold, top-nms_pre,
 * batched NMS, top-nms_post (postprocess.py:102-154) -- reads the box heads only; writes out_bbox / out_cls / out_count /
 * out_keep and the detections' mask constants into the workspace.  assemble: the masks (postprocess.py:69-72,141-144,156-164) of
 * those detections from the orientation head, with the same workspace.  Apart they let the first half run on another stream
 * while the forward is still computing the orientation branch: om_model_attach_postprocess. */
int om_postprocess_detect(const om_post_cfg* cfg, const float* bbox32, const float* bbox16, const float* bbox8, int B,
                          float* out_bbox, int64_t* out_cls, int32_t* out_count, int32_t* out_keep, void* workspace, size_t ws_bytes,
                          om_stream stream);
int om_postprocess_assemble(const om_post_cfg* cfg, const float* oriens, int B, const int32_t* out_count, uint8_t* out_mask,
                            void* workspace, size_t ws_bytes, om_stream stream);
/* The step as ONE call sequence on the forward (tester.py:39-44's two lines; infer.py:154-156).  While a postprocess is
 * attached, om_forward (fp32 / split precision) also runs it into the attached buffers: decode + select are launched on a second
 * stream that the library creates, forked off the caller's stream by an event as soon as the last box-head layer is launched and
 * joined behind the forward's last layer -- they read the box heads only, the select kernel is ONE workgroup per image, so beside
 * the skips, neck4 and the orientation head they cost nothing -- and the mask kernel follows on the caller's stream.  On return
 * everything is ordered before later work on the caller's stream; under stream capture the second stream joins the capture
 * through the same events.  Same kernels on the same inputs as om_forward followed by om_postprocess: same bits.  cfg == NULL
 * detaches.  The buffers must stay valid while attached (orienmask_amd/eval.py attaches around one forward). */
int om_model_attach_postprocess(om_model* m, const om_post_cfg* cfg, float* out_bbox, int64_t* out_cls, uint8_t* out_mask,
                                int32_t* out_count, int32_t* out_keep, void* post_workspace, size_t post_ws_bytes);

/* The same postprocess around a caller-supplied NMS callable -- the reference takes ANY nms_func(dets, cls) -> (dets[keep],
 * cls[keep], keep) (/root/reference/eval/orienmask_yolo_postprocess.py:9-11,146-148); the fused om_postprocess implements
 * batched_nms itself.  om_postprocess_candidates: decode, threshold and top-nms_pre (postprocess.py:102-122): cand_dets
 * [B,nms_pre,5] (cx, cy, w, h, score), cand_cls [B,nms_pre], cand_field [B,nms_pre] (anchor field of the candidate: its
 * orientation channels are 2 * field, 2 * field + 1), cand_count [B], in the order the reference hands them to self.nms.  The
 * caller runs its callable per image, applies the top-nms_post of postprocess.py:150-154 and hands the survivors to
 * om_postprocess_masks: dets [B,nms_post,5], field [B,nms_post], count [B] (device) -> out_mask [B,nms_post,image_h,image_w]
 * (postprocess.py:156-164).  Same workspace size as om_postprocess. */
int om_postprocess_candidates(const om_post_cfg* cfg, const float* bbox32, const float* bbox16, const float* bbox8, int B,
                              float* cand_dets, int64_t* cand_cls, int32_t* cand_field, int32_t* cand_count, void* workspace,
                              size_t ws_bytes, om_stream stream);
int om_postprocess_masks(const om_post_cfg* cfg, const float* oriens, int B, const float* dets, const int32_t* field,
                         const int32_t* count, uint8_t* out_mask, void* workspace, size_t ws_bytes, om_stream stream);

/* measurement: launch geometry and resource use of the three postprocess kernels (which: 0 = post_decode_kernel,
 * 1 = post_select_kernel, 2 = post_mask_kernel) as the runtime reports them for this device: threads per workgroup, VGPRs
 * per lane, static LDS bytes per workgroup and the number of workgroups one CU can hold (hipOccupancyMaxActiveBlocks...).
 * bench.py turns them into waves/SIMD against the gfx950 limit of 8 (north_star: "occupancy for NMS/mask-assembly"). */
int om_post_kernel_occupancy(int which, int* threads, int* vgprs, int* lds_bytes, int* max_blocks_per_cu);

/* ---- COCO-format conversion ------------------------------------------------------------
 * om_recover_bbox: COCOMetrics._recover_shape_bbox, /root/reference/eval/coco_eval.py:146-189.
 *   bbox [K,stride] normalised (cx,cy,w,h,..) -> out_xywh [K,4] top-left x, y, w, h in original-image pixels.
 *   collate_pad6 = (left,right,top,down,h,w) and pad6 = (top,down,left,right,h,w) are HOST arrays or NULL.
 * om_recover_masks_rle: COCOMetrics._recover_shape_segm (:191-205: crop the paddings, flips, bilinear resize
 *   to the original size, round) + the column-major run lengths of pycocotools' rleEncode (:120-122).
 *   mask [K,H,W] u8 0/1; crop_* = total padding to strip on each side; counts [K][max_runs] u32 receives the
 *   run lengths (first run counts zeros); n_runs [K] their number (> max_runs: buffer too small, counts of
 *   that mask are undefined); resized_or_null: optional [K,orig_h,orig_w] u8 copy of the resized masks. */
int om_recover_bbox(const float* bbox, int K, int stride, const int32_t* collate_pad6, const int32_t* pad6, int hflip,
                    int vflip, int orig_h, int orig_w, float* out_xywh, om_stream stream);
int om_recover_masks_rle(const uint8_t* mask, int K, int H, int W, int crop_top, int crop_down, int crop_left,
                         int crop_right, int hflip, int vflip, int orig_h, int orig_w, uint32_t* counts, int max_runs,
                         int32_t* n_runs, uint8_t* resized_or_null, om_stream stream);
/* om_recover_masks_rle_strings: the same conversion for a whole BATCH in one launch, ending on the device with what the
 *   reference gets from maskUtils.encode(...)['counts'] (/root/reference/eval/coco_eval.py:120-122): pycocotools' rleToString
 *   of every mask's run lengths (published algorithm of cocoapi common/maskApi.c; the library is absent offline, so the
 *   STRING is pinned against oracle/rle_ref.c only).  images: HOST array, one entry per image (K may be 0); masks are numbered
 *   image after image.  counts [sum K][max_runs] scratch for the run lengths, n_runs [sum K] (> max_runs: that mask needs a
 *   larger buffer, its str_off is -1).  Every mask appends its string to ONE byte buffer: str_cursor[0] = bytes reserved
 *   (zeroed by the caller), str_cursor[1] = masks whose string did not fit str_capacity; str_off / str_len [sum K].  The host
 *   then copies the cursor + offsets and bytes[0:cursor] once per batch instead of 30 MB of masks per image.  counts, n_runs,
 *   str_bytes, str_off and str_len: contents undefined on entry; both str_cursor words are the caller's to zero. */
typedef struct om_rle_image {
    const uint8_t* mask;        /* [K,H,W] u8 0/1, device */
    int32_t K, H, W;
    int32_t crop_top, crop_down, crop_left, crop_right;
    int32_t hflip, vflip, orig_h, orig_w;
} om_rle_image;
int om_recover_masks_rle_strings(const om_rle_image* images, int n_images, uint32_t* counts, int max_runs, int32_t* n_runs,
                                 uint8_t* str_bytes, long long str_capacity, int32_t* str_cursor, int32_t* str_off,
                                 int32_t* str_len, om_stream stream);

/* ---- InferenceVisualizer (utils/visualizer.py:33-127 of the reference; orienmask_amd/visualizer.py) ------------------------
 * om_visualize: the device part of InferenceVisualizer.__call__ for a BATCH of images of any sizes -- _recover_shape_segm (crop
 *   the paddings, bilinear resize align_corners=False, float values kept), the ascending sort by resized area, plot_all_mask's
 *   alpha composite and round() to uint8 -- in one pass over each output, without a [K,h,w] intermediate: per pixel, every kept
 *   mask whose nonzero extent covers it is sampled with the bilinear code of om_recover_masks_rle, the cumulative product is
 *   kept in double (torch's cumprod) and the weighted colour sum in float, in the reference's association.  Optionally the
 *   thickness-1 box outlines cv2.rectangle would draw (rows y1, y2 over [x1, x2], columns x1, x2 over [y1, y2], clipped; where
 *   outlines cross, the later box in kept order wins).  Two launches per OM_VIS_BATCH images (a per-mask pre-pass, then the
 *   composite).  images: HOST array; the source images are only read.  workspace: om_visualize_workspace_bytes(images, n)
 *   bytes of device memory (32 B per kept mask), contents undefined on entry. */
#define OM_VIS_MAX_KEPT 512     /* kept detections per image */
#define OM_VIS_BATCH 16         /* images per launch pair */
typedef struct om_vis_image {
    const float* image;         /* [h,w,3] float32 HWC, device, 16-byte aligned */
    uint8_t* out;               /* [h,w,3] uint8 HWC, device, 4-byte aligned */
    float* out_float;           /* optional [h,w,3] float32: the composite before rounding (tests); NULL: not written */
    const uint8_t* mask;        /* [K,Hn,Wn] 0/1 bytes at the network input size, device; read when with_mask and n_keep > 0 */
    const int32_t* keep;        /* [n_keep] device: index into mask of each kept detection, in kept order */
    const float* colors;        /* [n_keep,3] device: RGB colour of each kept detection */
    const int32_t* boxes;       /* [n_keep,4] device: x1, y1, x2, y2 of each kept detection; read when draw_boxes */
    int32_t n_keep, Hn, Wn;
    int32_t crop_left, crop_right, crop_top, crop_down;    /* pad_info[:4] */
    int32_t h, w;
    int32_t with_mask, draw_boxes;
    float alpha;
} om_vis_image;
size_t om_visualize_workspace_bytes(const om_vis_image* images, int n_images);
int om_visualize(const om_vis_image* images, int n_images, void* workspace, size_t ws_bytes, om_stream stream);

/* ---- COCO evaluation without pycocotools (orienmask_amd/cocoeval.py; the reference's eval/coco_eval.py:80-105 calls
 * pycocotools' COCO / COCOeval).  Masks are column-major bit-packed bitmaps: with hw = ceil(h/32), word x * hw + yb holds rows
 * 32 yb .. 32 yb + 31 of column x; bits past row h are zero.  Every array below is a caller-allocated DEVICE buffer.
 * om_cocoeval_masks builds n_masks bitmaps from sources.  Mask m: mask_hw[2m] = h, [2m+1] = w, its bitmap at word
 *   mask_word_off[m] of the workspace; its sources' bitmaps are at the words mask_src_word_off[mask_src_first[m] ..
 *   mask_src_first[m+1]) and are ORed into it (maskUtils.merge).
 *   Source s: src_kind 0 = polygon (src_len doubles x0 y0 x1 y1 ... at poly + src_data_off; pycocotools' rleFrPoly, at most
 *   4096 vertices), 1 = uncompressed RLE (src_len uint32 counts at counts + src_data_off), 2 = compressed RLE string
 *   (src_len bytes at strings + src_data_off; rleFrString); src_mask = its mask, src_word_off = its own bitmap (the mask's
 *   when it is the mask's only source).  Sources [0, n_poly) are the polygons.  bitmap_words = words of every bitmap in the
 *   workspace; workspace: om_cocoeval_workspace_bytes(bitmap_words, n_masks) bytes, 256-byte aligned, contents undefined on
 *   entry; after the call it holds the bitmaps, then per mask {area, first column, last column} (int32; empty: w, -1).
 * om_cocoeval_mask_stats copies those [n_masks][3] int32 out.
 * om_cocoeval_mask_iou: for pair p = (pairs[2p] det mask, pairs[2p+1] gt mask) of one workspace, maskUtils.iou: i / u in
 *   double, 0 when i == 0, u = the det's area when pair_crowd[p]; -1 for masks of different sizes.
 * om_cocoeval_bbox_iou: the same pairs over boxes [.][4] x, y, w, h (double): pycocotools' bbIou.
 * om_cocoeval_match: COCOeval.evaluateImg for n_groups (image, category) groups, one wave each: dets [dt_first[g],
 *   dt_first[g+1]) already in score order and cut to maxDets[-1], gts [gt_first[g], gt_first[g+1]) in json order, ious
 *   [D][G] at iou_off[g].  area_rng [4][2], iou_thrs [10] (numpy's linspace values).  Lane t + 10 a (IoU threshold t, area
 *   range a) writes dt_match[lane][det] = matched gt id (0: none) and dt_ignore[lane][det]; gt_matched [40][n_gt_total] is
 *   scratch.  As in pycocotools, a match is "gt id != 0": a gt with id 0 counts as unmatched. */
size_t om_cocoeval_workspace_bytes(long long bitmap_words, int n_masks);
int om_cocoeval_masks(int n_masks, const int32_t* mask_hw, const int64_t* mask_word_off, const int32_t* mask_src_first,
                      const int64_t* mask_src_word_off, int n_poly, int n_srcs, const int32_t* src_kind, const int32_t* src_mask, const int64_t* src_data_off,
                      const int32_t* src_len, const int64_t* src_word_off, const double* poly, const uint32_t* counts,
                      const uint8_t* strings, long long bitmap_words, void* workspace, size_t ws_bytes, om_stream stream);
int om_cocoeval_mask_stats(int n_masks, long long bitmap_words, const void* workspace, int32_t* stats, om_stream stream);
int om_cocoeval_mask_iou(int n_pairs, const int32_t* pairs, const uint8_t* pair_crowd, int n_masks, const int32_t* mask_hw,
                         const int64_t* mask_word_off, long long bitmap_words, const void* workspace, double* iou,
                         om_stream stream);
int om_cocoeval_bbox_iou(int n_pairs, const int32_t* pairs, const uint8_t* pair_crowd, const double* det_box,
                         const double* gt_box, double* iou, om_stream stream);
int om_cocoeval_match(int n_groups, const int32_t* dt_first, const int32_t* gt_first, const int64_t* iou_off,
                      const double* ious, const double* dt_area, const double* gt_area, const uint8_t* gt_crowd,
                      const int64_t* gt_id, const double* area_rng, const double* iou_thrs, int n_dt_total, int n_gt_total,
                      uint8_t* gt_matched, int64_t* dt_match, uint8_t* dt_ignore, om_stream stream);

/* ---- Ground-truth segmentations decoded on the device (orienmask_amd/augment.py, samples that carry 'segm'; the reference's
 * data/dataset.py:89-100 calls pycocotools' frPyObjects / merge / decode per annotation in the loader worker).
 * om_segm_decode turns the sources of n_masks masks (0 ... 65535) into row-packed bits, the layout om_augment reads and
 *   np.packbits(mask > 0, axis=1) produces: mask m is mask_hw[2m] * ceil(mask_hw[2m+1] / 8) bytes at out + mask_out_off[m],
 *   row-major, bit 7 - (x & 7) of byte x >> 3 of a row holds column x, the pad bits of a row's last byte are zero.  Every byte
 *   of every mask is written exactly once (`out` needs no clearing) and no byte outside the masks is touched; neither `out`, the
 *   offsets nor ceil(w / 8) need any alignment.
 *   The source tables are om_cocoeval_masks': source s has src_kind (0 polygon, 1 uint32 counts, 2 string bytes), src_mask,
 *   src_data_off / src_len into poly / counts / strings and src_word_off, the word offset of ITS OWN bitmap in the workspace
 *   (w * ceil(h / 32) words each; bitmap_words = their sum); sources [0, n_poly) are the polygons (at most 4096 vertices each).
 *   Mask m is the OR (maskUtils.merge) of the bitmaps at the words mask_src_word_off[mask_src_first[m] .. mask_src_first[m+1]);
 *   a mask without sources is all zeros.  Every array is a caller-allocated DEVICE buffer.
 *   workspace: om_segm_decode_workspace_bytes(bitmap_words, n_masks) bytes, 4-byte aligned, contents undefined on entry.
 *   All launches go to `stream`; nothing is allocated, nothing synchronises; the bytes are identical from call to call (the
 *   toggles are XORed in with atomics, and XOR commutes; the pack kernel has none).  n_masks == 0 returns OM_OK at once. */
size_t om_segm_decode_workspace_bytes(long long bitmap_words, int n_masks);
int om_segm_decode(int n_masks, const int32_t* mask_hw, const int32_t* mask_src_first, const int64_t* mask_src_word_off,
                   const int64_t* mask_out_off, int n_poly, int n_srcs, const int32_t* src_kind, const int32_t* src_mask,
                   const int64_t* src_data_off, const int32_t* src_len, const int64_t* src_word_off, const double* poly,
                   const uint32_t* counts, const uint8_t* strings, long long bitmap_words, void* workspace, size_t ws_bytes,
                   uint8_t* out, om_stream stream);

/* ---- unit-test entry: the elementary functions the decode uses, restated bit-exactly from what torch-CPU runs at the
 * reference's call sites eval/orienmask_yolo_postprocess.py:127-136 (csrc/ref_math.h).  func: 0 = glibc expf (torch's
 * scalar loop), 1 = Sleef expf_u10 (torch's vectorised loop), 2 / 3 = sigmoid through either, 4 = sigmoid of a
 * [rows][num_classes] array exactly as predict[..., 5:].sigmoid() evaluates it (classes below (C/32)*32 vectorised, the
 * row tail scalar), 5 = correctly rounded expf, 6 = the mask predicate's building block (post.hip: abs_minus_bits): y[i] = the IEEE
 * difference |x[i]| - x[i ^ 1] (n even), whose SIGN decides |d| < t in post_mask_kernel -- the test checks the signs of the
 * infinite and NaN cases on the device. */
int om_ref_math(const float* x, long long n, int func, int num_classes, float* y, om_stream stream);

/* ---- NMS: the reference's native export nms(dets[n,5], threshold) -> keep (eval/src/nms_cpu.cpp:65-75,
 *      eval/src/nms_cuda.cpp:8-17), n <= 65536 (0 from om_nms_workspace_bytes above that).
 *      om_nms = om_nms_ex(semantics 0): the CPU backend (IoU >= thresh suppresses, areas from the corners cx +- w/2, keep
 *      in ascending input order, nms_cpu.cpp:4-63).  semantics 1: the CUDA backend (IoU > thresh, areas w*h, keep in
 *      score-descending order, nms_kernel.cu:13-140); score ties, which torch's CUDA sort leaves unspecified, are visited
 *      in ascending input order.  workspace: om_nms_workspace_bytes(n) bytes, 256-byte aligned, contents undefined on entry (the
 *      sorted boxes and the suppression bit matrix); keep is defined below *n_keep. */
size_t om_nms_workspace_bytes(int n);
int om_nms(const float* dets, int n, float thresh, int64_t* keep, int32_t* n_keep, void* workspace,
           size_t ws_bytes, om_stream stream);
int om_nms_ex(const float* dets, int n, float thresh, int semantics, int64_t* keep, int32_t* n_keep, void* workspace,
              size_t ws_bytes, om_stream stream);

/* ---- Loss of the validation epoch: OrienMaskYOLOMultiScaleLoss (eval/orienmask_yolo_loss.py, eval/base.py), values
 *      (om_loss) and, for training, the gradient with respect to the heads (om_loss_backward, below).
 *
 * om_loss_cfg: the loss's constants.  Per scale s < num_scales: grid_h/grid_w, anchors_of_scale[s] (1..3) anchors
 * anchor_mask[s][.] into anchor_w/anchor_h (num_anchors_total <= 9), weight[s][0..6] = the scale's per-item weight
 * (scales_weight[s] * weight[j], or 1 without `weight`: eval/orienmask_yolo_loss.py:313-315).  label_smooth / label_on are the
 * values tcls holds off / on the GT's class (float32 of ls and of 1 - ls, ls = 1 / max(C, 40) or 0).  num_classes <= OM_LOSS_MAX_CLASSES; orientation maps are exactly image/4 per side.
 *
 * Heads: per scale a bbox head [B, A*(5+C), nH, nW] and an orientation head [B, 2A, H/4, W/4], each read through its element
 * strides (bbox_stride[s] = b, channel, row, column; orien_stride[s] = b, channel, row; the orientation column stride is 1).
 * Targets as the reference's collate makes them: gt_bbox [N][4] f32 (normalised cx, cy, w, h), gt_cls [N] i64,
 * gt_index [B+1] i64 prefix offsets, gt_mask [N][H][W] u8 (0/1), all contiguous.  At most OM_LOSS_MAX_GT GTs per image.
 *
 * om_loss writes `result` (device, OM_LOSS_RESULT_FLOATS floats): per scale s at s*OM_LOSS_SCALE_FLOATS the 7 weighted terms
 * (loss_xy, loss_wh, loss_obj, loss_noobj, loss_cls, loss_orien_pos, loss_orien_neg) then 8 (numerator, count) pairs
 * (cls_conf, obj_pos, obj_neg, avg_iou, recall50, recall75, orien_pos_acc, orien_neg_acc); at OM_LOSS_FLAG_OFF a flag word
 * (int32 bits, OM_LOSS_FLAG_*).  No host synchronisation, no allocation; workspace: om_loss_workspace_bytes(cfg, B, N) bytes,
 * 256-byte aligned, contents undefined on entry (the match records and the partial sums; the layout moves with N, and a larger
 * workspace kept from another call is as good as a fresh one); `result` is cleared by the call.  N = 0 (a batch without a GT):
 * gt_bbox, gt_cls and gt_mask are not addressed and may be null.
 * The result is bit-identical from call to call: every sum has a fixed order (workgroup partials, then one fixed-order pass).
 *
 * om_loss_targets (test entry): scale s's built targets.  Any output may be null.  [B][A][nH][nW](x2 / xC) f32: bbox_pos,
 * bbox_neg, pos_scale, txy, twh, tiou, tcls; [B][A][H][W] i32 orien_mask (-1 positive, k > 0 negative count, 0 neither)
 * and [B][A][H][W][2] f32 torien (final: divided by anchor/2 and by the count).  Its workspace: om_loss_workspace_bytes + 512. */
#define OM_LOSS_MAX_CLASSES 2047
#define OM_LOSS_MAX_GT 1024
#define OM_LOSS_TERMS 7
#define OM_LOSS_METRICS 8
#define OM_LOSS_SCALE_FLOATS (OM_LOSS_TERMS + 2 * OM_LOSS_METRICS)
#define OM_LOSS_FLAG_OFF (OM_MAX_SCALES * OM_LOSS_SCALE_FLOATS)
#define OM_LOSS_RESULT_FLOATS (OM_LOSS_FLAG_OFF + 1)
#define OM_LOSS_FLAG_NONFINITE_WH 1     /* a pred_wh element is not finite (the reference prints and exits) */
#define OM_LOSS_FLAG_TOO_MANY_GT 2      /* an image has more than OM_LOSS_MAX_GT GTs or gt_index is not a valid prefix */
#define OM_LOSS_FLAG_BAD_CLASS 4        /* a gt_cls value outside [0, num_classes) */

typedef struct om_loss_cfg {
    int32_t num_scales;
    int32_t grid_h[OM_MAX_SCALES], grid_w[OM_MAX_SCALES];
    int32_t image_h, image_w;
    int32_t anchors_of_scale[OM_MAX_SCALES];
    int32_t anchor_mask[OM_MAX_SCALES][3];
    int32_t num_anchors_total;
    float anchor_w[OM_MAX_ANCHORS], anchor_h[OM_MAX_ANCHORS];
    int32_t num_classes;
    float center_region, valid_region;
    float label_smooth, label_on;        /* tcls off / on values: float32(ls) and float32(1 - ls) */
    float obj_ignore_threshold;
    float weight[OM_MAX_SCALES][OM_LOSS_TERMS];
    int64_t bbox_stride[OM_MAX_SCALES][4];
    int64_t orien_stride[OM_MAX_SCALES][3];
} om_loss_cfg;

size_t om_loss_workspace_bytes(const om_loss_cfg* cfg, int B, int N);
int om_loss(const om_loss_cfg* cfg, const float* const* bbox, const float* const* orien, int B, const float* gt_bbox,
            const int64_t* gt_cls, const int64_t* gt_index, const uint8_t* gt_mask, int N, float* result, void* workspace,
            size_t ws_bytes, om_stream stream);
int om_loss_targets(const om_loss_cfg* cfg, const float* const* bbox, int B, const float* gt_bbox, const int64_t* gt_cls,
                    const int64_t* gt_index, const uint8_t* gt_mask, int N, int scale, float* bbox_pos, float* bbox_neg,
                    float* pos_scale, float* txy, float* twh, float* tiou, float* tcls, int32_t* orien_mask, float* torien,
                    void* workspace, size_t ws_bytes, om_stream stream);

/* ---- The loss's backward: d(out) / d(pred_bbox) and d(out) / d(pred_orien) for every scale, following the reference's autograd
 *      chain (BCELoss / sigmoid / MSELoss / SmoothL1Loss backward and the adjoint of the x4 bilinear up-sample, in torch-CPU's
 *      float32 operation order), multiplied by grad_out = d(out) / d(loss_sum), a device float read by the kernels (no host
 *      synchronisation).  scales_weight: host array of num_scales floats, the multi-scale weights (eval/base.py:119); the
 *      per-item weights come from cfg->weight, which already holds them once more, as the reference's chain does.
 *
 *      Call it after om_loss on the same cfg, heads and targets, with that call's `result` and `workspace` untouched since: it reads
 *      the match records from the workspace and the bbox_pos / orientation pos / neg counts from the result vector.  grad_bbox[s]
 *      and grad_orien[s] are written through the SAME strides as the heads (cfg->bbox_stride / orien_stride), every element exactly
 *      once, zeros included; the result is bit-identical from call to call.  Two launches; no atomics, no allocation.  (Like
 *      om_postprocess_assemble, an entry whose workspace is an INPUT: what it held before om_loss does not matter.) */
int om_loss_backward(const om_loss_cfg* cfg, const float* const* bbox, const float* const* orien, int B, const int64_t* gt_index,
                     const uint8_t* gt_mask, int N, const float* result, const void* workspace, size_t ws_bytes,
                     const float* grad_out, const float* scales_weight, float* const* grad_bbox, float* const* grad_orien,
                     om_stream stream);

/* ---- The loop's per-step bookkeeping on the device: what orienmask_amd/loss.py's _finish (eval/base.py:90-121) and
 *      EvalCounter.update (eval/counter.py) do on the host after every om_loss, as ONE launch of one wave, so a training step
 *      holds no device-to-host copy.  Call it after om_loss on the same stream with that call's `result`.
 *
 * Per-step values, float32, every operation rounded once (no fused multiply-add), t = a scale's 7 terms, m = its 8 (numerator,
 * count) pairs, w = scales_weight, S = num_scales; sums over scales run over s < S only, left to right from the first scale:
 *      s_k               = (((((t0 + t1) + t2) + t3) + t4) + t5) + t6             the scale sum of scale k
 *      cross row j       = ((w0 * v0j) + (w1 * v1j)) + (w2 * v2j)                 v_kj = t_kj for j < 7, s_k for j = 7
 *      loss_sum          = ((w0 * s0) + (w1 * s1)) + (w2 * s2)                    (= cross row 7)
 *      cross metric j    = ((n0j + n1j) + n2j, (c0j + c1j) + c2j)                 numerators and counts summed separately
 *
 * The counter block (device, OM_COUNTER_BLOCK_DOUBLES float64, caller-owned, zeroed by the caller before the first call): one
 * (sum, items) pair per key at OM_COUNTER_STAGE_OFF + 2 * key; the keys are 'loss', then per scale its 7 terms and scale sum,
 * then the 8 cross-scale rows, then per scale its 8 metrics, then the 8 cross-scale metrics: 1 + 16 * (S + 1) keys, packed.
 * 'loss' and the loss keys add (double(value), 1); the metric keys add (double(numerator), double(count)) and only when
 * with_metrics != 0 (the reference's metric_log is empty for training=True).  The pairs at OM_COUNTER_EPOCH_OFF belong to the
 * caller (orienmask_amd.loss.DeviceEvalCounter folds the stage into them); the kernel never touches them.
 * Two int64 words behind the pairs latch status: at OM_COUNTER_FLAG_OFF the OR of every call's OM_LOSS_FLAG_* bits and of
 * OM_COUNTER_FLAG_NONFINITE_LOSS (this call's loss_sum is not finite); at OM_COUNTER_STEP_OFF the `step` argument of the first
 * call that set any bit, which later calls never overwrite.  The sums are added whatever the flags say.
 * `loss_sum` (device float, caller-owned) receives this call's loss_sum.  No allocation, no host synchronisation, no atomics;
 * bit-identical from run to run.
 * Pointers: `result`, `counter` and `loss_sum` are DEVICE pointers (4-, 8- and 4-byte aligned).  `scales_weight` is a HOST
 * array of num_scales floats: the launcher reads it before the launch and passes the values to the kernel by value, so the
 * caller may free or change it as soon as the call returns. */
#define OM_COUNTER_MAX_KEYS (1 + 2 * (OM_MAX_SCALES + 1) * OM_LOSS_METRICS)
#define OM_COUNTER_STAGE_OFF 0
#define OM_COUNTER_EPOCH_OFF (2 * OM_COUNTER_MAX_KEYS)
#define OM_COUNTER_FLAG_OFF (4 * OM_COUNTER_MAX_KEYS)
#define OM_COUNTER_STEP_OFF (OM_COUNTER_FLAG_OFF + 1)
#define OM_COUNTER_BLOCK_DOUBLES (OM_COUNTER_FLAG_OFF + 2)
#define OM_COUNTER_FLAG_NONFINITE_LOSS 256
int om_loss_accumulate(const float* result, int num_scales, const float* scales_weight, int with_metrics, long long step,
                       double* counter, float* loss_sum, om_stream stream);

/* ---- Training / validation augmentation: COCOTransform + collate (data/transform.py:65-441, data/collate.py:13-30 of the
 *      reference; orienmask_amd/augment.py plans every random draw on the host, these kernels do the pixel work).
 *      One record per image, in DEVICE memory; every offset and window in it was checked by the host planner.  Per output pixel:
 *      undo the flips, write the pad colour in the pad region, else cv2 INTER_LINEAR (or the INTER_AREA 2x2 mean of an exact 2x
 *      downscale) into the crop window with the jitter chain applied to each tap, then (x - mean) / std, NCHW.  Per output GT o:
 *      gt_table[2o] is the source GT (batch-global index, ToTensor's randperm already applied), gt_table[2o+1] its image;
 *      cv2 INTER_NEAREST from the row-packed bits (np.packbits, MSB first), pad 0, flips, one byte 0/1 per pixel.
 *      When any image's chain has contrast, two extra launches first reduce the grey mean of its full source in a fixed order
 *      (per-workgroup double partials, then one fixed tree per image: bit-identical from run to run, no atomics).
 *      workspace: om_augment_workspace_bytes(n_images) bytes of device memory, contents undefined on entry. */
#define OM_AUG_MAX_OPS 4
#define OM_AUG_BRIGHTNESS 0
#define OM_AUG_CONTRAST 1
#define OM_AUG_SATURATION 2
#define OM_AUG_HUE 3
typedef struct om_aug_sample {
    int64_t image_off;          /* element offset of the [src_h,src_w,3] HWC source in `images` */
    int64_t mask_off;           /* byte offset of the image's first packed mask ([src_h, (src_w+7)/8] bytes per GT) */
    double scale_x, scale_y;    /* cv2: 1 / ((double)nw / crop_w), 1 / ((double)nh / crop_h) */
    int32_t src_h, src_w;
    int32_t crop_top, crop_left, crop_h, crop_w;
    int32_t nh, nw, pad_top, pad_left;
    int32_t hflip, vflip, area2x, n_ops;
    int32_t op[OM_AUG_MAX_OPS];   /* OM_AUG_*, in the shuffled order */
    float fa[OM_AUG_MAX_OPS];     /* float32(factor) */
    float fb[OM_AUG_MAX_OPS];     /* float32(1 - factor); hue: float32(factor * 360) */
    float pad_value[3];
    int32_t gt_first, n_gt, reserved;
} om_aug_sample;
size_t om_augment_workspace_bytes(int n_images);
int om_augment(const om_aug_sample* samples, int n_images, const void* images, int images_u8, const float* mean3,
               const float* std3, int out_h, int out_w, float* out_image, const uint8_t* masks, const int32_t* gt_table, int n_gt,
               uint8_t* out_mask, int any_contrast, void* workspace, size_t ws_bytes, om_stream stream);

/* ---- The optimizer step: torch.optim.SGD (trainer/trainer.py:53 `self.optimizer.step()`, the optimizer trainer/builder.py:118-130
 *      builds) for every tensor of every parameter group in ONE launch; orienmask_amd/optim.py (class SGD) is the host side.
 *      Per element, float32, in torch-CPU's rounding (each add(alpha=) is one fma, buf.mul_(momentum) rounds on its own):
 *          d   = fma(p, wd, g)                           (OM_SGD_HAS_WD;  g negated first under OM_SGD_MAXIMIZE)
 *          buf = d                                       (OM_SGD_FIRST: the tensor's first step)
 *          buf = fma(d, 1 - dampening, buf * momentum)   (later steps)
 *          d   = nesterov ? fma(buf, momentum, d) : buf  (both only under OM_SGD_HAS_MOMENTUM)
 *          p   = fma(d, -lr, p)
 *      table: one om_sgd_tensor per tensor in DEVICE memory; lr, weight_decay and the three pointers are read from it by the
 *      kernel, so a scheduler step changes a row and nothing else.  table_host (may be null: the device table is used as it is):
 *      n_tensors rows in pinned host memory, copied to `table` on `stream` ahead of the launch (hipMemcpyAsync; the caller keeps
 *      the host rows unchanged until that copy has run).  chunks: the DEVICE work list, one om_sgd_chunk per OM_SGD_CHUNK
 *      elements of a tensor (chunk k of tensor t covers elements [k * OM_SGD_CHUNK, min(n, (k + 1) * OM_SGD_CHUNK))), built once
 *      from the element counts; rows flagged OM_SGD_SKIP (grad is None) are passed over.  param / grad / buf are dense tensors
 *      of n floats in the SAME storage order; 16-byte accesses where all three are 16-byte aligned, 4-byte accesses otherwise.
 *      No allocation, no host synchronisation; every element is written exactly once. */
#define OM_SGD_CHUNK 4096
#define OM_SGD_SKIP 1
#define OM_SGD_FIRST 2
#define OM_SGD_NESTEROV 4
#define OM_SGD_MAXIMIZE 8
#define OM_SGD_HAS_MOMENTUM 16
#define OM_SGD_HAS_WD 32
typedef struct om_sgd_tensor {
    float* param;
    const float* grad;
    float* buf;                 /* momentum buffer; unused without OM_SGD_HAS_MOMENTUM */
    int64_t n;
    float neg_lr, weight_decay, momentum, one_minus_dampening;   /* float32(-lr), float32(wd), float32(m), float32(1 - dampening) */
    uint32_t flags;             /* OM_SGD_* */
    uint32_t reserved[3];
} om_sgd_tensor;
typedef struct om_sgd_chunk {
    int32_t tensor, chunk;
} om_sgd_chunk;
int om_sgd_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                om_stream stream);

/* ---- The same step behind global L2 gradient-norm clipping: torch.nn.utils.clip_grad_norm_(params, max_norm) followed by
 *      SGD.step(), decided and applied on the device in THREE launches on `stream` (the table copy ahead of the first), without
 *      atomics, allocation or host synchronisation; bit-identical from run to run.  table_host / table / chunks as om_sgd_step.
 *        1. partials[c] = the float64 sum of g * g over chunk c (0 for a chunk of an OM_SGD_SKIP row).  Element j of a chunk belongs
 *           to lane (j / 4) % 256 whatever the gradient's alignment; a lane adds its elements in ascending order; the 256 lanes
 *           are summed by a fixed tree (lane l with l ^ 32, ^ 16, ... ^ 1 within a wave, then (w0 + w1) + (w2 + w3)).
 *        2. one workgroup: lane l adds partials l, l + 256, ... in ascending order, the same tree gives S;
 *               total_norm = (float)sqrt(S)
 *               coef       = min(1, (1 / (total_norm + 1e-6f)) * max_norm)      (float32, each operation rounded once: torch
 *                            2.10's `max_norm / (total_norm + 1e-6)` is reciprocal-then-multiply; a NaN stays a NaN)
 *               skip       = (mode & OM_CLIP_SKIP_NONFINITE) && total_norm is not finite
 *           and the state block is updated (below).
 *        3. om_sgd_step's update with every gradient element read as g * coef (rounded once, ahead of OM_SGD_MAXIMIZE's negation
 *           and of weight decay; the gradient in memory is NOT modified).  Under `skip` the launch returns without touching a
 *           parameter or a momentum buffer.  A row flagged OM_SGD_DEVICE_FIRST decides "first step" on the device:
 *           valid_since[tensor] is 0 until an update has been applied to the tensor, then the number of that step; the step is the
 *           tensor's first (buf = d) when the word is 0 or equals `step`.  A skipped step so leaves "first" pending.
 *      partials: n_chunks doubles, undefined on entry.  valid_since: n_tensors int64, zeroed by the caller once.  step: this call's
 *      number, from 1, increasing.  state: OM_CLIP_STATE_DOUBLES 8-byte words, caller-owned, zeroed by the caller before the first
 *      call: float64 at OM_CLIP_NORM_OFF / OM_CLIP_COEF_OFF (this call's total_norm and coef, float32 values), OM_CLIP_SUM_OFF and
 *      OM_CLIP_MAX_OFF (sum and maximum of the finite norms); int64 at OM_CLIP_SKIP_OFF (this call's decision), OM_CLIP_STEPS_OFF
 *      (calls), OM_CLIP_CLIPPED_OFF (finite norm and coef < 1), OM_CLIP_NONFINITE_OFF (norm not finite) and
 *      OM_CLIP_FIRST_NONFINITE_OFF (the `step` of the first such call, latched as OM_COUNTER_STEP_OFF is: never overwritten).
 *      The words from OM_CLIP_STEPS_OFF up to OM_CLIP_FIRST_NONFINITE_OFF may be zeroed by the caller between calls.
 *      max_norm must be positive and finite. */
#define OM_SGD_DEVICE_FIRST 64
#define OM_CLIP_SKIP_NONFINITE 1
#define OM_CLIP_NORM_OFF 0
#define OM_CLIP_COEF_OFF 1
#define OM_CLIP_SKIP_OFF 2
#define OM_CLIP_STEPS_OFF 3
#define OM_CLIP_SUM_OFF 4
#define OM_CLIP_MAX_OFF 5
#define OM_CLIP_CLIPPED_OFF 6
#define OM_CLIP_NONFINITE_OFF 7
#define OM_CLIP_FIRST_NONFINITE_OFF 8
#define OM_CLIP_STATE_DOUBLES 9
int om_sgd_clip_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                     double* partials, double* state, long long* valid_since, float max_norm, int mode, long long step,
                     om_stream stream);

/* ---- The same two steps with an exponential moving average (EMA) of the weights kept inside the update kernel: one more float32
 *      stream per tensor, its SHADOW, read and written beside parameter and momentum buffer (8 more bytes per element, no further
 *      launch).  shadows: n_tensors pointers in DEVICE memory, one per row of the table; a shadow holds n floats in its parameter's
 *      storage order; a null entry means the tensor is not averaged.  The shadow joins the alignment test of the 16-byte path.
 *      Per element of a row that is stepped (not OM_SGD_SKIP), with p' the parameter's new value:
 *          diff = p' - e                                  (rounded once)
 *          e    = fma(diff, omd, e)                       (one rounding)
 *      omd = float32(1 - d_k), d_k = decay, or with warm-up min(decay, (1 + k) / (10 + k)), evaluated in float64, k the number of
 *      EMA updates applied before this one.  Parameter and momentum buffer get exactly the bits om_sgd_step / om_sgd_clip_step
 *      give them.  A row under OM_SGD_SKIP keeps its shadow; k counts steps, not rows.  NaN and Inf propagate as the arithmetic
 *      gives them.
 *      om_sgd_ema_step: every step is applied, so the caller knows k and passes omd (0 < omd <= 1).
 *      om_sgd_clip_ema_step: the single workgroup that takes the skip decision also keeps ema_state, OM_EMA_STATE_DOUBLES 8-byte
 *      words, caller-owned, zeroed (or set to a resumed count) by the caller before the first call: int64 at OM_EMA_UPDATES_OFF
 *      (EMA updates applied so far; never reset by the library) and float64 at OM_EMA_OMD_OFF (the float32 omd of the latest
 *      applied step).  When the step is not skipped it computes omd from the count, `decay` (inside (0, 1)) and `warmup`, then
 *      increments the count; a skipped step leaves the block, every shadow, parameter and buffer bit-unchanged.  The other
 *      arguments are om_sgd_clip_step's, and the clip state block is OM_CLIP_STATE_DOUBLES words as there.
 *      om_ema_swap exchanges parameter and shadow of every row with a shadow, element for element as 32-bit words (NaN payloads
 *      survive; twice is the identity), over the same chunk table; it reads `param` and `n` of a row and none of its flags.
 *      No atomics, no allocation, no host synchronisation in any of the three. */
#define OM_EMA_UPDATES_OFF 0
#define OM_EMA_OMD_OFF 1
#define OM_EMA_STATE_DOUBLES 2
int om_sgd_ema_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                    float* const* shadows, float omd, om_stream stream);
int om_sgd_clip_ema_step(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks,
                         int n_chunks, double* partials, double* state, long long* valid_since, float max_norm, int mode,
                         long long step, float* const* shadows, double* ema_state, double decay, int warmup, om_stream stream);
int om_ema_swap(const om_sgd_tensor* table_host, om_sgd_tensor* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                float* const* shadows, om_stream stream);

/* ---- The Adam family: torch.optim.Adam / AdamW (amsgrad=False) for every tensor of every parameter group, with the SGD step's
 *      chunk list, staging, clipping, skip decision and EMA; orienmask_amd/optim.py (HipAdam, HipAdamW) is the host side.  Per
 *      element, float32, every operation rounded once, sqrt and / IEEE-correct, denormals kept:
 *          g   = g * coef                                  (clipped form only; ahead of everything else; memory is not modified)
 *          g   = -g                                        (OM_ADAM_MAXIMIZE)
 *          p   = p * dm                                    (OM_ADAM_HAS_WD and OM_ADAM_DECOUPLED: AdamW)
 *          g   = fma(p, weight_decay, g)                   (OM_ADAM_HAS_WD alone: Adam)
 *          d   = g - m
 *          m'  = |w| < 0.5 ? fma(w, d, m) : fma(w - 1, d, g)          (lerp; w - 1 in float32)
 *          v'  = fma(omb2 * g, g, v * beta2)                          (both products rounded)
 *          den = sqrt(v') / bc2s + eps
 *          p'  = p + (nss * m') / den                                 (three roundings, no fma)
 *      and, with shadows, the EMA of om_sgd_ema_step on p'.
 *      table / table_host: n_tensors rows of 96 bytes (csrc/optim.hip: struct om_adam_tensor; optim.ADAM_ROW in Python), staged as
 *      om_sgd_step stages its rows:
 *          float* param; const float* grad; float* exp_avg; float* exp_avg_sq;   dense, n floats each, one storage order
 *          int64_t n;
 *          double lr;                the group's lr (read for OM_ADAM_DEVICE_COUNTED rows only)
 *          float w, beta2, omb2, eps;                 float32(1 - beta1), float32(beta2), float32(1 - beta2), float32(eps)
 *          float weight_decay, dm, nss, bc2s;         float32(wd), float32(1 - lr * wd), float32(-(lr / bc1)), float32(bc2s), with
 *                                    bc1 = 1 - beta1**step and bc2s = (1 - beta2**step) ** 0.5 in the host's doubles
 *          int32_t bias_table;       which bias table the row's betas use (OM_ADAM_DEVICE_COUNTED)
 *          uint32_t flags;           OM_ADAM_*
 *          uint32_t reserved[2];
 *      chunks: om_sgd_step's work list.  16-byte accesses where all four (with shadows, five) streams are 16-byte aligned, 4-byte
 *      accesses otherwise; every element is written exactly once; no atomics, no allocation, no host synchronisation.
 *      om_adam_step: ONE launch.  shadows may be null (no EMA; omd is then not read); otherwise omd as in om_sgd_ema_step.  A row
 *      flagged OM_ADAM_DEVICE_COUNTED is refused.
 *      om_adam_clip_step: THREE launches as om_sgd_clip_step (partials, state, max_norm, mode, step as there; shadows may be null,
 *      otherwise ema_state, decay and warmup as in om_sgd_clip_ema_step).  counts: n_tensors int64, caller-owned, the number of
 *      steps APPLIED to each tensor.  The single workgroup that takes the skip decision adds 1 to the count of every row flagged
 *      OM_ADAM_DEVICE_COUNTED and not OM_ADAM_SKIP when the step is not skipped; a skipped step leaves parameters, both moments,
 *      every count, every shadow and the EMA block bit-unchanged.  The update of such a row takes its step number k from counts
 *      and its corrections from the bias tables: bias holds (bc1, bc2s) pairs of doubles, table after table; bias_dir holds, per
 *      table, int64 (first pair, pairs); pair k of a table is step k's, and for k at or beyond the table's length both are 1.0.
 *      Then nss = float32(-(lr / bc1)) with one IEEE double division and bc2s = float32(bc2s).  Rows without the flag use the
 *      row's own nss and bc2s and leave their count alone.
 *      om_adam_ema_swap: om_ema_swap over om_adam_tensor rows. */
#define OM_ADAM_SKIP 1
#define OM_ADAM_MAXIMIZE 2
#define OM_ADAM_HAS_WD 4
#define OM_ADAM_DECOUPLED 8
#define OM_ADAM_DEVICE_COUNTED 16
#define OM_ADAM_ROW_BYTES 96
int om_adam_step(const void* table_host, void* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                 float* const* shadows, float omd, om_stream stream);
int om_adam_clip_step(const void* table_host, void* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks, double* partials,
                      double* state, long long* counts, const double* bias, const long long* bias_dir, int n_bias_tables,
                      float max_norm, int mode, long long step, float* const* shadows, double* ema_state, double decay, int warmup,
                      om_stream stream);
int om_adam_ema_swap(const void* table_host, void* table, int n_tensors, const om_sgd_chunk* chunks, int n_chunks,
                     float* const* shadows, om_stream stream);

/* ---- The Conv -> BatchNorm2d -> LeakyReLU(0.1) block of the reference without its convolution (model/base.py:104-137,278-279: the
 *      nn.BatchNorm2d and nn.LeakyReLU of ConvBNRelu.conv_block), optionally with the residual add that closes a DarkNet block
 *      (model/backbone/darknet.py:14-15 `x + self.conv(x)`), for the training forward of trainer/trainer.py:47 and its backward (:52).
 *      x, y, residual, dy, dx: fp32 NCHW contiguous [B,C,H,W]; gamma, beta and the running buffers: C floats; save_mean and
 *      save_invstd: 2C floats each, [0,C) the float32 value (what torch reports) and [C,2C) the float32 remainder of the double the
 *      kernels computed with, so that the backward rebuilds z with the forward's bits.  Every element-wise intermediate is a double;
 *      each output is rounded to float32 once.
 *      Forward, training != 0: per-channel batch mean and biased variance (every element accumulated in double around the channel's
 *      first element, never E[x^2] - E[x]^2), save_mean / save_invstd = 1 / sqrt(var + eps) written, running_mean and running_var
 *      (unbiased variance) updated with `momentum` and *num_batches_tracked incremented on the device as torch.nn.BatchNorm2d does
 *      (each of the three may be null); needs B*H*W >= 2.  training == 0: the running statistics normalise, no buffer changes,
 *      save_mean / save_invstd receive what was used.  Then z = fma(x - mean, gamma * invstd, beta), y = z > 0 ? z : z * slope,
 *      plus residual[i] when residual is not null.
 *      Backward: z is recomputed from x with the same expression; dz = dy * (z > 0 ? 1 : slope); dbeta = sum dz; dgamma = sum dz * xhat;
 *      dx = gamma * invstd * (dz - dbeta / M - xhat * dgamma / M) with M = B*H*W (training) or gamma * invstd * dz (eval); dx may be
 *      null (the input needs no gradient): only the sums are computed.  The residual's gradient is dy itself.
 *      One launch where a channel has at most 16384 elements, else two (per-workgroup partial sums in `workspace`, summed in a fixed
 *      order by the second): no atomics, bit-identical from run to run, no allocation, no host synchronisation.  workspace: the
 *      number of bytes the size query returns for the shape (0 for a shape that is refused), 16-byte aligned, undefined on entry. */
size_t om_bn_act_workspace_bytes(int B, int C, int H, int W);
int om_bn_act_forward(const float* x, int B, int C, int H, int W, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, int training, double momentum, double eps, float slope,
                      const float* residual, float* y, float* save_mean, float* save_invstd, void* workspace, size_t ws_bytes,
                      om_stream stream);
int om_bn_act_backward(const float* x, const float* dy, int B, int C, int H, int W, const float* gamma, const float* beta,
                       const float* save_mean, const float* save_invstd, int training, float slope, float* dx, float* dgamma,
                       float* dbeta, void* workspace, size_t ws_bytes, om_stream stream);

/* ---- The same block with batch statistics over R ranks (torch.nn.SyncBatchNorm; trainer/builder.py:85-87), as four staged calls
 *      with the caller's collectives between them.  Tensors, save vectors, arithmetic and workspace as above; R >= 1.
 *      om_bn_sync_stats: this rank's per-channel RECORD, doubles [3][C]: n = B*H*W, mean = K + s1/n, M2 = s2 - s1*(s1/n) clamped at
 *      0, with K the channel's first element and s1, s2 the sums of (x-K), (x-K)^2 in the unsynchronised kernel's order; B*H*W >= 1.
 *      om_bn_sync_forward: `records` is [R][3][C], the all-gather of every rank's record.  Per channel the records are merged in rank
 *      order, starting from record 0: delta = mean_r - mean, M2 += M2_r + delta*delta*n*n_r/(n+n_r), mean += delta*n_r/(n+n_r),
 *      n += n_r.  Then var = M2/N, invstd = 1/sqrt(var+eps), the running buffers take mean and var*N/(N-1), the counter is
 *      incremented, the save vectors are written, *n_total_out (device) = N, y as above.  Every rank merges the same bytes in the same
 *      order: save vectors and running buffers are bit-identical across ranks.  Every rank holds at least one value per channel, so
 *      N >= B*H*W + R - 1; a call for which that is below 2 is refused.
 *      om_bn_sync_backward_sums: this rank's doubles [2][C] = (sum dz, sum dz * xhat), and its own float32 dgamma / dbeta (they stay
 *      local, as in torch's SyncBatchNorm: DistributedDataParallel averages them).
 *      om_bn_sync_backward_dx: `sums_all` is [R][2][C], summed in rank order; n_total the device double of the forward;
 *      dx = gamma * invstd * (dz - Sdz/N - xhat * Sdzxhat/N).
 *      With R == 1, records = this rank's record and sums_all = its sums, every output has the bits of om_bn_act_forward /
 *      om_bn_act_backward.  Three passes over the activation forward, five backward; no atomics, no host synchronisation. */
int om_bn_sync_stats(const float* x, int B, int C, int H, int W, double* record, void* workspace, size_t ws_bytes, om_stream stream);
int om_bn_sync_forward(const float* x, int B, int C, int H, int W, const double* records, int R, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked, double momentum, double eps, float slope,
                       const float* residual, float* y, float* save_mean, float* save_invstd, double* n_total_out, om_stream stream);
int om_bn_sync_backward_sums(const float* x, const float* dy, int B, int C, int H, int W, const float* gamma, const float* beta,
                             const float* save_mean, const float* save_invstd, float slope, double* sums, float* dgamma, float* dbeta,
                             void* workspace, size_t ws_bytes, om_stream stream);
int om_bn_sync_backward_dx(const float* x, const float* dy, int B, int C, int H, int W, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_invstd, float slope, const double* sums_all, int R,
                           const double* n_total, float* dx, om_stream stream);

/* ---- The gradients of the training model's convolutions (trainer/trainer.py:52 `loss.backward()` through every nn.Conv2d of
 *      model/base.py:104-137 and the four plain head convolutions), for the three geometries the two models contain: ksize 1 stride 1,
 *      ksize 3 stride 1, ksize 3 stride 2, padding ksize / 2, no dilation, no groups; anything else returns OM_EINVAL.  All tensors
 *      fp32 NCHW contiguous: x, dx [B,cin,H,W]; dy [B,cout,Ho,Wo] with Ho = (H + 2*(ksize/2) - ksize) / stride + 1; w, dw
 *      [cout,cin,ksize,ksize]; dbias [cout].  H and W are the INPUT's.  Any B, cin, cout, H, W >= 1 (B <= 16383, B*H*W < 2^30);
 *      no alignment is required.
 *      om_conv2d_grad_input:  dx = sum over co and the taps that reach the pixel of dy * w; at stride 2 the four parity classes of
 *      input pixels are separate tile families with 1, 2, 2 and 4 taps.  An accumulation chain of the matrix instruction holds at
 *      most 32 products; the chains of an element are summed in double and rounded once.  Needs no workspace (the arguments are
 *      accepted and ignored).
 *      om_conv2d_grad_weight: dw = sum over b and the output pixels of dy * x, the pixels split over workgroups, at most 2048 each: a
 *      chain of the matrix instruction holds 32 products, a workgroup sums its chains in fp32 (at most 64), and with more than one
 *      split the partial tiles go to `workspace` and a second kernel sums them in split order in double.  dbias (may be null) = sum
 *      of dy over b and the plane, in double; dw may be null when dbias is not.  The number of splits is a function of the shape
 *      and of the device's compute-unit count.  workspace: om_conv2d_grad_workspace_bytes for the shape on the current device (0
 *      where one split suffices or the geometry is refused), undefined on entry; too small: OM_ENOMEM.
 *      Fp32 operands on the f32 matrix instruction, fp32 accumulation.  Everything is enqueued on `stream`; no allocation, no host
 *      synchronisation, no atomics, bit-identical from run to run.  A null dy / w / x / dx, or dw and dbias both null, returns OM_EINVAL. */
size_t om_conv2d_grad_workspace_bytes(int B, int cin, int H, int W, int cout, int ksize, int stride);
int om_conv2d_grad_input(const float* dy, const float* w, int B, int cin, int H, int W, int cout, int ksize, int stride, float* dx,
                         void* workspace, size_t ws_bytes, om_stream stream);
int om_conv2d_grad_weight(const float* x, const float* dy, int B, int cin, int H, int W, int cout, int ksize, int stride, float* dw,
                          float* dbias, void* workspace, size_t ws_bytes, om_stream stream);

/* ---- The forward of the same convolutions (orienmask_amd.train.conv2d with forward='hip'; the models with conv_forward='hip'):
 *      y[b,co,oy,ox] = bias[co] + sum over ci and the taps of x[b,ci,oy*stride+kh-pad,ox*stride+kw-pad] * w[co,ci,kh,kw], for the
 *      geometries, layouts and size limits of the gradients above; y [B,cout,Ho,Wo], bias [cout] or null.  H and W are the INPUT's.
 *      One kernel (csrc/conv_fwd.hip): 128 consecutive output pixels of the flat (b, oy, ox) index by 64 (or 32) output channels
 *      per workgroup, the whole k = cin * ksize^2 in that workgroup: no split, no workspace.  An accumulation chain of the matrix
 *      instruction holds at most 32 products (8 input channels x the 3 column taps of one row tap; 32 input channels at 1x1); the
 *      chains of an element are summed in double in ci order, row taps in kh order, the bias is added as a double and the sum is
 *      rounded once.  That order is a function of the geometry only -- not of the pixel's place in a tile, the image index, B or
 *      the device -- so an image's y has the same bits alone and in any batch.
 *      Fp32 operands on the f32 matrix instruction.  Everything is enqueued on `stream`; no allocation, no host synchronisation,
 *      no atomics, bit-identical from run to run.  A null x / w / y, another geometry or sizes outside the limits return OM_EINVAL
 *      and nothing is written. */
int om_conv2d_forward(const float* x, const float* w, const float* bias, int B, int cin, int H, int W, int cout, int ksize, int stride,
                      float* y, om_stream stream);

/* ---- A FROZEN Conv -> BatchNorm -> LeakyReLU (+ residual) block in one kernel (orienmask_amd.train.conv_bn_leaky_frozen; the
 *      models' frozen_stages with conv_forward='hip'): the bias-free convolution above with another epilogue, so the convolution
 *      output never reaches memory and nothing is saved for a backward.  x, w, the geometries, layouts and size limits are
 *      om_conv2d_forward's; gamma, beta, running_mean, running_var [cout]; residual [B,cout,Ho,Wo] or null; y [B,cout,Ho,Wo].
 *      Per output element, with h the element's double sum (om_conv2d_forward's chains in its order):
 *          z = fma(h - mean, gamma * invstd, beta),   y = (float)((z > 0 ? z : z * slope) + residual)
 *      in double, rounded once; without a residual nothing is added.  mean = (double)running_mean and invstd = 1/sqrt((double)
 *      running_var + eps), carried through a float32 (value, remainder) pair, are the doubles om_bn_act_forward(training=0) builds
 *      (one definition, csrc/bn_channel.h): where every convolution sum is an exact float32, y has the bits of that call on
 *      om_conv2d_forward's output.  The statistics are read only; eps > 0.
 *      The channel records are built once per workgroup.  Enqueued on `stream`; no workspace, no allocation, no host synchronisation,
 *      no atomics, bit-identical from run to run, and an image's y has the same bits alone and in any batch.  A null x / w / y /
 *      gamma / beta / running_mean / running_var, y aliasing x, w or the residual, another geometry, sizes outside the limits or
 *      eps <= 0 return OM_EINVAL and nothing is written. */
int om_conv2d_frozen_forward(const float* x, const float* w, int B, int cin, int H, int W, int cout, int ksize, int stride,
                             const float* gamma, const float* beta, const float* running_mean, const float* running_var, double eps,
                             float slope, const float* residual, float* y, om_stream stream);

/* ---- The same forward on bf16 activations (orienmask_amd.train.conv2d_bf16; the models with amp='bf16', conv_forward='hip'):
 *      x [B,cin,H,W] bf16 (uint16_t bits), w [cout,cin,ksize,ksize] the FLOAT32 master weight, bias [cout] float32 or null; the
 *      geometries, layouts and size limits of om_conv2d_forward.  y [B,cout,Ho,Wo]: float32 where y_is_f32 != 0, bf16 otherwise.
 *      One kernel (csrc/conv_fwd_bf16.hip) with om_conv2d_forward's tiles (128 consecutive output pixels of the flat (b, oy, ox)
 *      index by 64 or 32 output channels, the whole k in one workgroup: no split, no workspace) on v_mfma_f32_32x32x16_bf16.
 *      Arithmetic: x is widened exactly; every weight is rounded to bf16 (nearest, ties to even: csrc/bf16.h, torch's
 *      .to(torch.bfloat16)) while it is staged -- no cast kernel, no bf16 copy.  Every product is exact in float32; an element's sum
 *      has TWO float32 levels: a chain in the matrix instruction's accumulators, 16 input channels of one tap per step, holds one
 *      block of input channels (16 at 3x3, in the order kh > kw: 144 products; 64 at 1x1), and the blocks' sums are added in block
 *      order into a second float32 accumulator (one add per block; one block: the chain itself); channels beyond cin as zeros.
 *      (One chain over the whole k was up to 4.6 x further from float64 than torch-CPU's float32 on in-network operands.)  That
 *      order is a function of the geometry only -- not of the tile, the image index, B or the co tile width -- so an image's y has
 *      the same bits alone, in any batch and on every run.  y32 = sum + bias (one float32 add; none without a bias); the float32 output is y32, the bf16 output
 *      its rounding to nearest even: bf16 y == rne(float32 y) bit for bit.
 *      No alignment beyond the element's own is required (a bf16 tensor may start at any uint16_t).  Enqueued on `stream`; no
 *      allocation, no host synchronisation, no atomics.  A null x / w / y, another geometry or sizes outside the limits return
 *      OM_EINVAL and nothing is written. */
int om_conv2d_bf16_forward(const uint16_t* x, const float* w, const float* bias, int B, int cin, int H, int W, int cout, int ksize,
                           int stride, void* y, int y_is_f32, om_stream stream);

/* ---- The FROZEN block on bf16 activations (orienmask_amd.train.conv_bn_leaky_frozen on a bf16 x; the models' frozen_stages with
 *      amp='bf16', conv_forward='hip'): om_conv2d_bf16_forward without a bias, with om_conv2d_frozen_forward's epilogue on its
 *      float32 sum h:  y = rne_bf16((float)((z > 0 ? z : z * slope) + residual)),  z = fma((double)h - mean, gamma * invstd, beta),
 *      the same per-channel doubles (csrc/bn_channel.h).  x, residual and y bf16; w and the statistics float32.  So y equals, bit
 *      for bit, om_conv2d_bf16_forward(y_is_f32 = 1), then om_bn_act_forward(training=0) on that tensor with the residual widened,
 *      then the rounding to bf16.  Refusals as om_conv2d_frozen_forward's (null pointers, y aliasing x, w or the residual, the
 *      geometry, eps <= 0): OM_EINVAL and nothing is written. */
int om_conv2d_bf16_frozen_forward(const uint16_t* x, const float* w, int B, int cin, int H, int W, int cout, int ksize, int stride,
                                  const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                  double eps, float slope, const uint16_t* residual, uint16_t* y, om_stream stream);

/* ---- The gradients of om_conv2d_bf16_forward (orienmask_amd.train.conv2d_bf16 with backward='hip'; the models with amp='bf16',
 *      conv_forward='hip', conv_grad='hip'; csrc/conv_grad_bf16.hip, csrc/conv_dw.hip): dy [B,cout,Ho,Wo] and x [B,cin,H,W] bf16 (uint16_t bits), w
 *      [cout,cin,ksize,ksize] the FLOAT32 master weight; dx [B,cin,H,W] float32 where dx_is_f32 != 0, bf16 otherwise; dw
 *      [cout,cin,ksize,ksize] and dbias [cout] float32.  The geometries, layouts and size limits of om_conv2d_grad_*; H and W are
 *      the INPUT's.  On v_mfma_f32_32x32x16_bf16.
 *      Arithmetic: dy and x are widened exactly; every weight is rounded to bf16 (nearest, ties to even: csrc/bf16.h) while it is
 *      staged, which is what the forward multiplied by -- no cast kernel, no bf16 copy.  Every product is exact in float32; all
 *      accumulation is float32 or wider.
 *      om_conv2d_bf16_grad_input: an element's sum has two float32 levels, as the forward's: a chain in the matrix instruction's
 *      accumulators over a block of output channels (stride 1: 16 at 3x3, 64 at 1x1; stride 2: 64) and the taps that reach the
 *      pixel, and the blocks' sums added in block order into a second float32 accumulator; an order that is a function of the
 *      geometry only -- not of B, the tile or the device -- so an image's dx
 *      has the same bits alone and in any batch; the bf16 output is the rounding of the float32 one, bit for bit.  Stride 1 is the
 *      forward kernel on dy with the weight read transposed and flipped; stride 2 takes the four parity classes of the input pixel
 *      (1, 2, 2 and 4 taps, no product with an absent tap) and writes every element of dx.  Needs no workspace (the arguments are
 *      accepted and ignored).  dx aliasing dy or w returns OM_EINVAL.
 *      om_conv2d_bf16_grad_weight: dw = sum over b and the output pixels of dy * x, the pixels split over workgroups by
 *      om_conv2d_grad_weight's rule (at most 2048 each; a function of the shape and the device's compute-unit count): a chain of
 *      the matrix instruction holds 32 pixels, a workgroup sums its chains in float32 (at most 64), and with more than one split the
 *      partial tiles go to `workspace` and a second kernel sums them in split order in double.  dbias = the sum of dy over b and the
 *      plane in double, rounded once.  dw or dbias may be null (not computed); both null returns OM_EINVAL.  workspace:
 *      om_conv2d_bf16_grad_workspace_bytes for the shape on the current device (0 where one split suffices or the geometry is
 *      refused), undefined on entry; too small: OM_ENOMEM.
 *      No alignment beyond the element's own is required.  Everything is enqueued on `stream`; no allocation, no host
 *      synchronisation, no atomics, bit-identical from run to run.  A null dy / w / x / dx, another geometry or sizes outside the
 *      limits return OM_EINVAL and nothing is written. */
size_t om_conv2d_bf16_grad_workspace_bytes(int B, int cin, int H, int W, int cout, int ksize, int stride);
int om_conv2d_bf16_grad_input(const uint16_t* dy, const float* w, int B, int cin, int H, int W, int cout, int ksize, int stride,
                              void* dx, int dx_is_f32, void* workspace, size_t ws_bytes, om_stream stream);
int om_conv2d_bf16_grad_weight(const uint16_t* x, const uint16_t* dy, int B, int cin, int H, int W, int cout, int ksize, int stride,
                               float* dw, float* dbias, void* workspace, size_t ws_bytes, om_stream stream);

/* ---- The training models' plumbing between the convolutions (model/orienmask_yolo_fpnplus.py:74-90, model/orienmask_yolo.py:71-86:
 *      F.interpolate(mode='nearest'), torch.cat and torch.split, with autograd's backward of the three; orienmask_amd.train's
 *      upsample_concat / split_channels, the models with route_backend='hip').  All tensors fp32 NCHW contiguous: y, dy
 *      [B, sum(chans), H, W]; source i [B, chans[i], H / scales[i], W / scales[i]], at the channels that start at chans[0] + ... +
 *      chans[i-1].  1 <= n <= 4 (the arrays' first n entries are read); every scale one of 1, 2, 4, 8 and a divisor of H and W; B
 *      and every chans[i] >= 1; B * sum(chans) * H * W < 2^31.  No alignment is required: a tensor may start at any float.
 *      om_route_concat_forward:  y[b, off_i + c, oy, ox] = src[i][b, c, oy / scales[i], ox / scales[i]] -- torch.cat of the
 *      nearest-up-sampled sources, copies only, so bit-identical to it.  A null src[i] stands for zeros.
 *      om_route_concat_backward: dsrc[i][b, c, sy, sx] = the scales[i] x scales[i] block of dy, summed sequentially in fp32: the
 *      accumulator starts as the block's first element, rows top to bottom, left to right within a row (torch-CPU's
 *      upsample_nearest2d backward order); at scale 1 a copy.  A null dsrc[i] needs no gradient: nothing is written for it.  With
 *      every scale 1 this is torch.split(dy, chans, 1) into dense tensors, and the forward is the split's backward.
 *      One kernel per call (csrc/route.hip), a flat grid-stride loop; each element of dy is read once, each element of y and dsrc
 *      written once.  Two forms, chosen by the entry point from the arguments: 16-byte accesses along W where W % 4 == 0 and y / dy
 *      and every non-null src / dsrc start on a 16-byte boundary, one element per lane otherwise; the values are the same.
 *      Enqueued on `stream`; no allocation, no host synchronisation, no atomics, no workspace, bit-identical from run to run, and
 *      an image's values do not depend on its place in the batch.  A null y / dy, every dsrc null, or arguments outside the
 *      limits return OM_EINVAL: nothing is launched and nothing is written. */
int om_route_concat_forward(const float* const src[4], const int chans[4], const int scales[4], int n, int B, int H, int W, float* y,
                            om_stream stream);
int om_route_concat_backward(const float* dy, const int chans[4], const int scales[4], int n, int B, int H, int W, float* const dsrc[4],
                             om_stream stream);

/* ---- bf16 activations (orienmask_amd.train's models with amp='bf16').  The _bf16 form of each entry point above takes the same
 *      arguments and returns the same codes; only the ACTIVATION tensors change type: x, residual, y, dy, dx, the route sources, the
 *      route output and their gradients are bf16 (uint16_t bits) NCHW contiguous.  gamma, beta, the running buffers, save_mean /
 *      save_invstd, dgamma / dbeta stay float32, workspace partials and SyncBatchNorm records stay doubles, in the layouts above; the
 *      workspace size is om_bn_act_workspace_bytes'.
 *      Arithmetic: a bf16 input is widened exactly, every intermediate is the fp32 entry point's expression on the same doubles in
 *      the same order, and a bf16 output is the float32 that entry point would have stored, rounded to bf16 to nearest even.  So
 *      f_bf16(X) == rne_bf16(f(float(X))) bit for bit, and the float32 and double outputs (save vectors, running buffers, dgamma,
 *      dbeta, records, sums) have f(float(X))'s bits.  om_route_concat_forward_bf16 is a copy; om_route_concat_backward_bf16 sums a
 *      block in float32 in the order above and rounds once.
 *      The 4-element unit of the fp32 kernels is kept (8 bytes of bf16: where H*W, or W for the routes, is a multiple of 4 and the
 *      tensors are 8-byte aligned; one element per lane otherwise), because the unit fixes the order of the per-channel sums. */
int om_bn_act_forward_bf16(const uint16_t* x, int B, int C, int H, int W, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, int64_t* num_batches_tracked, int training, double momentum, double eps, float slope,
                           const uint16_t* residual, uint16_t* y, float* save_mean, float* save_invstd, void* workspace,
                           size_t ws_bytes, om_stream stream);
int om_bn_act_backward_bf16(const uint16_t* x, const uint16_t* dy, int B, int C, int H, int W, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, int training, float slope, uint16_t* dx, float* dgamma,
                            float* dbeta, void* workspace, size_t ws_bytes, om_stream stream);
int om_bn_sync_stats_bf16(const uint16_t* x, int B, int C, int H, int W, double* record, void* workspace, size_t ws_bytes,
                          om_stream stream);
int om_bn_sync_forward_bf16(const uint16_t* x, int B, int C, int H, int W, const double* records, int R, const float* gamma,
                            const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked, double momentum,
                            double eps, float slope, const uint16_t* residual, uint16_t* y, float* save_mean, float* save_invstd,
                            double* n_total_out, om_stream stream);
int om_bn_sync_backward_sums_bf16(const uint16_t* x, const uint16_t* dy, int B, int C, int H, int W, const float* gamma,
                                  const float* beta, const float* save_mean, const float* save_invstd, float slope, double* sums,
                                  float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, om_stream stream);
int om_bn_sync_backward_dx_bf16(const uint16_t* x, const uint16_t* dy, int B, int C, int H, int W, const float* gamma,
                                const float* beta, const float* save_mean, const float* save_invstd, float slope,
                                const double* sums_all, int R, const double* n_total, uint16_t* dx, om_stream stream);
int om_route_concat_forward_bf16(const uint16_t* const src[4], const int chans[4], const int scales[4], int n, int B, int H, int W,
                                 uint16_t* y, om_stream stream);
int om_route_concat_backward_bf16(const uint16_t* dy, const int chans[4], const int scales[4], int n, int B, int H, int W,
                                  uint16_t* const dsrc[4], om_stream stream);

/* ---- Several batches in flight.  Every entry point only enqueues kernels on the caller's stream and keeps no per-call state in
 *      the model handle (profiling apart): om_forward / om_forward_f16 / om_postprocess may be issued for different batches
 *      on different HIP streams at the same time, provided each batch in flight has its OWN workspace (and output buffers);
 *      the weights are only read.  Kernels of the streams then share compute units, and results do not depend on what the
 *      other stream runs (tests/test_hip_parity.py::test_postprocess_and_forward_are_stable_beside_other_streams).  The host
 *      side of this is orienmask_amd/pipeline.py (InFlightPipeline): +13 % fp32 / +19 % fp16 images/s at 32 x 544 x 544. */

#ifdef __cplusplus
}
#endif
#endif /* ORIENMASK_HIP_H */
