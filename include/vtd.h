/*
 * vtd.h -- C ABI of libvtd_hip.so, the MI355X (gfx950) implementation of the per-frame
 * text-detection / recognition hot path of malak29/video-text-detection-system.
 *
 * The reference has no FFI for this path: its boundary is the Python class API of app/ml
 * (TextDetector / TextRecognizer / VideoTextPipeline).  The entry points below are what a binding
 * for those classes needs; each cites the reference interface it replaces (file:line relative to the
 * reference repository).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain C, opaque handles, caller-owned device buffers, no torch / C++ types in signatures
 *   - every call returns 0 on success, a negative value on failure: -(hipError_t) for HIP errors,
 *     -1000 and below for argument / shape validation errors; vtd_strerror() names them
 *   - every launching call takes the HIP stream to enqueue on (pass NULL for the default stream);
 *     nothing synchronises the device unless documented
 *   - no process-global state: N handles (one per GPU / per worker thread) coexist; a handle must be
 *     used from one stream at a time
 *   - "dev" pointers are device memory on the handle's device; "host" pointers are host memory
 */
#ifndef VTD_H
#define VTD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtd_detector vtd_detector;
typedef struct vtd_recognizer vtd_recognizer;
typedef struct vtd_postproc vtd_postproc;
typedef void* vtd_stream; /* hipStream_t */

/* One detection, as TextDetector._post_process emits it (app/ml/models/text_detector.py:172-176):
 * bbox in frame pixels, polygon (4 x (x,y)) in map space, confidence = mean probability. */
typedef struct vtd_detection {
    int32_t bbox[4];
    int32_t polygon[8];
    float confidence;
    float area;            /* contour area of the component (diagnostic) */
    int32_t first_x, first_y; /* raster-first pixel of the component (diagnostic / ordering) */
} vtd_detection;

/* ---- library ---------------------------------------------------------------------------------- */
const char* vtd_version(void);
const char* vtd_strerror(int code);
/* number of visible HIP devices, or a negative error */
int vtd_device_count(void);

/* ---- detector: DBNet (text_detector.py:12-86) -------------------------------------------------- */
/* backbone: "resnet18" | "resnet50" (text_detector.py:16-20; 'resnet18' is the documented repair A2).
 * max_batch frames of 640x640 network input are provisioned in HBM at creation. */
int vtd_detector_create(const char* backbone, int max_batch, vtd_detector** out);
void vtd_detector_destroy(vtd_detector* d);
/* Feed one tensor of the reference checkpoint's model_state_dict (text_detector.py:108-109) by its key,
 * e.g. "backbone.0.weight", "fpn.inner_blocks.2.bias", "head.probability_head.3.weight"; float32,
 * PyTorch memory order.  Unknown keys are rejected, "num_batches_tracked" keys are accepted and ignored. */
int vtd_detector_set_tensor(vtd_detector* d, const char* key, const float* host_data, int64_t numel);
/* Build options, before finalize.  "fuse_fpn_head" (default 1): evaluate FPN lateral(C2) + top-down add + P2 smooth +
 * head conv as one algebraically composed convolution (the 256-channel P2 map is never formed; its "p2" tap is then
 * unavailable).  0 keeps the layer-by-layer graph.
 * "fuse_stem_pool" (default 1): backbone conv1 7x7/s2 + bn1 + relu + maxpool 3x3/s2 run as one kernel that only writes the
 * pooled map (tap "pool"); 0 runs the generic convolution + a separate pool kernel and exposes the tap "stem".
 * "fuse_downsample" (default 1): the 1x1 projection + BatchNorm on the residual branch of a ResNet downsample block
 * (text_detector.py:16-19 -> torchvision BasicBlock / Bottleneck `downsample`) is evaluated inside the block's last
 * convolution as extra K-steps over the block input (the projected map is never written); 0 runs it as its own launch. */
int vtd_detector_set_option(vtd_detector* d, const char* name, int value);
/* Folds BatchNorm, repacks to the kernels' fp16 layouts and uploads.  Fails (-1103) if a key is missing. */
int vtd_detector_finalize(vtd_detector* d, vtd_stream stream);
/* K1 = cvtColor(BGR2RGB) + ToPILImage + Resize((640,640)) + ToTensor + Normalize (text_detector.py:99-104,
 * 119-124) for n frames of identical size: frames_dev is [n,H,W,3] uint8 BGR.  Fills the network input. */
int vtd_detector_preprocess(vtd_detector* d, const uint8_t* frames_dev, int n, int height, int width, vtd_stream stream);
/* Alternative input: the tensor the reference hands to DBNet.forward, [n,3,640,640] float32 (text_detector.py:124). */
int vtd_detector_set_input_nchw(vtd_detector* d, const float* x_dev, int n, vtd_stream stream);
/* DBNet.forward (text_detector.py:25-29) on the current input: prob_dev receives [n,640,640] float32
 * probabilities (the 'probability' map); thresh_dev, if not NULL, the 'threshold' map. */
int vtd_detector_forward(vtd_detector* d, int n, float* prob_dev, float* thresh_dev, vtd_stream stream);
/* Debug / test taps: copies an internal activation as dense NCHW float32 to host.  name: "input", "c2".."c5",
 * "p2", "stem", "head1", "head2".  Synchronises the stream. */
int vtd_detector_read_tap(vtd_detector* d, const char* name, int n, float* host_out, int64_t capacity, vtd_stream stream);
/* Algorithmic live work of one frame through this detector, in MACs (for roofline accounting). */
int64_t vtd_detector_macs_per_frame(const vtd_detector* d);
/* Per-launch HIP-event timing on the launch stream (bench.py's roofline leg).  set_profiling(1) resets the
 * accumulators; while enabled every vtd_detector_forward brackets each of its launches with events (enable = 2 + k:
 * only launch slot k, two events per forward, so the timed region is not perturbed).
 * get_profile resolves pending events (synchronises the stream) and returns, for launch slot op_index in
 * [0, vtd_detector_num_ops), a description, the accumulated milliseconds, launch count and algorithmic MACs. */
int vtd_detector_set_profiling(vtd_detector* d, int enable);
int vtd_detector_num_ops(const vtd_detector* d);
int vtd_detector_get_profile(vtd_detector* d, int op_index, char* name, int name_cap, double* total_ms, int64_t* calls,
                             double* total_macs, vtd_stream stream);

/* Kernel-selection table.  Which tile configuration / kernel variant runs a convolution is decided per launch slot and
 * power-of-two batch bucket: from the table when it holds a valid entry, else by a timing contest on first use (whose result
 * joins the table).  set_tuning merges a table (text lines "<signature>|n<bucket> <config id>", '#' comments) -- the one shipped
 * with the package, or rank 0's, so that every process and every rank selects the same kernels and produces bit-identical
 * maps; get_tuning serialises the current table into buf (NUL-terminated, truncated to capacity) and returns the size
 * needed; tuning_measured tells whether any entry came from this process's own contest.  The reference has no counterpart
 * (ATen picks its kernels internally). */
int vtd_detector_set_tuning(vtd_detector* d, const char* table_text);
int64_t vtd_detector_get_tuning(const vtd_detector* d, char* buf, int64_t capacity);
int vtd_detector_tuning_measured(const vtd_detector* d);

/* ---- post-process: TextDetector._post_process (text_detector.py:143-178) ------------------------ */
/* Workspace for maps of map_h x map_w (the reference hard-codes 640 in the bbox arithmetic but its tests feed
 * 160x160 maps: any 2-D size works) and up to max_batch maps per call; max_out detections kept per frame. */
int vtd_postproc_create(int max_batch, int map_h, int map_w, int max_out, vtd_postproc** out);
void vtd_postproc_destroy(vtd_postproc* pp);
/* prob_dev: [n,map_h,map_w] float32.  orig_w/orig_h: frame sizes (host arrays of n).  Strict `p > threshold`.
 * out_dev: [n,max_out] records in the order cv2.findContours(RETR_EXTERNAL) yields contours (reverse raster
 * discovery); counts_dev[i] = number of detections of frame i before truncation to max_out. */
int vtd_postproc_run(vtd_postproc* pp, const float* prob_dev, int n, const int32_t* orig_w_host, const int32_t* orig_h_host,
                     float threshold, vtd_detection* out_dev, int32_t* counts_dev, vtd_stream stream);
/* Copy `bytes` of device memory to PINNED host memory (hipHostMalloc / torch pin_memory; both pointers 16-byte aligned) with a kernel on
 * `stream` instead of hipMemcpyAsync -- a launch never makes the host wait for the GPU, which the asynchronous copy of the detection records
 * was seen to do once per drained pipeline.  Order the host behind it with an event on `stream`.  Fails (HIP error) for pageable memory. */
int vtd_copy_to_pinned_host(const void* src_dev, void* dst_pinned_host, int64_t bytes, vtd_stream stream);

/* ---- training loss, forward and backward (app/ml/training/trainer.py:48-56 training_step, :66-71 validation_step, :130-142 DiceLoss) --
 * total = nn.BCELoss()(probability, probability_map) + nn.BCELoss()(threshold, threshold_map) + DiceLoss()(probability,
 * probability_map) over `numel` float32 elements per map (any shape; 16-byte aligned device pointers), in ONE pass that reads every
 * element once.  out4_dev = {probability BCE, threshold BCE, dice loss, total} as float32 (the reference's scalar tensors);
 * sums5_dev (optional) = the five float64 sums behind them (BCE numerators, sum p*t, sum p, sum t).  thresh_dev / thresh_target_dev
 * may both be null (DiceLoss alone, or a detector run without its threshold branch): that term is then 0.  smooth = DiceLoss.smooth
 * (1e-5).  workspace_dev: vtd_dbloss_workspace_bytes() bytes, caller-owned, one per concurrent call.  fp64 accumulation in a fixed
 * order: bitwise repeatable.  The plateau scheduler (trainer.py:114-128) is torch's, as in the reference; the AdamW update
 * (trainer.py:107-112) is torch's by default and vtd_adamw_step below on request. */
int64_t vtd_dbloss_workspace_bytes(void);
int vtd_dbloss_forward(const float* prob_dev, const float* thresh_dev, const float* prob_target_dev, const float* thresh_target_dev, int64_t numel,
                       float smooth, void* workspace_dev, float* out4_dev, double* sums5_dev, vtd_stream stream);
/* Backward of the four scalars above (what torch autograd forms on trainer.py:52-56 with DiceLoss :135-142), one element-wise pass.
 * sums5_dev: the sums vtd_dbloss_forward returned for the same maps (nothing is recomputed); grad_out4_dev: the upstream gradients of
 * {probability BCE, threshold BCE, dice loss, total}, read on the device (no host wait).  With g_p = g[0] + g[3], g_th = g[1] + g[3],
 * g_d = g[2] + g[3], n = numel, den = P + T + smooth and num = 2 I + smooth formed in fp32 from the fp32-rounded sums as the forward forms them:
 *   grad_prob[i]   = ((g_p (p - t)) / max((1 - p) p, 1e-12)) / n  +  (t (2 (-g_d / den)) + g_d ((num / den) / den))
 *   grad_thresh[i] = ((g_th (th - th_t)) / max((1 - th) th, 1e-12)) / n
 * (aten binary_cross_entropy_backward with its 1e-12 clamp: p in {0, 1} against the other label gives +-1e12 g / n).  Either gradient
 * pointer may be null (that map is then neither read nor written); grad_thresh needs thresh_dev / thresh_target_dev.  Same 16-byte
 * alignment rule as the forward, for the gradients too.  Element-wise: bitwise repeatable.  Errors -2711 (argument), -2712 (alignment). */
int vtd_dbloss_backward(const float* prob_dev, const float* thresh_dev, const float* prob_target_dev, const float* thresh_target_dev, int64_t numel,
                        float smooth, const double* sums5_dev, const float* grad_out4_dev, float* grad_prob_dev, float* grad_thresh_dev,
                        vtd_stream stream);
/* ---- validation metrics (app/ml/training/trainer.py:83-103 on_validation_epoch_end: precision_recall_fscore_support(average='binary',
 * zero_division=0) of `probability > 0.5` against probability_map) -- the counts behind them, never the maps.  ADDS {TP, FP, FN, number of
 * targets not in {0, 1}} of `pred > threshold` (strict) into the caller-owned int64[4] counts4_dev (8-byte aligned; zero it once per epoch),
 * so a whole epoch runs without a host sync.  NaN predictions count as negative, NaN targets as "not in {0, 1}".  pred_dev / target_dev:
 * numel float32 each, 16-byte aligned.  Integer sums: the same counts on every run.  Errors -2721 (argument), -2722 (alignment). */
int vtd_binary_counts_accumulate(const float* pred_dev, const float* target_dev, int64_t numel, float threshold, int64_t* counts4_dev,
                                 vtd_stream stream);

/* ---- AdamW step (app/ml/training/trainer.py:107-112 configure_optimizers: torch.optim.AdamW(self.parameters(), lr, weight_decay)) -------
 * One multi-tensor pass: every tensor of the table is updated in place, 28 B of HBM traffic per element (p, g, m, v read; p, m, v written).
 * Per element, all float32, every operation rounded once (no fused multiply-add), in torch's order:
 *   p1  = p * decay
 *   m'  = m + one_minus_beta1 * (g - m)
 *   v'  = v * beta2 + (one_minus_beta2 * g) * g
 *   den = sqrt(v') / bc2_sqrt + eps
 *   p'  = p1 - step_size * (m' / den)
 * with IEEE division and square root and subnormals kept.  The caller forms the scalars in double and rounds each once to float, as torch
 * does with its Python scalars: decay = 1 - lr * weight_decay, step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step); step
 * is per tensor (torch keeps one per parameter; a parameter without a gradient does not advance and is simply left out of the table).
 * tensors: a HOST array of `count` entries whose p / g / m / v are device pointers to n float32 each (parameter, gradient, exp_avg,
 * exp_avg_sq).  The table travels in kernel arguments, VTD_ADAMW_SLICE tensors a launch (ceil(count / 64) launches: 2 for the 96 tensors
 * of the ResNet-18 detector): nothing is staged in device memory, nothing has to outlive the call, no host synchronisation, no
 * allocation, no atomics; a workgroup takes VTD_ADAMW_CHUNK elements of one tensor at a time and the grid depends on the n values only:
 * bitwise repeatable.  A tensor whose four pointers are all 16-byte aligned moves in 16-byte accesses (n % 4 elements singly); any
 * other 4-byte aligned tensor (a view that starts mid-row) takes dword accesses with the same results.  Entries with n == 0 are
 * skipped (their pointers are not looked at).
 * Errors, all before any launch: -3601 for count < 0, a null tensors / hyper pointer, n < 0 or n >= 2^40, a non-finite or non-positive
 * bc2_sqrt, a non-finite step_size or hyper-parameter, and, for entries with n > 0, a null pointer or one that is not 4-byte aligned.
 * count == 0 returns 0 and launches nothing. */
#define VTD_ADAMW_SLICE 64      /* tensors per launch */
#define VTD_ADAMW_CHUNK 4096    /* elements one workgroup takes at a time (a multiple of 1024) */
typedef struct vtd_adamw_tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    float step_size;
    float bc2_sqrt;
} vtd_adamw_tensor;   /* 48 bytes */
typedef struct vtd_adamw_hyper {
    float decay, one_minus_beta1, beta2, one_minus_beta2, eps;
} vtd_adamw_hyper;
int vtd_adamw_step(const vtd_adamw_tensor* tensors, int count, const vtd_adamw_hyper* hyper, vtd_stream stream);

/* ---- DB head training, forward and backward (text_detector.py:58-86 DBHead, both branches, BatchNorm in train or eval mode) ---------
 * Fine-tunes the probability and threshold heads over a frozen trunk and FPN, and forms the gradient of the head's input: the features are P2 (fpn.layer_blocks.3's output, 256
 * channels at H x W = 160 x 160 for 640^2 input) in the layout the kernels read, "padded features": ring-padded NHWC fp16
 * [n][H+2][W+2][256] whose one-pixel ring is zero.  M1 = n H W positions at the head input, M2 = 4 M1 at 2H x 2W.
 *
 * vtd_detector_forward_features: trunk + FPN of the current input (vtd_detector_set_input_nchw / _preprocess) up to P2, copied into the
 * caller-owned padded buffer feats_dev (16-byte aligned) -- a later forward on the handle never touches it, so autograd may keep it.
 * Needs a handle finalized with "fuse_fpn_head" = 0 (the composed head entry never forms P2): -2801 otherwise.
 * vtd_dbhead_pack_features: [n][256][H][W] NCHW float32 (dtype 0) or fp16 (dtype 1) -> padded features, ring included; any H, W >= 1.
 *
 * Parameters are torch's own tensors, passed as device pointers in PyTorch layouts, float32, contiguous, per branch (0 = probability_head,
 * 1 = threshold_head; the Sequential index of each is in brackets): conv_w [0] Conv2d [64][256][3][3], conv_b [64], bn1_w / bn1_b /
 * bn1_mean / bn1_var [1] [64], ct1_w [3] ConvTranspose2d [64 in][64 out][2][2], ct1_b [64], bn2_* [4] [64], ct2_w [6] [64][1][2][2],
 * ct2_b [1].  Both branches always run (the training loss reads both maps).
 *
 * vtd_dbhead_train_forward: DBHead.forward.  Weights are converted to the kernels' fp16 layouts on the device inside the call, so an
 * in-place optimizer step is seen by the next call.  training = 1: BatchNorm normalises with the batch statistics (biased variance) and
 * updates bn*_mean / bn*_var in place as torch does (x = (1 - momentum) x + momentum s, unbiased variance for the running value; the
 * statistics are combined as (count, mean, M2) partials in a fixed order, fp64); training = 0: the running statistics normalise and
 * nothing is written to them.  prob_dev / thresh_dev: [n][4H][4W] float32.  stats_dev (optional): [4][2][64] float32 = batch mean and
 * biased variance of BN1, then of BN2 (training = 1), or the running values used (training = 0).  workspace_dev: saved activations,
 * vtd_dbhead_train_workspace_bytes(n, H, W, 0) bytes, 256-byte aligned; keep it, the features and the two maps for the backward.
 * vtd_dbhead_train_backward: gradients of every learnable head parameter, both branches, written (not accumulated) as float32 into the
 * grads struct's pointers (running-statistic entries ignored), given grad_prob_dev / grad_thresh_dev ([n][4H][4W] float32; either may be
 * null = zero).  training must equal the forward's.  scratch_dev: vtd_dbhead_train_workspace_bytes(n, H, W, 1) bytes, or (n, H, W, 2) when
 * vtd_dbhead_train_backward_input follows.  This call forms no gradient for the features.  Backward GEMM operands are fp16 with an exact power-of-two scale per branch and tensor, chosen from a bound
 * on max |.| taken in the preceding reduction pass and undone in the fp32 epilogue.  No atomics, shape-only grids: bitwise repeatable.
 * vtd_dbhead_train_backward_input: the gradient of the features (dgrad into P2), dP2 = conv3x3^T(dy1) summed over both branches as one
 * implicit GEMM (K = 9 x 128, N = 256).  Call it after vtd_dbhead_train_backward on the same stream with the same n, H, W and the same
 * scratch_dev, which must then hold vtd_dbhead_train_workspace_bytes(n, H, W, 2) bytes (mode 2 = mode 1 plus this call's buffers; the
 * backward's results and bits do not depend on which of the two sizes it was given).  params: only the two conv_w are read.  dfeats_dev:
 * [n][H][W][256] float32 (NHWC, 16-byte aligned) = dP2 times dscale_dev[0]; dscale_dev: float32[2] (8-byte aligned) = {scale, 1 / scale},
 * an exact power of two: the smaller of the two branches' dy1 scales (the other branch's ratio is folded into its packed weights).
 * vtd_dbhead_unpack_input_grad: dfeats_dev / dscale_dev -> the gradient in torch's layout, [n][256][H][W] float32, scale undone.
 * Errors: -2801 (handle built with the fused head entry), -2802 (argument / shape), -2803 (alignment). */
typedef struct vtd_dbhead_branch {
    float *conv_w, *conv_b, *bn1_w, *bn1_b, *bn1_mean, *bn1_var, *ct1_w, *ct1_b, *bn2_w, *bn2_b, *bn2_mean, *bn2_var, *ct2_w, *ct2_b;
} vtd_dbhead_branch;
typedef struct vtd_dbhead_params {
    vtd_dbhead_branch branch[2];
} vtd_dbhead_params;
int vtd_detector_forward_features(vtd_detector* d, int n, void* feats_dev, vtd_stream stream);
int vtd_dbhead_pack_features(const void* x_dev, int dtype, int n, int height, int width, void* feats_dev, vtd_stream stream);
int64_t vtd_dbhead_train_workspace_bytes(int n, int height, int width, int backward);
int vtd_dbhead_train_forward(const void* feats_dev, int n, int height, int width, const vtd_dbhead_params* params, int training, float momentum,
                             float eps, void* workspace_dev, float* prob_dev, float* thresh_dev, float* stats_dev, vtd_stream stream);
int vtd_dbhead_train_backward(const void* feats_dev, int n, int height, int width, const vtd_dbhead_params* params, int training,
                              const void* workspace_dev, const float* prob_dev, const float* thresh_dev, const float* grad_prob_dev,
                              const float* grad_thresh_dev, const vtd_dbhead_params* grads, void* scratch_dev, vtd_stream stream);
int vtd_dbhead_train_backward_input(int n, int height, int width, const vtd_dbhead_params* params, void* scratch_dev, float* dfeats_dev,
                                    float* dscale_dev, vtd_stream stream);
int vtd_dbhead_unpack_input_grad(const float* dfeats_dev, const float* dscale_dev, int n, int height, int width, float* grad_nchw_dev,
                                 vtd_stream stream);

/* ---- FPN training, forward and backward (text_detector.py:31-56 FeaturePyramidNetwork in the wiring of SURVEY.md B.3), over a frozen trunk
 * L5 = inner_blocks[0](C5), L(k) = inner_blocks[5-k](C(k)) + nearest-2x(L(k+1)), P2 = layer_blocks[3](L2); layer_blocks[0..2] are dead and get no
 * gradient.  The geometry is given by the C5 size: C(5-k) is [n][c5_channels >> k][h5 << k][w5 << k]; c5_channels is a multiple of 512
 * (512 = ResNet-18, 2048 = ResNet-50) up to 4096.  Every other combination is refused.
 *
 * Taps are "padded taps": ring-padded NHWC fp16 [n][H+2][W+2][C] with a one-pixel ring (the detector engine's own layout), passed as an
 * array of four device pointers ordered C2, C3, C4, C5 (16-byte aligned).
 * vtd_detector_forward_trunk: the detector's ops up to the last residual stage of the current input, then a copy of the four taps into
 * caller-owned buffers.  Needs a handle finalized with "fuse_fpn_head" = 0 (the fused graph pads C2 differently): -2901 otherwise.
 * vtd_detector_forward_pool: the detector's ops up to the pooled stem output (what layer1 reads), then a copy of that padded tap,
 * [n][162][162][64] fp16 with a zero ring, into pool_dev (16-byte aligned).  Works on a handle of either "fuse_fpn_head" and either
 * "fuse_stem_pool" setting; -2901 if the tap's ring is not 1, -2903 for a misaligned buffer.
 * vtd_detector_forward_c2: the detector's ops up to the first residual stage's output (the stem and res2 / layer1; no later stage runs),
 * then a copy of that padded tap, C2 [n][162][162][c] fp16 (c = 64 for ResNet-18, 256 for ResNet-50), into c2_dev (16-byte aligned): the bits
 * vtd_detector_forward_trunk writes into its c2_dev.  vtd_detector_forward_trunk's conditions and codes: a handle finalized with
 * "fuse_fpn_head" = 0 and a C2 tap of ring 1, -2901 otherwise; -2903 for a misaligned buffer.
 * vtd_fpn_train_pack_tap: [n][channels][H][W] NCHW float32 (dtype 0) or fp16 (dtype 1) -> a padded tap, ring included; channels % 64 == 0.
 *
 * Parameters are torch's own tensors as device pointers, float32, contiguous: inner_w[i] / inner_b[i] = fpn.inner_blocks.i
 * ([256][c5_channels >> i][1][1], [256]; i = 0 reads C5), layer_w / layer_b = fpn.layer_blocks.3 ([256][256][3][3], [256]).  Weights are
 * converted to the kernels' fp16 layouts on the device inside every call, so an in-place optimizer step is seen by the next call.
 * vtd_fpn_train_workspace_bytes: mode 0 = the forward's workspace (the four padded laterals and the packed weights), mode 1 = the
 * backward's scratch; negative for a refused geometry.
 * vtd_fpn_train_forward: writes P2 as padded features (what vtd_dbhead_train_forward reads: [n][8 h5 + 2][8 w5 + 2][256] fp16, ring zeroed)
 * into p2_dev (16-byte aligned) and keeps padded L2 in workspace_dev (256-byte aligned) for the backward.
 * vtd_fpn_train_unpack_p2: padded P2 -> [n][256][H][W] float32.  vtd_fpn_train_pack_grad: an upstream gradient of P2, [n][256][H][W]
 * float32 -> NHWC float32 [n][H][W][256] (with dscale = {1, 1} what the backward reads).
 * vtd_fpn_train_backward: gradients of the ten live tensors, written (not accumulated) as float32 into the grads struct's pointers.
 * dp2_dev / dscale_dev are exactly what vtd_dbhead_train_backward_input writes: dP2 as NHWC float32 [n][H][W][256] times dscale_dev[0], and
 * {scale, 1 / scale}.  GEMM operands are fp16 with an exact power-of-two scale per tensor chosen on the device from max |.|; the sum-pool
 * chain dL(k+1) = sumpool2x2(dL(k)) and the bias sums are fp32 / fp64.  No atomics, shape-only grids: bitwise repeatable.  No gradient
 * of C2..C5 is formed by this call.
 * vtd_fpn_train_backward_input: the gradients of the taps, dC(k) = inner_w[5-k]^T dL(k), one GEMM per level (M = n h w, K = 256, N = the
 * tap's channels).  Call it after vtd_fpn_train_backward, on the same stream, with the same scratch_dev, which must then have
 * vtd_fpn_train_input_workspace_bytes (the backward's scratch with this call's buffers behind it; the backward writes the same bits into a
 * scratch of either size).  level_mask: bit lv asks for the gradient of C(2 + lv).  dtaps_dev: four device pointers ordered C2..C5 (16-byte
 * aligned; entries of levels not asked for are ignored); each requested one receives NHWC float32 [n][h][w][C] times an exact power of two.
 * dscale_dev: [4][2] floats, row lv = {scale, 1 / scale} of dtaps_dev[lv] (rows of levels not asked for are left alone): the convention of
 * vtd_dbhead_train_backward_input.  vtd_fpn_train_unpack_tap_grad: one such tensor and its {scale, 1 / scale} -> [n][C][H][W] float32 with
 * the scale undone.
 * Errors: -2901 (handle built with the fused head entry), -2902 (argument / shape), -2903 (alignment). */
typedef struct vtd_fpn_params {
    float *inner_w[4], *inner_b[4];
    float *layer_w, *layer_b;
} vtd_fpn_params;
int vtd_detector_forward_trunk(vtd_detector* d, int n, void* c2_dev, void* c3_dev, void* c4_dev, void* c5_dev, vtd_stream stream);
int vtd_detector_forward_pool(vtd_detector* d, int n, void* pool_dev, vtd_stream stream);
int vtd_detector_forward_c2(vtd_detector* d, int n, void* c2_dev, vtd_stream stream);
int vtd_fpn_train_pack_tap(const void* x_dev, int dtype, int n, int channels, int height, int width, void* tap_dev, vtd_stream stream);
int64_t vtd_fpn_train_workspace_bytes(int n, int h5, int w5, int c5_channels, int mode);
int vtd_fpn_train_forward(const void* const* taps, int n, int h5, int w5, int c5_channels, const vtd_fpn_params* params, void* workspace_dev,
                          void* p2_dev, vtd_stream stream);
int vtd_fpn_train_unpack_p2(const void* p2_dev, int n, int height, int width, float* p2_nchw_dev, vtd_stream stream);
int vtd_fpn_train_pack_grad(const float* grad_nchw_dev, int n, int height, int width, float* dp2_dev, vtd_stream stream);
int vtd_fpn_train_backward(const void* const* taps, int n, int h5, int w5, int c5_channels, const vtd_fpn_params* params, const void* workspace_dev,
                           const float* dp2_dev, const float* dscale_dev, const vtd_fpn_params* grads, void* scratch_dev, vtd_stream stream);
int64_t vtd_fpn_train_input_workspace_bytes(int n, int h5, int w5, int c5_channels);
int vtd_fpn_train_backward_input(int n, int h5, int w5, int c5_channels, const vtd_fpn_params* params, void* scratch_dev, int level_mask,
                                 float* const* dtaps_dev, float* dscale_dev, vtd_stream stream);
int vtd_fpn_train_unpack_tap_grad(const float* dtap_dev, const float* dscale_dev, int n, int channels, int height, int width, float* grad_nchw_dev,
                                  vtd_stream stream);

/* ---- ResNet BasicBlock training with frozen-statistics BatchNorm (csrc/resblock_train.hip): y = relu(bn2(conv2(relu(bn1(conv1(x))))) + id),
 * id = x or ds_bn(ds(x)).  The running statistics normalise and are never written, whatever mode the caller's module is in; gamma and beta
 * are learnable and get the gradients torch's eval-mode BatchNorm gives them.  Tensors are padded taps (ring-padded NHWC fp16, ring 1):
 * x_dev [n][h_in+2][w_in+2][cin], y_dev [n][h+2][w+2][width] with h = h_in / stride.  Parameters are torch's own float32 tensors as device
 * pointers; weights are folded (w gamma rstd) and packed on the device in every call, so an in-place optimizer step is seen by the next call.
 * Two geometries are built, the blocks of ResNet-18's layer4: (cin 256, width 512, stride 2, even h_in and w_in, with downsample: ds_*
 * set) and (cin 512, width 512, stride 1, identity: ds_* ignored).  Every other geometry is refused with -3001.
 * vtd_basicblock_train_workspace_bytes: mode 0 = the forward's workspace (kept for the backward: the post-ReLU activation a1 and the
 * downsample's output), mode 1 = the backward's scratch.
 * vtd_basicblock_train_backward: dy_dev is NHWC float32 [n][h][w][width] times dscale_dev[0] (a power of two; dscale_dev = {scale,
 * 1 / scale}), y_dev the forward's output.  Gradients are written (not accumulated) into the grads struct's conv1_w, bn1_w, bn1_b, conv2_w,
 * bn2_w, bn2_b and, with a downsample, ds_w, ds_bn_w, ds_bn_b (the *_mean / *_var fields are ignored).  Per convolution + BatchNorm pair,
 * with g the gradient at the BatchNorm output, G = g^T x (MFMA, slabs summed in order) and s = sum g:  dW = gamma rstd G, dbeta = s,
 * dgamma = rstd (sum_k w G - mean s): exact for gamma = 0, nothing divides by gamma.  dx_dev (optional): the input gradient as NHWC float32
 * [n][h][w][512] times dxscale_dev[0], with dxscale_dev = {scale, 1 / scale}.  LIMITATION: the input gradient is formed for the stride-1
 * block only through these entries: a non-NULL dx_dev on the stride-2 block is refused with -3003 (vtd_resblock_train_backward, below,
 * forms it with a strided dgrad).
 * No atomics, shape-only grids: bitwise repeatable.
 * Errors: -3001 (argument / unsupported geometry), -3002 (alignment), -3003 (input gradient of the stride-2 block). */
typedef struct vtd_basicblock_params {
    float *conv1_w, *bn1_w, *bn1_b, *bn1_mean, *bn1_var;
    float *conv2_w, *bn2_w, *bn2_b, *bn2_mean, *bn2_var;
    float *ds_w, *ds_bn_w, *ds_bn_b, *ds_bn_mean, *ds_bn_var;
} vtd_basicblock_params;
int64_t vtd_basicblock_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_basicblock_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                 float eps, void* workspace_dev, void* y_dev, vtd_stream stream);
int vtd_basicblock_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                  float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                  const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* The same block on six geometries (cin, width, stride): (64, 128, 2) and (128, 128, 1), ResNet-18's layer2, (128, 256, 2) and
 * (256, 256, 1), its layer3, and (256, 512, 2) and (512, 512, 1), its layer4; stride 2 needs even h_in and w_in and the downsample's
 * tensors.  Arguments, layouts, numerics and the parameter gradients are those of vtd_basicblock_train_* (for layer4's geometries: the
 * same bits).  The 128-wide blocks differ in two fixed orders: their per-channel sums add two row halves per workgroup, and each of their
 * weight-gradient launches cuts the rows into min(ceil(512 / q-tiles), ceil(rows / 1024)) slabs (the wider blocks: min(8, ceil(rows /
 * 4096)) for every launch); (64, 128, 2)'s weight gradients gather the 64-channel input a tap per 64-column group.  dx_dev (optional) is
 * formed for all six: NHWC float32 [n][h_in][w_in][cin] times dxscale_dev[0].  For a stride-2 block dx = conv1^T(g1) + ds^T(g2) at the input's
 * resolution: input row i receives tap t of output row o where 2 o + t - 1 = i (even rows: the centre tap; odd rows: the two outer taps;
 * row h_in - 1 has no contribution from o = h), columns alike, computed as the stride-1 3x3 path over g1 written into the even positions
 * of a zeroed plane of the input's size (4x the multiply-adds of a phase-split form); the 1x1 stride-2 transpose lands on the even (row,
 * column) positions only, brought to g1's power-of-two scale before the add.  The workspace sizes differ from vtd_basicblock_train_*'s:
 * ask vtd_resblock_train_workspace_bytes.  Errors: -3101 (argument / unsupported geometry), -3102 (alignment), before any launch. */
/* vtd_resblock_train_combine: a_dev [numel] float32 (times ascale_dev[0]) <- a + b (times bscale_dev[0]), both brought to the smaller of
 * the two power-of-two scales, which is written to outscale_dev = {scale, 1 / scale} (a buffer of its own).  numel is a multiple of 4.
 * It adds two gradients of one tensor that arrive from different stages: layer4.0's input gradient and the FPN's dC4, layer3.0's and the
 * FPN's dC3. */
int64_t vtd_resblock_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_resblock_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                               float eps, void* workspace_dev, void* y_dev, vtd_stream stream);
int vtd_resblock_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream);
int vtd_resblock_train_combine(float* a_dev, const float* ascale_dev, const float* b_dev, const float* bscale_dev, int64_t numel, float* outscale_dev,
                               vtd_stream stream);

/* The same block on ResNet-18's layer1 geometry, (cin 64, width 64, stride 1, identity: ds_* ignored), and on no other: the six geometries
 * above and everything else are refused here, as (64, 64, 1) is refused by vtd_resblock_train_* and vtd_basicblock_train_*.  Arguments,
 * layouts and numerics are those of vtd_resblock_train_*, argument for argument; dx_dev (optional) is NHWC float32 [n][h_in][w_in][64] times
 * dxscale_dev[0].  Two fixed orders are the 64-wide block's own.  Its per-channel sums add four row quarters per workgroup: a workgroup's r
 * rows are cut at ceil(k r / 4), k = 0..4, each quarter is summed in row order in fp64 and the partial is (q0 + q1) + (q2 + q3); the
 * partials are then added in workgroup order as for every width.  Each of its two weight-gradient launches (K = 9 x 64 = 576: five q-tiles of
 * 128 columns, a tap per 64-column group, the last group empty) cuts the rows into min(ceil(512 / 5), ceil(rows / 1024)) slabs of [64][576]
 * floats, the 128-wide rule, summed in slab order.  There is no downsample and no strided input gradient.  No atomics, shape-only grids:
 * bitwise repeatable.  Errors: -3201 (argument / unsupported geometry), -3202 (alignment), before any launch. */
int64_t vtd_block64_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_block64_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                              float eps, void* workspace_dev, void* y_dev, vtd_stream stream);
int vtd_block64_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                               float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                               const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* ---- ResNet Bottleneck training with frozen-statistics BatchNorm (csrc/bottleneck_train.hip), v1.5 (the stride sits on the 3x3):
 * y = relu(bn3(conv3(a2)) + id), a2 = relu(bn2(conv2(a1))), a1 = relu(bn1(conv1(x))), id = x or ds_bn(ds(x)); conv1 is 1x1 cin -> width,
 * conv2 3x3 width -> width at `stride`, conv3 1x1 width -> 4 width, ds 1x1 cin -> 4 width at `stride`.  Tensors, layouts, the folded weights
 * packed on the device in every call, the running statistics that normalise and are never written, the power-of-two gradient scales and
 * the "written, not accumulated" rule are those of vtd_basicblock_train_*: x_dev [n][h_in+2][w_in+2][cin], y_dev [n][h+2][w+2][4 width]
 * with h = h_in / stride, padded taps.  Two geometries are built, the blocks of ResNet-50's last stage (res5, torchvision's layer4), width
 * 512: (cin 1024, stride 2, even h_in and w_in, with downsample: ds_* set) and (cin 2048, stride 1, identity: ds_* ignored).  Every other
 * geometry, n > 65535, an extent above 4096 and a tensor of 2^31 elements or more are refused with -3901.
 * vtd_bottleneck_train_workspace_bytes, with a256(b) = b rounded up to a multiple of 256, W = 512, pin = n (h_in+2) (w_in+2),
 * pout = n (h+2) (w+2), M = n h w, Min = n h_in w_in and S(r) = min(8, max(1, ceil(r / 4096))):
 *   mode 0, the forward's workspace, which the backward keeps: a256(2 pin W) [a1, padded at the INPUT's extent] + a256(2 pout W) [a2] +
 *     a256(2 pout 4W) [id, stride 2 only] + a256(2 W cin) + a256(2 W 9 W) + a256(2 4W W) + a256(2 4W cin) [stride 2 only] (the four folded
 *     panels) + a256(4 (2 W + 2 4W)) [the biases];
 *   mode 1, the backward's scratch: a256(4 M 4W) + a256(4 M W) + a256(4 Min W) [g3, g2, g1 fp32] + a256(2 M 4W) + a256(2 M W) +
 *     a256(2 Min W) [flat fp16 operands] + a256(2 pout 4W) + 2 a256(2 pin W) [padded fp16 operands; g2's is the zero-inserted plane at stride
 *     2] + a256(2 W 9 W) [transposed panel] + a256(4 4W) [zero bias] + a256(8 256 4W) + a256(4 256) [partials] + a256(8 4W) + 2 a256(8 W) [sums]
 *     + a256(48) [scales] + a256(4 max(S(M) W 9 W, S(Min) W cin)) [weight-gradient slabs].
 * vtd_bottleneck_train_backward: dy_dev is NHWC float32 [n][h][w][4 width] times dscale_dev[0] (dscale_dev = {scale, 1 / scale}, a power
 * of two).  Gradients are written into the grads struct's twelve (stride 1: nine) learnable fields; its *_mean / *_var are ignored.  Per
 * convolution + BatchNorm pair, with g the gradient at the BatchNorm output, G = g^T im2col(input) (MFMA, wgrad_mfma.h MODE 3, slabs
 * summed in slab order in fp64) and s = sum g:  dW = gamma rstd G, dbeta = s, dgamma = rstd (sum_k w G - mean s); nothing divides by gamma.
 * Fixed orders: the 2048-wide gradient g3 = dy (y > 0) is summed per channel by min(256, ceil(M / 32)) workgroups of ceil(M / that)
 * consecutive rows each, every row in row order in fp64, the partials then in workgroup order; the 512-wide g2 = conv3^T(g3) (a2 > 0) and
 * g1 = conv2^T(g2) (a1 > 0) by min(256, ceil(rows / 256)) workgroups the same way; every weight-gradient launch cuts ITS rows into
 * S(rows) slabs -- conv3, conv2 and the downsample the M output rows, conv1 the Min rows of the input's extent, where g1 lives.
 * conv2^T at stride 2 is the stride-1 rotated, transposed 3x3 path over g2 written into the even positions of a zeroed plane of the
 * input's size, as vtd_resblock_train_backward's.  dx_dev (optional, with dxscale_dev = {scale, 1 / scale}) is formed for both
 * geometries: NHWC float32 [n][h_in][w_in][cin] times dxscale_dev[0] = conv1^T(g1), plus g3 (stride 1) or ds^T(g3) at the even (row,
 * column) positions (stride 2), each summand brought to g1's power-of-two scale before the add.
 * No atomics, shape-only grids: bitwise repeatable.  Errors, before any launch: -3901 (a null pointer, eps <= 0, dx_dev without dxscale_dev,
 * a missing ds_* tensor at stride 2, a mode outside {0, 1}, an unsupported geometry), -3902 (alignment: taps, dy and dx 16 bytes, workspace
 * and scratch 256, scales 8, parameters and gradients 4). */
typedef struct vtd_bottleneck_params {
    float *conv1_w, *bn1_w, *bn1_b, *bn1_mean, *bn1_var;
    float *conv2_w, *bn2_w, *bn2_b, *bn2_mean, *bn2_var;
    float *conv3_w, *bn3_w, *bn3_b, *bn3_mean, *bn3_var;
    float *ds_w, *ds_bn_w, *ds_bn_b, *ds_bn_mean, *ds_bn_var;
} vtd_bottleneck_params;
int64_t vtd_bottleneck_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_bottleneck_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                 float eps, void* workspace_dev, void* y_dev, vtd_stream stream);
int vtd_bottleneck_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                  float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                  const vtd_bottleneck_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* ---- The 256-wide Bottlenecks of ResNet-50's res4 (torchvision's layer3), the same file, host path and kernels at W = 256.  Signatures,
 * the vtd_bottleneck_params struct, tensors, layouts, scales and the "written, not accumulated" rule are those of vtd_bottleneck_train_*:
 * x_dev [n][h_in+2][w_in+2][cin], y_dev [n][h+2][w+2][1024], dy_dev NHWC float32 [n][h][w][1024].  Exactly two geometries are accepted,
 * width 256: (cin 512, stride 2, even h_in and w_in, with downsample: ds_* set) and (cin 1024, stride 1, identity: ds_* ignored).  Every
 * other geometry (width 512 included: that is vtd_bottleneck_train_*'s), n > 65535, an extent above 4096 and a tensor of 2^31 elements or
 * more are refused with -3903.
 * vtd_bottleneck256_train_workspace_bytes, with a256(b) = b rounded up to a multiple of 256, W = 256 (4W = 1024), pin = n (h_in+2) (w_in+2),
 * pout = n (h+2) (w+2), M = n h w, Min = n h_in w_in and S(r) = min(8, max(1, ceil(r / 4096))):
 *   mode 0, the forward's workspace, which the backward keeps: a256(2 pin W) [a1, padded at the INPUT's extent] + a256(2 pout W) [a2] +
 *     a256(2 pout 4W) [id, stride 2 only] + a256(2 W cin) + a256(2 W 9 W) + a256(2 4W W) + a256(2 4W cin) [stride 2 only] (the four folded
 *     panels) + a256(4 (2 W + 2 4W)) [the biases];
 *   mode 1, the backward's scratch: a256(4 M 4W) + a256(4 M W) + a256(4 Min W) [g3, g2, g1 fp32] + a256(2 M 4W) + a256(2 M W) +
 *     a256(2 Min W) [flat fp16 operands] + a256(2 pout 4W) + 2 a256(2 pin W) [padded fp16 operands; g2's is the zero-inserted plane at stride
 *     2] + a256(2 W 9 W) [transposed panel] + a256(4 4W) [zero bias] + a256(8 256 4W) + a256(4 256) [partials] + a256(8 4W) + 2 a256(8 W) [sums]
 *     + a256(48) [scales] + a256(4 max(S(M) W 9 W, S(Min) W cin)) [weight-gradient slabs].
 * Fixed orders: the 1024-wide gradient g3 = dy (y > 0) is summed per channel by min(256, ceil(M / 32)) workgroups of ceil(M / that)
 * consecutive rows each (one 16-byte load per thread and row), every row in row order in fp64, the partials then in workgroup order; the
 * 256-wide g2 and g1 by min(256, ceil(rows / 256)) workgroups the same way; every weight-gradient launch (wgrad_mfma.h MODE 3) cuts ITS rows
 * into S(rows) slabs, summed in slab order in fp64 -- conv3, conv2 and the downsample the M output rows, conv1 the Min rows of the input's
 * extent.  dx_dev (optional) as vtd_bottleneck_train_backward's.  No atomics, shape-only grids: bitwise repeatable.  Errors, before any
 * launch: -3903 (a null pointer, eps <= 0, dx_dev without dxscale_dev, a missing ds_* tensor at stride 2, a mode outside {0, 1}, an
 * unsupported geometry), -3904 (alignment: taps, dy and dx 16 bytes, workspace and scratch 256, scales 8, parameters and gradients 4). */
int64_t vtd_bottleneck256_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_bottleneck256_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                    float eps, void* workspace_dev, void* y_dev, vtd_stream stream);
int vtd_bottleneck256_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride,
                                     const vtd_bottleneck_params* params, float eps, const void* workspace_dev, const void* y_dev,
                                     const float* dy_dev, const float* dscale_dev, const vtd_bottleneck_params* grads, void* scratch_dev,
                                     float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* ---- The 128-wide Bottlenecks of ResNet-50's res3 (torchvision's layer2), the same file and host path at W = 128.  Signatures, the
 * vtd_bottleneck_params struct, tensors, layouts, scales and the "written, not accumulated" rule are those of vtd_bottleneck_train_*:
 * x_dev [n][h_in+2][w_in+2][cin], y_dev [n][h+2][w+2][512], dy_dev NHWC float32 [n][h][w][512].  Exactly two geometries are accepted,
 * width 128: (cin 256, stride 2, even h_in and w_in, with downsample: ds_* set) and (cin 512, stride 1, identity: ds_* ignored).  Every
 * other geometry (widths 256 and 512 included: those are vtd_bottleneck256_train_*'s and vtd_bottleneck_train_*'s), n > 65535, an extent
 * above 4096 and a tensor of 2^31 elements or more are refused with -3905.
 * vtd_bottleneck128_train_workspace_bytes: vtd_bottleneck256_train_workspace_bytes's sums at W = 128 (4W = 512), but for the last term of
 * mode 1, the weight-gradient slabs.  With T(r, w) = min(ceil(512 / w), max(1, ceil(r / 1024))), the slabs of a launch over r rows with w
 * workgroups per slab (its q-tiles times its 128-column tiles; 512 workgroups when the rows allow slabs of 1024 rows), the term is
 * a256(4 max(T(M, 9) W 9 W [conv2], T(Min, cin / 128) W cin [conv1], T(M, 4) 4W W [conv3], T(M, 4 cin / 128) 4W cin [the downsample, stride 2
 * only])): 33.6 MB at n = 32 on a 160 x 160 or 80 x 80 input, where every launch has 512 workgroups.
 * Fixed orders: the 512-wide gradient g3 = dy (y > 0) is summed per channel by min(256, ceil(M / 32)) workgroups of r = ceil(M / that)
 * consecutive rows each; in a workgroup threads 0 .. 127 own the 512 channels (four each, one 16-byte load per thread and row) over its first
 * ceil(r / 2) rows and threads 128 .. 255 over the rest, every half in row order in fp64, then first half + second half, the partials then
 * in workgroup order; the 128-wide g2 and g1 by min(256, ceil(rows / 256)) workgroups with the same two halves (one channel per thread);
 * every weight-gradient launch (wgrad_mfma.h MODE 3) cuts ITS rows into T slabs, summed in slab order in fp64.  dx_dev (optional) as
 * vtd_bottleneck_train_backward's.  No atomics, shape-only grids: bitwise repeatable.  Errors, before any launch: -3905 (a null pointer,
 * eps <= 0, dx_dev without dxscale_dev, a missing ds_* tensor at stride 2, a mode outside {0, 1}, an unsupported geometry), -3906
 * (alignment: taps, dy and dx 16 bytes, workspace and scratch 256, scales 8, parameters and gradients 4). */
int64_t vtd_bottleneck128_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_bottleneck128_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                    float eps, void* workspace_dev, void* y_dev, vtd_stream stream);
int vtd_bottleneck128_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride,
                                     const vtd_bottleneck_params* params, float eps, const void* workspace_dev, const void* y_dev,
                                     const float* dy_dev, const float* dscale_dev, const vtd_bottleneck_params* grads, void* scratch_dev,
                                     float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* ---- The 64-wide Bottlenecks of ResNet-50's res2 (torchvision's layer1), the same file and host path at W = 64.  Signatures, the
 * vtd_bottleneck_params struct, tensors, layouts, scales and the "written, not accumulated" rule are those of vtd_bottleneck_train_*:
 * x_dev [n][h_in+2][w_in+2][cin], y_dev [n][h+2][w+2][256], dy_dev NHWC float32 [n][h][w][256].  Exactly two geometries are accepted,
 * width 64, both at stride 1 (h = h_in, w = w_in): (cin 64, with a 1x1 downsample at stride 1: ds_* set) and (cin 256, identity: ds_*
 * ignored).  Every other geometry (stride 2 and widths 128, 256 and 512 included: those widths are the other three families'), n > 65535,
 * an extent above 4096 and a tensor of 2^31 elements or more (pin max(cin, W) or pout 4W) are refused with -3907.
 * vtd_bottleneck64_train_workspace_bytes: vtd_bottleneck256_train_workspace_bytes's sums at W = 64 (4W = 256) with "cin 64" where they say
 * "stride 2" (id and the downsample's panel exist for the first block), but for the last term of mode 1, the weight-gradient slabs.  With
 * T(r, w) = min(ceil(512 / w), max(1, ceil(r / 1024))) as vtd_bottleneck128_train_workspace_bytes's, w = the launch's q-tiles (ceil(K / 128))
 * times its column tiles (one for the 64-wide gradients, two for the 256-wide ones), the term is a256(4 max(T(M, 5) W 9 W [conv2],
 * T(M, ceil(cin / 128)) W cin [conv1], T(M, 2) 4W W [conv3], T(M, 2) 4W cin [the downsample, cin 64 only])).  At n = 32 on a 160 x 160
 * input (M = 819 200): workspace 215.1 MB (cin 256) or 645.1 MB (cin 64, with id), scratch 2.55 GB for either, of which the slabs are
 * 16.8 MB (256 slabs of [64][256] or [256][64], or 512 of [64][64]; conv2 has 103 of [64][576], 15.2 MB): 512 to 515 workgroups a launch.
 * Fixed orders: the 256-wide gradient g3 = dy (y > 0) is summed per channel by min(256, ceil(M / 32)) workgroups of r = ceil(M / that)
 * consecutive rows each; in a workgroup threads 64 k .. 64 k + 63 own the 256 channels (four each, one 16-byte load per thread and row) over
 * quarter k of its rows, rows ceil(k r / 4) .. ceil((k + 1) r / 4) - 1 (15 rows: 4, 4, 4, 3), every quarter in row order in fp64, then
 * (q0 + q1) + (q2 + q3), the partials then in workgroup order; the 64-wide g2 and g1 by min(256, ceil(rows / 256)) workgroups with the same
 * four quarters (one channel per thread); conv2 and conv1's weight gradients run on wgrad_mfma.h MODE 5 (the 64-row tile), conv3's and the
 * downsample's on MODE 4 (64 input channels: half a q-tile), each launch cutting ITS rows into T slabs, summed in slab order in fp64.
 * dx_dev (optional, with dxscale_dev) is formed for both geometries: conv1^T(g1) plus g3 (cin 256) or the dense ds^T(g3) at every pixel
 * (cin 64), each summand brought to g1's power-of-two scale before the add.  No atomics, shape-only grids: bitwise repeatable.  Errors,
 * before any launch: -3907 (a null pointer, eps <= 0, dx_dev without dxscale_dev, a missing ds_* tensor at cin 64, a mode outside {0, 1}, an
 * unsupported geometry), -3908 (alignment: taps, dy and dx 16 bytes, workspace and scratch 256, scales 8, parameters and gradients 4). */
int64_t vtd_bottleneck64_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_bottleneck64_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                   float eps, void* workspace_dev, void* y_dev, vtd_stream stream);
int vtd_bottleneck64_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride,
                                    const vtd_bottleneck_params* params, float eps, const void* workspace_dev, const void* y_dev,
                                    const float* dy_dev, const float* dscale_dev, const vtd_bottleneck_params* grads, void* scratch_dev,
                                    float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* ---- ResNet BasicBlock training with batch-statistics BatchNorm (csrc/resblock_bn_train.hip): the same block as torch's train() mode
 * computes it.  Tensors, layouts, the vtd_basicblock_params struct, the power-of-two gradient scales and the "written, not accumulated" rule
 * are those of vtd_basicblock_train_*.  Two geometries are built, ResNet-18's layer4: (cin 256, width 512, stride 2, even h_in and w_in, with
 * downsample) and (cin 512, width 512, stride 1, identity: ds_* ignored); every other geometry is refused with -3401.
 * vtd_resblock_bn_train_workspace_bytes: mode 0 = the forward's workspace (kept for the backward), mode 1 = the backward's scratch; each
 * serves either value of `training`.
 * training = 0: the running statistics normalise and nothing is written (stats_dev included).  The call is handed to
 * vtd_basicblock_train_forward / _backward: y, the parameter gradients and dx are their bits.
 * training = 1, forward, per convolution + BatchNorm pair (conv1 / bn1, conv2 / bn2, the downsample): the raw weights are rounded to fp16 on
 * the device in every call (no fold); the convolution writes z, float32 [n h w][width], kept in the workspace.  Per-channel statistics are
 * (count, mean, M2) partials in fp64 -- min(256, ceil(n h w / 256)) workgroups of ceil(n h w / workgroups) consecutive rows, each summing the
 * first ceil(r / 2) of its r rows in row order, then the rest, lower + upper -- combined in workgroup order (Chan) into the batch mean mu and
 * the biased variance sigma^2.  The running values in `params` are updated in place: mean <- (1 - momentum) mean + momentum mu, var <-
 * (1 - momentum) var + momentum sigma^2 M / (M - 1), M = n h w.  stats_dev (optional) receives float32 [3][2][width]: mu and sigma^2 of bn1,
 * bn2 and the downsample's BatchNorm (the third row is untouched without a downsample).  a1 = relu(((z1 - mu) rstd) gamma + beta), the
 * downsample's normalised output (no ReLU) and y = relu(((z2 - mu) rstd) gamma + beta + id) are stored as ring-padded fp16 taps.  The caller
 * advances num_batches_tracked.
 * training = 1, backward: g2 = dy (y > 0).  Per pair, with g the gradient at the BatchNorm output (g2 for bn2 and the downsample, conv2^T(dz2)
 * (a1 > 0) for bn1) and xh = (z - mu) rstd recomputed from the saved z: s1 = sum g and s2 = sum g xh in fp64, rows and workgroups in the
 * forward's order; dbeta = s1, dgamma = s2; dz = gamma rstd (g - s1 / M - xh s2 / M) in float32, then times a power of two taken from the bound
 * max_c |gamma rstd| (max |g| + |s1| / M + max |xh| |s2| / M) and rounded to fp16; dW = dz^T im2col(input) (MFMA, min(8, ceil(M / 4096)) slabs
 * summed in order in fp64): dz carries gamma rstd, no factor follows.  Exact for gamma = 0 and gamma < 0: nothing divides by gamma or sigma.
 * dx_dev (optional, the stride-1 block only): conv1^T(dz1) + g2 as NHWC float32 [n][h][w][512] times dxscale_dev[0].  LIMITATION: a non-NULL
 * dx_dev on the stride-2 block is refused with -3403.  The statistics are not fused into the convolution's epilogue: z makes one round trip
 * through HBM per pair and direction.
 * No atomics, shape-only grids: bitwise repeatable; a dy scaled by a power of two gives the same gradient bits, scaled.
 * Errors, before any launch: -3401 (argument / unsupported geometry / training = 1 with n h w < 2 / momentum outside [0, 1]), -3402
 * (alignment), -3403 (input gradient of the stride-2 block). */
int64_t vtd_resblock_bn_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_resblock_bn_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                  int training, float momentum, float eps, void* workspace_dev, void* y_dev, float* stats_dev, vtd_stream stream);
int vtd_resblock_bn_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                   int training, float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                   const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* ---- The same with layer3's width too (csrc/resblock_bn_train.hip, the same launch functions): vtd_block_bn_train_* take the arguments of
 * vtd_resblock_bn_train_*, one for one, and build four geometries: (cin 128, width 256, stride 2, even h_in and w_in, with downsample),
 * (cin 256, width 256, stride 1), (cin 256, width 512, stride 2, even extents, with downsample) and (cin 512, width 512, stride 1); every
 * other geometry is refused with -3501.  training = 0 hands the call to vtd_resblock_train_forward / _backward (the frozen path with the
 * strided dx): their bits.  For the two width-512 geometries y, the statistics, the running update, every parameter gradient and the
 * stride-1 dx are the bits of vtd_resblock_bn_train_*.
 * The per-channel reductions of a 256-wide z (the statistics' partials and the backward's s1, s2): 64 threads x 4 channels cover the width,
 * so the 256 threads of a workgroup are four quarters of its r rows.  Quarter k sums rows ceil(k r / 4) .. ceil((k + 1) r / 4) - 1 in row
 * order in fp64; the workgroup's partial is (q0 + q1) + (q2 + q3); the workgroups -- min(256, ceil(n h w / 256)) of ceil(n h w / workgroups)
 * consecutive rows, as at width 512 -- are combined in workgroup order (Chan's combination for the statistics).  Shape-only.
 * dx_dev on a stride-2 block is accepted: dz1 goes to the even positions of a zeroed ring-padded plane of the input's extent, the stride-1
 * 3x3 dgrad runs over it on the raw conv1 weights (rotated, transposed), and ds^T(dz_d) -- a 1x1 GEMM of the downsample BatchNorm's own dz on
 * the transposed raw downsample weights -- is added at the even (row, column) positions after the power-of-two factor sc2 sc1 / scd that
 * brings dz_d's scale to dz1's (exact).  The parameter gradients do not depend on whether dx is asked for.  The statistics are still not
 * fused into the convolution's epilogue.  No atomics, shape-only grids: bitwise repeatable.
 * Errors, before any launch: -3501 (argument / unsupported geometry / training outside {0, 1} / training = 1 with n h w < 2 / momentum
 * outside [0, 1] / dx_dev without dxscale_dev), -3502 (alignment). */
int64_t vtd_block_bn_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_block_bn_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                               int training, float momentum, float eps, void* workspace_dev, void* y_dev, float* stats_dev, vtd_stream stream);
int vtd_block_bn_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                int training, float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* ---- The same with layer2's width too (csrc/resblock_bn_train.hip, the same launch functions): vtd_trunk_bn_train_* take the arguments of
 * vtd_block_bn_train_*, one for one, and build six geometries: layer2's (cin 64, width 128, stride 2, even h_in and w_in, with downsample)
 * and (cin 128, width 128, stride 1), and the four of vtd_block_bn_train_* (and layer1's, below); every other geometry is refused with
 * -3701.  This is the family that later stages join (layer1: below; the stem: vtd_stem_bn_train_*, further down, behind entries of its own);
 * the older families keep their gates and their bits.
 * training = 0 hands the call to vtd_resblock_train_forward / _backward: their bits.  For the four geometries of vtd_block_bn_train_* every output -- y, the statistics, the
 * running update, every parameter gradient and the dx of either stride -- is the bits of vtd_block_bn_train_*.
 * The per-channel reductions of a 128-wide z (the statistics' partials and the backward's s1, s2): 32 threads x 4 channels cover the width,
 * so the 256 threads of a workgroup are eight parts of its r rows.  Part k sums rows ceil(k r / 8) .. ceil((k + 1) r / 8) - 1 in row order
 * in fp64; the workgroup's partial is ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)); the workgroups -- min(256, ceil(n h w / 256)) of
 * ceil(n h w / workgroups) consecutive rows, as at the other widths -- are combined in workgroup order (Chan's combination for the
 * statistics).  Shape-only, no atomics.
 * The weight gradients of a 128-wide block have one 128-column tile, so each of the block's launches takes its own slab count, the rule of
 * vtd_resblock_train_*'s 128-wide blocks: ceil(ksz^2 cin / 128) q-tiles (a tap per 64-column group over layer2.0's 64-channel input: K = 576
 * is 4.5 q-tiles, K = 64 half of one) and min(ceil(512 / q-tiles), ceil(n h w / 1024)) slabs of rows, summed in slab order in fp64.  The
 * wider blocks keep min(8, ceil(n h w / 4096)) slabs for every launch.
 * dx_dev is accepted at either stride, as in vtd_block_bn_train_*; layer2.0's is NHWC float32 [n][h_in][w_in][64].  The statistics are still
 * not fused into the convolution's epilogue: z makes one round trip through HBM per pair and direction.  Bitwise repeatable.
 * A seventh geometry, ResNet-18's layer1: (cin 64, width 64, stride 1, identity: ds_* ignored).  The gate names it alone: (64, 64, 2) and
 * (32, 64, 2) are refused with -3701, and the older families keep refusing (64, 64, 1) with -3401 / -3501.  training = 0 hands the call to
 * vtd_block64_train_forward / _backward (the frozen 64-wide path): their bits, nothing written; the workspace query answers at least
 * vtd_block64_train_workspace_bytes, so either value of `training` runs in one allocation.  training = 1 is the batch path of the other
 * widths -- raw weights rounded to fp16 per call, z kept in fp32, stats_dev rows 0 and 1 (row 2 untouched), the running update with the
 * unbiased variance, the full BatchNorm backward, dx_dev (optional) as NHWC float32 [n][h][w][64] -- with the convolutions and the dgrad at 64
 * output channels, as the frozen 64-wide block runs them.
 * The per-channel reductions of a 64-wide z: 16 threads x 4 channels cover the width, so the 256 threads of a workgroup are sixteen parts of
 * its r rows.  Part k sums rows ceil(k r / 16) .. ceil((k + 1) r / 16) - 1 in row order in fp64 (a part without rows, r < 16, contributes
 * exact zeros); the workgroup's partial is the balanced pairwise tree, the eight-part order on each half and then lower + upper:
 * (((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7))) + (((q8 + q9) + (q10 + q11)) + ((q12 + q13) + (q14 + q15))); workgroups and their
 * combination as at the other widths.
 * Its two weight-gradient launches (conv2 and conv1, K = 9 x 64 = 576) run the 64-row tile on dz [n h w][64], which already carries gamma
 * rstd, by the slab rule of vtd_block64_train_*: five q-tiles, min(ceil(512 / 5), ceil(n h w / 1024)) slabs of [64][576] floats, summed in
 * slab order in fp64.  The statistics stay unfused from the convolution's epilogue at this width too.
 * Errors, before any launch: -3701 (argument / unsupported geometry / training outside {0, 1} / training = 1 with n h w < 2 / momentum
 * outside [0, 1] / dx_dev without dxscale_dev), -3702 (alignment). */
int64_t vtd_trunk_bn_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_trunk_bn_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                               int training, float momentum, float eps, void* workspace_dev, void* y_dev, float* stats_dev, vtd_stream stream);
int vtd_trunk_bn_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_basicblock_params* params,
                                int training, float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev, const float* dscale_dev,
                                const vtd_basicblock_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev, vtd_stream stream);

/* ---- ResNet Bottleneck training with batch-statistics BatchNorm (csrc/bottleneck_bn_train.hip): ResNet-50's res5 and res4 blocks as torch's
 * train() mode computes them.  vtd_bottleneck_bn_train_* take the arguments of vtd_trunk_bn_train_*, one for one, with the
 * vtd_bottleneck_params struct; tensors, layouts, the power-of-two gradient scales and the "written, not accumulated" rule are those of
 * vtd_bottleneck_train_*.  Four geometries are built, W = width, 4W the output's channels: (cin 1024, width 512, stride 2, even h_in and w_in,
 * with downsample), (cin 2048, width 512, stride 1, identity: ds_* ignored), (cin 512, width 256, stride 2, even extents, with downsample)
 * and (cin 1024, width 256, stride 1); every other geometry (widths 128 and 64 included: res3, res2 and the stem keep frozen statistics) is
 * refused with -4001.
 * training = 0 hands the call to vtd_bottleneck_train_forward / _backward (width 512) or vtd_bottleneck256_train_forward / _backward (width
 * 256) unchanged: their bits, nothing written (stats_dev included).  The workspace query answers at least theirs, so either value of
 * `training` runs in one allocation.
 * training = 1, forward, per convolution + BatchNorm pair (conv1 / bn1, conv2 / bn2, the downsample, conv3 / bn3): the raw weights are
 * rounded to fp16 on the device in every call (no fold); the convolution writes z in float32, kept in the workspace: z1 [n h_in w_in][W]
 * (conv1 is 1x1 at the input's extent, and a1 is padded at the input's extent), z2 [n h w][W], z_d and z3 [n h w][4W].  Per-channel statistics
 * are (count, mean, M2) partials in fp64, combined in workgroup order (Chan) into mu and the biased sigma^2.  The W-wide pairs reduce as
 * vtd_block_bn_train_* states for widths 512 and 256: min(256, ceil(rows / 256)) workgroups of ceil(rows / workgroups) consecutive rows, two
 * halves (lower + upper) or four quarters ((q0 + q1) + (q2 + q3)) of them in row order.  The 4W-wide pairs: min(256, ceil(n h w / 32))
 * workgroups of ceil(n h w / workgroups) consecutive rows; thread t of 256 owns channels 1024 j + 4 t .. 1024 j + 4 t + 3 (j < 4W / 1024) and
 * sums them over the workgroup's rows in row order: one thread per channel, no join.  The reduce grid is per pair: bn1's rows are the input's.
 * The running values in `params` are updated in place: mean <- (1 - momentum) mean + momentum mu, var <- (1 - momentum) var + momentum sigma^2
 * M / (M - 1), M the pair's rows.  stats_dev (optional) receives float32 [4][2][4W]: rows bn1, bn2, bn3 and the downsample's BatchNorm, each
 * {mu, sigma^2}; rows 0 and 1 use the first W columns; a row (or column) the call does not write is left untouched.  a1, a2, the downsample's
 * normalised output (no ReLU) and y = relu(((z3 - mu) rstd) gamma + beta + id) are stored as ring-padded fp16 taps.  The caller advances
 * num_batches_tracked.
 * training = 1, backward: g3 = dy (y > 0), formed in the same pass that reduces it.  Per pair, with g the gradient at the BatchNorm output (g3
 * for bn3 and the downsample, conv3^T(dz3) (a2 > 0) for bn2, conv2^T(dz2) (a1 > 0) for bn1) and xh = (z - mu) rstd recomputed from the saved z:
 * s1 = sum g and s2 = sum g xh in fp64, rows and workgroups in the forward's order; dbeta = s1, dgamma = s2; dz = gamma rstd (g - s1 / M - xh
 * s2 / M) in float32, then times a power of two taken from the bound max_c |gamma rstd| (max |g| + |s1| / M + max |xh| |s2| / M) and rounded to
 * fp16; dW = dz^T im2col(input) (MFMA, min(8, ceil(rows / 4096)) slabs of the launch's rows, summed in slab order in fp64): dz carries gamma
 * rstd, no factor follows.  The transposed convolutions run on the raw weights, rotated and transposed.  Stride 2: dz2 goes to the even
 * positions of a zeroed ring-padded plane of the input's extent; the downsample pair has its own statistics and its own dz_d, and
 * ds^T(dz_d) is added to dx at the even (row, column) positions after the power-of-two factor sc3 sc2 sc1 / scd that brings it to dz1's scale
 * (exact).  Stride 1: dx = conv1^T(dz1) + g3 at one scale.  dx_dev (optional at either stride): NHWC float32 [n][h_in][w_in][cin] times
 * dxscale_dev[0].  Exact for gamma = 0 and gamma < 0: nothing divides by gamma or sigma.  The statistics are not fused into the convolution's
 * epilogue: z makes one write and two or three reads through HBM per pair.  No atomics, shape-only grids, fixed summation orders: bitwise
 * repeatable; a dy scaled by a power of two gives the same gradient bits, scaled.
 * vtd_bottleneck_bn_train_workspace_bytes: the larger of the frozen family's answer and, with a256(b) = b rounded up to a multiple of 256,
 * pin = n (h_in+2) (w_in+2), pout = n (h+2) (w+2), M = n h w, Min = n h_in w_in and ds = 1 with a downsample, else 0:
 *   mode 0: a256(2 pin W) + a256(2 pout W) + ds a256(8 pout W) + a256(4 Min W) + a256(4 M W) + (1 + ds) a256(16 M W) + a256(2 W cin) +
 *           a256(18 W^2) + a256(8 W^2) + ds a256(8 W cin) + a256(16 W) + a256(256 x 96 W) + 2 a256(16 W) + (1 + ds) a256(64 W) + a256(8 W)
 *   mode 1: a256(16 M W) + a256(4 M W) + a256(4 Min W) + a256(2 max(4 M W, Min W)) + a256(8 pout W) + 2 a256(2 pin W) + a256(18 W^2) +
 *           a256(16 W) + a256(256 x 64 W) + a256(256 x 32 W) + a256(48 W) + a256(64) +
 *           a256(4 max(min(8, ceil(M / 4096)) 9 W^2, min(8, ceil(Min / 4096)) W cin))
 * At n = 32 a 40 x 40 res5 input (1024 -> 512 -> 2048, stride 2) takes 502624256 bytes of workspace (the frozen family: 149180416; the
 * difference is the four float32 z) and 579634432 bytes of scratch; an 80 x 80 res4 input (512 -> 256 -> 1024, stride 2) 945600512 bytes of
 * workspace (frozen: 257697792) and 1065895168 bytes of scratch.  Both scratch figures are the frozen family's, which keeps flat operands
 * per stage and is the larger sum at these shapes.
 * Errors, before any launch: -4001 (argument / unsupported geometry / training outside {0, 1} / training = 1 with fewer than two rows in any
 * pair / momentum outside [0, 1] / dx_dev without dxscale_dev), -4002 (alignment). */
int64_t vtd_bottleneck_bn_train_workspace_bytes(int n, int h_in, int w_in, int cin, int width, int stride, int mode);
int vtd_bottleneck_bn_train_forward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                    int training, float momentum, float eps, void* workspace_dev, void* y_dev, float* stats_dev, vtd_stream stream);
int vtd_bottleneck_bn_train_backward(const void* x_dev, int n, int h_in, int w_in, int cin, int width, int stride, const vtd_bottleneck_params* params,
                                     int training, float eps, const void* workspace_dev, const void* y_dev, const float* dy_dev,
                                     const float* dscale_dev, const vtd_bottleneck_params* grads, void* scratch_dev, float* dx_dev, float* dxscale_dev,
                                     vtd_stream stream);

/* ---- ResNet stem training with frozen-statistics BatchNorm (csrc/stem_train.hip): pool = maxpool3x3/s2/p1(relu(bn(conv7x7/s2/p3(x)))) on an
 * image x [n,3,height,width]; height and width are the image's, even and at least 2 (the product's 640 is not built in).  hc x wc = height / 2
 * x width / 2 is the conv map, hp x wp = ceil(hc / 2) x ceil(wc / 2) the pooled map.  The running statistics normalise and are never written;
 * w, gamma and beta learn.  No gradient of the image is formed.
 * vtd_stem_train_pack_input: x_dev NCHW float32 (dtype 0) or fp16 (dtype 1) -> tap_dev, the stem's input layout [n][height+6][width+6][4]
 * fp16 (ring 3, a zero fourth channel, a zero ring).
 * vtd_stem_train_workspace_bytes: mode 0 = the forward's workspace (the folded weights and bias: it does not depend on the shape; kept for
 * the backward), mode 1 = the backward's scratch.
 * vtd_stem_train_forward: one launch behind the fold (half(w gamma rstd), bias = beta - mean gamma rstd, on the device, every call): conv +
 * bias + ReLU as fp16 in LDS, pooled from there.  pool_tap_dev receives the padded tap [n][hp+2][wp+2][64] fp16 with a zero ring (what
 * vtd_block64_train_forward reads), idx_dev one byte per pooled element [n][hp][wp][64]: the window position 3 ky + kx of the first maximum
 * in scan order (ky, then kx), the element torch's CPU max_pool2d backward routes to; only in-image positions win.  Where the pooled value
 * is 0 the byte is unspecified.  The conv map is not written.
 * vtd_stem_train_backward: dpool_dev is NHWC float32 [n][hp][wp][64] times dscale_dev[0] (a power of two; dscale_dev = {scale, 1 / scale}):
 * what vtd_block64_train_backward leaves in dx_dev / dxscale_dev.  m = dpool (pool > 0); s = the channel sums of m in fp64 (at most 256
 * workgroups of consecutive pooled pixels, each four row quarters added as (q0 + q1) + (q2 + q3), the partials in workgroup order); dZ
 * [n hc wc][64] fp16 is gathered: a conv pixel takes m, times a power of two chosen from max |m| with a factor 4 of headroom, of each of its
 * 1, 2 or 4 windows whose idx names it.  G[c][q] = sum dZ[row][c] X[row][q] on v_mfma_f32_16x16x32_f16 with q = 32 ky + 4 kx + ci (224
 * columns, 147 kept), rows cut into min(512, ceil(rows / 1024)) slabs, summed in slab order in fp64.  grads->w = gamma rstd G, grads->beta = s,
 * grads->gamma = rstd (sum_k w G - mean s): nothing divides by gamma (grads->mean / var are ignored).  Gradients are written, not accumulated.
 * No atomics, shape-only grids: bitwise repeatable.  Errors: -3301 (argument / unsupported geometry), -3302 (alignment), before any launch. */
typedef struct vtd_stem_params {
    float *w, *gamma, *beta, *mean, *var;
} vtd_stem_params;
int vtd_stem_train_pack_input(const void* x_dev, int dtype, int n, int height, int width, void* tap_dev, vtd_stream stream);
int64_t vtd_stem_train_workspace_bytes(int n, int height, int width, int mode);
int vtd_stem_train_forward(const void* x_tap_dev, int n, int height, int width, const vtd_stem_params* params, float eps, void* workspace_dev,
                           void* pool_tap_dev, void* idx_dev, vtd_stream stream);
int vtd_stem_train_backward(const void* x_tap_dev, int n, int height, int width, const vtd_stem_params* params, float eps, const void* workspace_dev,
                            const void* pool_tap_dev, const void* idx_dev, const float* dpool_dev, const float* dscale_dev, const vtd_stem_params* grads,
                            void* scratch_dev, vtd_stream stream);

/* ---- The stem with batch-statistics BatchNorm (csrc/stem_train.hip, torch's train() mode): the stem joins the batch-statistics family of
 * vtd_trunk_bn_train_*, behind entries of its own because its tensors are the stem's (an image tap in, the pooled tap and the index bytes
 * out).  The arguments are those of vtd_stem_train_*, plus `training`, `momentum` and stats_dev.  training = 0 hands the call to
 * vtd_stem_train_forward / _backward: their bits, and nothing is written to the statistics.  The workspace query (mode 0 = the forward's
 * workspace, kept for the backward; mode 1 = the backward's scratch) answers at least vtd_stem_train_workspace_bytes, so either value of
 * `training` runs in one allocation.
 * vtd_stem_bn_train_forward, training = 1: the raw 7x7 weights are rounded to fp16 per call into the frozen path's fragment layout (no fold:
 * gamma rstd is not known yet, no bias); the convolution runs in the frozen forward's tiling (7 x 8 pooled pixels = 15 x 17 conv outputs
 * per workgroup on v_mfma_f32_16x16x32_f16) and writes its fp32 accumulators to z [n hc wc][64] in the workspace.  Neighbouring tiles share
 * one conv row and one conv column; a tile writes its local rows 1 .. 14 and columns 1 .. 16, so conv pixel (y, x) is written by tile
 * (y / 14, x / 16) alone.  The statistics of z over its M = n hc wc rows take the 64-wide order documented above for layer1: min(256,
 * ceil(M / 256)) workgroups of ceil(M / workgroups) consecutive rows, sixteen parts each joined by the balanced pairwise tree, (count,
 * mean, M2) combined by Chan's rule in workgroup order, all in fp64; the same pass takes each channel's minimum and maximum of z, from which
 * the backward has max |xh|.  params->mean and params->var are updated in place: mean <- (1 - momentum) mean + momentum mu, var <- (1 -
 * momentum) var + momentum sigma^2 M / (M - 1); the caller advances num_batches_tracked.  stats_dev (optional, float32 [2][64]) receives mu
 * and the biased sigma^2.  Then a = half(relu(((z - mu) rstd) gamma + beta)) is pooled 3x3/s2/p1 straight from z (a is not stored):
 * pool_tap_dev and idx_dev as vtd_stem_train_forward writes them, by the same rule -- the first maximum in (ky, kx) scan order, only in-image
 * positions, the byte unspecified where the pooled value is 0.
 * vtd_stem_bn_train_backward, training = 1: dpool_dev / dscale_dev as in vtd_stem_train_backward; m = dpool (pool > 0).  Every live pooled
 * element routes to exactly one conv position, so the sums over the conv map of g and g xh (g the gradient at the BatchNorm's output
 * behind the ReLU, xh = (z - mu) rstd) are s1 = sum m and s2 = sum m xh[the position idx names], taken at pooled resolution with z
 * gathered, in the row order of vtd_stem_train_backward's reduction (at most 256 workgroups of consecutive pooled pixels, four quarters as
 * (q0 + q1) + (q2 + q3), partials in workgroup order, fp64).  An element whose pooled value is 0 adds nothing and its byte is not decoded.
 * grads->beta = s1, grads->gamma = s2 (scale undone).  dZ [n hc wc][64] fp16 = gamma rstd (g - s1 / M - xh s2 / M) times a power of two,
 * M = n hc wc (the conv rows, not the pooled ones); g is gathered from the 1, 2 or 4 windows that hold the conv pixel and whose idx names
 * it, added in (py, px) order, nothing is scattered.  The power of two comes from the bound max_c |gamma rstd| (4 max |m| + |s1| / M + max
 * |xh| |s2| / M) under the block kernels' target 16384.  The weight-gradient kernel of vtd_stem_train_backward runs unchanged on this dZ with
 * the same slab rule; grads->w = G / scale: dZ carries gamma rstd, so no factor follows, and the result is exact for gamma = 0 and gamma <
 * 0 -- nothing divides by gamma or sigma.  Gradients are written, not accumulated (grads->mean / var are ignored).  z makes one round trip
 * through HBM per direction; the statistics are not fused into the convolution's epilogue.  No atomics, shape-only grids: bitwise repeatable.
 * Errors, before any launch: -3801 (a null pointer, odd or too small extents, eps <= 0, training outside {0, 1}, momentum outside [0, 1],
 * training = 1 with n hc wc < 2, a mode outside {0, 1} in the workspace query), -3802 (alignment). */
int64_t vtd_stem_bn_train_workspace_bytes(int n, int height, int width, int mode);
int vtd_stem_bn_train_forward(const void* x_tap_dev, int n, int height, int width, const vtd_stem_params* params, int training, float momentum, float eps,
                              void* workspace_dev, void* pool_tap_dev, void* idx_dev, float* stats_dev, vtd_stream stream);
int vtd_stem_bn_train_backward(const void* x_tap_dev, int n, int height, int width, const vtd_stem_params* params, int training, float eps,
                               const void* workspace_dev, const void* pool_tap_dev, const void* idx_dev, const float* dpool_dev, const float* dscale_dev,
                               const vtd_stem_params* grads, void* scratch_dev, vtd_stream stream);

/* ---- recogniser: CRNN (app/ml/models/text_recognizer.py:12-37,114-167) --------------------------- */
/* vocab_size = len(TextRecognizer.vocab) = 97 (text_recognizer.py:86-91); max_crops text regions per call. */
int vtd_recognizer_create(int vocab_size, int max_crops, vtd_recognizer** out);
void vtd_recognizer_destroy(vtd_recognizer* r);
/* One tensor of the CRNN checkpoint (text_recognizer.py:95-96): "cnn.N.*", "rnn.weight_ih_l0[_reverse]", ...,
 * "classifier.weight|bias"; float32, PyTorch memory order. */
int vtd_recognizer_set_tensor(vtd_recognizer* r, const char* key, const float* host_data, int64_t numel);
/* Build options, before finalize.  "fuse_pools" (default 1): the MaxPool2d((2,2)) / ((2,1)) layers behind conv2, conv4 and
 * conv6 + ReLU (text_recognizer.py:17-22) are taken in those convolutions' epilogues (the un-pooled maps are never written;
 * bit-identical results); 0 runs them as separate pool launches. */
int vtd_recognizer_set_option(vtd_recognizer* r, const char* name, int value);
int vtd_recognizer_finalize(vtd_recognizer* r, vtd_stream stream);
/* K6: for every box (frame, x1, y1, x2, y2) take frame[y1:y2, x1:x2] (pipeliine.py:121) out of frames_dev
 * ([n_frames,H,W,3] uint8 BGR) and cv2.resize it to 128x32 (text_recognizer.py:118), then run conv1.  boxes_dev is
 * [ncrops][5] int32 in device memory.  A box must name a frame in [0, n_frames) and lie inside it with x2 > x1, y2 > y1; any
 * other box yields an all-zero crop and nothing is read for it. */
int vtd_recognizer_crop_resize(vtd_recognizer* r, const uint8_t* frames_dev, int n_frames, int height, int width,
                               const int32_t* boxes_dev, int ncrops, vtd_stream stream);
/* Alternative input: the tensor the reference hands to CRNN.forward, [ncrops,3,32,128] float32 (text_recognizer.py:122). */
int vtd_recognizer_set_input_nchw(vtd_recognizer* r, const float* x_dev, int ncrops, vtd_stream stream);
/* CRNN.forward (text_recognizer.py:29-37) on the current input: logits_dev receives [ncrops,31,vocab] float32. */
int vtd_recognizer_forward(vtd_recognizer* r, int ncrops, float* logits_dev, vtd_stream stream);
/* Test taps as dense NCHW float32 on the host: "resized" ([n,32,128,3] uint8 values); the convolution stages, each behind
 * its BN + ReLU and (where the layer has one) its max-pool, in both fuse_pools modes: "conv1" ([n,64,16,64]), "conv2"
 * ([n,128,8,32]), "conv3" ([n,256,8,32]), "conv4" ([n,256,4,32]), "conv5" ([n,512,4,32]), "conv6" ([n,512,2,32]), "cnn"
 * (conv7, [n,512,1,31]); "h0", "h1" ([n,512,1,31]: LSTM layer outputs [n,31,512] seen as NCHW, forward units 0-255, reverse
 * units 256-511).  The hoisted input projections and the cell state have no tap.  Synchronises the stream. */
int vtd_recognizer_read_tap(vtd_recognizer* r, const char* name, int ncrops, float* host_out, int64_t capacity, vtd_stream stream);
int64_t vtd_recognizer_macs_per_crop(const vtd_recognizer* r);
/* Kernel-selection table of the recogniser (see vtd_detector_set_tuning); buckets are powers of two of the crop count. */
int vtd_recognizer_set_tuning(vtd_recognizer* r, const char* table_text);
int64_t vtd_recognizer_get_tuning(const vtd_recognizer* r, char* buf, int64_t capacity);
int vtd_recognizer_tuning_measured(const vtd_recognizer* r);
/* [softmax(dim=2) +] TextRecognizer._decode_prediction (text_recognizer.py:126,142-167) for n sequences of
 * dense [T,V] rows (T <= 128): apply_softmax=1 takes logits and fuses the softmax, 0 takes probabilities as
 * _decode_prediction itself does.  id2char_dev[V]: code point per class id or -1 for ids that emit nothing
 * ('<blank>', '<unk>').  out_dev: [n][2+T] int32 = length, float confidence bits, then the code points. */
int vtd_ctc_greedy_decode(const float* logits_dev, int n, int T, int V, const int32_t* id2char_dev, int blank_id, int apply_softmax,
                          int32_t* out_dev, vtd_stream stream);

/* ---- Transformer recogniser: TrOCR (app/ml/models/text_recognizer.py:39-69) ----------------------------------------------
 * TransformerRecognizer loads VisionEncoderDecoderModel "microsoft/trocr-base-printed" (ViT encoder + TrOCR decoder) and calls
 * generate(pixel_values, max_length=50).  The architecture is a parameter (the checkpoint's config.json values; defaults of the
 * Python binding restate trocr-base-printed), weights arrive by their transformers-4.36 state-dict keys. */
typedef struct vtd_trocr vtd_trocr;
typedef struct vtd_trocr_config {
    int32_t image_size, patch_size;                       /* 384, 16 */
    int32_t enc_hidden, enc_layers, enc_heads, enc_ffn;   /* 768, 12, 12, 3072; head width must be 64 */
    int32_t enc_qkv_bias;                                 /* 0 for the TrOCR checkpoints */
    float enc_ln_eps;                                     /* 1e-12 */
    int32_t dec_hidden, dec_layers, dec_heads, dec_ffn;   /* 1024, 12, 16, 4096 */
    int32_t vocab_size, max_positions;                    /* 50265, 512 */
    float dec_ln_eps;                                     /* 1e-5 */
    int32_t decoder_start_token_id, eos_token_id, pad_token_id; /* 2, 2, 1 */
    int32_t max_length;                                   /* 50: text_recognizer.py:58 */
} vtd_trocr_config;
int vtd_trocr_create(const vtd_trocr_config* cfg, int max_crops, vtd_trocr** out);
void vtd_trocr_destroy(vtd_trocr* t);
/* Build options, before finalize.
 * "slots" (1 or 2, default 1): encoder-output slots.  With 2, vtd_trocr_encode_*_slot(1) may run while slot 0 still waits for or runs its
 * decode (events inside the handle order the passes); the *_slot entry points reject slot indices >= the configured count.
 * "xattn" (default 1): the form of the decoder's cross-attention (TrOCRAttention with encoder_hidden_states, reached from
 * text_recognizer.py:58).  0 -- as the reference computes it: the encoder pass projects the encoder states E to keys and values per decoder
 * layer (K = E Wk^T + bk, V = E Wv^T + bv; 28 MB per crop and slot) and every decode step reads both.  1 -- the same attention with the two
 * linear projections moved across it: scores = (q_h Wk_h) . E[t] (the q . bk term is the same for every token and leaves the softmax),
 * context = (sum_t P[t] E[t]) Wv_h^T + bv (the probabilities sum to 1); the slot holds E itself (0.89 MB per crop), a decode step reads 0.89
 * instead of 2.36 MB per live row and layer, the encoder pass has 24 projections less.  Results agree within the tolerances the goldens are
 * held to and greedy ids are identical on them (tests/test_gpu_trocr.py).  Encoders wider than 768 channels or with more than 16 decoder
 * heads keep form 0 (vtd_trocr_get_option tells which one runs after finalize); 2 -- form 1 or -1106 at finalize. */
int vtd_trocr_set_option(vtd_trocr* t, const char* name, int value);
int vtd_trocr_get_option(const vtd_trocr* t, const char* name, int* value);
/* One tensor of VisionEncoderDecoderModel.state_dict() (text_recognizer.py:42): "encoder.embeddings.*",
 * "encoder.encoder.layer.N.*", "encoder.layernorm.*", "decoder.model.decoder.*", "decoder.output_projection.weight" (optional: tied to
 * embed_tokens when absent); "encoder.pooler.*" is accepted and ignored.  float32, PyTorch memory order. */
int vtd_trocr_set_tensor(vtd_trocr* t, const char* key, const float* host_data, int64_t numel);
int vtd_trocr_finalize(vtd_trocr* t, vtd_stream stream);
/* text_recognizer.py:48-55 for every box (frame, x1, y1, x2, y2) of frames_dev ([n_frames,H,W,3] uint8 BGR): crop, BGR->RGB,
 * TrOCRProcessor (Pillow bilinear resize to image_size^2, /255, (x-0.5)/0.5), then the ViT encoder and the decoder's cross-attention
 * keys / values.  boxes_host: [ncrops][5] int32 in HOST memory (the filter tables depend on the crop sizes). */
int vtd_trocr_encode_crops(vtd_trocr* t, const uint8_t* frames_dev, int n_frames, int height, int width, const int32_t* boxes_host, int ncrops,
                           vtd_stream stream);
/* Alternative input: the pixel_values tensor the reference hands to generate(), [ncrops,3,S,S] float32 (text_recognizer.py:55). */
int vtd_trocr_encode_pixels(vtd_trocr* t, const float* pixel_values_dev, int ncrops, vtd_stream stream);
/* generate(pixel_values, max_length) (text_recognizer.py:58), greedy: ids_dev [ncrops][max_length] int32 receives
 * decoder_start_token_id, the arg-max tokens up to and including <eos>, then pad_token_id.  logits_dev, if not NULL, receives the
 * logits of every step as [ncrops][max_length-1][vtd_trocr_logits_stride()] float32.  forced_ids_dev ([ncrops][forced_len], optional):
 * teacher forcing -- these tokens are fed instead of the arg-max (tensor-level tests).  Synchronises the stream now and then (to stop
 * once every row has finished). */
int vtd_trocr_generate(vtd_trocr* t, int ncrops, int max_length, const int32_t* forced_ids_dev, int forced_len, int32_t* ids_dev, float* logits_dev,
                       vtd_stream stream);
/* Test taps as float32 on the host: "pixel_values" [n,3,S,S], "encoder" (last_hidden_state) [n,tokens,enc_hidden]. */
/* Two encoder-output slots per handle (vtd_trocr_num_slots): the encoder pass of the next crop batch (ViT + the cross-attention keys /
 * values of all decoder layers, MFMA-bound) can run on one stream into slot 1 while the previous batch is decoded out of slot 0 on
 * another (latency- / HBM-bound): `*_slot` variants of the three calls above; the plain ones are slot 0.  The handle orders the passes
 * itself with events (an encoder pass waits for the decode that last read its slot and for the previous encoder pass; a decode waits for
 * its slot's encoder pass and for the previous decode), so callers only choose streams.  generate() stops computing a row once it has
 * emitted </s> (rows leave a compact live list; the ids equal those of generate(), which pads such rows) and returns when all but the
 * last two steps have run; vtd_trocr_last_steps = decoder steps the last call enqueued. */
int vtd_trocr_num_slots(const vtd_trocr* t);
int vtd_trocr_encode_crops_slot(vtd_trocr* t, int slot, const uint8_t* frames_dev, int n_frames, int height, int width, const int32_t* boxes_host,
                                int ncrops, vtd_stream stream);
int vtd_trocr_encode_pixels_slot(vtd_trocr* t, int slot, const float* pixel_values_dev, int ncrops, vtd_stream stream);
/* encode_crops in two halves, so that one encoder pass + decode can serve the crops of SEVERAL frame batches (their frame sizes may
 * differ): stage_crops runs the processor (text_recognizer.py:49-52) for the boxes of one resident frame batch into rows
 * [row_offset, row_offset + ncrops) of the slot, encode_staged runs the ViT encoder and the cross-attention keys / values over the first
 * ncrops staged rows.  The decode's cost per step is mostly fixed, so merged recogniser batches are much cheaper per crop. */
int vtd_trocr_stage_crops_slot(vtd_trocr* t, int slot, const uint8_t* frames_dev, int n_frames, int height, int width, const int32_t* boxes_host,
                               int ncrops, int row_offset, vtd_stream stream);
int vtd_trocr_encode_staged_slot(vtd_trocr* t, int slot, int ncrops, vtd_stream stream);
int vtd_trocr_generate_slot(vtd_trocr* t, int slot, int ncrops, int max_length, const int32_t* forced_ids_dev, int forced_len, int32_t* ids_dev,
                            float* logits_dev, vtd_stream stream);
int vtd_trocr_last_steps(const vtd_trocr* t);
/* Measurement hook (bench.py roofline of the Transformer line): mode bit 0 (value 1) brackets the cross-attention launch of decoder layer 0 of every
 * step with HIP events on the decode stream; get_profile returns their summed time, the number of launches and the summed row counts the
 * launches read (exact live-row counts), then resets.  While profiling is on, generate() waits for its own completion. */
int vtd_trocr_set_profiling(vtd_trocr* t, int mode);
int vtd_trocr_get_profile(vtd_trocr* t, double* total_ms, int64_t* launches, int64_t* row_launches, vtd_stream stream);
/* Mode bit 1 (value 2, may be or-ed with 1): every dense-GEMM launch of the encoder pass (the kernel with the largest share of the
 * Transformer recogniser's time) is bracketed with HIP events on its stream; returns summed time, launches and executed FLOPs (2 M N K). */
int vtd_trocr_get_gemm_profile(vtd_trocr* t, double* total_ms, int64_t* launches, double* total_flops, vtd_stream stream);
int vtd_trocr_read_tap(vtd_trocr* t, const char* name, int ncrops, float* host_out, int64_t capacity, vtd_stream stream);
int vtd_trocr_encoder_tokens(const vtd_trocr* t);
int vtd_trocr_logits_stride(const vtd_trocr* t);
int64_t vtd_trocr_macs_per_crop(const vtd_trocr* t);
/* Kernel-selection table (see vtd_detector_set_tuning). */
int vtd_trocr_set_tuning(vtd_trocr* t, const char* table_text);
int64_t vtd_trocr_get_tuning(const vtd_trocr* t, char* buf, int64_t capacity);
int vtd_trocr_tuning_measured(const vtd_trocr* t);

#ifdef __cplusplus
}
#endif
#endif /* VTD_H */
