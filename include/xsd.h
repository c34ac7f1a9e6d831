/*
 * xsd.h -- C ABI of the MI355X-native RRDB-generator engine (libxsd_hip.so).
 *
 * Drop-in boundary for the hot path of SamSweere/xmm-superres-denoise.  All pointers named
 * "dev" are device (HBM) pointers owned by the caller; the engine borrows them for the duration of a call and
 * launches asynchronously on the given hipStream_t (passed as void*; NULL = the null stream).  Every entry point
 * returns 0 on success or a negative xsd_status; xsd_last_error() returns a thread-local message.  No C++ types,
 * no torch types, never throws across the ABI.  One engine per process/GPU; calls on one engine are stream-ordered,
 * not thread-safe.
 *
 * Parameter vector layout ("flat params"): fp32, the reference's state_dict order, each tensor OIHW:
 *   conv_first.{weight,bias}, rrdb.{i}.RDB{r}.conv{c}.{weight,bias} (i<blocks, r=1..3, c=1..5), trunk_conv.*,
 *   conv_last.*, and for SR: upsampling.{3u}.* (u<num_upsample), HRconv.*
 *   (xmm_superres_denoise/models/modules/generator_rrdb.py:10-64,73-101; rrdb_blocks.py:23-32,60-64).
 * Images are NCHW fp32: x [B][in_channels][H][W], y [B][out_channels][sH][sW] (the shipped models have one channel: plain [B][H][W]).
 *
 * This file is also read by a program: xmm_superres_denoise/engine/_lib.py derives the Python (ctypes) binding from it at import,
 * after stripping comments and preprocessor lines.  The forms it accepts:
 *   - `typedef struct xsd_X xsd_X;` (an opaque handle) and enums: skipped;
 *   - `typedef struct xsd_X { ... } xsd_X;` with fields of the types below, fixed arrays of a literal length (`int32_t a[16]`) and several
 *     declarators of one scalar type per statement (`double x, y;`);
 *   - function declarations named xsd_*, over any number of lines, with named parameters of the types below or `(void)`, returning
 *     one of the scalars, void or `const char*`;
 *   - scalars: int, int32_t, int64_t, long long, float, double;
 *   - pointers of any depth and constness to any named type: a single pointer to a struct defined above its use becomes a typed pointer
 *     to the generated class, every other pointer (handles, `T**`, `const float* const*`, `void*`) an untyped address.
 * Anything else -- another scalar type, a struct by value, an array or function-pointer parameter, a nested struct, a global -- makes
 * the import fail and quote the declaration: extend the parser with the header, never around it.
 */
#ifndef XSD_H
#define XSD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xsd_engine xsd_engine;

enum xsd_status {
    XSD_OK = 0,
    XSD_ERR_ARG = -1,     /* bad argument / unsupported configuration */
    XSD_ERR_HIP = -2,     /* a HIP runtime call failed */
    XSD_ERR_STATE = -3,   /* call sequence error (e.g. backward without a saved forward) */
    XSD_ERR_NOMEM = -4    /* a device (or host) allocation failed -- in every create, every growth path and xsd_debug_stamps, whatever the family.  What the
                             call had allocated before is freed again; a create leaves *out as it was; a handle that could not grow
                             keeps no half-built state: its held shape and the refused one both work at the next call, with the
                             results of a fresh handle, and its destroy gives everything back (tests/test_hip_lifetime.py) */
};

enum xsd_kind { XSD_KIND_DN = 0, XSD_KIND_SR = 1 };

/* Mirrors the constructor arguments of GeneratorRRDB_DN / GeneratorRRDB_SR
 * (generator_rrdb.py:114-121 / :73-81) as mapped from RrdbCfg by Model.configure_model (models/model.py:157-186). */
typedef struct xsd_config {
    int32_t kind;          /* xsd_kind */
    int32_t in_channels;   /* 1..1024 (models.toml: 1).  DN: must equal out_channels or be 1 (`out + x`, generator_rrdb.py:134) */
    int32_t out_channels;  /* 1..1024 (models.toml: 1) */
    int32_t num_filters;   /* 1..1024 (models.toml: filters = 32).  up to 256 filters with up to 8 image channels in and out run on the
                              split-precision MFMA kernels (a feature tensor = 1..8 planes of 32 channels; widths that are no
                              multiple of 32 are zero-padded internally, the flat vectors keep the reference's layout); beyond
                              that the exact-fp32 kernels of csrc/generic_net.hip (xsd_set_math does not apply there) */
    int32_t num_res_blocks;/* >= 1 (models.toml: residual_blocks = 4) */
    int32_t num_upsample;  /* SR only: (hr_res/lr_res)/2, 1 or 2 */
    int32_t memory_efficient; /* rrdb_blocks.py:39-47 recompute policy; numerics identical. Enforced by the host (chunked recompute), not here */
    int32_t reserved;
} xsd_config;

const char* xsd_last_error(void);
const char* xsd_version(void);

/* replaces GeneratorRRDB_*.__init__ (engine state only; weights stay in the caller's flat buffer) */
int xsd_create(const xsd_config* cfg, xsd_engine** out);
void xsd_destroy(xsd_engine* e);
int64_t xsd_param_count(const xsd_engine* e);

/* Math mode of the MFMA convs (forward, input-gradient, weight-gradient).  Three modes, all carrying fp32 planes:
 * 0 = "fp32": exact fp32 on v_mfma_f32_32x32x2_f32 (bitwise an fp32 fma chain; 157 TFLOP/s peak).
 * 3 = "bf16x6" (strict): every fp32 operand is split EXACTLY into three bf16 terms (8+8+8 = fp32's 24 bits) and a product is
 *     six bf16 MFMA products (dropped terms <= 2^-23 relative); v_mfma_f32_32x32x16_bf16 sums its 16 products and the fp32
 *     accumulator exactly and rounds once.  Measured against float64 (tests/test_hip_precision.py, several seeds and sizes):
 *     error <= torch's fp32 CPU path and <= mode 0, forward and backward, on every tensor.
 * 4 = "f16x3" (default, the benchmark headline): every operand TENSOR is scaled by a power of two chosen from its max |x|
 *     (reported by the kernel that produced it) and split into two fp16 terms, x * s = h + l * 2^-11: 22-23 of fp32's 24
 *     significant bits per OPERAND (not 24); a product is three fp16 MFMA products, accumulation as in mode 3, the epilogue
 *     undoes the scales exactly.  What the tests hold it to, against float64: forward error <= torch fp32 and <= mode 0;
 *     backward (every parameter-gradient tensor and dL/dx) within 2x of torch's fp32 CPU path and within 1.25x of mode 0
 *     -- i.e. at the level of an fp32 fma chain, NOT below torch's blocked-summation kernel (measured 1.2-1.6x of it).  Three
 *     to four orders of magnitude inside the 1e-3 parity tolerance of the task; the label "fp32" without qualification
 *     belongs to modes 0 and 3 only.
 * (Modes 1 and 2 -- two-term bf16 splits with 16-bit significands -- existed in rounds 1-2 and were removed.)
 * Default: 4 (f16x3), or the environment variable XSD_MATH ("fp32" | "bf16x6" | "f16x3"; anything else fails xsd_create).
 * Changing it invalidates the packed weights and the plan.
 * XSD_MATH is the ONLY environment variable the production library (lib/libxsd_hip.so) reads.  Since round 6 the A/B switches and
 * test hooks below are compiled only into the test-hooks variant (make -C csrc hooks -> lib/libxsd_hip_hooks.so = the product's
 * objects with xsd_engine.hip built -DXSD_TEST_HOOKS; selected with XSD_LIB=<path>, as the diagnostic variant is) -- a shipped
 * library does not replan on an environment variable (tests/test_hip_network.py holds the product to that):
 *   XSD_WGRAD_BLOCK=0   the weight gradients of a dense block as one launch per G (five launches) instead of ONE pair-list launch
 *                       over its 15 (X, G) pairs (default 1; A/B switch, tools/ab_env.sh; tests hold the two forms to 2e-6);
 *   XSD_WGRAD_TAIL=0    no extra part on the CUs the block launch's 8 m x 15 workgroups leave (default 1; MI355X: a 17th part);
 *   XSD_TEST_NCU=n      plan the block launch as if the device had n compute units (n < 120: one launch per G);
 *   XSD_TEST_AMAX_CAP=n initial capacity of the max-|x| slot array (default 65536 floats), so that a small net exercises the
 *                       grow / copy / rebuild path a 256-filter x 64-block net would take.
 * Modes 3 and 4 address a plane's batch slice with 32-bit byte offsets: images of 2^24 or more output pixels are rejected
 * by xsd_forward (mode 0 takes them). */
int xsd_set_math(xsd_engine* e, int mode);
/* The mode the kernels of THIS engine compute in: the setting above on the plane kernels; 0 on the exact-fp32 path that serves
 * more than 256 filters / more than 8 image channels, whatever was set. */
int xsd_get_math(const xsd_engine* e);

/* Repack the caller's flat OIHW parameters into MFMA fragment-order panels (forward + transposed/flipped for the
 * input-gradient).  Must be called after every parameter update and before forward.  Replaces nothing in the
 * reference (torch reads OIHW directly); it is the engine's weight-layout step. */
int xsd_pack_weights(xsd_engine* e, const float* dev_params, void* stream);

/* replaces Model.forward = clamp(GeneratorRRDB_*.forward(x), 0, 1) (models/model.py:48-49;
 * generator_rrdb.py:66-69,103-110,130-137).  x: [B][in_channels][H][W]; y: [B][out_channels][sH][sW], s = 2^num_upsample (SR) or 1 (DN).
 * save_for_backward != 0 keeps every activation needed by xsd_backward (about 7.7 KB per LR pixel). */
int xsd_forward(xsd_engine* e, const float* dev_x, float* dev_y, int B, int H, int W, int save_for_backward, void* stream);

/* replaces torch autograd through the module for the last xsd_forward(save_for_backward=1):
 * dy: gradient wrt the (clamped) output y; dx_or_null: gradient wrt x; dev_grads: flat gradient vector in the flat-params
 * layout (overwritten, not accumulated). */
int xsd_backward(xsd_engine* e, const float* dev_dy, float* dev_dx_or_null, float* dev_grads, void* stream);

/* Data-parallel overlap support: the backward pass split into num_res_blocks + 2 stages, executed in order
 * stage 0 (output head + trunk_conv), stages 1..blocks (RRDB blocks-1 .. 0), stage blocks+1 (conv_first).
 * After stage s returns, the gradient ranges reported by xsd_grad_range(stage) are final on the stream, so the caller
 * can start their all-reduce on a side stream while later stages run. */
/* Several backwards after ONE forward (different dy) are allowed: stage 0 resets what the previous backward left. */
int xsd_backward_num_stages(const xsd_engine* e);
int xsd_backward_stage(xsd_engine* e, int stage, const float* dev_dy, float* dev_dx_or_null, float* dev_grads, void* stream);
int xsd_grad_range(const xsd_engine* e, int stage, int range_idx, int64_t* offset, int64_t* count); /* returns number of ranges */

/* mean-L1 loss (torchmetrics MeanAbsoluteError / F.l1_loss; utils/loss_functions.py:16): writes *dev_loss (float) and,
 * if dev_dy != NULL, d loss / d y = sign(y - t) / n. */
int xsd_l1_loss(xsd_engine* e, const float* dev_y, const float* dev_target, float* dev_dy_or_null, float* dev_loss,
                int64_t n, void* stream);

/* replaces create_loss + the per-batch Metric.forward of the composed loss (utils/loss_functions.py:11-47;
 * models/model.py:78; constants res/configs/loss_functions.toml:5-42).  w_* are the EFFECTIVE weights of the terms
 * (relative percentage x paper scaling; 0 = term absent), correction is added to the total when > 0
 * (loss_functions.py:44-45).  ssim / ms_ssim follow torchmetrics 1.x with gaussian_kernel=True: window
 * int(3.5*sigma+0.5)*2+1 taps, data_range from the images, k1/k2 as given, kernel_size only for the MS-SSIM size check
 * (the reference passes kernel_size=13, sigma=2.5, k2=0.05; k1 defaults to 0.01).  psnr/ssim/ms_ssim parity is unpinned
 * (torchmetrics absent here); see oracle/loss.py for the restated algorithm.
 * y, target: [B][H][W].  dev_out (XSD_LOSS_OUT = 12 device floats): [0] total, [1] l1, [2] poisson, [3] psnr, [4] ssim,
 * [5] ms_ssim (inactive terms 0), [6] mean squared error, [7] min(target), [8] max(target) (the last three when any of
 * l1 / poisson / psnr is active; they are the per-batch states the epoch-level metrics accumulate,
 * metrics/xmm_metric_collection.py:14-38), [9..11] reserved.  dev_dy_or_null receives d total / d y. */
#define XSD_LOSS_OUT 12
typedef struct xsd_loss_config {
    float w_l1, w_poisson, w_psnr, w_ssim, w_ms_ssim;
    float correction;
    float sigma, k1, k2;
    int32_t kernel_size;
} xsd_loss_config;
typedef struct xsd_loss_fn xsd_loss_fn;   /* the object create_loss returns; owns a device workspace */
int xsd_loss_create(const xsd_loss_config* cfg, xsd_loss_fn** out);
void xsd_loss_destroy(xsd_loss_fn* f);
int xsd_loss_eval(xsd_loss_fn* f, const float* dev_y, const float* dev_target, float* dev_dy_or_null, float* dev_out,
                  int B, int H, int W, void* stream);
/* Multi-channel images ([B][C][H][W] contiguous = B*C images of H x W): tell the loss how many consecutive images form one SAMPLE
 * (default 1).  Two terms reduce per sample, as the reference's metrics do: the Poisson term divides the element mean by the number
 * of samples (metrics/metrics.py:30-39: `self.total += preds.size()[0]`), and MS-SSIM averages every scale's statistic over a
 * sample's channels before the product over scales (torchmetrics: `.reshape(B, -1).mean(-1)` over C, H, W).  l1, psnr and ssim are
 * the same either way.  xsd_loss_eval then requires B to be a multiple of `channels`. */
int xsd_loss_set_channels(xsd_loss_fn* f, int channels);

/* The reference's extended test metrics (get_ext_metrics / get_in_ext_metrics, metrics/xmm_metric_collection.py:41-61,91-111;
 * metrics/metrics.py:42-101, every default, chromatic=False) on single-channel images in [0, 1]: piq 0.7.x gmsd, multi_scale_gmsd,
 * haarpsi (scales=3, subsample=True, c=30, alpha=4.2), mdsi (c1=140, c2=55, c3=550, combination="sum", alpha=0.6, rho=1, q=0.25,
 * o=0.25; the reference's key spells it "msdi") and torchmetrics 1.x VisualInformationFidelity(sigma_n_sq=2.0).  The formulas are
 * restated from the libraries' published code (tests/golden/ext_metrics_torch.py holds them in plain torch):
 * neither library is available to this project, so parity with the libraries themselves is unpinned, as for psnr / ssim / ms_ssim.
 * fsim is not part of this call: it has its own object, xsd_fsim below.
 * preds, target: [B][H][W] fp32; values outside [0, 1] are not checked.  dev_out: B x XSD_EXTM_OUT device DOUBLES, per image
 *   [0] gmsd   [1] ms_gmsd   [2] haarpsi   [3] mdsi   [4] vif numerator   [5] vif denominator   (vif_p = [4] / [5]; a constant
 *   target gives 0 / 0 as in torchmetrics).
 * Per-image values, not batch means: the caller does the reference's reductions (metrics/metrics.py:9-27).  The maps are fp32, every
 * sum over an image is carried in double in a fixed order: an image's six values are bitwise independent of its batch-mates and of
 * the run, and a NaN / inf pixel stays in its image.  A fixed number of launches (11) whatever B is.  The object owns a device
 * workspace sized at first use per (B, H, W), on the device that is current at that call.
 * Refused with XSD_ERR_ARG: null pointers, B < 1, H or W < 41 (VIF's 17-tap valid filter over four scales). */
#define XSD_EXTM_OUT 6
typedef struct xsd_ext_metrics xsd_ext_metrics;
int xsd_ext_metrics_create(xsd_ext_metrics** out);
void xsd_ext_metrics_destroy(xsd_ext_metrics* m);
int xsd_ext_metrics_eval(xsd_ext_metrics* m, const float* dev_preds, const float* dev_target, double* dev_out, int B, int H, int W,
                         void* stream);
/* Test entry, in the product library like xsd_loss_test_scale: after an xsd_ext_metrics_eval on the handle, copy ONE region of that
 * eval's workspace into dev_dst (device memory, dst_bytes long) on `stream` (the eval's stream, or one ordered after it).  The offsets
 * come from the same host function the eval lays its workspace out with.  Images (fp32, [B][h][w]; side 0 = preds, 1 = target):
 *   U1..U3  the pool2 chain (GMSD / MS-GMSD scales 1..3, HaarPSI's input)      M  MDSI's k x k mean      V1..V3  VIF's chain, scales 1..3.
 * Tile partials (doubles, [B][ntiles][entries]; `side` must still be 0 or 1 and is otherwise ignored), tiles in row-major order:
 *   GMS0..3   4 entries: sum g, sum g^2 (MS-GMSD form), sum g, sum g^2 (GMSD form; zeros except at scale 1); 4 x 64 tiles of the scale's map
 *   HAAR      2: sum sigmoid * weight, sum weight (both orientations); 4 x 64 tiles of U1
 *   MDSI1     2: sum re, sum im;    MDSI2   1: sum |z - mean z|; 4 x 64 tiles of M
 *   VIF0..3   2: numerator, denominator; 16 x 16 WINDOWS per tile of the scale's valid-window map.
 * info (8 host ints, filled whenever the handle, the stage and the side are accepted -- also when the buffer is then refused as too
 * small, so a caller can size it): [0] B  [1] rows  [2] columns of the image or of the map the tiles cover (windows for VIF)
 * [3] entries per tile (0: an image)  [4] tiles_x  [5] ntiles per image  [6] tile rows  [7] tile columns ([4..7] are 0 for images).
 * Refused with XSD_ERR_ARG: null pointers, an unknown stage or side, a buffer too small, a handle that has not evaluated. */
enum {
    XSD_EXTM_STAGE_U1 = 0, XSD_EXTM_STAGE_U2, XSD_EXTM_STAGE_U3, XSD_EXTM_STAGE_M, XSD_EXTM_STAGE_V1, XSD_EXTM_STAGE_V2, XSD_EXTM_STAGE_V3,
    XSD_EXTM_STAGE_GMS0, XSD_EXTM_STAGE_GMS1, XSD_EXTM_STAGE_GMS2, XSD_EXTM_STAGE_GMS3, XSD_EXTM_STAGE_HAAR, XSD_EXTM_STAGE_MDSI1,
    XSD_EXTM_STAGE_MDSI2, XSD_EXTM_STAGE_VIF0, XSD_EXTM_STAGE_VIF1, XSD_EXTM_STAGE_VIF2, XSD_EXTM_STAGE_VIF3, XSD_EXTM_STAGES
};
int xsd_ext_metrics_test_stage(xsd_ext_metrics* m, int stage, int side, void* dev_dst, int64_t dst_bytes, int* info, void* stream);

/* The sixth extended test metric: piq 0.7.x fsim(x, y, chromatic=False) with every default (data_range=1, scales=4, orientations=4,
 * min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2, k=2.0) on single-channel images in [0, 1], restated from piq's published code
 * (tests/golden/fsim_torch.py holds it in plain torch): parity with piq itself is unpinned.  csrc/fsim.hip.
 * preds, target: [B][1][H][W] fp32.  dev_out: B device DOUBLES, one fsim value per image (per-image values, not the batch mean: the caller
 * does the reference's reduction).  A pair without structure (sum of pc_max = 0, e.g. two all-zero images) gives NaN (0 / 0) as written.
 * The images are pooled by ks = max(1, round_half_even(min(H, W) / 256)) to h x w = H / ks x W / ks (remainder dropped); what depends on
 * (h, w) only -- the 16 log-Gabor filters, their noise constants, the two DFT matrices, all computed in double -- is a plan kept with the
 * object; it holds the XSD_FSIM_PLANS most recently used sizes, so calls of two sizes can alternate without rebuilding.  The 2-D
 * transforms are dense products with the DFT matrices (any length: no factorisation), accumulated in double; filter responses are stored
 * fp32, every map and sum after them is double, summed in a fixed order without atomics: an image's value is bitwise independent of its
 * batch-mates, of B and of the run, and a NaN / inf pixel makes its own image's value non-finite and no other's.  A fixed number of
 * launches (9) whatever B is.  The workspace is sized at first use per (B, h, w) on the device that is current at that call: about
 * 1008 h w bytes per image pair (the 32 inverse column transforms kept as complex doubles are 512 h w of them, the 32 fp32 responses
 * 256 h w), i.e. 77 MB per pair at 277 x 277 and 157 + 78 MB for those two arrays at B = 4; it grows linearly with B and is never
 * shrunk.  A workspace that cannot be allocated is refused with XSD_ERR_NOMEM before anything is enqueued.
 * Refused with XSD_ERR_ARG and a message naming the limit: null pointers, B < 1 or > 2047, C != 1, a pooled side < 3 or > 1024. */
#define XSD_FSIM_PLANS 4
typedef struct xsd_fsim xsd_fsim;
int xsd_fsim_create(xsd_fsim** out);
void xsd_fsim_destroy(xsd_fsim* m);
int xsd_fsim_eval(xsd_fsim* m, const float* dev_preds, const float* dev_target, double* dev_out, int B, int C, int H, int W, void* stream);
/* Test entries, in the product library like xsd_sw_test_gemm.  test_dft2: the 2-D transform of xsd_fsim_eval alone, on B complex
 * n1 x n2 arrays (interleaved re, im fp32; 3 <= n1, n2 <= 1024): forward (inverse = 0, no scaling) or inverse (1 / (n1 n2)), as
 * torch.fft.fft2 / ifft2; every output element is written.  test_median: per row of n fp32 values the element torch.median picks (the
 * lower of the two middle ones for even n), by radix select on the values' bit patterns; a row that holds a NaN gives NaN.  The keys
 * order -0.0 below +0.0, which torch.median treats as equal: on a row that mixes the two the zero returned may carry the other sign
 * (the engine's own rows are squares, never negative). */
int xsd_fsim_test_dft2(xsd_fsim* m, const float* dev_in, float* dev_out, int B, int n1, int n2, int inverse, void* stream);
int xsd_fsim_test_median(const float* dev_in, float* dev_out, int rows, int n, void* stream);
/* test_stage: after an xsd_fsim_eval on the handle, copy ONE region of that eval's workspace, or of the plan it used, into dev_dst
 * (device memory, dst_bytes long) on `stream`; the offsets come from the host function the eval lays its workspace out with.
 * sb = s * B + image, s = 0 preds, 1 target; NO = 4 orientations, NF = 16 filters (index o * 4 + scale):
 *   POOLED  double [2B][h][w]          EO    float (re, im) [2B][NF][h][w]      EN, AN  double [2B][NO][h][w]
 *   A0SQ    float [2B][NO][h][w]       T     double [2B][NO]                    PART    double [B][ntiles][2], 4 x 64 tiles, row-major
 *   FILT    double [NF][h][w] (plan)   NOISE double [3][NO]: em_n, sum_an2, sum_ai_aj (plan).
 * info (8 host ints, filled whenever the handle and the stage are accepted, also when the buffer is then refused as too small):
 * [0] the leading count (2B, B, NF or 3)  [1] h  [2] w  [3] entries per tile (PART: 2, else 0)  [4] tiles_x  [5] ntiles  [6] tile rows
 * [7] tile columns ([4..7] are 0 except for PART).
 * Refused with XSD_ERR_ARG: null pointers, an unknown stage, a buffer too small, a handle that has not evaluated (or whose plan of that
 * eval has since been evicted by XSD_FSIM_PLANS other sizes). */
enum {
    XSD_FSIM_STAGE_POOLED = 0, XSD_FSIM_STAGE_EO, XSD_FSIM_STAGE_EN, XSD_FSIM_STAGE_AN, XSD_FSIM_STAGE_A0SQ, XSD_FSIM_STAGE_T,
    XSD_FSIM_STAGE_PART, XSD_FSIM_STAGE_FILT, XSD_FSIM_STAGE_NOISE, XSD_FSIM_STAGES
};
int xsd_fsim_test_stage(xsd_fsim* m, int stage, void* dev_dst, int64_t dst_bytes, int* info, void* stream);

/* torch.optim.Adam(lr, betas, eps=1e-8) single fused step over flat buffers (models/model.py:241-245).
 * step is 1-based; grad_scale multiplies the gradient on read (1/world_size for data-parallel mean). */
int xsd_adam_step(xsd_engine* e, float* dev_params, const float* dev_grads, float* dev_m, float* dev_v, int64_t n,
                  int step, float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);

/* Input pipeline: counts (int32 or fp32, [B][Hin][Win]) * detector mask (uint8 {0,1} [Hin][Win] or NULL)
 * -> centred zero pad / crop to [B][res][res] -> optional Normalize.normalize_image(max_val, stretch)
 * (data/dataset.py:41-47; data/tools.py:103-126; transforms/normalize.py:66-82).
 * stretch: 0 linear, 1 sqrt, 2 asinh, 3 log.  do_normalize = 0 returns the masked, padded counts (bit-exact). */
int xsd_mask_pad_normalize(const void* dev_counts, int counts_is_int32, const uint8_t* dev_mask_or_null, float* dev_out,
                           int B, int Hin, int Win, int res, int do_normalize, float max_val, int stretch, void* stream);
/* Whole sample composition of XmmDataset (data/dataset.py:24-49 + :267-268) in one kernel, straight from FITS payload
 * words: img (+ agn) (+ background) summed in fp32 like load_fits' float images, * detector mask, optional nearest
 * upsample x s with / s^2 (ImageUpsample, dataset.py:44-45), centred pad / crop to res, optional normalize.
 * is_int32: BITPIX 32 counts (else IEEE float32); big_endian != 0: words are in FITS byte order (byte-swapped on load),
 * so a primary HDU's data block can be copied to the device unmodified.  Bit-exact when do_normalize = 0. */
int xsd_compose_input(const void* dev_img, const void* dev_agn_or_null, const void* dev_bkg_or_null, int is_int32, int big_endian,
                      const uint8_t* dev_mask_or_null, float* dev_out, int B, int Hin, int Win, int upsample, int res,
                      int do_normalize, float max_val, int stretch, void* stream);
/* Batched xsd_compose_input from a device pool of FITS data blocks (XmmDataset.load_sample + __getitem__, data/dataset.py:24-49,
 * :237-268; transforms/normalize.py:66-82; transforms/imageupsample.py:10-26; data/tools.py:103-126).  dev_pool holds n_slots
 * equal slots of slot_elems words (>= Hin x Win), each one file's primary-HDU data block: BITPIX 32 (is_int32) or -32 words, in
 * FITS byte order when big_endian != 0.  Sample b: out[b] = normalize(pad(upsample(mask * ((pool[img_idx[b]] + pool[agn_idx[b]])
 * + pool[bkg_idx[b]])))), the arithmetic of xsd_compose_input, so the two are bitwise equal.  The index arrays are HOST arrays of
 * B int32 (-1 in agn / bkg = absent for that sample; a NULL array = absent for all): they are checked here before anything is
 * launched (an index outside [0, n_slots) is XSD_ERR_ARG naming the sample) and travel in the kernel's argument block, so a
 * batch needs no device index buffer.  One launch per 128 samples; no cross-sample work, so a sample's bits do not depend on
 * its batch. */
int xsd_compose_batch(const void* dev_pool, int is_int32, int big_endian, int64_t slot_elems, int64_t n_slots,
                      const int32_t* img_idx, const int32_t* agn_idx_or_null, const int32_t* bkg_idx_or_null,
                      const uint8_t* dev_mask_or_null, float* dev_out, int B, int Hin, int Win, int upsample, int res,
                      int do_normalize, float max_val, int stretch, void* stream);
/* Normalize.normalize_image (inverse = 0) / denormalize_image (inverse = 1), max_val > 0 (transforms/normalize.py:66-92) */
int xsd_normalize(const float* dev_in, float* dev_out, int64_t n, float max_val, int stretch, int inverse, void* stream);
/* ImageUpsample: nearest x scale then / scale^2 (transforms/imageupsample.py:10-26); in [N][H][W] */
int xsd_image_upsample(const float* dev_in, float* dev_out, int N, int H, int W, int scale, void* stream);

/* ---- Restormer denoiser, forward only (csrc/restormer.hip) ---------------------------------------------------
 * The reference's Restormer (models/transformer/restormer.py:217-406; factory models/model.py:226-234, XMM configuration
 * res/configs/models.toml:58-64: dim = 24, 1 -> 1 channels).  Exact fp32 on the vector ALUs; xsd_set_math does not apply.
 * Reductions over an image (the channel attention's row norms and Gram) are fixed-order partial sums: outputs are bitwise
 * reproducible and each image's output is independent of the batch it is computed in.  No backward: training Restormer is not
 * on this engine.
 * Flat parameter layout: fp32, the reference's state_dict order (patch_embed.proj.weight, encoder_level1.{i}.{norm1.body.weight,
 * norm1.body.bias, attn.temperature, attn.qkv.*, attn.qkv_dwconv.*, attn.project_out.*, norm2.*, ffn.project_in.*, ffn.dwconv.*,
 * ffn.project_out.*}, down1_2.body.0.weight, ..., output.weight[, output.bias]; biases of the convs only when bias != 0,
 * norm*.body.bias only for WithBias). */
typedef struct xsd_restormer xsd_restormer;
typedef struct xsd_restormer_config {   /* Restormer.__init__ arguments (restormer.py:218-230) */
    int32_t inp_channels;          /* 1..1024 */
    int32_t out_channels;          /* must equal inp_channels: `output(x) + inp_img` (:404) */
    int32_t dim;                   /* even, 2..1024 (Downsample halves it, :188) */
    int32_t num_blocks[4];         /* 0..64 each */
    int32_t num_refinement_blocks; /* 0..64 */
    int32_t heads[4];              /* heads[l] divides dim * 2^l (heads[0] also 2 dim) into at most 128 channels per head */
    int32_t bias;                  /* 0/1: conv biases */
    int32_t layernorm_bias_free;   /* 0 = "WithBias", 1 = "BiasFree" (:61-73) */
    int32_t dual_pixel_task;       /* must be 0 (refused) */
    double ffn_expansion_factor;   /* hidden width of a level with C channels = (int)(C * factor) (:82) */
} xsd_restormer_config;
/* replaces Restormer.__init__ (engine state only; weights stay in the caller's flat buffer) */
int xsd_restormer_create(const xsd_restormer_config* cfg, xsd_restormer** out);
void xsd_restormer_destroy(xsd_restormer* r);
int64_t xsd_restormer_param_count(const xsd_restormer* r);
/* the engine's weight-layout step (1x1 conv weights transposed to [cin][cout]); after every parameter update, before forward.
 * The engine keeps reading dev_params (LayerNorm, temperature, depthwise and 3x3 weights, biases) until the next pack. */
int xsd_restormer_pack_weights(xsd_restormer* r, const float* dev_params, void* stream);
/* replaces Restormer.forward (restormer.py:368-406; no clamp there -- Model.forward clamps, models/model.py:48-49).
 * x: [B][inp_channels][H][W], y: [B][out_channels][H][W], H and W divisible by 8 (three PixelUnshuffle(2) levels), B >= 1.
 * A workspace that cannot fit is refused with XSD_ERR_NOMEM before anything is enqueued. */
int xsd_restormer_forward(xsd_restormer* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream);
/* The Restormer kernels on their own (tests).  Each runs the launch helper the forward runs, allocates its own scratch, refuses a shape
 * outside its kernel's limits with XSD_ERR_ARG before any launch, and synchronises the stream.  All tensors NCHW fp32, B <= 65535 (the
 * images are the grid's z), H W <= 2^28.
 * The 1x1 conv: x [B][>= cin][HW] with a batch stride of xbs floats (>= cin HW: the first cin channels of a wider slab are read),
 * y likewise with ybs and cout; dev_w [cout][cin] as a Conv2d stores it, or with per_image set [B][cout][cin], one matrix per image
 * (the call transposes it to the [cin][cout] the kernel reads); dev_bias [cout] or NULL; ln 0 none, 1 WithBias, 2 BiasFree LayerNorm over
 * the cin channels of each pixel in front (dev_lnw [cin], dev_lnb [cin], the latter unused by 2); with residual set y += conv(x) in place,
 * else y = conv(x).  cin, cout <= 131072. */
int xsd_restormer_test_pw(const float* dev_x, int64_t xbs, const float* dev_w, int per_image, const float* dev_bias, int ln, const float* dev_lnw,
                          const float* dev_lnb, int residual, float* dev_y, int64_t ybs, int B, int cin, int cout, int64_t HW, void* stream);
/* The depthwise 3x3 conv, zero padding 1, any H, W >= 1.  gate 0: x [B][cout][H][W], dev_w [cout][9], dev_bias [cout] or NULL ->
 * y [B][cout][H][W].  gate 1: x [B][2 cout][H][W], dev_w [2 cout][9], dev_bias [2 cout] or NULL -> y = gelu(x1) * x2 of the two
 * halves of the conv's channels (exact-erf GELU).  cout <= 65535. */
int xsd_restormer_test_dw(const float* dev_x, const float* dev_w, const float* dev_bias, float* dev_y, int B, int cout, int gate, int H, int W,
                          void* stream);
/* The channel attention behind the depthwise conv (restormer.py:126-139): qkv [B][3 C][HW], temperature [heads], dev_wpo [C][C] and
 * dev_bpo [C] or NULL project_out as stored; x [B][C][HW] in place: x += project_out(softmax(normalize(q) normalize(k)^T temperature) v).
 * heads divides C into at most 64 channels per head, C <= 8192: what the forward runs up to that width. */
int xsd_restormer_test_attention(const float* dev_qkv, const float* dev_temperature, const float* dev_wpo, const float* dev_bpo, float* dev_x, int B,
                                 int C, int heads, int64_t HW, void* stream);
/* The same contract through the wide kernels, which the forward runs from 65 to 128 channels per head: here at any width in [1, 128]
 * (up to 64 the result is bitwise that of xsd_restormer_test_attention). */
int xsd_restormer_test_attention_wide(const float* dev_qkv, const float* dev_temperature, const float* dev_wpo, const float* dev_bpo, float* dev_x,
                                      int B, int C, int heads, int64_t HW, void* stream);
/* The dense 3x3 conv, zero padding 1: x [B][cin][H][W], dev_w [cout][cin][3][3], dev_bias [cout] or NULL, any H, W >= 1.
 * mode 0: y [B][cout][H][W] (+ dev_skip [B][cout][H][W] unless NULL); mode 1: y = PixelUnshuffle(2) of it, [B][4 cout][H/2][W/2], H and W
 * even; mode 2: y = PixelShuffle(2) of it, [B][cout/4][2 H][2 W], cout a multiple of 4.  dev_skip must be NULL in modes 1 and 2. */
int xsd_restormer_test_conv3(const float* dev_x, const float* dev_w, const float* dev_bias, const float* dev_skip, float* dev_y, int B, int cin,
                             int cout, int H, int W, int mode, void* stream);

/* ---- SwinFIR super-resolution, forward only (csrc/swinfir.hip) ----------------------------------------------
 * The reference's SwinFIR (models/transformer/swinfir.py:120-441 with the Swin blocks of modules.py; factory models/model.py:187-200,
 * XMM configuration res/configs/models.toml [swinfir]: img_size 416, patch_size 32, window_size 16 -> an effective window of 13 without
 * shift, embed_dim 180, 6 x 6 blocks of 6 heads, in_chans 1, upscale 2).  Eval-mode forward in exact fp32: the linear layers, the
 * window attention and the 3x3 convs on the fp32 MFMA, the FourierUnit's FFTs on the vector ALUs.  xsd_set_math and XSD_MATH do not
 * apply; xsd_swinfir_set_math below switches the linear layers and the 3x3 convs (nothing else) to the strict bf16x6 split.  No
 * float atomics: outputs are bitwise reproducible and each image's output is independent of the batch it is computed in.
 * Flat parameter layout: fp32, the order of SwinFIR.parameters() (conv_first.*, patch_embed.norm.* (patch_norm), per layer i and
 * block j layers.i.residual_group.blocks.j.{norm1.*, attn.relative_position_bias_table, attn.qkv.weight[, .bias], attn.proj.*, norm2.*,
 * mlp.fc1.*, mlp.fc2.*}, then layers.i.conv.* (SFB: S.body.0, S.body.2, F.conv1.0, F.fu.conv_layer, F.conv2, fusion; 1conv: the conv),
 * norm.*, conv_after_body.*, conv_before_upsample.0.*, upsample.{0,2,..}.*, conv_last.*).  The buffers relative_position_index and
 * attn_mask are not in it: the engine computes both from the configuration. */
typedef struct xsd_swinfir xsd_swinfir;
typedef struct xsd_swinfir_config {   /* SwinFIR.__init__ arguments (swinfir.py:291-313) */
    int32_t img_size[2];           /* (H, W); with patch_size it sets the effective window: min(img // patch) if <= window_size */
    int32_t patch_size[2];
    int32_t in_chans;              /* 1..64 (3: the reference subtracts its RGB mean) */
    int32_t embed_dim;             /* 2..4096 */
    int32_t num_layers;            /* 0..16 */
    int32_t depths[16];            /* 0..64 each */
    int32_t num_heads[16];         /* divides embed_dim into at most 32 channels per head */
    int32_t window_size;           /* the effective window must be <= 16 */
    int32_t qkv_bias;              /* 0/1 */
    int32_t ape;                   /* must be 0 (refused) */
    int32_t patch_norm;            /* 0/1 */
    int32_t upscale;               /* 2, 3, 4, 8 */
    int32_t upsampler;             /* 0 = "pixelshuffle" (the only one supported); 1 "pixelshuffledirect", 2 "nearest+conv", 3 "" are refused */
    int32_t resi_connection;       /* 0 = "SFB", 1 = "1conv"; 2 "HSFB", 3 "identity" are refused */
    double mlp_ratio;              /* hidden width (int)(embed_dim * mlp_ratio) */
    double qk_scale;               /* 0: head_dim^-0.5 (the reference's `qk_scale or ...`); > 0 as given; < 0 refused */
    double img_range;              /* > 0 */
} xsd_swinfir_config;
/* replaces SwinFIR.__init__ (engine state only; weights stay in the caller's flat buffer) */
int xsd_swinfir_create(const xsd_swinfir_config* cfg, xsd_swinfir** out);
void xsd_swinfir_destroy(xsd_swinfir* r);
int64_t xsd_swinfir_param_count(const xsd_swinfir* r);
/* the engine's weight-layout step (Linear / conv weights to [taps][cin][cout]); after every parameter update, before forward.
 * The engine keeps reading dev_params (LayerNorms, bias tables, biases) until the next pack. */
int xsd_swinfir_pack_weights(xsd_swinfir* r, const float* dev_params, void* stream);
/* replaces SwinFIR.forward (swinfir.py:420-441; no clamp there -- Model.forward clamps, models/model.py:48-49).
 * x: [B][in_chans][H][W], y: [B][in_chans][upscale H][upscale W]; H and W multiples of the effective window and, with SFB, FFT sizes
 * (<= 4096, prime factors <= 13).  A workspace that cannot fit is refused with XSD_ERR_NOMEM before anything is enqueued. */
int xsd_swinfir_forward(xsd_swinfir* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream);
/* Math mode of the engine's GEMMs -- every Linear, 1x1 and 3x3 conv of the forward (csrc/sw_gemm_s3x.h) -- in the mode numbers of
 * xsd_set_math: 0 = "fp32" (default; these engines do not read XSD_MATH) and 3 = "bf16x6": both operands split exactly into three bf16
 * terms, the six products hh, hm, mh, hl, lh, mm on v_mfma_f32_32x32x16_bf16, fp32 accumulation (hh apart from the five small ones).
 * Window attention, LayerNorm and the FFT stay exact fp32 in every mode.  4 ("f16x3") is refused with XSD_ERR_ARG: its fp16 terms need
 * a per-tensor scale that these kernels do not publish; any other number is refused with the list of modes.  May be called at any
 * time and in any order: the mode holds from the next forward, and nothing but the usual xsd_swinfir_pack_weights is asked of the
 * caller (the bf16 planes of the weights are made from dev_params at the first forward after a pack or a switch to bf16x6, so
 * dev_params must still hold what was packed).  nparams and the flat layout do not depend on the mode.  Outputs stay bitwise
 * reproducible and independent of the batch.  One limit of bf16x6: an fp32 value above bf16's largest finite value (3.39e38)
 * splits to inf, which makes the output of ITS image non-finite. */
int xsd_swinfir_set_math(xsd_swinfir* r, int mode);
int xsd_swinfir_get_math(const xsd_swinfir* r);
/* 1 if the FourierUnit's FFT takes a length of n, else 0 */
int xsd_swinfir_fft_supported(int n);
/* the FourierUnit's transform pair on its own: x [B][H][W][C2] (token-major real) -> spec [B][H][W/2+1][2 C2] (re, im interleaved)
 * = rfftn(x, norm="ortho"); with inverse set, x += irfftn(spec, s=(H, W), norm="ortho") and spec is overwritten. */
int xsd_swinfir_test_fft(xsd_swinfir* r, float* dev_x, float* dev_spec, int B, int H, int W, int C2, int inverse, void* stream);

/* The GEMM that SwinFIR and HAT share, on its own (tests): y = act(A W^T + bias), written token-major with a row pitch of ldy >= N floats
 * (only the B H W x N results are written).  conv3 = 0: A is [B H W][cin] token rows and dev_w [N][cin] as a Linear stores it;
 * conv3 = 1: A is a token-major image [B][H W][cin], dev_w [N][cin][3][3] as a Conv2d stores it, zero padding 1.  The call packs the
 * weights itself.  dev_bias [N] or NULL; act 0 none, 1 GELU (exact erf), 2 LeakyReLU(slope); math 0 (fp32) or 3 (bf16x6).  Synchronises
 * the stream. */
int xsd_sw_test_gemm(const float* dev_a, const float* dev_w, const float* dev_bias, float* dev_y, int conv3, int B, int H, int W, int cin,
                     int N, int64_t ldy, int act, float slope, int math, void* stream);
/* One launch of the same GEMM described as the forwards describe theirs (tests): the views, the residual and the store modes that
 * xsd_sw_test_gemm leaves out.  Every pointer is a device pointer.  The call packs the weights itself, fills the kernel's parameters
 * through the helpers the forwards use plus the field assignments they make, launches in `math` and synchronises the stream.  The
 * caller sizes the buffers; an inconsistent description is refused with XSD_ERR_ARG and a message that names the field. */
typedef struct xsd_sw_gemm_view {
    int32_t conv3;                 /* 0: token rows, M = B H W of them; 1: 3x3 conv (zero padding 1) over B images of H x W */
    int32_t B, H, W, cin, N;
    const float* a;                /* token-major rows of pitch lda >= cin floats (conv3: lda = cin), or with a_nchw (conv3 only) [B][cin][H][W] */
    int32_t a_nchw;
    int64_t lda;
    const float* imean;            /* conv3 only, [cin] or NULL: the conv reads (x - imean[ci]) * irange inside the image, 0 outside */
    float irange;
    const float* w;                /* [N][cin] (Linear) or [N][cin][3][3] (Conv2d) */
    const float* bias;             /* [N] or NULL */
    int32_t act;                   /* 0 none, 1 GELU (exact erf), 2 LeakyReLU(slope) */
    float slope;
    const float* res;              /* NULL, or + res[b rbs + p rps + n] after the activation (image b, row p of it, column n); may be y itself.
                                    * Token rows are one image: rbs must be 0 there. */
    int64_t rbs, rps;
    int32_t omode;                 /* 0 token-major y[row ldy + n], ldy >= N; 1 PixelShuffle(r) into the token-major r H x r W image of N / r^2
                                    * channels (conv3 only); 2 NCHW [B][N][H][W] = v / orange + omean[n] (conv3 only); 3 see below */
    float* y;
    int64_t ldy;
    int32_t r;
    const float* omean;            /* [N] (omode 2) or [N / r^2] (omode 3) */
    float orange;
    int32_t math;                  /* 0 fp32, 3 bf16x6 */
    /* xsd_swinir_test_gemm_view only; xsd_sw_test_gemm_view refuses a non-zero value in any of them */
    int32_t rnchw;                 /* the residual is NCHW: res[b rbs + n H W + p] */
    int32_t cH, cW;                /* omode 2: store only rows < cH and columns < cW, as [B][N][cH][cW] (both 0: no crop).  omode 3: PixelShuffle(r)
                                    * of the N columns, v / orange + omean[ch], into [B][N / r^2][cH][cW], the crop of r H x r W (both required) */
    int32_t up2;                   /* conv3 only: the conv runs over the nearest-2x upsampling of the H x W input, which is never made: 4 B H W
                                    * output rows, and H and W of the residual, the store and the crop are 2 H and 2 W */
} xsd_sw_gemm_view;
int xsd_sw_test_gemm_view(const xsd_sw_gemm_view* view, void* stream);
/* The shifted-window attention that SwinFIR and HAT share, on its own (tests; modules.py:115-140 between the qkv Linear and proj, with the
 * roll, window partition and reverse of :316-340): qkv [B][H W][3 C] token rows in image order (q, k, v; head h at channels h hd .. of
 * each), table [(2 ws - 1)^2][heads] the relative-position bias -> out [B][H W][C] in image order.  With shift > 0 the windows are
 * those of the image rolled by -shift and the -100 mask of the run-time size applies.  1 <= ws <= 16, H and W multiples of ws,
 * 0 <= shift < ws, heads divides C into at most 32 channels per head.  Synchronises the stream. */
int xsd_sw_test_attention(const float* dev_qkv, const float* dev_table, float* dev_out, int B, int H, int W, int C, int heads, int ws, int shift,
                          float scale, void* stream);
/* The token LayerNorm of both networks on its own (tests): x [M][C] -> y [M][C] = (x - mean) / sqrt(var + 1e-5) * w + b over the C
 * channels of each row (biased variance), w and b [C]; 1 <= C <= 4096, 1 <= M <= 2^31.  Synchronises the stream. */
int xsd_sw_test_layernorm(const float* dev_x, const float* dev_w, const float* dev_b, float* dev_y, int64_t M, int C, void* stream);

/* ---- HAT super-resolution, forward only (csrc/hat.hip) ------------------------------------------------------
 * The reference's HAT (models/transformer/hat.py:10-913; factory models/model.py:216-229, XMM configuration res/configs/models.toml
 * [hat]: img_size 416, patch_size 16, window_size 16, embed_dim 180, 6 groups of 6 HABs + 1 OCAB with 6 heads, in_chans 1, upscale 2,
 * overlap_ratio 0.5 -> 24 x 24 keys per 16 x 16 window).  Eval-mode forward in exact fp32 on SwinFIR's kernels (GEMM / conv3x3, window
 * attention, LayerNorm) plus the overlapping cross-attention, the channel attention and the HAB combine.  xsd_set_math and XSD_MATH do
 * not apply; xsd_hat_set_math below switches the linear layers and the 3x3 convs (nothing else) to the strict bf16x6 split.
 * No float atomics: outputs are bitwise reproducible and each image's output is independent of the batch it is computed in.
 * Flat parameter layout: fp32, the order of HAT.parameters() (conv_first.*, patch_embed.norm.* (patch_norm), per layer i:
 * layers.i.residual_group.blocks.j.{norm1.*, attn.relative_position_bias_table, attn.qkv.weight[, .bias], attn.proj.*,
 * conv_block.cab.0.*, conv_block.cab.2.*, conv_block.cab.3.attention.1.*, conv_block.cab.3.attention.3.*, norm2.*, mlp.fc1.*, mlp.fc2.*},
 * layers.i.residual_group.overlap_attn.{relative_position_bias_table, norm1.*, qkv.weight[, .bias], proj.*, norm2.*, mlp.fc1.*,
 * mlp.fc2.*}, layers.i.conv.* ("1conv"); then norm.*, conv_after_body.* ("1conv"), conv_before_upsample.0.*, upsample.{0,2,..}.*,
 * conv_last.*).  The buffers relative_position_index_SA / _OCA are not in it: the engine computes both indices, and the shift mask of
 * the run-time size, from the configuration. */
typedef struct xsd_hat xsd_hat;
typedef struct xsd_hat_config {       /* HAT.__init__ arguments (hat.py:642-669) */
    int32_t img_size[2];           /* (H, W); min(img // patch) must be >= window_size; equal: no block shifts (hat.py:186-189) */
    int32_t patch_size[2];
    int32_t in_chans;              /* 1..64 (3: the reference subtracts its RGB mean, hat.py:680-684) */
    int32_t embed_dim;             /* 2..4096 */
    int32_t num_layers;            /* 0..16 */
    int32_t depths[16];            /* 0..64 each */
    int32_t num_heads[16];         /* divides embed_dim into at most 32 channels per head */
    int32_t window_size;           /* <= 16 */
    int32_t compress_ratio;        /* CAB: embed_dim // compress_ratio >= 1 */
    int32_t squeeze_factor;        /* ChannelAttention: embed_dim // squeeze_factor >= 1 */
    int32_t qkv_bias;              /* 0/1 */
    int32_t ape;                   /* must be 0 (refused) */
    int32_t patch_norm;            /* 0/1 */
    int32_t upscale;               /* 2, 3, 4, 8 */
    int32_t upsampler;             /* 0 = "pixelshuffle" (the only one supported); 1 "pixelshuffledirect", 2 "nearest+conv", 3 "" are refused */
    int32_t resi_connection;       /* 0 = "1conv", 1 = "identity"; anything else (2) is refused */
    double mlp_ratio;              /* hidden width (int)(embed_dim * mlp_ratio), of the HABs and the OCABs */
    double qk_scale;               /* 0: head_dim^-0.5 (the reference's `qk_scale or ...`); > 0 as given; < 0 refused */
    double img_range;              /* > 0 */
    double conv_scale;             /* weight of the CAB branch (hat.py:268) */
    double overlap_ratio;          /* overlap window = window_size + (int)(window_size * overlap_ratio): the added part even, the window <= 32 */
} xsd_hat_config;
/* replaces HAT.__init__ (engine state only; weights stay in the caller's flat buffer) */
int xsd_hat_create(const xsd_hat_config* cfg, xsd_hat** out);
void xsd_hat_destroy(xsd_hat* r);
int64_t xsd_hat_param_count(const xsd_hat* r);
/* the engine's weight-layout step (Linear / conv weights to [taps][cin][cout]); after every parameter update, before forward.
 * The engine keeps reading dev_params (LayerNorms, bias tables, biases, the squeeze MLP's 1x1 weights) until the next pack. */
int xsd_hat_pack_weights(xsd_hat* r, const float* dev_params, void* stream);
/* replaces HAT.forward (hat.py:900-913 with forward_features :875-898, RHAG :603-611, AttenBlocks :493-507, HAB :220-271, OCAB :326-396,
 * CAB / ChannelAttention :27-44; no clamp there -- Model.forward clamps, models/model.py:48-49).
 * x: [B][in_chans][H][W], y: [B][in_chans][upscale H][upscale W]; H and W multiples of window_size (the reference does not pad).
 * A workspace that cannot fit is refused with XSD_ERR_NOMEM before anything is enqueued. */
int xsd_hat_forward(xsd_hat* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream);
/* Math mode of the engine's GEMMs (linear layers, CAB convs, conv_first, the group convs, the upsampling tail): exactly
 * xsd_swinfir_set_math above.  The window attention, the overlapping cross-attention, LayerNorm and the channel attention stay exact
 * fp32 in every mode. */
int xsd_hat_set_math(xsd_hat* r, int mode);
int xsd_hat_get_math(const xsd_hat* r);
/* the OCAB's attention on its own (hat.py:334-391 between the qkv Linear and proj): qkv [B][H W][3 C] token rows, table
 * [(ws + ow - 1)^2][heads] -> out [B][H W][C]; ws <= 16, ws <= ow <= 32, ow - ws even. */
int xsd_hat_test_ocab(const float* dev_qkv, const float* dev_table, float* dev_out, int B, int H, int W, int C, int heads, int ws, int ow,
                      float scale, void* stream);
/* the channel attention's AdaptiveAvgPool2d(1) on its own (hat.py:20): x [B][HW][C] token-major -> mean [B][C]; synchronises the stream */
int xsd_hat_test_channel_mean(const float* dev_x, float* dev_mean, int B, int64_t HW, int C, void* stream);
/* what a HAB does with its CAB branch, on its own (tests; hat.py:20-29, :268): x and t [B][HW][C] token-major, dev_w1 [Cs][C], dev_b1
 * [Cs], dev_w2 [C][Cs], dev_b2 [C] the squeeze MLP's 1x1 convs as stored: y[b] = sigmoid(w2 relu(w1 mean_p(t[b]) + b1) + b2), then
 * x += (t * y[b]) * scale in place; dev_y [B][C] receives the gates unless NULL.  With dev_w1 NULL (then dev_y must be NULL and the other
 * weights and Cs are ignored): the plain x += t * scale of the "identity" branches.  B <= 65535, HW <= 2^28, C and Cs in [1, 4096].
 * Synchronises the stream. */
int xsd_hat_test_ca_combine(float* dev_x, const float* dev_t, const float* dev_w1, const float* dev_b1, const float* dev_w2, const float* dev_b2,
                            float scale, int B, int64_t HW, int C, int Cs, float* dev_y, void* stream);

/* ---- SwinIR restoration / super-resolution, forward only (csrc/swinir.hip) ----------------------------------
 * The reference's SwinIR (models/transformer/swinir.py:133-395 with the Swin blocks of modules.py; exported by models/transformer but
 * with no factory entry and no models.toml name).  Eval-mode forward in exact fp32 on SwinFIR's kernels (GEMM / conv3x3, window attention,
 * LayerNorm, the per-block launch sequence), with all four reconstruction heads and both resi_connection forms.  Unlike SwinFIR and HAT
 * it takes ANY image size: H and W are reflect-padded on the right and bottom to multiples of window_size and the output is cropped
 * back (check_image_size, swinir.py:328-333, :395).  No float atomics: outputs are bitwise reproducible and each image's output is
 * independent of the batch it is computed in; a NaN stays in its image.
 * Flat parameter layout: fp32, the order of SwinIR.parameters(): conv_first.*, patch_embed.norm.* (patch_norm), per layer i and block j
 * layers.i.residual_group.blocks.j.{norm1.*, attn.relative_position_bias_table, attn.qkv.weight[, .bias], attn.proj.*, norm2.*, mlp.fc1.*,
 * mlp.fc2.*}, then layers.i.conv.* ("1conv") or layers.i.conv.{0,2,4}.* ("3conv"); norm.*; conv_after_body.* or conv_after_body.{0,2,4}.*;
 * then the head -- "pixelshuffle": conv_before_upsample.0.*, upsample.{0,2,..}.*, conv_last.*; "pixelshuffledirect": upsample.0.*;
 * "nearest+conv": conv_before_upsample.0.*, conv_up1.*, conv_up2.* (upscale 4 only), conv_hr.*, conv_last.*; "": conv_last.*.  The buffers
 * relative_position_index and attn_mask are not in it: the engine computes both from the configuration and the run-time size. */
typedef struct xsd_swinir xsd_swinir;
typedef struct xsd_swinir_config {    /* SwinIR.__init__ arguments (swinir.py:161-184) */
    int32_t img_size[2];           /* (H, W); with patch_size it sets the effective window: min(img // patch) if <= window_size, and then no
                                      block shifts (SwinTransformerBlock.__init__, modules.py:236-239) */
    int32_t patch_size[2];
    int32_t in_chans;              /* 1..64 (3: the reference subtracts its RGB mean, swinir.py:190-194) */
    int32_t embed_dim;             /* 2..4096; >= 4 with "3conv" */
    int32_t num_layers;            /* 0..16 */
    int32_t depths[16];            /* 0..64 each */
    int32_t num_heads[16];         /* divides embed_dim into at most 32 channels per head */
    int32_t window_size;           /* the pad goes to multiples of this; the effective window must be <= 16 */
    int32_t qkv_bias;              /* 0/1 */
    int32_t ape;                   /* must be 0 (refused) */
    int32_t patch_norm;            /* 0/1 */
    int32_t upscale;               /* 1, 2, 3, 4, 8; "nearest+conv": 2 or 4 */
    int32_t upsampler;             /* 0 = "pixelshuffle", 1 = "pixelshuffledirect", 2 = "nearest+conv", 3 = "" (denoising: x + conv_last(res)) */
    int32_t resi_connection;       /* 0 = "1conv", 1 = "3conv" */
    double mlp_ratio;              /* hidden width (int)(embed_dim * mlp_ratio) */
    double qk_scale;               /* 0: head_dim^-0.5 (the reference's `qk_scale or ...`); > 0 as given; < 0 refused */
    double img_range;              /* > 0 */
} xsd_swinir_config;
/* replaces SwinIR.__init__ (swinir.py:161-318; engine state only, weights stay in the caller's flat buffer).  Refused with XSD_ERR_ARG
 * and a message that names the argument: ape, an effective window > 16, a head dim > 32, embed_dim < 4 with "3conv", "nearest+conv" with
 * an upscale other than 2 or 4 (the reference's output size would disagree with upscale), an upscale outside {1, 2, 3, 4, 8}. */
int xsd_swinir_create(const xsd_swinir_config* cfg, xsd_swinir** out);
void xsd_swinir_destroy(xsd_swinir* r);
int64_t xsd_swinir_param_count(const xsd_swinir* r);
/* the engine's weight-layout step, as xsd_swinfir_pack_weights: after every parameter update, before forward */
int xsd_swinir_pack_weights(xsd_swinir* r, const float* dev_params, void* stream);
/* replaces SwinIR.forward (swinir.py:350-395 with check_image_size :328-333, forward_features :335-348, RSTB.forward :114-120,
 * UpsampleOneStep modules.py:398-415; Model.forward's clamp is not part of it).  x: [B][in_chans][H][W], any H and W >= 1;
 * y: [B][in_chans][Ho][Wo] contiguous, (Ho, Wo) = xsd_swinir_out_size.  Refused with XSD_ERR_ARG before anything is enqueued: a pad that
 * is not smaller than the image (F.pad's reflect raises there), and a padded size that is no multiple of the effective window (when
 * img_size // patch_size clamped it; the reference fails in window_partition).  A workspace that cannot fit: XSD_ERR_NOMEM. */
int xsd_swinir_forward(xsd_swinir* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream);
/* the size of forward's output for an H x W input: x[:, :, :H * upscale, :W * upscale] (swinir.py:395) of what the head produced */
int xsd_swinir_out_size(const xsd_swinir* r, int H, int W, int* Ho, int* Wo);
/* Math mode of the engine's GEMMs: exactly xsd_swinfir_set_math above (0 = "fp32", 3 = "bf16x6"; 4, "f16x3", is refused by name) */
int xsd_swinir_set_math(xsd_swinir* r, int mode);
int xsd_swinir_get_math(const xsd_swinir* r);
/* check_image_size and the input affine on their own (tests; swinir.py:328-333, :355): x [B][C][H][W] -> y [B][C][Hp][Wp] =
 * (F.pad(x, (0, Wp - W, 0, Hp - H), "reflect") - mean) * img_range, Hp and Wp the multiples of ws; every element of y is written.
 * mean: C floats in HOST memory, or NULL for zeros.  Synchronises the stream. */
int xsd_swinir_test_pad(const float* dev_x, float* dev_y, int B, int C, int H, int W, int ws, const float* mean, float img_range, void* stream);
/* conv_up1 / conv_up2 with their activation on their own (tests; swinir.py:373-385): a [B][H W][cin] token-major, dev_w [N][cin][3][3],
 * dev_bias [N] or NULL -> y [B][4 H W][N] token-major = LeakyReLU_slope(conv3x3(nearest2x(a))), zero padding 1 at the 2 H x 2 W extent;
 * the upsampled image is never stored.  math 0 (fp32) or 3 (bf16x6).  Synchronises the stream. */
int xsd_swinir_test_nearest_conv(const float* dev_a, const float* dev_w, const float* dev_bias, float* dev_y, int B, int H, int W, int cin, int N,
                                 float slope, int math, void* stream);
/* xsd_sw_test_gemm_view on SwinIR's instance of the GEMM, which takes the last four fields of the view too and adds the bias inside its
 * double sum (one rounding to fp32). */
int xsd_swinir_test_gemm_view(const xsd_sw_gemm_view* view, void* stream);

/* ---- differentiable Swin ops (csrc/sw_ops.hip) ----------------------------------------------------------------
 * The four operations of the Swin-family engines (the GEMM as a Linear and as a 3x3 conv, the token LayerNorm, the shifted-window
 * attention) with one forward and one backward entry each, for torch.autograd.Functions that compose a trainable network in Python
 * (xmm_superres_denoise/ops.py; models/modules/swinir_train.py).  The forwards of layer_norm and window_attention run the kernels of
 * xsd_sw_test_layernorm / _attention with the same arguments (the same bits); linear and conv3x3 run a kernel of their own that carries
 * the whole sum over K and the bias in double and rounds once (within a few ulp of xsd_sw_test_gemm; csrc/sw_ops.hip says why).
 * Unlike those hooks every entry here is ASYNCHRONOUS on `stream` (no synchronisation) and allocates
 * nothing: `scratch` is a device buffer of at least the bytes the matching *_scratch query returns (-1 with xsd_last_error for a refused
 * shape), free to reuse once the call's work on the stream is done.  fp32 only: math 0; 3 ("bf16x6") is refused by name.  Exact fp32
 * products, sums over K / tokens / pixels in double, no float atomics, every reduction in a fixed order: results are bitwise
 * reproducible, and da / dx / dqkv of an image do not depend on the batch it shares.  Weights are taken as torch stores them and packed
 * per call.  act: 0 none, 1 GELU (exact erf), 2 LeakyReLU(slope).
 *
 * linear: y [M][N] = act(a [M][K] w[N][K]^T + bias [N] or NULL).  With dev_z (and act != 0) the pre-activation is stored there and
 * y = act(z) by the epilogue's own expression (the same bits); the backward of an activated op needs it.  backward: dev_dy [M][N] ->
 * dev_da [M][K], dev_dw [N][K], dev_db [N]; each may be NULL (not computed).  `chunk`: token rows per weight-gradient partial (0: chosen
 * by the library; the partials are summed in ascending order); the same value goes to the scratch query.  M <= 2^28, K and N <= 65536. */
int64_t xsd_sw_op_linear_scratch(int64_t M, int K, int N, int act, int64_t chunk, int backward);
int xsd_sw_op_linear_forward(const float* dev_a, const float* dev_w, const float* dev_bias, float* dev_y, float* dev_z, int64_t M, int K, int N,
                             int act, float slope, int math, void* scratch, int64_t scratch_bytes, void* stream);
int xsd_sw_op_linear_backward(const float* dev_dy, const float* dev_a, const float* dev_w, const float* dev_z, float* dev_da, float* dev_dw,
                              float* dev_db, int64_t M, int K, int N, int act, float slope, int math, int64_t chunk, void* scratch,
                              int64_t scratch_bytes, void* stream);
/* conv3x3: x [B][H][W][cin] token-major, w [N][cin][3][3], zero padding 1 -> y [B][H][W][N]; otherwise as linear (dw per tap:
 * sum over p of x[p + off(tap)][ci] dy[p][co] inside the image; dx: the same conv of dy with the weight flipped and transposed). */
int64_t xsd_sw_op_conv3x3_scratch(int B, int H, int W, int cin, int N, int act, int64_t chunk, int backward);
int xsd_sw_op_conv3x3_forward(const float* dev_x, const float* dev_w, const float* dev_bias, float* dev_y, float* dev_z, int B, int H, int W,
                              int cin, int N, int act, float slope, int math, void* scratch, int64_t scratch_bytes, void* stream);
int xsd_sw_op_conv3x3_backward(const float* dev_dy, const float* dev_x, const float* dev_w, const float* dev_z, float* dev_dx, float* dev_dw,
                               float* dev_db, int B, int H, int W, int cin, int N, int act, float slope, int math, int64_t chunk, void* scratch,
                               int64_t scratch_bytes, void* stream);
/* layer_norm: as xsd_sw_test_layernorm.  backward: dx [M][C] (or NULL), dw and db [C] (both or neither); the statistics are recomputed
 * from x in double.  1 <= C <= 4096; the weight gradient takes M <= 65535 * 128 rows. */
int xsd_sw_op_layernorm_forward(const float* dev_x, const float* dev_w, const float* dev_b, float* dev_y, int64_t M, int C, void* stream);
int64_t xsd_sw_op_layernorm_scratch(int64_t M, int C);
int xsd_sw_op_layernorm_backward(const float* dev_dy, const float* dev_x, const float* dev_w, float* dev_dx, float* dev_dw, float* dev_db,
                                 int64_t M, int C, void* scratch, int64_t scratch_bytes, void* stream);
/* window_attention: as xsd_sw_test_attention (same limits).  backward: dev_dout [B][H W][C] -> dev_dqkv [B][H W][3 C] (every element
 * written) and dev_dtable [(2 ws - 1)^2][heads].  The probabilities are recomputed from qkv; the table gradient is one partial per
 * (window, head) in scratch, summed in a fixed order. */
int xsd_sw_op_attention_forward(const float* dev_qkv, const float* dev_table, float* dev_out, int B, int H, int W, int C, int heads, int ws,
                                int shift, float scale, void* stream);
int64_t xsd_sw_op_attention_scratch(int B, int H, int W, int C, int heads, int ws);
int xsd_sw_op_attention_backward(const float* dev_dout, const float* dev_qkv, const float* dev_table, float* dev_dqkv, float* dev_dtable, int B,
                                 int H, int W, int C, int heads, int ws, int shift, float scale, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- differentiable HAT ops (csrc/hat_ops.hip) ----------------------------------------------------------------
 * The two operations a trainable HAT needs on top of the differentiable Swin ops above (xmm_superres_denoise/ops.py:
 * overlap_attention, channel_attention; models/modules/hat_train.py), under the same rules: every entry is asynchronous on `stream`,
 * allocates nothing (`scratch`: at least the bytes of the matching *_scratch query, which returns -1 with xsd_last_error for a refused
 * shape), fp32 with sums in double, no float atomics, every reduction in a fixed order (bitwise reproducible), and every element of
 * every output is written.  Refusals (null pointers, shapes out of range, a scratch too small) name the op and come before anything
 * is enqueued.
 *
 * overlap_attention: the OCAB's attention, the kernel and the arguments of xsd_hat_test_ocab (the same bits; the same limits: 1 <= ws
 * <= 16, ws <= ow <= 32, ow - ws even, at most 32 channels per head, H and W multiples of ws).  backward: dev_dout [B][H W][C] and the
 * forward's dev_out -> dev_dqkv [B][H W][3 C] and dev_dtable [(ws + ow - 1)^2][heads].  The probabilities are recomputed from qkv.  dk
 * and dv leave as one slab per window in scratch and are summed per token over the windows that hold it, in ascending window order;
 * the table gradient is one partial per (window, head), summed in a fixed order; a negative index lands in the bin the forward reads;
 * keys outside the image get no dk / dv and do count in the table gradient.  B H W C <= 2^37.
 * Scratch bytes, each term rounded up to a multiple of 256, with nwin = B (H / ws) (W / ws):
 *   4 nwin ow^2 2 C   +   4 nwin (ws + ow - 1)^2 heads. */
int xsd_hat_op_ocab_forward(const float* dev_qkv, const float* dev_table, float* dev_out, int B, int H, int W, int C, int heads, int ws, int ow,
                            float scale, void* stream);
int64_t xsd_hat_op_ocab_scratch(int B, int H, int W, int C, int heads, int ws, int ow);
int xsd_hat_op_ocab_backward(const float* dev_dout, const float* dev_qkv, const float* dev_table, const float* dev_out, float* dev_dqkv,
                             float* dev_dtable, int B, int H, int W, int C, int heads, int ws, int ow, float scale, void* scratch,
                             int64_t scratch_bytes, void* stream);
/* channel_attention: t [B][HW][C] token-major, dev_w1 [Cs][C], dev_b1 [Cs], dev_w2 [C][Cs], dev_b2 [C] the squeeze MLP's 1x1 convs as
 * stored -> dev_gates [B][C] (or NULL: kept in scratch) = sigmoid(w2 relu(w1 mean_p(t[b]) + b1) + b2), bitwise the dev_y of xsd_hat_test_ca_combine, and
 * dev_y [B][HW][C] = t * gates[b].  backward: dev_dy and t -> dev_dt [B][HW][C] = dy g + dmean / HW, dev_dw1, dev_db1, dev_dw2, dev_db2
 * (per-image partials summed over the images in ascending order).  The mean, the hidden vector and the gate are recomputed from t in
 * double: the forward's fp32 gates are not an input (their rounding would go straight into dt).
 * B <= 65535, HW <= 2^28, C and Cs in [1, 4096], B HW C <= 2^38.
 * Scratch bytes, each term rounded up to a multiple of 256, with chunks = ceil(HW / 256):
 *   forward   8 B chunks C   +   4 B C
 *   backward  8 B chunks 2 C   +   8 B (3 C + Cs)   +   8 B (2 Cs C + Cs + C). */
int xsd_hat_op_ca_forward(const float* dev_t, const float* dev_w1, const float* dev_b1, const float* dev_w2, const float* dev_b2, float* dev_y,
                          float* dev_gates, int B, int64_t HW, int C, int Cs, void* scratch, int64_t scratch_bytes, void* stream);
int64_t xsd_hat_op_ca_scratch(int B, int64_t HW, int C, int Cs, int backward);
int xsd_hat_op_ca_backward(const float* dev_dy, const float* dev_t, const float* dev_w1, const float* dev_b1, const float* dev_w2,
                           const float* dev_b2, float* dev_dt, float* dev_dw1, float* dev_db1, float* dev_dw2, float* dev_db2,
                           int B, int64_t HW, int C, int Cs, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- measurement / test hooks ------------------------------------------------------------------------------- */
/* Per-kernel-class HIP-event timing of the kernels launched by this engine (bench.py roofline block), with each launch's
 * ALGORITHMIC flop and bytes (SURVEY.md 8d counting rule: every operand once).  MFMA-bound classes: 0 = conv (forward +
 * input-gradient), 1 = weight gradient.  HBM-bound classes (round 6): 2 = edge_expand (conv_first forward, conv_last input-gradient:
 * 1 -> 32 channels), 3 = edge_reduce (conv_last forward + skip + clamp, conv_first input-gradient: 32 -> 1), 4 = edge_wgrad
 * (weight gradients of the two edge layers), 5 = xsd_l1_loss, 6 = xsd_adam_step, 7 = clamp backward, 8 = max-|x| sweeps of
 * planes no producer reported (f16x3).  enable resets the counters; unknown classes read as zero launches. */
int xsd_profile_enable(xsd_engine* e, int enable);
int xsd_profile_read(xsd_engine* e, int klass, double* total_ms, int64_t* launches, double* total_flop, double* total_bytes);

/* What the matrix pipes of the current device SUSTAIN on the conv kernels' own MFMA stream (csrc/mfma_stream_probe.hip): eight
 * waves per CU issuing the v_mfma_f32_32x32x16_{f16 (fmt 0), bf16 (fmt 1)} sequence of one conv half-step with its LDS fragment
 * reads, on realistic split operands, no staging, no global traffic -- for `seconds` (0 < seconds <= 30) of back-to-back
 * launches; reported over the second half (the package-power governor has settled by then): dense 16-bit MFMA TFLOP/s and the
 * in-kernel shader clock in GHz (sclk_ghz may be NULL).  bench.py's `roofline.sustained_peak` = this rate / products per
 * multiply, measured in the bench process on the bench's device.  Blocks the host until done. */
int xsd_probe_mfma_stream(int fmt, double seconds, double* mfma_tflops, double* sclk_ghz, void* stream);

/* Diagnostic only: accumulated shader-cycle stamps of the kernels' phases (32 slots; read with enable = 0).  Conv:
 * [0] prologue, [1] prefetch issue, [2] MFMA loop, [3] epilogue, [4] wait+barrier, [5] split+LDS write+barrier, [6] items,
 * [7] s_memrealtime ticks, [8..12] staging wave, [13..15] youngest MFMA wave; weight gradient: [16] staging rounds,
 * [17] MFMA walk, [18] MFMA wave at the barrier, [19] staging wave at the barrier, [21] tiles. */
int xsd_debug_stamps(xsd_engine* e, int enable, unsigned long long* out32);
/* Diagnostic only (pure host arithmetic, no device needed): the number of workgroups a persistent split-mode conv launch over `ntiles`
 * tiles uses on a device of `ncu` compute units (csrc/xsd_kernels.h: persistent_grid -- `ntiles` when ntiles <= ncu; with
 * rounds = ceil(ntiles / ncu), the balanced grid ceil(ntiles / rounds) when rounds <= 8; otherwise the full grid, `ncu`). */
int xsd_debug_persistent_grid(int ntiles, int ncu);
/* Diagnostic only: hipOccupancyMaxActiveBlocksPerMultiprocessor of the split forward conv kernel at a dynamic LDS size. */
int xsd_debug_occupancy(int lds_bytes);
/* Diagnostic only: wall time (ms) of a grid of `grid` workgroups that each sleep `us` microseconds holding `lds_bytes` of LDS
 * (a census of how many such workgroups are resident at once). */
float xsd_debug_residency_ms(int grid, int threads, int lds_bytes, int us);

/* Every xsd_test_* / xsd_loss_test_* entry from here on is defined in csrc/xsd_test_entries.hip, one object in the product and the
 * test-hooks library alike, and calls the functions the engine calls (csrc/xsd_engine_impl.h).
 * Single-layer entry points used by the kernel-level parity tests (one 3x3 conv over NHWC 32-channel planes).
 * dev_in: [n_in] plane pointers on the host (each plane [B][H][W][32]); w_oihw: device OIHW [32*n_out][32*n_in][3][3]. */
int xsd_test_conv3x3(xsd_engine* e, const float* const* host_in_planes, int n_in, const float* dev_w_oihw, const float* dev_bias,
                     float* const* host_out_planes, int n_out, float slope, int B, int H, int W, void* stream);
int xsd_test_conv3x3_bwd(xsd_engine* e, const float* const* host_in_planes, int n_in, const float* dev_w_oihw,
                         const float* dev_g_plane, float* const* host_dx_planes, float* dev_dw_oihw, float* dev_db,
                         int B, int H, int W, void* stream);

/* One output chunk (32 channels) of xsd_test_conv3x3_ex and its fused epilogue, in the kernels' order:
 *   v = conv + bias; v *= a1; if (accumulate) v += p; if (e1) v += s1 * e1; v *= a2; if (e2) v += s2 * e2; if (e3) v += s3 * e3;
 *   v = v > 0 ? v : v * slope; if (mask) v = mask > 0 ? v : v * mslope; p = v
 * e1, e2, e3, mask: device planes [B][H][W][32] or NULL.  bits_out (split math modes): receives the compact mask of the stored values,
 * one 16-bit word per pixel and lane half h, [B][H][W][2]: bit 4q + t <-> channel 8q + 4h + t is > 0.  bits_in (with mask): such words,
 * read instead of the mask plane. */
typedef struct xsd_test_out {
    float* p;
    const float* e1;
    const float* e2;
    const float* e3;
    const float* mask;
    float a1, s1, a2, s2, s3, slope, mslope;
    int accumulate;
    unsigned short* bits_out;
    const unsigned short* bits_in;
} xsd_test_out;
/* One conv launch of the engine's math mode with a caller-supplied epilogue per output chunk (kernel-level tests; synchronous).
 * Inputs: n_in planes [B][H][W][32] (host array of device pointers), or with shuffle_in != 0 ONE plane [B][2H][2W][32] in host_in_planes[0]
 * read as its four sub-pixel views (n_in must be 4; view n = 2i + j holds pixels (2y + i, 2x + j)).  Outputs: n_out chunks (n_in > 1 and
 * n_out > 1 exclude each other, both <= 5), or with shuffle_out != 0 the four sub-pixel views of ONE plane [B][2H][2W][32], outs[0].p
 * (n_out must be 4; the other fields are still per chunk).  dev_w_oihw: [32 n_out][32 n_in][3][3], chunk j = output channels 32j .. 32j + 31;
 * dev_bias: [32 n_out] or NULL.  host_amax11 (or NULL): in math mode f16x3 receives the launch's max-|x| slots -- [0..4] the input planes or
 * views, [5] the packed weights, [6..10] the output chunks (zeroed before the launch) -- and zeros in the other modes.
 * A launch the kernel's launcher refuses returns XSD_ERR_HIP and writes nothing. */
int xsd_test_conv3x3_ex(xsd_engine* e, const float* const* host_in_planes, int n_in, int shuffle_in, const float* dev_w_oihw,
                        const float* dev_bias, const xsd_test_out* host_outs, int n_out, int shuffle_out, float* host_amax11,
                        int B, int H, int W, void* stream);
/* One weight-gradient launch over the n_in x n_g rectangle of (X, G) plane pairs plus its fixed-order reduction into dev_dw_oihw
 * [cout_total][cin_total][3][3] and dev_db [cout_total] (kernel-level tests; synchronous; the number of partial sums follows the plan's rule).
 * G: n_g planes [B][H][W][32], or with shuffle_g != 0 ONE plane [B][2H][2W][32] in host_g_planes[0] read as its four sub-pixel views
 * (n_g must be 4).  The launch writes input channels 32 j0 .. 32 (j0 + n_in) - 1 of output channels 32 (n0 + n) + co, or with shuffle != 0
 * (n_g = 4) of output channels 4 (32 plane + co) + n; everything is multiplied by `scale`.  Refused with XSD_ERR_ARG: n_in > 5, n_g > 4,
 * a rectangle the partial-sum buffer does not hold, a block outside [cout_total][cin_total]. */
int xsd_test_wgrad_ex(xsd_engine* e, const float* const* host_x_planes, int n_in, const float* const* host_g_planes, int n_g, int shuffle_g,
                      float scale, int shuffle, int plane, int j0, int n0, int cin_total, int cout_total,
                      float* dev_dw_oihw, float* dev_db, int B, int H, int W, void* stream);
/* A dense block's weight gradients as the plan of the shipped configuration launches them (kernel-level tests; synchronous; split math
 * modes only): ONE pair-list launch over the fifteen (x_j, G_n) pairs, j <= n, then the five convs' fixed-order reductions as one launch
 * (separate_reduces != 0: as five).  host_x_planes: x_0 .. x_4, host_g_planes: G_1 .. G_5 (host arrays of five device planes
 * [B][H][W][32]).  Conv n + 1 (n = 0 .. 4) owns dw [32][32 (n + 1)][3][3] (OIHW) at dev_grads + host_w_off[n] and db [32] at
 * dev_grads + host_b_off[n]; conv 5's are multiplied by gscale.  nparts 0: the plan's own count for this device (the function the plan
 * asks), else 8 m or 8 m + 1 with 1 <= m <= 10; *host_nparts (or NULL) = what ran.  The launch and the reductions are filled by the
 * function the plan calls.  Both partial-sum buffers of the engine are filled with 0xFF bytes before the launch: a panel or bias row
 * that no workgroup writes arrives as NaN.  In f16x3 the ten planes' max |x| are reduced here.  Refused with XSD_ERR_ARG, nothing
 * launched: an engine in fp32 mode or of the generic-width path, a null plane, an nparts of another form or one whose 15 panels or
 * 5 x 32 bias sums per part the partial-sum buffers do not hold. */
int xsd_test_wgrad_block(xsd_engine* e, const float* const* host_x_planes, const float* const* host_g_planes, float gscale, float* dev_grads,
                         const long long* host_w_off, const long long* host_b_off, int nparts, int separate_reduces, int* host_nparts,
                         int B, int H, int W, void* stream);

/* The edge layers one by one (csrc/aux_kernels.hip; kernel-level tests; synchronous; an engine of the plane path).  Every hook packs
 * ONE (32, 9) weight block with the engine's own packer (pack_edge_kernel) and launches through the engine's own launcher.
 * dev_w with w_last == 0: W_first[:, ch], 32 rows of 9 taps `first_cstride` (= 9 * in_channels) floats apart; with w_last != 0:
 * W_last[o], [32][9].  flipped != 0 selects the packed form with the taps reversed (the input-gradient forms).
 * A launch the launcher refuses returns XSD_ERR_HIP and writes nothing. */
/* 1 -> 32: out[B][H][W][32] (+)= bias + sum_tap s[p + tap] w[tap][c]; then the mask select (mask plane, or its compact words `bits`
 * in the layout of xsd_test_out.bits_out): kept where the mask is > 0, times mslope elsewhere.  s_bs: floats between images of s
 * (0: H * W).  dev_amax (or NULL): slot that receives max |out| by an atomic maximum (the caller zeroes it). */
int xsd_test_edge_expand(xsd_engine* e, const float* dev_s, long long s_bs, const float* dev_w, int w_last, int flipped, int first_cstride,
                         const float* dev_bias, float* dev_out, const float* dev_mask, float mslope, const unsigned short* dev_bits,
                         int accumulate, float* dev_amax, int B, int H, int W, void* stream);
/* 32 -> 1: v = bias + sum_tap sum_c f[p + tap][c] w[tap][c] (+ skip) (+ addto); pre = v; y = clamp01 ? clamp(v, 0, 1) : v.
 * y_bs: floats between images of y / pre / addto, skip_bs: of skip (0: H * W). */
int xsd_test_edge_reduce(xsd_engine* e, const float* dev_f, const float* dev_w, int w_last, int flipped, int first_cstride,
                         const float* dev_bias, const float* dev_skip, long long skip_bs, float* dev_pre, float* dev_y, long long y_bs,
                         int clamp01, const float* dev_addto, int B, int H, int W, void* stream);
/* Edge weight gradient of f [B][H][W][32] against s [B][H][W] (s_bs as above) plus its fixed-order final sum.  mode 0 (conv_first):
 * dw[c * cstride + tap], db[c] = sum f; mode 1 (conv_last): dw[c * 9 + 8 - tap], db[0] = sum s.  nblocks 0: the engine's own rule
 * (the function the plan asks), else that many workgroups (at most the rule's: the partial-sum buffer); *host_nblocks = what ran. */
int xsd_test_edge_wgrad(xsd_engine* e, const float* dev_f, const float* dev_s, long long s_bs, int mode, float* dev_dw, float* dev_db,
                        int cstride, int nblocks, int* host_nblocks, int B, int H, int W, void* stream);

/* The generic-width kernels one by one (csrc/generic_net.hip; kernel-level tests; synchronous; no engine: each call builds a GenericNet
 * that is ONE conv (cout, cin), packs it with the net's own pack() and calls the net's own conv() / wgrad(), dispatch included).
 * Tensors are NCHW views: channel stride H * W, batch stride given.  The epilogue in the kernels' order:
 *   v = (conv + bias) * a1; if (e1 && ch < e1c) v += s1 * e1; v *= a2; if (e2) v += s2 * e2; v = v > 0 ? v : v * slope;
 *   if (skip) v += skip[skipc == 1 ? 0 : ch]; if (accumulate) v += y; if (pre) pre = v; if (clamp01) v = clamp(v, 0, 1); y = v
 * shuffle: y (and pre) are [B][cout / 4][2H][2W], channel oc -> (oc >> 2, sub-pixel ((oc >> 1) & 1, oc & 1)). */
typedef struct xsd_test_gconv_args {
    const float* x; long long xbs;
    float* y; long long ybs;
    float a1; const float* e1; long long e1bs; float s1; int e1c;
    float a2; const float* e2; long long e2bs; float s2;
    float slope; int accumulate; int shuffle;
    const float* skip; long long skipbs; int skipc;
    float* pre; int clamp01;
} xsd_test_gconv_args;
/* dev_params: the flat parameter buffer; the conv's OIHW weight stands at param_off, its bias behind it.  transposed != 0: the
 * input-gradient conv (cout -> cin channels, flipped taps, no bias).  *host_path: 1 = direct kernel, 2 = matrix-instruction kernel. */
int xsd_test_gconv(int cout, int cin, const float* dev_params, long long param_off, int transposed, const xsd_test_gconv_args* host_args,
                   int B, int H, int W, int* host_path, void* stream);
/* dev_grads: flat gradient buffer laid out like dev_params (dw at param_off, db behind it; nothing else is written).
 * *host_parts: the number of partial sums the net's rule chose. */
int xsd_test_gwgrad(int cout, int cin, long long param_off, const float* dev_x, long long xbs, const float* dev_g, long long gbs,
                    float* dev_grads, int B, int H, int W, int* host_path, int* host_parts, void* stream);
/* The net's elementwise launches over [B][C][H * W] views.  op 0: d = a * s; 1: d += a * s; 2: d = s > 0 ? d : d * a (dbs / sbs: batch strides);
 * 3: d[B][C][H][W] = unshuffle(s = dU, s2 = U: [B][C / 4][2H][2W]) with d = U > 0 ? dU : dU * a; 4: d[B][H * W] += sum over the C channels
 * of s[B][C][H * W]; 5: d = (0 <= s <= 1) ? s2 : 0 over B * C * H * W elements (s = pre, s2 = dy). */
int xsd_test_gop(int op, float* dev_d, long long dbs, const float* dev_s, long long sbs, const float* dev_s2, int B, int C, int H, int W,
                 float a, void* stream);
/* Packs a table of n convs (at most 8; parameters from offset 0 of dev_params, conv after conv: weight, bias) with the net's pack() and
 * copies the transposed buffer and the block-packed buffer out (either may be NULL; capacities in floats).  host_off[3 i + 0 .. 2]:
 * conv i's offsets in wt, and in wblk of its forward and its input-gradient blocks (-1: none); host_count[0 .. 1]: floats of wt and wblk. */
int xsd_test_gpack(int n, const int* host_cout, const int* host_cin, const float* dev_params, float* dev_wt, long long wt_cap,
                   float* dev_wblk, long long wblk_cap, long long* host_off, long long* host_count, void* stream);

/* The loss kernels below the whole terms (csrc/loss_kernels.hip; kernel-level tests; synchronous; no product path calls these).
 * xsd_loss_test_scale: ONE SSIM scale through the two host functions the SSIM / MS-SSIM chain runs per scale.  Forward: minmax,
 * minmax_final, ssim_kernel<false>, image_stat -> dev_stat [B][2] device DOUBLES (per-image mean ssim, mean contrast term).  With
 * dev_dy (and then dev_gup [B][2] = d loss / d (ssim_b, cs_b)) also: ties, ssim_kernel<true>, scale_bwd_scalars, back_filter ->
 * dev_dy [B][H][W] (added to when accumulate != 0), plus 0.25 * dev_coarse [B][H / 2][W / 2] (or NULL) spread over 2 x 2 pixels as
 * the chain does with the pooled scale's gradient.  Of cfg only sigma, k1, k2 are read.  host_scal11: the scale's scalars after the
 * last launch -- pmin, pmax, tmin, tmax, data_range, c1, c2, from_p (1: the range is the prediction's), nmax, nmin (tie counts of the
 * prediction's extremes; 1 after a forward-only call), ddr (d loss / d data_range).  Refused with XSD_ERR_ARG: what xsd_loss_eval
 * refuses for the ssim term, dy without gup or the reverse, a coarse gradient without dy. */
int xsd_loss_test_scale(const xsd_loss_config* cfg, const float* dev_y, const float* dev_target, const float* dev_gup, const float* dev_coarse,
                        float* dev_dy, int accumulate, double* dev_stat, float* host_scal11, int B, int H, int W, void* stream);
/* pool2_kernel alone: po, to [B][H / 2][W / 2] = the 2 x 2 means of p, t [B][H][W] (an odd last row / column is dropped). */
int xsd_loss_test_pool2(const float* dev_p, const float* dev_t, float* dev_po, float* dev_to, int B, int H, int W, void* stream);
/* launch_clamp_bwd alone (csrc/aux_kernels.hip): dpre = (0 <= pre <= 1) ? dy : 0 over n elements. */
int xsd_test_clamp_bwd(const float* dev_pre, const float* dev_dy, float* dev_dpre, int64_t n, void* stream);

/* Test entry, in the product library like xsd_ext_metrics_test_stage (host code only, on no product path; synchronous): copy ONE region
 * of what the last xsd_pack_weights of a plane-path engine produced into dev_dst (device memory, dst_bytes long).  info[0] (host)
 * receives the region's size in bytes; with dev_dst NULL the call reports the size only.  A region may be empty (0 bytes: PK_SBIAS
 * of a DN engine, PARAMS_PAD of a width that is a multiple of 32).
 *   PK_FWD, PK_BWD, PK_FWD_S, PK_BWD_S   pk_floats x 4 B each (what they hold depends on the math mode: xsd_set_math)
 *   AMAX         2 floats: max |x| of the forward and of the input-gradient panels (math mode f16x3)
 *   PK_EDGE      [first_fwd | first_bwd][in channel][plane][tap][c], [last_fwd | last_bwd][out channel][plane][tap][c]
 *   PK_SBIAS     the pixel-shuffle convs' biases in chunk order, 128 planes floats per conv
 *   PARAMS_PAD   the zero-padded flat parameter vector of a width that is no multiple of 32
 *   TABLE        HOST data, copied to a HOST buffer dev_dst, int64 words: ndesc, nup, first_w, last_w, planes, nf_pad (0: not padded),
 *                pk_floats, floats of the flat vector the offsets refer to (the padded one if there is one); then per pack descriptor
 *                (read back from the device table the pack kernels use) src_w, dst_fwd, dst_bwd, cout, cin, shuffle, the bits of
 *                bwd_scale; then per pixel-shuffle conv b_off, sbias_off.
 * Refused, copying nothing: XSD_ERR_ARG for null e / info, a generic-width engine, an unknown region, a buffer too small;
 * XSD_ERR_STATE before the first xsd_pack_weights. */
enum {
    XSD_PACKED_PK_FWD = 0, XSD_PACKED_PK_BWD, XSD_PACKED_PK_FWD_S, XSD_PACKED_PK_BWD_S, XSD_PACKED_AMAX, XSD_PACKED_PK_EDGE,
    XSD_PACKED_PK_SBIAS, XSD_PACKED_PARAMS_PAD, XSD_PACKED_TABLE, XSD_PACKED_REGIONS
};
int xsd_test_packed_region(xsd_engine* e, int region, void* dev_dst, int64_t dst_bytes, int64_t* info, void* stream);
/* The gather direction of the zero-padded widths alone: exactly the launch xsd_backward_stage makes, over all descriptors at once, from
 * the caller's padded gradient vector (TABLE word 7 floats) into the caller's real-width one.  XSD_ERR_ARG when the width is not padded. */
int xsd_test_pad_gather(xsd_engine* e, float* dev_grads_real, const float* dev_grads_padded, void* stream);
/* launch_add_channels alone (csrc/aux_kernels.hip): dst[B][HW] += sum over the C channels of src[B][C][HW]. */
int xsd_test_add_channels(float* dev_dst, const float* dev_src, int C, int64_t HW, int B, void* stream);

/* The device-memory ledger (csrc/xsd_ledger.h, csrc/xsd_mem.h): every device allocation of the library and every free goes through one
 * account, per loaded library and process-wide (all handles, all threads).  Host code only, on no product path, no device call.
 * xsd_test_mem_stats: copies the first n (1..6) counters into out (host): live_blocks, live_bytes (allocations held now and their
 *   bytes as asked for), allocs, frees (since the library was loaded), foreign_frees (a free of a non-null pointer the ledger never
 *   handed out), refused (allocations refused by the arm below).  XSD_ERR_ARG for null out or n outside 1..6.
 * xsd_test_mem_refuse: nth >= 1 arms a one-shot refusal: the nth device allocation from now fails as out of memory WITHOUT calling the
 *   runtime (the entry that asked answers XSD_ERR_NOMEM); the arm is spent when it fires.  nth = 0 disarms.  Returns the number of
 *   allocation attempts since the previous call of this entry: arm-free runs measure how many allocations a path makes. */
int xsd_test_mem_stats(int64_t* out, int n);
int64_t xsd_test_mem_refuse(int64_t nth);

#ifdef __cplusplus
}
#endif
#endif /* XSD_H */
