/*
 * snap_hip.h -- C ABI of libsnap_hip.so: the MI355X (gfx950) kernels behind the
 * SNAP BEV-fusion + pose-matching hot path.
 *
 * The reference (google-research/snap) is pure Python/JAX and exposes NO FFI /
 * plugin ABI; its boundary is the Flax module API.  This
 * header is therefore the build-defined boundary a JAX custom-call / XLA FFI
 * handler (or ctypes, as snap_amd/_lib.py does) would bind.  Each entry point
 * cites the reference expression (file:line under /root/reference) it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes; no torch / C++ types; the caller owns every buffer
 *     and pre-allocates outputs; the only hidden state is none (no allocation).
 *   - tensors are row-major, channels-last, contiguous; float = IEEE fp32;
 *     masks are uint8 (0/1); indices are int32.
 *   - asynchronous on `stream` (a hipStream_t passed as void*); no internal sync;
 *     re-entrant and thread-safe for distinct streams.
 *   - returns SNAP_OK (0) or a negative SnapStatus; never throws across the ABI.
 */
#ifndef SNAP_HIP_H_
#define SNAP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum SnapStatus {
  SNAP_OK = 0,
  SNAP_ERR_BAD_SHAPE = -1,    /* inconsistent / unsupported sizes */
  SNAP_ERR_UNSUPPORTED = -2,  /* option not implemented */
  SNAP_ERR_NULL = -3,         /* required pointer is NULL */
  SNAP_ERR_LAUNCH = -4,       /* hipGetLastError() != hipSuccess after launch */
  SNAP_ERR_WORKSPACE = -5     /* workspace too small */
} SnapStatus;

/* Library / device introspection. */
/* (snap_vote_prior_workspace_bytes / snap_vote_prior_f32 were ADDED at version 29 without a bump: an addition changes no
 * existing prototype, struct or constant, and a library built without them fails to load on the missing symbol.
 * snap_vote_raster_workspace_bytes / snap_vote_raster_f32 were added the same way.) */
#define SNAP_ABI_VERSION 30   /* bump on any change to this header's prototypes, structs or constants */
int snap_abi_version(void);                 /* SNAP_ABI_VERSION of the built library */
const char* snap_status_string(int status);
const char* snap_build_arch(void);          /* "gfx950" */

/* ------------------------------------------------------------------------- *
 * Encoder: implicit-GEMM convolution engine on f32 MFMA (v_mfma_f32_32x32x2_f32)
 *   replaces flax.linen.Conv / StdConv / Dense as used by
 *   snap/models/resnet.py:73-132,183-216, snap/models/image_encoder.py:53-94,
 *   snap/models/layers.py:55-78 (MLP Dense stack) and, with a (H x W x D)-sized
 *   kernel, the direct rotated-template correlation of
 *   snap/models/pose_exhaustive_voting.py:86-91.
 * ------------------------------------------------------------------------- */
enum { SNAP_PRO_NONE = 0, SNAP_PRO_AFFINE = 1, SNAP_PRO_GN_RELU = 2,
       SNAP_PRO_RELU_GN = 3, SNAP_PRO_RELU = 4 };
enum { SNAP_EPI_BIAS = 1, SNAP_EPI_RELU = 2, SNAP_EPI_RESIDUAL = 4,
       SNAP_EPI_UPSAMPLE2X_ADD = 8, SNAP_EPI_ROWMASK = 16,
       SNAP_EPI_GELU = 32 /* tanh-approximated GELU (ViT MLP), applied where ReLU is */ };

typedef struct SnapConvDesc {
  int32_t N, H, W, Cin, Cin_stride;   /* input  x[N,H,W,Cin_stride], first Cin used */
  int32_t KH, KW, stride, pad_t, pad_l;
  int32_t Ho, Wo, Cout, Cout_stride;  /* output y[N,Ho,Wo,Cout_stride]            */
  int32_t prologue;                   /* SNAP_PRO_*  applied to every input element
                                         BEFORE zero padding                       */
  int32_t epilogue;                   /* OR of SNAP_EPI_*                          */
  float in_scale, in_shift;           /* SNAP_PRO_AFFINE: x*in_scale + in_shift    */
  int32_t tile_hint;                  /* 0 = the engine picks the output tile; bm * 1000 + bn
                                         (128128 | 128064 | 64128 | 64064) forces one -- part of
                                         the descriptor because the size queries depend on it
                                         (tests and tuning tools; the library reads no
                                         environment variables).  + 1 000 000 x mode selects
                                         among the 1x1 bodies of the split engine (conv_rs.hip):
                                         0 automatic, 1 tiled body only, 2 the stationary
                                         kernels also below their row-count threshold, 3 no
                                         weights-stationary kernel, 4 = 2 and 3              */
} SnapConvDesc;

/* y = epilogue( conv( prologue(x), w ) ).  w is HWIO flattened: [KH*KW*Cin, Cout].
 * gn_mu/gn_sc: [N, Cin] per-(image, channel) mean and rstd*gamma (from
 * snap_group_norm_stats_f32); gn_beta: [Cin].  residual: same layout as y.
 * up_prev: [N, Ho/2, Wo/2, Cout_stride] (bilinear x2, half-pixel centres, edge
 * clamp == jax.image.resize, image_encoder.py:90).  row_mask: [N*Ho*Wo] uint8.
 * Unused pointers may be NULL. */
int snap_conv2d_nhwc_f32(const SnapConvDesc* desc, const float* x, const float* w,
                         float* y, const float* gn_mu, const float* gn_sc,
                         const float* gn_beta, const float* bias,
                         const float* residual, const float* up_prev,
                         const uint8_t* row_mask, void* stream);

/* Optional extras of a conv launch (all may be NULL / 0):
 *  - row-indexed launch over a masked voxel list (the fusion MLP of
 *    streetview_encoder.py:281 runs over every voxel and the result is then masked by
 *    visibility; unobserved voxels never reach any output, so only the observed rows are
 *    multiplied).  rows_in: GEMM row m reads output pixel rows_in[m] of x; rows_out: GEMM
 *    row m is stored to row rows_out[m] of y; row_count: DEVICE scalar with the number of
 *    rows (<= N*Ho*Wo, the launch bound) -- no host synchronisation.  Only
 *    SNAP_EPI_BIAS / SNAP_EPI_RELU epilogues.
 *  - gn_partial: the epilogue also emits per-(image, row tile, channel) sums of y and y^2
 *    (of relu(y) if gn_partial_relu), from which snap_group_norm_stats_from_partial_f32
 *    produces the GroupNorm statistics the NEXT layer's fused prologue needs
 *    (resnet.py:46-60) without re-reading y.  Size: snap_conv2d_gn_partial_bytes(desc);
 *    0 means "not available for this shape" (Ho*Wo smaller than a row tile); a launch that
 *    emits statistics never splits K.  */
typedef struct SnapConvExtras {
  const int32_t* rows_in;
  const int32_t* rows_out;
  const int32_t* row_count;
  float* gn_partial;
  size_t gn_partial_bytes;
  int32_t gn_partial_relu;
  void* workspace;            /* split-K scratch: snap_conv2d_workspace_bytes(desc) (may be 0) */
  size_t workspace_bytes;
  const void* w_bf16;         /* non-NULL selects a bf16 matrix-core engine (see below) */
  size_t w_bf16_bytes;
  int32_t w_split_parts;      /* 0: w_bf16 = rounded weights (training-precision engine);
                                 2 | 3: w_bf16 = split weights (f32-grade split-bf16 engine) */
  int32_t w_split_root;       /* 1: the 7 x 7 / stride 2 / pad 3 root convolution (resnet.py:200-205)
                                 of an RGB image stored with 4 floats per pixel (Cin = 3,
                                 Cin_stride = 4): w_bf16 = snap_conv2d_pack_weights_split_root_bf16,
                                 a K slab = 4 consecutive pixels of one kernel row */
  float* gn_partial2;         /* with gn_partial (gn_partial_relu = 0): a second buffer of the same
                                 size that MAY receive the partial sums of relu(y) -- for an output
                                 read by a GroupNorm->ReLU layer AND a ReLU->GroupNorm layer (the
                                 last unit of a ResNet stage: next stage / FPN level).  A request,
                                 honoured by one kernel variant (split-bf16 engine, GroupNorm->ReLU
                                 prologue, 128 x 128 tiles): */
  size_t gn_partial2_bytes;
  int32_t gn_partial2_done;   /* OUT: 1 if gn_partial2 was written by this launch, else 0 (take
                                 snap_group_norm_stats_f32 for the second statistic) */
  int32_t x_presplit;         /* 1: `x` is NOT f32 but the pre-split image of the (already normalised)
                                 input, [N*H*W][Cin/16][hi 16 | lo 16] bf16 as written by
                                 snap_gn_norm_split_f32 / snap_presplit_f32; needs w_split_parts = 2,
                                 prologue NONE, Cin % 16 == 0, no row lists.  Both operands then
                                 travel by LDS-DMA (conv_ps.hip); sizes come from the
                                 snap_conv2d_presplit_* queries below instead of the plain ones.
                                 With w_split_parts = 1 (w_bf16 = the ONE-part image of
                                 snap_conv2d_pack_weights_split_bf16): `x` is a plain bf16 tensor
                                 [N,H,W,Cin] (Cin_stride == Cin) and the launch is the
                                 training-precision arithmetic (operands rounded to bf16, f32
                                 accumulate: the bits of the x_half engine) on the same ring; no
                                 statistics / split-K / up-sampling epilogue; y_half allowed */
  int32_t ps_tile;            /* ... 0 = automatic, 1 = 128-row tiles, 2 = 256-row tiles (tuning) */
  int32_t ps_res_init;        /* ... 1 = a residual is loaded into the accumulators before the K loop
                                 (r + p1 + p2 + ... instead of (p1 + p2 + ...) + r) */
  int32_t bk_hint;            /* f32 engine: K-slab depth 16 | 32 of the large tiles (0 = default 16) */
  int32_t tune_flags;         /* SNAP_TUNE_*: A/B switches for tests and tuning tools (0 = defaults) */
  int32_t gn_partial_rows;    /* 0: gn_partial is laid out per row tile of the launch
                                 (snap_conv2d_tile_rows_ex); 32: per 32-row slab, sized by
                                 snap_conv2d_splitk_gn_partial_bytes -- a split-K launch of the
                                 split-operand engine (workspace given), whose reduce pass then emits
                                 the partial sums (a split-K launch has no epilogue that sees
                                 finished outputs) */
  int32_t w_half;             /* with w_split_parts = 0: 1 = the training-precision engine in IEEE
                                 half -- w_bf16 holds snap_conv2d_pack_weights[_multi]_f16 images,
                                 the A operand is rounded to f16 (RNE; beyond 65504 -> inf) and the
                                 products run on v_mfma_f32_32x32x16_f16 (f32 accumulate): the
                                 reference's dtype=float16 train config (train_localization.py:93,
                                 resnet.py:97), driven by DynamicScale (trainer.py:391-392) */
  int32_t x_half;             /* with w_split_parts = 0 (training-precision engine), prologue NONE, no row
                                 lists, Cin_stride % 8 == 0: 1 = `x` is NOT f32 but the tensor already
                                 rounded to the engine's element type (bf16, or IEEE half with w_half),
                                 [N, H, W, Cin_stride] -- the half-precision twin a GroupNorm VJP wrote
                                 next to its f32 gradient (snap_group_norm_bwd_ex_f32).  The
                                 data-gradient convolution then moves both operands by LDS-DMA: half the
                                 input bytes, no conversion in the loop; same bits as the f32 input.
                                 rows_out / row_count are honoured (compact row buffers), rows_in is not */
  void* y_half;               /* with w_split_parts = 0, prologue NONE / RELU, no statistics: the stored
                                 values ALSO go, rounded (RNE) to the engine's element type, to y_half
                                 (same indexing as y, 2-byte elements) -- and ONLY there when y is NULL:
                                 the hidden activations / inter-layer gradients of the masked MLP
                                 (layers.py:55-78), which every consumer rounds to that type anyway */
  /* The statistics pass of a GroupNorm VJP inside the data-gradient convolution that produces its incoming
   * gradient (x_half launches without split-K, Cout_stride == Cout, no row lists; gn_partial / gn_partial_bytes
   * as for the forward statistics: snap_conv2d_gn_partial_bytes_ex(desc, 0)).  gnb_mode = SNAP_PRO_GN_RELU /
   * SNAP_PRO_RELU_GN (0 = off): with dz = the stored output, xh = (x - mu) * rstd (relu(x) for RELU_GN) and
   * dyp = dz gated by (xh * gamma + beta > 0) (GN_RELU) the epilogue emits, per (image, row tile, channel), the
   * sums of dyp and dyp * xh -- what snap_group_norm_bwd_ex_f32's first pass computes by re-reading x and dz;
   * snap_group_norm_bwd_stats_f32 consumes them.  gnb_x [N, Ho, Wo, Cout] f32 (the layer input the GroupNorm
   * normalises), gnb_mu / gnb_rstd [N, Cout], gnb_gamma / gnb_beta [Cout]. */
  const float* gnb_x;
  const float* gnb_mu;
  const float* gnb_rstd;
  const float* gnb_gamma;
  const float* gnb_beta;
  int32_t gnb_mode;
} SnapConvExtras;
#define SNAP_TUNE_NO_HALO 1   /* split engine: the im2col body for every 3x3 convolution */
/* tune bit 2 is retired (it selected a raw-row ring body, measured slower: DESIGN.md 5a): a launch
 * that sets it returns SNAP_ERR_UNSUPPORTED */
#define SNAP_TUNE_NO_PLAIN 8   /* split engine: the general A loader also for 1x1 / stride-1 / unpadded layers */
#define SNAP_TUNE_RS_NSPLIT_SHIFT 4   /* bits 4..7: row-stationary kernel, forced column split (0 = automatic) */
/* Pre-split launches (extras->x_presplit): row tile, GroupNorm partial-sum bytes and split-K
 * workspace bytes of the launch `desc` + `ps_tile` describes (the counterparts of
 * snap_conv2d_tile_rows / _gn_partial_bytes / _workspace_bytes). */
int32_t snap_conv2d_presplit_tile_rows(const SnapConvDesc* desc, int32_t ps_tile);
size_t snap_conv2d_presplit_gn_partial_bytes(const SnapConvDesc* desc, int32_t ps_tile);
size_t snap_conv2d_presplit_workspace_bytes(const SnapConvDesc* desc, int32_t ps_tile);
/* 1 when the pre-split engine takes the shape `desc` describes (prologue NONE, Cin % 16 == 0, the
 * input window of a row tile and one column tile of the weight image below its 32-bit offset
 * limits), else 0: callers that have another engine for the shape (the exhaustive voting of
 * pose_exhaustive_voting.py:72-104 on very large templates) ask before they pre-split. */
int32_t snap_conv2d_presplit_supported(const SnapConvDesc* desc);
/* GroupNorm -> ReLU (resnet.py:34-60,117-130) of a conv output y [N, HW, C] whose partial sums
 * came out of the producing conv's epilogue (extras->gn_partial, row tile `tile_rows`), written
 * ONCE in the pre-split format: out [N*HW][C/16][hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15] bf16
 * (N*HW*C*4 bytes), hi = bf16(v), lo = bf16(v - hi).  Replaces the statistics finalize launch of
 * that tensor AND the normalise / split work of every consumer tile; mu / sc (optional, both or
 * neither): the statistics of the plain partial sums, var = (T2 - 2 mean T1 + n mean^2) / n -- WITHOUT
 * the re-reduction snap_group_norm_stats_from_partial_f32 gives a group with mean^2 > 4 var, so on
 * such a group the variance is off by about 2^-24 mean^2 and differs from that function's.  C % 16 == 0,
 * C <= 2048, groups a power of two <= 64. */
int snap_gn_norm_split_f32(const float* y, const float* partial, int32_t N, int32_t HW, int32_t C,
                           int32_t groups, float eps, int32_t tile_rows, const float* gamma,
                           const float* beta, void* out, float* mu, float* sc, void* stream);
/* The plain two-part split of x [rows, C] f32 into the same format (C % 16 == 0). */
int snap_presplit_f32(const float* x, int64_t rows, int32_t C, void* out, void* stream);

int snap_conv2d_nhwc_ex_f32(const SnapConvDesc* desc, const float* x, const float* w,
                            float* y, const float* gn_mu, const float* gn_sc,
                            const float* gn_beta, const float* bias,
                            const float* residual, const float* up_prev,
                            const uint8_t* row_mask, const SnapConvExtras* extras,
                            void* stream);
/* Training-precision engine: the analogue of the reference's float16 train config
 * (snap/configs/train_localization.py:25).  Tensors stay f32 in memory; the prologue runs in
 * f32, then both operands are rounded to bf16 (round-to-nearest-even) and multiplied on the
 * bf16 matrix cores with f32 accumulation; epilogue in f32.  The caller packs the weights
 * once per launch (or per step) with snap_conv2d_pack_weights_bf16 -- out is
 * [Cout][taps][roundup(Cin, 8)] bf16, taps = KH*KW -- and passes them as extras->w_bf16; `w`
 * is still required (shapes the bf16 engine does not carry -- Cin < 4, unaligned channel
 * rows -- run on the exact f32 engine instead).  All fusions, row-indexed launches, GroupNorm
 * partial sums and split-K behave as on the f32 engine. */
size_t snap_conv2d_packed_weights_split_root_bytes(int32_t Cout, int32_t parts);
int snap_conv2d_pack_weights_split_root_bf16(const float* w /* [7,7,3,Cout] */, int32_t Cout,
                                             int32_t parts, void* out, size_t out_bytes,
                                             void* stream);
size_t snap_conv2d_packed_weights_bytes(int32_t taps, int32_t Cin, int32_t Cout);
int snap_conv2d_pack_weights_bf16(const float* w, int32_t taps, int32_t Cin, int32_t Cout,
                                  void* out, size_t out_bytes, void* stream);
/* ... the same image in IEEE half for extras->w_half = 1 (the reference's float16 compute /
 * parameter dtype, train_localization.py:93, resnet.py:97): same size, same layout */
int snap_conv2d_pack_weights_f16(const float* w, int32_t taps, int32_t Cin, int32_t Cout,
                                 void* out, size_t out_bytes, void* stream);
/* f32-grade engine on the bf16 matrix cores (inference / parity path; replaces the same
 * flax.linen.Conv / Dense calls: resnet.py:73-132, image_encoder.py:67-94, layers.py:55-78).
 * Each f32 operand is split into `parts` bf16 values (hi = bf16(v), then bf16 of the exact f32
 * residual, ...); a*b is the f32-accumulated sum of the part products above the f32 rounding
 * level: parts = 2 -> a_lo b_hi + a_hi b_lo + a_hi b_hi (relative error ~2^-17 per product),
 * parts = 3 -> six products (operands exact to 24 bits, ~2^-24 per product: the accuracy class
 * of an f32 fmaf chain).  The caller splits the weights with
 * snap_conv2d_pack_weights_split_bf16 -- out is the engine's own tile-major image
 * ([Cout/128][taps][Cin/16][parts][128][16] bf16, zero padded; an opaque blob to the caller) --
 * and passes them as extras->w_bf16 with extras->w_split_parts = parts; activations are split
 * on the fly after the f32 prologue.  Fusions, row-indexed launches, GroupNorm partial sums
 * and split-K as on the f32 engine; shapes it does not carry (Cin < 4, unaligned channel rows)
 * run on the exact f32 engine. */
size_t snap_conv2d_packed_weights_split_bytes(int32_t taps, int32_t Cin, int32_t Cout,
                                              int32_t parts);
int snap_conv2d_pack_weights_split_bf16(const float* w, int32_t taps, int32_t Cin, int32_t Cout,
                                        int32_t parts, void* out, size_t out_bytes, void* stream);
/* ... every kernel of an encoder in ONE launch: `items` is a DEVICE array sorted by block_begin;
 * item i owns workgroups [block_begin, block_begin + snap_conv2d_pack_weights_split_blocks(...));
 * out: snap_conv2d_packed_weights_split_bytes(taps, Cin, Cout, parts) bytes, 16-byte aligned. */
typedef struct SnapPackItem {
  const float* w;
  void* out;
  int32_t taps, Cin, Cout, block_begin;
} SnapPackItem;
int32_t snap_conv2d_pack_weights_split_blocks(int32_t taps, int32_t Cin, int32_t Cout);
/* The same for the bf16-operand engine's images (training precision): one launch for every kernel
 * of a step.  An item with taps < 0 asks for the ROTATED image of |taps| taps that the
 * data-gradient convolution reads -- the image of w.flip(0, 1).permute(0, 1, 3, 2) with the output
 * channels padded to a multiple of four: out = snap_conv2d_packed_weights_bytes(|taps|, Cout,
 * roundup(Cin, 4)) bytes.  Items sorted by block_begin; item i owns
 * snap_conv2d_pack_weights_blocks(taps, Cin, Cout) workgroups. */
int32_t snap_conv2d_pack_weights_blocks(int32_t taps, int32_t Cin, int32_t Cout);
int snap_conv2d_pack_weights_multi_bf16(const SnapPackItem* items, int32_t n_items,
                                        int32_t total_blocks, void* stream);
/* ... the same images in IEEE half (SnapConvExtras.w_half; same sizes and layout) */
int snap_conv2d_pack_weights_multi_f16(const SnapPackItem* items, int32_t n_items,
                                       int32_t total_blocks, void* stream);
int snap_conv2d_pack_weights_split_multi_bf16(const SnapPackItem* items, int32_t n_items,
                                              int32_t total_blocks, int32_t parts, void* stream);

/* Generic N-D grid operators (snap/utils/grids.py:116-153); n = 1..3 leading grid axes.
 * snap_interpolate_nd_f32: array [size..., D], points [K, n] in corner-origin coordinates (cell
 * centres at k + 0.5), optional valid_array [size...] -> values [K, D], valid [K]:
 * jax.scipy.ndimage.map_coordinates(order=1, mode='nearest') per channel after the -0.5 shift
 * (:129-130); valid = 0 <= p < size on every axis AND no tap -- not even a zero-weight one --
 * is invalid (the 0 * NaN mask of :131-136).  `size` is a HOST array.
 * snap_expectation_nd_f32: pdf [rows, size...] -> out [rows, n] = sum_cells index(cell) pdf(cell)
 * (:148-153; deterministic fixed-order sums).  argmax_nd (:140-145) = snap_argmax_rows_f32 over
 * the flattened grid + GridND.id_to_index on the host side. */
int snap_interpolate_nd_f32(const float* array, const int32_t* size, int32_t n, int32_t D,
                            const uint8_t* valid_array, const float* points, int64_t K,
                            float* values, uint8_t* valid, void* stream);
int snap_expectation_nd_f32(const float* pdf, int64_t rows, const int32_t* size, int32_t n,
                            float* out, void* stream);
/* OccupancyNet query path (snap/models/occupancy_net.py).  Point source: rays when `hits` is
 * non-NULL -- hits / origins [B, num_rays, 3], ray_mask [B, num_rays] -- sampled as
 * sample_queries_from_rays (:34-60): P = num_samples * num_rays points per scene, element
 * k * num_rays + n, k = 0 the hit (label 1), k >= 1 origin + linspace(0, 1, S - 1)[k - 1] * dir with
 * dir = (hit - origin) * (|d| - margin) / max(|d|, 1) (label 0); otherwise explicit `points`
 * [B, num_points, 3] (data['occupancy_queries'], :91-105).  out_points [B, P, 3], out_labels /
 * out_ray_valid [B, P] are optional (NULL: not written).  The volume is [B, X, Y, Z, D] with an
 * optional volume_valid [B, X, Y, Z]; each point is sampled as interpolate_nd(volume,
 * point / cell_size, volume_valid) (:107-111, grids.py:116-137), bitwise the arithmetic of
 * snap_interpolate_nd_f32.
 * snap_occupancy_ray_features_f32 -> features [B * P, D], valid [B * P]. */
int snap_occupancy_ray_features_f32(const float* hits, const float* origins, const uint8_t* ray_mask,
                                    int64_t num_rays, int32_t num_samples, float margin, const float* points,
                                    int64_t num_points, int32_t B, const float* volume,
                                    const uint8_t* volume_valid, int32_t X, int32_t Y, int32_t Z, int32_t D,
                                    float cell_size, float* out_points, uint8_t* out_labels,
                                    uint8_t* out_ray_valid, float* features, uint8_t* valid, void* stream);
/* 1 when snap_occupancy_head_f32 takes D -> h1 [-> h2] -> 1 (every width a multiple of 32, at most
 * 256; h2 = 0: one hidden layer), else 0: the caller runs the producer + the Dense engine. */
int32_t snap_occupancy_head_supported(int32_t D, int32_t h1, int32_t h2);
/* The whole query chain of occupancy_net.py:84-116 in one launch: samples -> trilinear gather ->
 * MLP(occupancy_mlp) (layers.py:55-78: Dense + ReLU between layers, kernels [in, out]) -> logits
 * [B * P] (the last Dense's only column, before the sigmoid) and valid [B * P].  Hidden layers on
 * the exact f32 MFMA (k-ordered accumulation, bias-then-ReLU epilogue: the f32 Dense engine's
 * arithmetic class); the width-1 layer as a fixed-order dot product per row.  No per-point
 * intermediate reaches memory; no atomics (bitwise repeatable). */
int snap_occupancy_head_f32(const float* hits, const float* origins, const uint8_t* ray_mask, int64_t num_rays,
                            int32_t num_samples, float margin, const float* points, int64_t num_points, int32_t B,
                            const float* volume, const uint8_t* volume_valid, int32_t X, int32_t Y, int32_t Z,
                            int32_t D, float cell_size, const float* w0, const float* b0, int32_t h1,
                            const float* w1, const float* b1, int32_t h2, const float* w_out,
                            const float* b_out, float* out_points, uint8_t* out_labels, uint8_t* out_ray_valid,
                            float* logits, uint8_t* valid, void* stream);
/* VJP of snap_occupancy_ray_features_f32 into the volume: the transpose of the trilinear gather of
 * interpolate_nd (grids.py:116-137) at the query points of occupancy_net.py:106-111.  Same point source
 * as the forward (rays or explicit points: they are data and get no gradient); volume validity does
 * not enter.  d_features [B * P, D] -> d_volume [B, X, Y, Z, D], every element written (untouched voxels
 * +0).  Each point's 8 taps are re-derived with the forward's f32 expressions and clamps; a tap's
 * contribution is w_tap * d_features[row, ch] (one f32 multiply).  Summation order per voxel (bitwise,
 * no float atomics): its contributions in ascending (point, tap) order, cut into consecutive chunks of
 * snap_occupancy_features_vjp_chunk() records; each chunk sum starts from its first contribution and
 * adds the rest in order, and the voxel's value starts from the first chunk sum and adds the others in
 * chunk order.  Refuses (SNAP_ERR_BAD_SHAPE) B * P * 8 >= 2^32 and B * X * Y * Z >= 2^32 - 1.
 * workspace: snap_occupancy_features_vjp_workspace_bytes(P, ...) bytes (0: shape refused), 256-byte
 * aligned. */
int32_t snap_occupancy_features_vjp_chunk(void);
size_t snap_occupancy_features_vjp_workspace_bytes(int64_t num_points, int32_t B, int32_t X, int32_t Y, int32_t Z,
                                                   int32_t D);
int snap_occupancy_ray_features_vjp_f32(const float* hits, const float* origins, const uint8_t* ray_mask,
                                        int64_t num_rays, int32_t num_samples, float margin, const float* points,
                                        int64_t num_points, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t D,
                                        float cell_size, const float* d_features, float* d_volume, void* workspace,
                                        size_t workspace_bytes, void* stream);

/* Semantic-raster embedding (snap/models/semantic_raster_encoder.py:63-79).  rasters [M, N]
 * uint8 (bool); idx_road / idx_other: HOST arrays with the raster channels of the mutually
 * exclusive surfel-road classes and of the independent binary classes (<= 32 each);
 * table_road [nr, E], table_other [2*no, E]; out [M, (1 + no) * E]:
 * [table_road[argmax road bits] | table_other[j + bit_j] for j < no]  (the reference's row
 * indexing, :72-75).  E % 4 == 0.  snap_semantic_onehot_f32 writes the [M, KP] one-hot matrix
 * (column c < nr: road label c; column nr + 2j + b: class j has bit b; KP % 4 == 0) whose
 * transpose times d out (snap_conv2d_wgrad_f32) gives the table gradients deterministically. */
int snap_semantic_embed_f32(const uint8_t* rasters, int64_t M, int32_t N, const int32_t* idx_road,
                            int32_t nr, const int32_t* idx_other, int32_t no,
                            const float* table_road, const float* table_other, int32_t E,
                            float* out, void* stream);
int snap_semantic_onehot_f32(const uint8_t* rasters, int64_t M, int32_t N, const int32_t* idx_road,
                             int32_t nr, const int32_t* idx_other, int32_t no, float* onehot,
                             int32_t KP, void* stream);

/* ViT encoder pieces (BASELINE.json configs[4]; the reference itself has no ViT --
 * snap/models/image_encoder.py:103 -- so these follow the published ViT block).
 * snap_layer_norm_f32: y[m,:] = (x[m,:] - mean) * rsqrt(var + eps) * gamma + beta over the C
 * channels of each of the M rows (biased variance); C % 4 == 0, C <= 1024.
 * snap_attention_bf16_f32: multi-head self-attention softmax(scale * Q K^T) V on the bf16
 * matrix cores (f32 softmax statistics and accumulation).  qkv [B, N, 3, H, D] f32 (the fused
 * QKV projection's output), out [B, N, H*D] f32; D must be 64. */
int snap_layer_norm_f32(const float* x, const float* gamma, const float* beta, float* y,
                        int64_t M, int32_t C, float eps, void* stream);
int snap_attention_bf16_f32(const float* qkv, float* out, int32_t B, int32_t N, int32_t H,
                            int32_t D, float scale, void* stream);
/* The same two with the result written ONLY rounded (RNE) to bf16 (y_bf16 [M, C] / out_bf16 [B, N, H*D]): the
 * inference path's operands of the dense layers that follow (snap_conv2d_nhwc_ex_f32 with extras->x_presplit = 1,
 * w_split_parts = 1: both operands by LDS-DMA), which round them to that type anyway -- the same values. */
int snap_layer_norm_bf16out_f32(const float* x, const float* gamma, const float* beta, void* y_bf16,
                                int64_t M, int32_t C, float eps, void* stream);
int snap_attention_bf16out_f32(const float* qkv, void* out_bf16, int32_t B, int32_t N, int32_t H,
                               int32_t D, float scale, void* stream);
/* ... and with qkv itself in bf16 (the QKV projection's bf16-only output, y_half): K and V are the values the f32 form
 * rounds to, moved at half the bytes (the kernel is bound by the L2 traffic of the K / V panels); Q is scaled after
 * its rounding. */
int snap_attention_bf16io(const void* qkv_bf16, void* out_bf16, int32_t B, int32_t N, int32_t H, int32_t D,
                          float scale, void* stream);
/* Training path of the ViT pieces.  snap_attention_lse_bf16_f32 also returns lse [B, H, N], the
 * base-2 log-sum-exp of the scaled scores; snap_attention_bwd_bf16_f32 turns (qkv, out, dout,
 * lse) into dqkv (same layout as qkv; delta [B, H, N] is scratch) with two atomic-free kernels
 * on the bf16 matrix cores.  snap_layer_norm_bwd_f32: dx, dgamma, dbeta (fixed-order column
 * sums; workspace from snap_layer_norm_bwd_workspace_bytes).  snap_gelu[_bwd]_f32: tanh-form
 * GELU and its VJP over n (% 4 == 0) elements (the training path keeps the pre-activation). */
int snap_attention_lse_bf16_f32(const float* qkv, float* out, float* lse, int32_t B, int32_t N,
                                int32_t H, int32_t D, float scale, void* stream);
int snap_attention_bwd_bf16_f32(const float* qkv, const float* out, const float* dout,
                                const float* lse, float* delta, float* dqkv, int32_t B, int32_t N,
                                int32_t H, int32_t D, float scale, void* stream);
/* Exact: no launch touches a byte beyond this size. */
size_t snap_layer_norm_bwd_workspace_bytes(int64_t M, int32_t C);
int snap_layer_norm_bwd_f32(const float* x, const float* dy, const float* gamma, float* dx,
                            float* dgamma, float* dbeta, int64_t M, int32_t C, float eps,
                            void* workspace, size_t workspace_bytes, void* stream);
int snap_gelu_f32(const float* x, float* y, int64_t n, void* stream);
int snap_gelu_bwd_f32(const float* x, const float* dy, float* dx, int64_t n, void* stream);

/* Scratch for split-K launches (small-M / deep-K layers that cannot fill 256 CUs with output
 * tiles: slices of K go to extra workgroups, partial tiles are summed in fixed order by a
 * second kernel that also applies the epilogue -- deterministic).  0 = the shape does not
 * split.  Without a workspace the launch simply does not split. */
size_t snap_conv2d_workspace_bytes(const SnapConvDesc* desc);
size_t snap_conv2d_gn_partial_bytes(const SnapConvDesc* desc);
int32_t snap_conv2d_tile_rows(const SnapConvDesc* desc);   /* row-tile height the launch uses */
/* ... of a launch on the split-operand engine with `split_parts` parts (SnapConvExtras.w_split_parts;
 * 0 = any other engine): the weights-stationary 1x1 kernel of the two-part engine emits its
 * GroupNorm partial sums per 32-row slab; a NEGATIVE value -S: S slabs per image, all of them live
 * (the weights-stationary 3x3 kernel: one slab per row-aligned tile) -- pass it on to
 * snap_group_norm_stats_from_partial_f32 as it is. */
int32_t snap_conv2d_tile_rows_ex(const SnapConvDesc* desc, int32_t split_parts);
size_t snap_conv2d_gn_partial_bytes_ex(const SnapConvDesc* desc, int32_t split_parts);
size_t snap_conv2d_splitk_gn_partial_bytes(const SnapConvDesc* desc);   /* see SnapConvExtras.gn_partial_rows */
/* Which body a split-bf16 launch (w_split_parts parts, no row lists) of this descriptor takes:
 * 0 = the tiled body, 1 = the row-stationary 1x1 kernel (activation tile in registers), 2 = the
 * weights-stationary 1x1 kernel (panel resident in LDS) -- conv_rs.hip: the bottleneck units' closing
 * / projection convolution, snap/models/resnet.py:112-132.  Same output bits whichever it is; a pure
 * function of the descriptor (desc->tile_hint carries the A/B mode).  For profiling labels and tests. */
int32_t snap_conv2d_stationary_kind(const SnapConvDesc* desc, int32_t parts);

/* The ResNet stem in one launch: the 7 x 7 / stride 2 / pad 3 root convolution of a 4-floats-per-pixel RGB
 * image (desc as for snap_conv2d_nhwc_ex_f32: Ho x Wo is the CONV output) and the 3 x 3 / stride 2 / pad 1
 * max-pool that reads it (snap_max_pool_3x3s2_f32), the conv output never written: y_pool is
 * [N, (Ho - 1) / 2 + 1, (Wo - 1) / 2 + 1, 64], bit for bit what the two launches give.  w_bf16 = the root
 * weight image (snap_conv2d_pack_weights_split_root_bf16, parts = 2).  Supported (the query is a pure host
 * function): two-part split engine, Cout = Cout_stride = 64, prologue NONE / AFFINE, epilogue nothing but
 * RELU; anything else returns SNAP_ERR_UNSUPPORTED and the caller launches the two kernels.  band_rows =
 * pooled rows a wave computes in one march (0 = chosen from the shape; every value gives the same bits). */
int32_t snap_conv2d_root_pool_supported(const SnapConvDesc* desc, int32_t parts);
int snap_conv2d_root_pool_f32(const SnapConvDesc* desc, const float* x, const void* w_bf16,
                              size_t w_bf16_bytes, int32_t parts, int32_t band_rows, float* y_pool,
                              void* stream);

/* mu / sc (/ rstd) [N, C] from a conv launch's gn_partial.  tile_rows =
 * snap_conv2d_tile_rows(desc of that launch); HW = Ho*Wo of its output.  y [N, HW, C]: the output that
 * launch wrote, relu_first: the sums are those of relu(y) (gn_partial_relu).  The partial sums are plain
 * f32 sums of y and y^2, whose variance loses about 2^-24 (1 + mean^2 / var) relative accuracy; a group
 * with mean^2 > 4 var is therefore re-reduced from y (two-pass, fp64), every other group is not read
 * and keeps the result of its sums. */
int snap_group_norm_stats_from_partial_f32(const float* partial, const float* y, int32_t N,
                                           int32_t HW, int32_t C, int32_t groups, float eps,
                                           int32_t tile_rows, int32_t relu_first,
                                           const float* gamma, float* mu, float* sc, float* rstd,
                                           void* stream);

/* Ascending list of the rows with mask != 0: index[0..count) (stable order,
 * deterministic), count written to *count (device).  index must hold M entries. */
/* Exact: no launch touches a byte beyond this size. */
size_t snap_compact_rows_workspace_bytes(int64_t M);
int snap_compact_rows_u8(const uint8_t* mask, int64_t M, int32_t* index, int32_t* count,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The same list for the rows with lo <= mask[m] <= hi (classed masks: SnapLiftDesc.class_rows). */
int snap_compact_rows_range_u8(const uint8_t* mask, int64_t M, int32_t lo, int32_t hi,
                               int32_t* index, int32_t* count, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- fusion MLP + vertical max pooling in one kernel (mlp_pool.hip) --------------------
 * The two Dense layers of StreetViewEncoder.fusion_mlp (streetview_encoder.py:279-286,
 * layers.py:55-78: Dense(H) -> relu -> Dense(D)) over the rows listed in `rows`, followed by
 * VerticalPooling('max') (bev_mapper.py:78-88) over the Z levels of a column:
 *   plane[col, :] = max over listed rows m with rows[m] / Z == col of Dense1(relu(Dense0(x[rows[m]])))
 *   pvalid[col]   = the column has a listed row;  plane = 0 where it has none.
 * Neither the hidden activations nor the [.., Z, D] feature volume are written.  Arithmetic:
 * the split-bf16 engine with 2 parts ("bf16x3"); the plane equals, bit for bit, the one
 * snap_conv2d_nhwc_ex_f32 (w_split_parts = 2) x 2 + snap_fill_masked_rows_f32 +
 * snap_vertical_pool_f32 produce.
 *   x [*, x_stride] f32 (Cin <= x_stride, x_stride % 4 == 0); rows / row_count from
 *   snap_compact_rows_u8 (ascending); M = upper bound of the row count;
 *   w0_split = snap_conv2d_pack_weights_split_bf16(W0 [Cin, H], taps 1, parts 2);
 *   w1_split = the same packing of W1 [H, D];  H % 32 == 0, H <= 256; D % 4 == 0, D <= 128;
 *   relu_in: MLP.apply_input_activation;  plane [ncols, D], pvalid [ncols].
 *   x_split = 1: x holds the rows pre-split (SnapLiftDesc.out_split: [slab][hi | lo][16] bf16,
 *   x_stride still in floats); the A operand then travels global -> LDS by LDS-DMA.  Same
 *   results bit for bit; relu_in must be 0.  x_split = 0 takes f32 rows; any other value returns
 *   SNAP_ERR_UNSUPPORTED. */
int snap_mlp2_pool_max_f32(const float* x, int64_t M, int32_t Cin, int32_t x_stride,
                           const int32_t* rows, const int32_t* row_count,
                           const void* w0_split, size_t w0_bytes, const float* b0, int32_t H,
                           const void* w1_split, size_t w1_bytes, const float* b1, int32_t D,
                           int32_t relu_in, int32_t x_split, int32_t Z, int64_t ncols,
                           float* plane, uint8_t* pvalid, void* stream);
/* Two row classes into ONE plane: `rows` as above, and `rows_z` (may be NULL) whose rows are
 * exactly zero over the 16-channel slabs [zero_slab_lo, zero_slab_lo + zero_slabs) of the
 * first Dense layer's input and need not hold them in memory (single-observation rows of a
 * lift with SnapLiftDesc.class_rows: the variance slabs).  Those slabs are not read and not
 * multiplied for that class -- a product with +0 leaves an f32 accumulator unchanged, so the
 * plane equals the one-list result bit for bit; max is order-independent across the two. */
int snap_mlp2_pool_max_classes_f32(const float* x, int64_t M, int32_t Cin, int32_t x_stride,
                                   const int32_t* rows, const int32_t* row_count,
                                   const int32_t* rows_z, const int32_t* row_count_z,
                                   int32_t zero_slab_lo, int32_t zero_slabs,
                                   const void* w0_split, size_t w0_bytes, const float* b0, int32_t H,
                                   const void* w1_split, size_t w1_bytes, const float* b1, int32_t D,
                                   int32_t relu_in, int32_t x_split, int32_t Z, int64_t ncols,
                                   float* plane, uint8_t* pvalid, void* stream);

/* The lift INSIDE the consumer (replaces k3-k6 for voxels with one visible observation:
 * streetview_encoder.py:69-105 gather, :141-178 pooling, :279-286 fusion MLP; bev_mapper.py:78-88 max):
 * `rows_g` lists voxels whose `pooled` row does not exist; tap_records [*, 8] u32
 * (snap_lift_pool_records_f32) hold their four-tap bilinear record, and the kernel gathers and blends
 * 16 channels of the four taps per GEMM0 slab while it stages the operand (mean = the observation,
 * variance slabs = 0: skipped, score slab from the record).  `rows` (several observations) are read
 * pre-split from x (SnapLiftDesc.out_split) as snap_mlp2_pool_max_classes_f32 does.  The plane equals
 * that entry point's bit for bit.  f_images [.., img_w, img_C] f32, f_bytes < 4 GB; Cin = 2 fd + 1,
 * feature_dim % 16 == 0; xcd_group: runs of that many 128-row tiles of rows_g per XCD (0: dispatch
 * order; results do not depend on it). */
int snap_mlp2_pool_max_gather_f32(const float* x, int64_t M, int32_t Cin, int32_t x_stride,
                                  const int32_t* rows, const int32_t* row_count,
                                  const int32_t* rows_g, const int32_t* row_count_g,
                                  const float* f_images, int64_t f_bytes, int32_t img_w,
                                  int32_t img_C, int32_t feature_dim, const uint32_t* tap_records,
                                  int32_t xcd_group, const void* w0_split, size_t w0_bytes,
                                  const float* b0, int32_t H, const void* w1_split, size_t w1_bytes,
                                  const float* b1, int32_t D, int32_t Z, int64_t ncols, float* plane,
                                  uint8_t* pvalid, void* stream);

/* y[m, 0..C) = value for every row with mask[m] == 0 (the masked voxels of a volume
 * whose observed rows were written through rows_out).  C % 4 == 0. */
int snap_fill_masked_rows_f32(float* y, const uint8_t* mask, int64_t M, int32_t C,
                              float value, void* stream);

/* pad_to_multiple (image_encoder.py:32-39) and optional zero channels in one pass:
 * x [N, H, W, C] -> y [N, H + pad_h, W + pad_w, C + pad_c], zeros bottom / right / extra channels. */
int snap_pad_image_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t pad_h,
                       int32_t pad_w, int32_t pad_c, float* y, void* stream);

/* Voxel-centre query points (bev_mapper.py:162-196): out [B, XY, Z, 3] = (xy[b, c, :], z[b, k]);
 * xy [XY, 2] (xy_batched = 0) or [B, XY, 2]; z [B, Z] (level heights per scene). */
int snap_voxel_points_f32(const float* xy, int32_t xy_batched, const float* z, int32_t B, int32_t XY,
                          int32_t Z, float* out, void* stream);

/* StdConv weight standardisation over (H,W,I) per output channel, eps inside the
 * sqrt (resnet.py:34-41,73-79).  w,out: [K, Cout]. */
int snap_weight_standardize_f32(const float* w, float* out, int32_t K,
                                int32_t Cout, float eps, void* stream);

/* All StdConv kernels of an encoder in one launch (training standardises ~53 kernels per
 * encoder every step; one launch per kernel is pure launch latency).  `items` is a DEVICE
 * array; item i owns workgroups [block_begin, block_begin + ceil(Cout / 32)) of the forward
 * and of the backward launch; items sorted by block_begin; total_blocks = sum.  Forward: out = standardise(w) (dws unused).
 * Backward (snap_weight_standardize_bwd_multi_f32): out = d w given dws = d standardise(w). */
typedef struct SnapWstdItem {
  const float* w;
  const float* dws;
  float* out;
  int32_t K, Cout, block_begin, reserved;
} SnapWstdItem;
int snap_weight_standardize_multi_f32(const SnapWstdItem* items, int32_t n_items,
                                      int32_t total_blocks, float eps, void* stream);
int snap_weight_standardize_bwd_multi_f32(const SnapWstdItem* items, int32_t n_items,
                                          int32_t total_blocks, float eps, void* stream);

/* GroupNorm statistics (resnet.py:46-60): two-pass mean / mean((x-mean)^2) over
 * (H,W,C/G) per (image, group).  relu_first != 0 computes them on relu(x)
 * (FPN order, image_encoder.py:80-83).  Outputs mu[N,C], sc[N,C] = rstd*gamma[c].
 * workspace: snap_group_norm_stats_workspace_bytes(N, HW, C, groups) bytes. */
/* Exact: no launch touches a byte beyond this size. */
size_t snap_group_norm_stats_workspace_bytes(int32_t N, int32_t HW, int32_t C,
                                             int32_t groups);
int snap_group_norm_stats_f32(const float* x, int32_t N, int32_t HW, int32_t C,
                              int32_t C_stride, int32_t groups, float eps,
                              int32_t relu_first, const float* gamma, float* mu,
                              float* sc, float* rstd /* optional [N,C] */,
                              void* workspace, size_t workspace_bytes,
                              void* stream);

/* Stand-alone GroupNorm apply (+optional ReLU before/after); used by tests and
 * for returning normalised tensors.  mode: SNAP_PRO_GN_RELU / SNAP_PRO_RELU_GN. */
int snap_group_norm_apply_f32(const float* x, float* y, int32_t N, int32_t HW,
                              int32_t C, const float* mu, const float* sc,
                              const float* beta, int32_t mode, void* stream);

/* 3x3 / stride 2 / pad 1 max-pool with -inf padding (resnet.py:99). NHWC. */
int snap_max_pool_3x3s2_f32(const float* x, float* y, int32_t N, int32_t H,
                            int32_t W, int32_t C, void* stream);

/* ------------------------------------------------------------------------- *
 * Lift: voxel -> view projection, top-K view selection, bilinear gather, depth
 * score interpolation and softmax-weighted multi-view pooling, fused.
 *   replaces snap/models/streetview_encoder.py:42-178 (k1-k5 of SURVEY 2.2) with
 *   snap/utils/geometry.py:52-69,198-221,260-280.
 * ------------------------------------------------------------------------- */
typedef struct SnapLiftDesc {
  int32_t B, V, h, w, C;       /* f_images [B,V,h,w,C], C = feature_dim + score bins */
  int32_t feature_dim;         /* 128 */
  int32_t num_bins;            /* 32  */
  int32_t N;                   /* voxels per scene */
  int32_t K;                   /* 0 => use all V views (interpolate_views_all),
                                  else top-K selection (V > K)                     */
  int32_t fisheye;             /* 1: FisheyeCamera, 0: pinhole Camera              */
  int32_t out_stride;          /* row stride (floats) of `pooled`, >= 2*fd+1, %4==0 */
  float depth_min, depth_max;  /* depth_min_max                                    */
  float max_view_distance;     /* < 0: disabled                                    */
  /* fusion options of pool_multiview_features (streetview_encoder.py:141-178); the reference
   * default is weighted = 1, use_variance = 1, add_minmax = 0 */
  int32_t weighted;            /* do_weighted_fusion: depth-score softmax weights + the
                                  score_max channel; 0: plain mean / variance (scores = None),
                                  f_images carries no score bins (C = feature_dim)  */
  int32_t use_variance;        /* fusion_use_variance                              */
  int32_t add_minmax;          /* fusion_add_minmax: + max, min over the valid views */
  /* traversal hint (results do not depend on it): the N points of a scene are the voxel
   * centres of an [N / (grid_y * grid_z), grid_y, grid_z] grid, level fastest
   * (bev_mapper.py:162-196); the kernel then walks 8 x 8 blocks of columns per XCD so that a
   * block's image taps stay in that XCD's L2.  0, 0 = unstructured points (query frustum). */
  int32_t grid_y, grid_z;
  /* 1: rows of `pooled` whose voxel no view sees are NOT written (their `valid` byte is 0;
   * the default options' batched kernel only) -- for consumers that read the rows of valid
   * voxels only (snap_mlp2_pool_max_f32, row-indexed conv launches).  0: zeros, as the
   * reference's pool_multiview_features returns. */
  int32_t valid_rows_only;
  /* 1: `pooled` rows are written pre-split for the split-bf16 engines instead of as f32:
   * row = [ceil(channels / 16) slabs][hi | lo][16] bf16 (64 B per slab; hi = bf16(v) RNE,
   * lo = bf16(v - hi)), out_stride (in floats) >= 16 * slabs -- what snap_mlp2_pool_max_f32
   * takes with x_split = 1.  Default fusion options, <= 4 selected views, feature_dim % 8 == 0. */
  int32_t out_split;
  /* 1 (with out_split; feature_dim % 16 == 0): rows are CLASSED by their number of visible
   * observations -- valid[] = 0 invalid, 1 one observation, 2 several -- and a one-observation
   * row does not write its variance slabs (slabs feature_dim/16 .. 2 feature_dim/16 - 1: the
   * weighted variance of a single observation is exactly 0; 72 % of the observed voxels of a
   * four-view map and every voxel of the query).  The consumer lists the two classes
   * separately (snap_compact_rows_range_u8) and skips those slabs for the first
   * (snap_mlp2_pool_max_classes_f32): 47 % fewer bytes written and re-read for such a row, same
   * plane bits (products with +0 leave an accumulator unchanged). */
  int32_t class_rows;
  /* A/B switches for tests and tools (0 = defaults).  Bit 0: snap_lift_pool_bwd_det_f32 takes the
   * half-wave-per-voxel record producer also where the batched one applies. */
  int32_t tune_flags;
} SnapLiftDesc;

/* cam: [B,V,11] = wh(2) f(2) c(2) k_radial(3) max_fov(1) tan(max_fov/2)(1) ALREADY scaled to
 * the feature-map resolution (the last entry is read by the fisheye path instead of
 * evaluating tanf per voxel and view: geometry.py:262 `radius < tan(0.5 * max_fov)`); Rt: [B,V,12] = R row-major (9) then t (3) of
 * T_view2scene; points: [B,N,3].
 * pooled: [B,N,out_stride] = mean(fd) | var(fd)? | max(fd), min(fd)? | score_max(1)? | zero pad
 * (default options: mean | var | score_max);  valid: [B,N] uint8. */
int snap_lift_pool_f32(const SnapLiftDesc* desc, const float* f_images,
                       const float* cam, const float* Rt, const float* points,
                       float* pooled, uint8_t* valid, void* stream);

/* The same with TAP RECORDS (class_rows, out_split and valid_rows_only set): a voxel with ONE visible
 * observation writes no row into `pooled` but tap_records[voxel][8] (u32) = byte offset of tap
 * (i0, j0) channel 0 in f_images | bit 8: i1 != i0, bit 9: j1 != j0 (the clamped upper taps), depth
 * bins | wi1 | wj1 (f32 bits) | depth score (f32 bits) | 0 0 0 -- streetview_encoder.py:93-124 for
 * that observation; its mean is the bilinear blend (softmax weight exactly 1), its variance 0.
 * snap_mlp2_pool_max_gather_f32 consumes the records.  Voxels with several observations write
 * their rows as above; valid[] carries the classes 0 / 1 / 2. */
int snap_lift_pool_records_f32(const SnapLiftDesc* desc, const float* f_images,
                               const float* cam, const float* Rt, const float* points,
                               float* pooled, uint8_t* valid, uint32_t* tap_records, void* stream);

/* depth_mlp fusion (streetview_encoder.py:263-267; do_weighted_fusion = False, so desc->weighted
 * = 0 and C = feature_dim): the lift in two passes around a per-observation MLP.
 *   observations: obs [B, N, S, fd + 4] = bilinear features | log10(clip(depth, 0.1, 100)) |
 *     unit ray in the camera frame (zero where the view does not see the point), S = K (top-K
 *     order) or V (view order); obs_feat [B, N, S, fd] = the features alone (the residual the
 *     caller adds the MLP output to); valid [B, N] as snap_lift_pool_f32.
 *   pool: pool_multiview_features(obs_feat', visible, scores = None, add_minmax, use_variance)
 *     of the corrected observations obs_feat' [B, N, S, fd] -> pooled [B, N, out_stride], valid. */
int snap_lift_observations_f32(const SnapLiftDesc* desc, const float* f_images, const float* cam,
                               const float* Rt, const float* points, float* obs, float* obs_feat,
                               uint8_t* valid, void* stream);
int snap_lift_pool_observations_f32(const SnapLiftDesc* desc, const float* cam, const float* Rt,
                                    const float* points, const float* obs_feat, float* pooled,
                                    uint8_t* valid, void* stream);

/* Debug/parity variant of k1: p2d[B,N,V,2] (ij), vis[B,N,V], depth[B,N,V]. */
int snap_project_points_f32(int32_t B, int32_t V, int32_t N, int32_t fisheye,
                            const float* cam, const float* Rt,
                            const float* points, float* p2d, uint8_t* vis,
                            float* depth, void* stream);

/* ------------------------------------------------------------------------- *
 * BEV: vertical pooling, modality fusion and matching head.
 *   replaces snap/models/bev_mapper.py:56-88 (k7), :225-252 (k8), :284-291 +
 *   snap/models/layers.py:45-52 (k9).
 * ------------------------------------------------------------------------- */
enum { SNAP_POOL_MAX = 0, SNAP_POOL_SUM = 1, SNAP_POOL_MEAN = 2 };

/* vol [M, Z, D] + vvalid [M, Z] -> plane [M, D], pvalid [M]. */
int snap_vertical_pool_f32(const float* vol, const uint8_t* vvalid, float* plane,
                           uint8_t* pvalid, int64_t M, int32_t Z, int32_t D,
                           int32_t pooling, void* stream);
/* The max pooling above (Z <= 64, D <= 128) that also records, per (column, channel), the level of the
 * maximum -- the first of equal ones, found with the comparisons of the VJP (`>` then `==` over the
 * valid levels in ascending order, a NaN never wins) -- and how many levels hold it (saturating at
 * 255): argz [M, D], ties [M, D] bytes (255 / 0 for a column without a valid level).  What
 * snap_vertical_pool_max_bwd_arg_f32 reads instead of the volume (VerticalPooling('max') in a
 * training step: snap/models/bev_mapper.py:56-88). */
int snap_vertical_pool_max_arg_f32(const float* vol, const uint8_t* vvalid, float* plane,
                                   uint8_t* pvalid, uint8_t* argz, uint8_t* ties, int64_t M,
                                   int32_t Z, int32_t D, void* stream);

/* Fuse `num_planes` modality planes (planes[i] [M,D], valids[i] [M] or NULL=all
 * valid) with masked max/sum/mean, then matching head: Dense(D->Dm)+bias, L2
 * normalise (eps), mask.  fused [M,D], fvalid [M], matching [M,Dm] (may be NULL
 * with Wm NULL). */
int snap_plane_fuse_match_f32(const float* const* planes,
                              const uint8_t* const* valids, int32_t num_planes,
                              int64_t M, int32_t D, int32_t pooling, float* fused,
                              uint8_t* fvalid, const float* Wm, const float* bm,
                              int32_t Dm, int32_t normalize, float eps,
                              float* matching, void* stream);

/* ------------------------------------------------------------------------- *
 * Pose: point-vs-map similarity, sampling, scoring, refinement.
 *   replaces snap/models/bev_localizer.py:157-173 (k10),
 *   snap/models/pose_estimation.py:126-165 (k11), :49-82 (k12), :168-205 (k13).
 * ------------------------------------------------------------------------- */
#define SNAP_SIM_CHUNK 64  /* cells per (max, sum) softmax chunk == one wave64 */

/* sim[B,Nq,XY] = relu(fq . fm) * scale / num_valid[b]  (relu iff clip_negative);
 * chunk_stats[B,Nq,ceil(XY/64),2] = per-chunk (max, sum exp(x - max)) of the
 * UN-normalised x = relu(.)*scale: enough to evaluate / sample
 * prob = softmax_XY(x) / num_valid without a second [B,Nq,XY] tensor.
 * Optional (may both be NULL): rowstats[B,Nq,2] = (row max, row sum) and
 * prob[B,Nq,XY] = the full prob_points tensor (needs rowstats).
 * num_valid: [B] float, already clipped to >= 1 (bev_localizer.py:171). */
int snap_sim_softmax_f32(const float* fq, const float* fm, int32_t B, int32_t Nq,
                         int32_t XY, int32_t Dm, float scale,
                         int32_t clip_negative, const float* num_valid,
                         float* sim, float* chunk_stats, float* prob,
                         float* rowstats, void* stream);

/* Bytes of the optional rowstats [B, Nq, 2] buffer of the similarity entry points (caller-owned). */
size_t snap_sim_rowstats_bytes(int32_t B, int32_t Nq);

/* add_confidence_query (bev_localizer.py:165-168): the 1 / num_valid normalisation of sim (and
 * prob) is replaced by per-point weights row_weight[B, Nq] = layers.masked_softmax(bev_confidence
 * of the query points, valid points).  row_weight == NULL is snap_sim_softmax_f32. */
int snap_sim_softmax_weighted_f32(const float* fq, const float* fm, int32_t B, int32_t Nq,
                                  int32_t XY, int32_t Dm, float scale, int32_t clip_negative,
                                  const float* num_valid, const float* row_weight, float* sim,
                                  float* chunk_stats, float* prob, float* rowstats, void* stream);
/* The same sim / chunk_stats with the Nq x XY x Dm contraction on the bf16 matrix cores at f32
 * grade: fq / fm are split into `parts` bf16 parts per element (3: six products per MAC, ~2^-24
 * per product -- the arithmetic of the conv engine's 'bf16x6'; 2: three products, ~2^-17) into
 * `workspace` first.  Dm in {16, 32, 64}.  (prob / rowstats: use snap_sim_softmax_weighted_f32.)
 * XY % 256 == 0 takes a leaner kernel with the same bits; clip_negative bit 1 (value 2) pins the
 * general kernel (tests compare the two). */
size_t snap_sim_split_workspace_bytes(int32_t B, int32_t Nq, int32_t XY, int32_t Dm, int32_t parts);
int snap_sim_softmax_split_f32(const float* fq, const float* fm, int32_t B, int32_t Nq, int32_t XY,
                               int32_t Dm, float scale, int32_t clip_negative,
                               const float* num_valid, const float* row_weight, int32_t parts,
                               float* sim, float* chunk_stats, void* workspace,
                               size_t workspace_bytes, void* stream);
/* layers.masked_softmax over the last axis (snap/models/layers.py:38-43: an all-false mask acts
 * as all-true) of x [B, N] + its inclusive CDF (the sampler's distribution over query points). */
int snap_masked_softmax_rows_f32(const float* x, const uint8_t* mask, int32_t B, int32_t N,
                                 float* weights, float* cdf, void* stream);
/* bev_confidence = where(valid, log_sigmoid(features . w + bias), 0)  (Dense(1) head of the BEV
 * plane, bev_mapper.py:154-157,292-295).  features [M, D], D % 4 == 0; valid may be NULL. */
int snap_confidence_head_f32(const float* features, const uint8_t* valid, const float* w,
                             const float* bias /* DEVICE scalar */, int64_t M, int32_t D, float* out,
                             void* stream);
/* Its VJP: d features [M, D] = ds w; prod [M, D] = ds f and dsv [M, 4] = (ds, 0, 0, 0) are the
 * per-row terms whose fixed-order column sums (snap_colsum_f32) are d w and d bias;
 * ds = dconf * sigmoid(-(f . w + bias)) * [valid]. */
int snap_confidence_head_bwd_f32(const float* features, const uint8_t* valid, const float* w,
                                 const float* bias, const float* dconf, int64_t M, int32_t D,
                                 float* dfeatures, float* prod, float* dsv, void* stream);
/* add_confidence_query (bev_localizer.py:165-168), training: rowdot[b, n] = sum_cells dsim * sim
 * (the row's share of the temperature gradient; / weight = the gradient of the point weight), then
 * dsim = dsim * [sim > 0] * row_coef[b, n] in place; and the VJP of layers.masked_softmax
 * (layers.py:38-43): dx = w * (dw - sum_n w dw). */
int snap_sim_bwd_prepare_rows_f32(float* dsim, const float* sim, int32_t B, int32_t Nq, int32_t XY,
                                  int32_t clip_negative, const float* row_coef, float* rowdot,
                                  void* stream);
int snap_masked_softmax_rows_bwd_f32(const float* weights, const float* dweights, int32_t B,
                                     int32_t N, float* dx, void* stream);

/* Draw S correspondences per scene ~ prob_points (iid categorical; counter-based
 * Philox4x32-10 keyed by (seed, b, s)).  corr[B,S,3] = (n, i, j).
 * If uniforms != NULL ([B,S,2] in [0,1)), they replace the Philox draws (tests). */
int snap_ransac_sample_f32(const float* fq, const float* fm,
                           const float* chunk_stats, int32_t B, int32_t Nq,
                           int32_t X, int32_t Y, int32_t Dm, float scale,
                           int32_t clip_negative, int32_t S, uint64_t seed,
                           const float* uniforms, int32_t* corr, void* stream);

/* Same samples, faster: with a workspace (snap_ransac_sample_workspace_bytes) the per-row
 * prefix of the chunk masses is built once per row instead of once per sample (~34 samples
 * share a row at the default sizes).  Bit-identical output. */
size_t snap_ransac_sample_workspace_bytes(int32_t B, int32_t Nq);
/* ... with sim [B, Nq, X*Y] (the tensor snap_sim_softmax*_f32 wrote) and row_unscale [B, Nq]
 * (num_valid[b], or 1 / row_weight[b, n]: x = sim * row_unscale) the selected chunk's 64 scores
 * are READ (256 contiguous bytes) instead of re-evaluated from 8 KB of map features; both NULL =
 * re-evaluate.  Same distribution; the scores agree to one rounding. */
int snap_ransac_sample_sim_f32(const float* fq, const float* fm, const float* chunk_stats,
                               const float* row_cdf, const float* sim, const float* row_unscale,
                               int32_t B, int32_t Nq, int32_t X, int32_t Y, int32_t Dm, float scale,
                               int32_t clip_negative, int32_t S, uint64_t seed,
                               const float* uniforms, int32_t* corr, void* workspace,
                               size_t workspace_bytes, void* stream);
/* ... with row_cdf [B, Nq] (inclusive, from snap_masked_softmax_rows_f32) the query point of a
 * sample is drawn from that distribution instead of uniformly (confidence-weighted prob_points). */
int snap_ransac_sample_rows_f32(const float* fq, const float* fm, const float* chunk_stats,
                                const float* row_cdf, int32_t B, int32_t Nq, int32_t X, int32_t Y,
                                int32_t Dm, float scale, int32_t clip_negative, int32_t S,
                                uint64_t seed, const float* uniforms, int32_t* corr,
                                void* workspace, size_t workspace_bytes, void* stream);
int snap_ransac_sample_ws_f32(const float* fq, const float* fm, const float* chunk_stats,
                              int32_t B, int32_t Nq, int32_t X, int32_t Y, int32_t Dm,
                              float scale, int32_t clip_negative, int32_t S, uint64_t seed,
                              const float* uniforms, int32_t* corr, void* workspace,
                              size_t workspace_bytes, void* stream);

/* snap_pose_score_f32 for pose sets CLUSTERED around one centre pose per scene -- the 41^3
 * refinement lattice of grid_refinement (pose_estimation.py:168-205): every pose of scene b maps every
 * query point to within `radius_cells` cells of where centers[b] (angle, tx, ty) maps it (the caller
 * guarantees it: |t - t_c| / cell + max |q| * |angle - angle_c| / cell, rounded up, + 1).  A point's
 * score plane is then read as ONE window of <= (2 r + 3) x (2 r + 6) cells instead of whole, once per
 * pose chunk (256 x 256 maps: 27 KB instead of 262 KB per point).  Same arithmetic per sample and the
 * same order of every sum as snap_pose_score_f32 (mask_oob = 0): the scores are the same bits.
 * snap_pose_score_window_supported: 1 when the window of that radius fits the kernel's LDS buffers
 * (else call snap_pose_score_f32).  A pose outside the promised radius reads a clamped cell of the
 * window (a wrong score, never out of bounds). */
/* snap_pose_score_workspace_bytes + the per-scene centre table (B x 4 floats) + 16 bytes that let the table start
 * 16-byte aligned behind the partial sums; no launch touches a byte beyond this size. */
size_t snap_pose_score_window_workspace_bytes(int32_t B, int32_t Nq, int32_t P, int32_t X, int32_t Y);
int32_t snap_pose_score_window_supported(int32_t X, int32_t Y, int32_t radius_cells);
int snap_pose_score_window_f32(const float* sim, const float* poses, const float* centers,
                               int32_t radius_cells, const float* q_xy, const uint8_t* valid_q,
                               int32_t B, int32_t Nq, int32_t X, int32_t Y, int32_t P, float cell_size,
                               float* scores, void* workspace, size_t workspace_bytes, void* stream);

/* corr[B,P*retries*2,3] -> poses[B,P,3] = (angle, tx, ty) of map_t_query:
 * most distance-consistent retry, 2-point Kabsch (pose_estimation.py:146-165). */
int snap_poses_from_corr_f32(const int32_t* corr, const float* q_xy, int32_t B,
                             int32_t Nq, int32_t P, int32_t retries,
                             float cell_size, float* poses, void* stream);

/* scores[B,P] = sum_n valid_q[b,n] * bilinear(sim[b,n], (R(theta) q_xy[n] + t)/cell)
 * (pose_estimation.py:63-82).  poses[B,P,3]; map_valid [B,X,Y] only read when
 * mask_oob != 0.  workspace: snap_pose_score_workspace_bytes(B,Nq,P,X,Y). */
/* Exact: no launch touches a byte beyond this size. */
size_t snap_pose_score_workspace_bytes(int32_t B, int32_t Nq, int32_t P,
                                       int32_t X, int32_t Y);
int snap_pose_score_f32(const float* sim, const float* poses, const float* q_xy,
                        const uint8_t* valid_q, const uint8_t* map_valid,
                        int32_t B, int32_t Nq, int32_t X, int32_t Y, int32_t P,
                        float cell_size, int32_t mask_oob, float* scores,
                        void* workspace, size_t workspace_bytes, void* stream);

/* out[B,nr*np*np,3] = init[b] o offset(ir,ix,iy)  (pose_estimation.py:178-193).
 * offs_r[nr] (radians), offs_p[np] (metres). */
int snap_refine_lattice_f32(const float* init, const float* offs_r,
                            const float* offs_p, int32_t B, int32_t nr,
                            int32_t np_, float* out, void* stream);

/* Row-wise argmax with first-index tie-break: idx[B] over scores[B, start:P].  NaN is the maximum and the
 * first NaN wins (np.argmax / jnp.argmax). */
int snap_argmax_rows_f32(const float* scores, int32_t B, int32_t P, int32_t start,
                         int32_t* idx, void* stream);

/* ------------------------------------------------------------------------- *
 * Exhaustive voting: rotated templates + direct correlation.
 *   replaces snap/models/pose_exhaustive_voting.py:37-69 (k14), :72-104 (k15).
 * ------------------------------------------------------------------------- */
/* feat[H,W,D], valid[H,W] (H==W), tfm[R/4,4] = (cos, sin, tx, ty) of
 * templates_t_grid for the first quadrant of rotations ->
 * templates[R,H,W,D], tvalid[R,H,W]; also the engine-layout copies
 * tw[H,W,D,R] (HWIO; R % 4 == 0) and cw[H,W,1,R] = 180-degree-rotated tvalid as
 * float (the reference's un-flipped mask convolution,
 * pose_exhaustive_voting.py:97-99); tcount[R] = sum(tvalid[r]). */
int snap_rotate_templates_f32(const float* feat, const uint8_t* valid,
                              const float* tfm, int32_t H, int32_t W, int32_t D,
                              int32_t R, float cell_size, float* templates,
                              uint8_t* tvalid, float* tw, float* cw,
                              float* tcount, void* stream);

/* map[H,W,D], mvalid[H,W] -> map_pad[3H-2,3W-2,D] (edge), mvalid_pad[3H-2,3W-2]
 * (zero padded, as float). */
/* Shift-stacked filter bank for the exhaustive correlation: tw [H, W, D, R] (HWIO) ->
 * tws [H+S-1, W+S-1, D, R*S*S], tws[i', j', d, (r*S + sa)*S + sb] = tw[i'-sa, j'-sb, d, r]
 * (zero outside).  A stride-S snap_conv2d over the padded map with tws computes, at output
 * pixel (a4, b4) and channel (r, sa, sb), exactly the direct-form output (r, S a4 + sa,
 * S b4 + sb) of pose_exhaustive_voting.py:86-91 -- same products, full 64-wide GEMM tiles
 * instead of R = 36 columns. */
int snap_stack_templates_f32(const float* tw, float* tws, int32_t H, int32_t W, int32_t D,
                             int32_t R, int32_t S, void* stream);
/* The same bank from the [R, H, W, D] template tensor of snap_rotate_templates_f32 (whose `tw`
 * output may then be NULL: the r-fastest HWIO copy is only needed by the unstacked path). */
int snap_stack_templates_rhwd_f32(const float* templates, float* tws, int32_t H, int32_t W,
                                  int32_t D, int32_t R, int32_t S, void* stream);
/* ... and written DIRECTLY as the split engine's two-part weight image of that bank (what
 * snap_conv2d_pack_weights_split_bf16(tws, taps = (H+S-1)(W+S-1), Cin = D, Cout = R S^2, parts = 2)
 * would produce, bit for bit): the f32 bank is never materialised.  out:
 * snap_conv2d_packed_weights_split_bytes(taps, D, R S^2, 2) bytes, 16-byte aligned; D % 4 == 0. */
int snap_pack_stacked_templates_split_bf16(const float* templates, int32_t H, int32_t W, int32_t D,
                                           int32_t R, int32_t S, void* out, size_t out_bytes,
                                           void* stream);
int snap_pad_map_f32(const float* map, const uint8_t* mvalid, int32_t H, int32_t W,
                     int32_t D, float* map_pad, float* mvalid_pad, void* stream);

/* Frequency-domain template matching (snap/models/pose_exhaustive_voting.py:72-104, padded mode) in
 * ONE call: templates[R,H,W,D] (zero where tvalid is 0), tvalid[R,H,W], map[Hm,Wm,D], mvalid[Hm,Wm],
 * tcount[R] = q_valid.sum((-1,-2)) -> scores[R, 3Hm-1-H, 3Wm-1-W]:
 *   scores[r,a,b] = sum_ijd templates[r,i,j,d] * edge_pad(map)[a+i, b+j, d]            (:82-91)
 *   -inf where the overlap count (the 180-degree rotated template mask correlated with the
 *   zero-padded map mask, :93-101) is <= overlap_threshold (= min_overlap * H * W) if use_overlap,
 *   then / tcount[r]                                                                    (:103).
 * The correlation is evaluated as FFT products (channel pairs packed as complex numbers, mixed-radix
 * 2/3/4 transforms of 2^a or 3*2^a points per axis in LDS, f32): ~1e-6 relative to the largest
 * score instead of the direct form's summation order -- snap_conv2d_* on the stacked template bank
 * remains the direct form (and the checker).  The overlap count is rounded to the nearest integer
 * (operands are 0/1): the -inf mask is the direct form's.
 * workspace: snap_voting_fft_workspace_bytes() bytes, 256-byte aligned; 0 = unsupported geometry
 * (3*max(Hm,Wm)-2 > 1024 points per axis), for which snap_voting_fft_f32 returns
 * SNAP_ERR_UNSUPPORTED.  templates / map 8-byte aligned. */
size_t snap_voting_fft_workspace_bytes(int32_t R, int32_t H, int32_t W, int32_t D, int32_t Hm,
                                       int32_t Wm);
int snap_voting_fft_f32(const float* templates, const uint8_t* tvalid, const float* map,
                        const uint8_t* mvalid, const float* tcount, int32_t R, int32_t H, int32_t W,
                        int32_t D, int32_t Hm, int32_t Wm, float overlap_threshold,
                        int32_t use_overlap, void* workspace, size_t workspace_bytes, float* scores,
                        void* stream);

/* exhaustive_pose_voting (snap/models/pose_exhaustive_voting.py:107-124) in one call: the query plane
 * feat[H,H,D] (already multiplied by its confidence), valid[H,H], tfm[R/4,4] = (cos, sin, tx, ty) of
 * templates_t_grid for the first quadrant of rotations (:44-50), cell_size; map[Hm,Wm,D],
 * mvalid[Hm,Wm] -> scores[R, 3Hm-1-H, 3Wm-1-H]; overlap_threshold = min_overlap * H * H (0.05 in the reference)
 * formed by the caller in double, as for snap_voting_fft_f32: an f32 min_overlap cannot carry the reference's
 * rule (f32(0.02) * 400 < 8 = 0.02 * 400 in double: a count of 8 would pass).
 * sample_query_templates (:37-69) runs inside the first transform: template rows are interpolated on
 * the fly with the arithmetic of snap_rotate_templates_f32 (bit for bit), rotations R/4..R-1 are rot90
 * index maps; the [R,H,H,D] template tensor is never written.  R % 4 == 0, square query plane.
 * workspace: snap_voting_fft_workspace_bytes(R, H, H, D, Hm, Wm). */
int snap_voting_fft_rotated_f32(const float* feat, const uint8_t* valid, const float* tfm,
                                float cell_size, const float* map, const uint8_t* mvalid, int32_t R,
                                int32_t H, int32_t D, int32_t Hm, int32_t Wm, float overlap_threshold,
                                void* workspace, size_t workspace_bytes, float* scores, void* stream);

/* raw[Ho,Wo,Rp], cnt[Ho,Wo,Rp] (engine outputs) -> scores[R,Ho,Wo]:
 * -inf where cnt <= min_overlap*H*W (if min_overlap >= 0), then / tcount[r]. */
int snap_template_finalize_f32(const float* raw, const float* cnt,
                               const float* tcount, int32_t Ho, int32_t Wo,
                               int32_t R, int32_t Rp, float overlap_threshold,
                               int32_t use_overlap, float* scores, void* stream);

/* The K best pose hypotheses of a vote volume, with non-maximum suppression: what turns the scores of
 * exhaustive_pose_voting (snap/models/pose_exhaustive_voting.py:107-137: the volume, and one index -> one
 * transform) into a ranked list of distinct poses.  votes[R,Ho,Wo] f32 of any shape (not tied to the voting's
 * geometry), flat(r,a,b) = (r*Ho + a)*Wo + b.
 *   PEAK: a cell c whose value is a number > -inf and which, for EVERY other cell n of its window
 *     |dr| <= radius_r (circular: r-1 of 0 is R-1), |da| <= radius_xy, |db| <= radius_xy (clipped at the
 *     border: cells outside do not exist), has v(c) > v(n) or (v(c) == v(n) and flat(c) < flat(n)).
 *     A NaN vote is never a peak and compares like -inf as a neighbour; +inf is an ordinary large value;
 *     == is the float comparison (-0 == +0).  Exactly one peak survives on any plateau of equal values.
 *   SELECTION: the K peaks of greatest value, ordered by value descending, then flat ascending.
 *   index[K,3] = (r, a, b); score[K] = the bits of the vote itself; count[2] = {peaks found, clipped to K;
 *     NaN votes in the volume}.  Rows past the found count: index -1,-1,-1 and score -inf.
 * Every output element is written by every call, and nothing depends on workgroup scheduling (no atomics:
 * per-workgroup candidates are ranked by their unique (value, flat) keys and merged in a fixed order).
 * Supported: 1 <= K <= 64, 0 <= radius_r <= 2 with 2*radius_r+1 <= R, 1 <= radius_xy <= 4, R*Ho*Wo < 2^31;
 * anything else returns SNAP_ERR_BAD_SHAPE before any launch (a NULL pointer SNAP_ERR_NULL, a short or not
 * 8-byte aligned workspace SNAP_ERR_WORKSPACE).  workspace: snap_vote_peaks_workspace_bytes() bytes (0 =
 * unsupported arguments); it needs no initialisation and no launch touches a byte beyond that size.
 * Only radius (1, 1) runs a kernel body with compile-time radii (unrolled window loops); every other setting
 * runs the same body with run-time radii: the same results, measured separately (profiles/vote_peaks_bench.json). */
size_t snap_vote_peaks_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t K, int32_t radius_r,
                                       int32_t radius_xy);
int snap_vote_peaks_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, int32_t K, int32_t radius_r,
                        int32_t radius_xy, int32_t* index, float* score, int32_t* count, void* workspace,
                        size_t workspace_bytes, void* stream);

/* The pose DISTRIBUTION of a vote volume: what the exhaustive path (snap/models/pose_exhaustive_voting.py:108-124:
 * the volume) needs to report a normalised posterior, its xy heat map and yaw histogram (snap/utils/grids.py:140-153:
 * the interpolation of a grid at a continuous index) and the negative log-likelihood of a ground-truth pose, the
 * counterpart of the sampled path's localization/nll (snap/models/bev_localizer.py:244-278).
 * votes[R,Ho,Wo] f32 unnormalised log-scores, flat(r,a,b) = (r*Ho + a)*Wo + b; scale: a finite float > 0 (the
 * temperature multiplier) with |scale * v| below the f32 maximum for every finite v (not checked; beyond it the
 * cell still counts as contributing and the outputs are NaN).
 *   A cell CONTRIBUTES iff its vote is finite.  -inf cells are masked and silently excluded (template_finalize's
 *   low-overlap mark); NaN and +inf cells are excluded and counted.  With x = scale * v over the contributing set F:
 *   log_z = log sum_F exp(x);
 *   log_prob_xy[Ho,Wo]: log sum_r exp(x[r,a,b]) - log_z, -inf where no rotation contributes;
 *   log_prob_r[R]:      log sum_ab exp(x[r,a,b]) - log_z, -inf where no pixel contributes (a rotation's cells
 *     enter its sum as f32 weights relative to their 256-pixel tile's maximum: a cell more than ~87 below that
 *     maximum underflows, so a rotation ALL of whose cells lie that far below their tiles' maxima also reads -inf;
 *     its probability is then below R*Ho*Wo*2^-126);
 *   with p = exp(x - log_z): E[a], E[b]; the central second moments Var a, Cov ab, Var b (index units);
 *   C = E[cos(2 pi r / R)], S = E[sin(2 pi r / R)]; the circular mean rotation index atan2(S, C) R / (2 pi) wrapped
 *   into [0, R); the resultant length hypot(C, S); the entropy log_z - E[x].
 *   stats[16] = { 0: log_z, 1: max x over F, 2: E[a], 3: E[b], 4: Var a, 5: Cov ab, 6: Var b, 7: C, 8: S,
 *                 9: mean rotation index, 10: resultant length, 11: entropy, 12: log_prob_gt, 13-15: written as 0 }.
 *   count[3] = { contributing cells; NaN or +inf cells; 1 if the ground-truth sample is valid, else 0 }.
 *   gt_index: NULL, or a DEVICE pointer to f32 [3] = (k, i, j) as exhaustive_tfm_to_index returns it, read by the
 *   kernel (no host synchronisation).  log_prob_gt = the trilinear interpolation of x at (k, i, j) minus log_z:
 *   circular in k (taps floor(k) mod R and (floor(k) + 1) mod R), taps floor and floor + 1 in i and j; a tap of
 *   weight exactly 0 is not read (so i = Ho-1 and j = Wo-1 are inside).  Valid iff k, i, j are finite,
 *   0 <= i <= Ho-1, 0 <= j <= Wo-1 and every tap of non-zero weight contributes; otherwise (and with NULL)
 *   log_prob_gt = NaN and count[2] = 0.
 *   F empty: log_z = max x = -inf, both marginals all -inf, stats[2..12] NaN.
 * The volume is read from HBM once (each workgroup walks its own 256 pixels' cells twice).  Sums of one pixel's
 * <= R terms and of one wave's 64 pixels of one rotation are f32, everything above is float64; every output is a
 * float64 expression rounded to f32 once.  No atomics: every reduction order is fixed by (R, Ho, Wo), so two calls
 * give the same bits.  Every output element is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31; anything else returns SNAP_ERR_BAD_SHAPE before any launch
 * (a NULL pointer other than gt_index SNAP_ERR_NULL; a scale that is not a finite number > 0 SNAP_ERR_UNSUPPORTED; a
 * short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE).  workspace: snap_vote_posterior_workspace_bytes() bytes
 * (0 = unsupported shape); it needs no initialisation and no launch touches a byte beyond that size.  Asynchronous
 * on `stream`; the caller owns every buffer. */
size_t snap_vote_posterior_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo);
int snap_vote_posterior_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale,
                            const float* gt_index, float* log_prob_xy, float* log_prob_r, float* stats,
                            int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* Multi-frame FUSION of aligned vote volumes: N query frames with known relative motion vote into the same map, and
 * the anchor frame's pose (r, a, b) puts frame n at the index (r + dk, a + da, b + db) with (dk, da, db) a function
 * of (n, r) alone (pose_exhaustive_voting.sequence_shift_table: the composition m_t_qn = m_t_q0 @ q0_t_qn pushed
 * through snap/models/pose_exhaustive_voting.py:127-149).  The result is again a vote volume.
 * volumes[N,R,Ho,Wo] f32 unnormalised log-scores (-inf = masked, as template_finalize writes it); shifts[N,R,3] f32
 * on the DEVICE = (dk, da, db); weights[N] f32 on the DEVICE, or NULL for all 1; fused[R,Ho,Wo] f32;
 * count[2] = { finite cells of `fused`; NaN cells of `fused` }.
 *   POSITION.  Each of the three shifts d is split ONCE, in f32: l = floorf(d), f = d - l (one f32 subtraction; where
 *   it rounds to 1, a tiny negative d, l += 1 and f = 0).  With these, frame n is sampled for output cell (r, a, b) at
 *   k' = r + lk + fk, a' = a + la + fa, b' = b + lb + fb; the integer parts are exact.
 *   TAPS.  In k: k0 = (r + lk) mod R and k1 = (k0 + 1) mod R with factors (1 - fk, fk); in a: a + la and a + la + 1
 *   with (1 - fa, fa); in b alike; 1 - f is one f32 subtraction.  A tap's weight is the f32 product
 *   (k factor * a factor) * b factor.  A tap one of whose factors is exactly 0 (an upper tap of an axis with f = 0) is
 *   NOT READ: an integer shift reads one cell, and a' = Ho-1 is inside.  (A weight that underflows to 0 from non-zero
 *   factors is still a tap.)
 *   A frame is IN RANGE at a cell iff its shift row is finite and 0 <= a' <= Ho-1 and 0 <= b' <= Wo-1; a frame that
 *   is not in range reads no tap.  Its sample is VALID iff it is in range and every tap is finite.
 *   VALUE.  If any tap of any in-range frame is NaN or +inf: NaN (0x7fc00000), whatever the other frames.  Otherwise,
 *   if any frame's sample is not valid (out of range, or a -inf tap): -inf -- the fused score exists only where EVERY
 *   frame sees the pose.  Otherwise sum_n w_n * blend_n in f32, in this order: blend_n = fma(weight_t, tap_t, blend_n)
 *   over the taps present in the order t = 4 kk + 2 aa + bb (k-major, then a, then b), fused = fma(w_n, blend_n, fused)
 *   over n ascending, both starting from -0 (so a single tap of weight 1 keeps its bits).  A weight w_n = 0 still
 *   applies the validity rule.  count is taken from the values written (an overflow to +-inf or a NaN weight counts as
 *   what it produced).
 * No atomics: count is the fixed-order fold of per-workgroup partials in a last small launch; two calls give the same
 * bits.  Every element of fused and count is written by every call.
 * Supported: 1 <= N <= 16, 1 <= R <= 64, Ho, Wo >= 1, N*R*Ho*Wo < 2^31; anything else returns SNAP_ERR_BAD_SHAPE
 * before any launch (a NULL pointer other than weights SNAP_ERR_NULL, checked first; a short or not 8-byte aligned
 * workspace SNAP_ERR_WORKSPACE).  workspace: snap_vote_fuse_workspace_bytes() bytes (0 = unsupported shape): the
 * [N][R] table of 64-byte entries and the per-workgroup counts; it needs no initialisation and no launch touches a
 * byte beyond that size.  Three launches, asynchronous on `stream`; the caller owns every buffer. */
size_t snap_vote_fuse_workspace_bytes(int32_t N, int32_t R, int32_t Ho, int32_t Wo);
int snap_vote_fuse_f32(const float* volumes, const float* shifts, const float* weights, int32_t N, int32_t R,
                       int32_t Ho, int32_t Wo, float* fused, int32_t* count, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Recursive pose FILTER over vote volumes (a histogram filter on the (r, a, b) lattice): one belief volume is carried
 * from frame to frame.  PREDICT transports the belief by the odometry increment and diffuses it by the odometry's
 * uncertainty; UPDATE multiplies by the new frame's votes and normalises.  The result is again a log-space vote volume
 * (-inf = impossible pose) for snap_vote_peaks_f32 / snap_vote_posterior_f32.
 * belief[R,Ho,Wo] f32 log-space, or NULL (no predict: the prior is uniform, exactly as uniform_mix = 1);
 * votes[R,Ho,Wo] f32; on the DEVICE: taps_k[Tk] f32 with first offset lk, taps_a[R,Ta] / taps_b[R,Tb] f32 and
 * offsets[R,2] i32 = (la, lb), the first offsets per OUTPUT rotation (pose_exhaustive_voting.motion_taps);
 * belief_out[R,Ho,Wo] f32 (must not overlap belief or votes: it holds intermediates during the call); stats[4] f32;
 * count[4] i32.
 *   TAPS (precondition, not checked): every tap is finite and >= 0, and either 0 or >= 2^-20.
 *   PREDICT.  M = the largest finite value of belief (exact).  A NaN or +inf cell is a caller error: no mass, counted.
 *   d = belief - M is ONE f32 subtraction; the cell has the mass p = fl32(exp((double)d)) iff d >= -40, else exactly 0
 *   (-inf cells, and anything below e^-40 of the peak): with the tap precondition every partial product below is a
 *   normal f32 number.  Three passes, in this order, each an f32 fma chain over its taps ascending, from 0, the
 *   intermediate volumes stored as f32:
 *     t0[r,a,b] = sum_tk taps_k[tk]   * p [(r + lk + tk) mod R, a, b]    (mathematical modulo: k is circular);
 *     t1[r,a,b] = sum_ta taps_a[r,ta] * t0[r, a + la[r] + ta, b];
 *     t2[r,a,b] = sum_tb taps_b[r,tb] * t1[r, a, b + lb[r] + tb];
 *   a source row / column outside the volume contributes 0 (the mass that leaves is lost).  The rotation pass works at
 *   the source cell and the xy passes use the output rotation's tables, as in snap_vote_fuse_f32.  S = sum t2, float64.
 *   UPDATE, float64 per cell, n = R*Ho*Wo, eps = uniform_mix: prior = ((1 - eps) * t2) / S + eps / n (the first term
 *   is 0 when S == 0 and with belief == NULL); u = (double)scale * votes + log(prior), log(0) = -inf; a -inf vote
 *   gives -inf; a NaN or +inf vote gives NaN (0x7fc00000) and the cell is left out of the normalisation;
 *   log_z = log sum exp(u) over the finite cells (float64); belief_out = fl32(u - log_z).  When no cell is finite,
 *   log_z = -inf and every cell that is not NaN is -inf.
 *   stats = { log_z (the log evidence of the frame under the predicted prior); S / sum p, the share of the mass that
 *   stayed in the volume (1 with belief == NULL, 0 when no cell has mass); M (-inf with belief == NULL or without a
 *   finite cell); the largest belief_out (NaN cells aside; -inf when there is none) }.
 *   count = { finite cells of belief_out; NaN or +inf cells of belief; NaN cells of belief_out; cells of belief with
 *   mass } (the belief's counts are 0 with belief == NULL).
 * Seven launches of min(R * ceil(Ho*Wo/256), 2048) workgroups of 256 threads (the last: one workgroup; three with
 * belief == NULL), a tile = one rotation and 256 consecutive pixels: the peak; the rotation pass with exp fused; the
 * row pass; the column pass; the evidence (log_z); the normalisation; the statistics.  t0 and t2 live in belief_out, t1
 * in the workspace.  No atomics: everything above the cell is float64 (counts int32) in an order fixed by (R, Ho, Wo),
 * so two calls give the same bits.  Every element of belief_out, stats and count is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, 1 <= Tk <= 16, 1 <= Ta, Tb <= 32; anything else returns
 * SNAP_ERR_BAD_SHAPE before any launch (a NULL pointer other than belief SNAP_ERR_NULL, checked first; a scale that is
 * not a finite number > 0 or a uniform_mix outside [0, 1] SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace
 * SNAP_ERR_WORKSPACE).  workspace: snap_vote_filter_workspace_bytes() bytes (0 = unsupported shape): t1 and the
 * per-workgroup partials; it needs no initialisation and no launch touches a byte beyond that size.  Asynchronous on
 * `stream`; the caller owns every buffer. */
size_t snap_vote_filter_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb);
int snap_vote_filter_f32(const float* belief, const float* votes, const float* taps_k, int32_t lk, const float* taps_a,
                         const float* taps_b, const int32_t* offsets, int32_t R, int32_t Ho, int32_t Wo, int32_t Tk,
                         int32_t Ta, int32_t Tb, float scale, float uniform_mix, float* belief_out, float* stats,
                         int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* Backward SMOOTHING step of the pose filter above (the other half of a histogram filter): from the filtered belief
 * of frame t and the smoothed belief of frame t+1 to the smoothed belief of frame t, p(x_t | all frames).  Run over
 * the stored beliefs of a track from the last frame (whose smoothed belief is its filtered one) to the first.
 * belief[R,Ho,Wo] f32 = the filter's belief_out at frame t (log alpha_t); next[R,Ho,Wo] f32 = the smoothed belief of
 * frame t+1 (log gamma_{t+1}); taps_k, lk, taps_a, taps_b, offsets: the very tables snap_vote_filter_f32 was given for
 * the step from t to t+1 (same layout, same precondition); uniform_mix = eps of that step; smoothed[R,Ho,Wo] f32 (must
 * not overlap belief or next: it holds intermediates during the call); stats[4] f32; count[4] i32.  n = R*Ho*Wo.
 *   PREDICT, exactly as snap_vote_filter_f32 does it with `belief` (its PREDICT paragraph: M, the masses p, the three
 *   passes t0, t1, t2 as f32 fma chains, S = sum t2 and sum p in float64) and per cell, float64,
 *   prior = ((1 - eps) * t2) / S + eps / n (the first term 0 when S == 0).  Both entry points are built from one set of
 *   device code: t2, S and prior are the bits the filter computed from the same belief and taps.
 *   RATIO, float64 per cell: a cell has ratio mass iff next is finite and prior > 0; then lg = (double)next -
 *   log(prior).  G = the largest lg (exact).  q = fl32(exp(lg - G)) if fl32(lg - G) >= -40, else exactly 0, and 0
 *   without ratio mass.  A NaN or +inf cell of next is a caller error: no mass, counted.  Q = sum q, float64.
 *   ADJOINT TRANSPORT.  Three gathers, in this order (the xy passes first, with their OWN rotation's tables; the
 *   rotation pass last), the intermediate volumes stored as f32:
 *     c1[r,a,b] = sum_tb taps_b[r,tb] * q [r, a, b - lb[r] - tb];
 *     c0[r,a,b] = sum_ta taps_a[r,ta] * c1[r, a - la[r] - ta, b];
 *     u [k,a,b] = sum_tk taps_k[tk]   * c0[(k - lk - tk) mod R, a, b]    (mathematical modulo);
 *   a source outside the volume contributes 0.  Each is an f32 fma chain from 0 over the SOURCE cell ascending, i.e.
 *   the tap index DESCENDING: link i = 0 .. T-1 reads the source x - l - (T-1) + i with tap T-1-i (in k: plane
 *   (k - lk - (Tk-1) + i) mod R, ascending before the modulo).  These are the filter's passes with each tap row
 *   reversed and first offset -l - (T-1): sum t2 * q == sum p * u up to rounding.
 *   COMBINE, float64 per cell: h = ((1 - eps) * (sum p / S)) * u + (eps / n) * Q (the first term 0 when S == 0);
 *   w = ((double)belief + G) + log(h); -inf for a -inf belief or h == 0; NaN (0x7fc00000) for a NaN or +inf belief,
 *   and the cell is left out of the normalisation; log_norm = log sum exp(w) over the finite cells (float64);
 *   smoothed = fl32(w - log_norm).  When no cell has ratio mass (or none is finite), log_norm = -inf and every cell that
 *   is not NaN is -inf.
 *   This is gamma_t(x) = alpha_t(x) * sum_x' K(x'|x) gamma_{t+1}(x') / prior(x') with K = (1 - eps)(sum p / S) T +
 *   eps / n, the kernel the filter applied, its renormalisation of the mass that left the volume included; for inputs
 *   that come from the filter with the same tables log_norm is 0 up to rounding (its size is a diagnostic of beliefs or
 *   tables that do not belong together).
 *   stats = { log_norm; S / sum p (0 when no cell has mass; the filter's stats[1] of that step, bit for bit); G (-inf
 *   without ratio mass); the largest smoothed (NaN cells aside; -inf when there is none) }.
 *   count = { finite cells of smoothed; NaN or +inf cells of belief; NaN or +inf cells of next; cells of next with
 *   ratio mass (those below the -40 cut included) }.
 * Eleven launches of min(R * ceil(Ho*Wo/256), 2048) workgroups of 256 threads (the last: one workgroup), a tile = one
 * rotation and 256 consecutive pixels: the filter's peak, rotation, row and column passes; the ratio's maximum; q,
 * written once (the float64 log and exp are per cell, not per tap); the adjoint column, row and rotation passes, the
 * last with the sum of exp(w) fused; the normalisation; the statistics.  t0, t2, c1 and u live in smoothed; t1, q and
 * c0 in the workspace.  22 passes over the volume (reads: belief 4, next 2, t0, t1, t2 twice, q, c1, c0, u; writes: t0,
 * t1, t2, q, c1, c0, u, smoothed), against the filter's 12.  No atomics: everything above the cell is float64 (counts
 * int32) in an order fixed by (R, Ho, Wo), so two calls give the same bits.  Every element of smoothed, stats and
 * count is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, 1 <= Tk <= 16, 1 <= Ta, Tb <= 32; anything else returns
 * SNAP_ERR_BAD_SHAPE before any launch (a NULL pointer SNAP_ERR_NULL, checked first; a uniform_mix outside [0, 1]
 * SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE).  workspace:
 * snap_vote_smooth_workspace_bytes() bytes (0 = unsupported shape): one volume and the per-workgroup partials; it
 * needs no initialisation and no launch touches a byte beyond that size.  Asynchronous on `stream`; the caller owns
 * every buffer. */
size_t snap_vote_smooth_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb);
int snap_vote_smooth_f32(const float* belief, const float* next, const float* taps_k, int32_t lk, const float* taps_a,
                         const float* taps_b, const int32_t* offsets, int32_t R, int32_t Ho, int32_t Wo, int32_t Tk,
                         int32_t Ta, int32_t Tb, float uniform_mix, float* smoothed, float* stats, int32_t* count,
                         void* workspace, size_t workspace_bytes, void* stream);

/* TAP POSTERIORS of one step of the pose filter above (the pairwise marginals of the forward-backward family, reduced
 * to what an EM fit of the motion noise consumes): given all frames, how the vehicle moved between frame t and frame
 * t+1.  Arguments as snap_vote_smooth_f32's: belief[R,Ho,Wo] f32 = the filter's belief_out at frame t; next[R,Ho,Wo]
 * f32 = the smoothed belief of frame t+1; the very tables of the step from t to t+1; uniform_mix = eps of that step.
 * Outputs, on the device: hist_k[Tk], hist_a[R,Ta], hist_b[R,Tb], stats[4] float64; count[4] i32.  n = R*Ho*Wo.
 *   The pairwise posterior xi(x, x') = alpha_t(x) K(x'|x) gamma_{t+1}(x') / prior(x'), with K and prior the filter's
 *   (snap_vote_smooth_f32's last paragraph), splits exactly into the JUMP branch, through the uniform share eps / n of
 *   the prior, and the STAY branch, through the tap triple (tk, ta, tb) that carried x to x'.
 *   PREDICT exactly as snap_vote_filter_f32 (M, the masses p, t0, t1, t2, S, sum p, prior) and RATIO exactly as
 *   snap_vote_smooth_f32 (G, q, Q): all three entry points are built from one set of device code, the same bits.
 *   ADJOINT, snap_vote_smooth_f32's first two gathers (named by pass here: its c1 is c0 and its c0 is c1), f32 fma
 *   chains stored as f32:  c0[r,a,b] = sum_tb taps_b[r,tb] * q[r, a, b - lb[r] - tb];
 *                          c1[r,a,b] = sum_ta taps_a[r,ta] * c0[r, a - la[r] - ta, b].
 *   HISTOGRAMS, raw; a source outside the volume contributes nothing, as in the passes:
 *     Hb[r,tb] = sum_{a,b}   fl32(fl32(taps_b[r,tb] * t1[r, a, b + lb[r] + tb]) * q [r,a,b]);
 *     Ha[r,ta] = sum_{a,b}   fl32(fl32(taps_a[r,ta] * t0[r, a + la[r] + ta, b]) * c0[r,a,b]);
 *     Hk[tk]   = sum_{r,a,b} fl32(fl32(taps_k[tk]   * p[(r + lk + tk) mod R, a, b]) * c1[r,a,b]);
 *   every term two f32 products (not contracted), every sum float64.  In exact arithmetic sum Hb = sum Ha = sum Hk =
 *   sum t2 * q.
 *   FINISH, float64: H = sum_tk Hk[tk] in index order; c = (1 - eps) / S (0 when S == 0); stay_raw = c * H;
 *   jump_raw = (eps / n) * Q; total = stay_raw + jump_raw.  hist_x = (c * Hx) / total for the three tables;
 *   stats = { stay = stay_raw / total; jump = jump_raw / total; log_norm = G + log(total); S / sum p rounded to f32 (0
 *   when no cell has mass): converted to f32 it is the filter's stats[1] of that step, bit for bit }.  total * e^G is
 *   the sum of gamma_{t+1} over the cells with ratio mass: log_norm is 0 up to rounding for arguments that belong
 *   together (snap_vote_smooth_f32's log_norm is this number plus the log of the sum of exp(belief), itself 0 for a
 *   normalised belief).  When total == 0 (no ratio mass) every histogram entry, stay and jump are 0 and log_norm = -inf.
 *   stay + jump = 1, and each table sums to stay, up to rounding.
 *   count = { cells of belief with mass (the filter's count[3]); then as snap_vote_smooth_f32's count[1..3]: NaN or
 *   +inf cells of belief; NaN or +inf cells of next; cells of next with ratio mass }.
 * Twelve launches of 256 threads: the filter's four; the ratio's two; then Hb, c0, Ha, c1, Hk; one workgroup that folds
 * the partial rows.  The predict, ratio and adjoint launches have min(R * ceil(Ho*Wo/256), 2048) workgroups; the three
 * reductions have R * gpr, gpr = min(ceil(Ho*Wo/256), 2048 / R) workgroups per rotation striding over that rotation's
 * tiles, so a workgroup keeps one tap row and float64 accumulators in registers over all its tiles and writes one
 * partial row.  22 passes over the volume, as the smoother.  No atomics: every order is fixed by (R, Ho, Wo, Tk, Ta, Tb),
 * so two calls give the same bits.  Every element of the five outputs is written by every call.
 * Supported shapes, error codes and their order as snap_vote_smooth_f32 (belief == NULL is SNAP_ERR_NULL: a step without
 * a previous frame has no pair).  workspace: snap_vote_pairs_workspace_bytes() bytes (0 = unsupported shape): four
 * volumes, the per-workgroup partials and the partial rows; it needs no initialisation and no launch touches a byte
 * beyond that size.  Asynchronous on `stream`; the caller owns every buffer. */
size_t snap_vote_pairs_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb);
int snap_vote_pairs_f32(const float* belief, const float* next, const float* taps_k, int32_t lk, const float* taps_a,
                        const float* taps_b, const int32_t* offsets, int32_t R, int32_t Ho, int32_t Wo, int32_t Tk,
                        int32_t Ta, int32_t Tb, float uniform_mix, double* hist_k, double* hist_a, double* hist_b,
                        double* stats, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* Highest-density CREDIBLE REGIONS of a vote volume, and where a ground-truth pose falls among them: the summary of a
 * multi-modal posterior that a covariance cannot give, and the statistic a calibration check needs (for a calibrated
 * model the mass ranked above the true pose is uniform on [0, 1]).
 * votes[R,Ho,Wo] f32 unnormalised log-scores, flat(r,a,b) = (r*Ho + a)*Wo + b; scale: a finite float > 0.
 *   A cell CONTRIBUTES iff its vote is finite (snap_vote_posterior_f32's rule: -inf cells are masked silently, NaN and
 *   +inf cells are excluded and counted); F is the set of contributing cells.  vmax = the largest contributing vote;
 *   the WEIGHT of a cell is w = exp((double)scale * ((double)v - (double)vmax)); Z = sum_F w.  The ORDER of cells is the
 *   f32 comparison of the votes themselves, with -0 = +0 (scale > 0 does not change it).
 *   levels: a HOST array q_0 < q_1 < ... < q_{L-1}, each strictly inside (0, 1), 1 <= L <= 8; read on the host,
 *   validated and passed to the kernels by value.
 *   REGION l = { c in F : v_c >= tau_l }, tau_l = the largest value t taken by a contributing cell with
 *   mass{v >= t} >= q_l * Z.  A class of tied cells is in or out as a whole, so the regions are nested.
 *   threshold[L]: tau_l, exactly a vote value of the volume (+0 for the class of zeros).
 *   mass[L]: mass{v >= tau_l} / Z, float64, rounded to f32 once.
 *   table[L,8] i32 = { cells of the region; pixels (a, b) with at least one rotation in it; rotations r with at least
 *   one pixel in it; a_min, a_max, b_min, b_max (the inclusive index bounding box); 0 }.
 *   The LEVEL of a cell is the smallest l with v >= tau_l, and L if there is none or the cell does not contribute.
 *   level_xy[Ho,Wo] u8: the minimum over r; level_r[R] u8: the minimum over the pixels; level_cell[R,Ho,Wo] u8, or NULL:
 *   the cells' own levels.  One u8 plane therefore carries all L nested footprints (region l = { level <= l }).
 *   gt_index: NULL, or a DEVICE pointer to f32 [3] = (k, i, j) as exhaustive_tfm_to_index returns it, read by the
 *   kernels.  The ground-truth cell is (rintf(k) mod R, rintf(i), rintf(j)) (round half to even, mathematical modulo);
 *   valid iff k, i, j are finite, |k| <= 2^20, 0 <= i <= Ho-1, 0 <= j <= Wo-1 and that cell contributes.
 *   gt_stats[4] = { v_gt; mass{v > v_gt} / Z, the CREDIBILITY of the ground truth; mass{v >= v_gt} / Z; 0 }: the ground
 *   truth lies in region l exactly when v_gt >= tau_l.  Invalid or NULL: the first three are NaN.
 *   count[4] = { contributing cells; NaN or +inf cells; 1 if the ground truth is valid, else 0; the ground truth's
 *   level (the smallest l with v_gt >= tau_l, L if none), -1 if invalid }.
 *   F empty: thresholds and masses NaN, every table row { 0, 0, 0, -1, -1, -1, -1, 0 }, the level maps all L,
 *   gt_stats NaN (and its last entry 0).
 * METHOD.  The thresholds come from a most-significant-digit radix select over the monotone 32-bit key of the vote,
 * 8 bits a pass, for all levels at once: a pass adds the cells' FIXED-POINT weights wfix = rint(w * 2^Q) (uint64,
 * Q = 62 - the bit length of R*Ho*Wo, so no sum can overflow) into 256 bins per distinct key prefix of the levels
 * (integer atomics, exact and order-independent: in LDS per workgroup, the non-empty bins then added to global bins),
 * and L workgroups pick the levels' next digits with the test (double)(cumulative wfix) >= (double)q_l * (double)Zfix
 * (Zfix = sum wfix; the conversions of the uint64 sums round to 53 bits, monotonically, and a digit's bins sum to their
 * parent's bin as integers, so the passes stay consistent).  The selection is exact for the quantised weights up to
 * those conversions: it returns the definition's tau_l whenever q_l differs from the normalised mass at every vote
 * value by more than EPS = R*Ho*Wo * 2^-Q / Z + 2^-40 (the quantum is 2^-Q; the second term covers the 2^-52 relative
 * error of the two conversions, of the product and of the float64 exp, each at most a few 2^-53 of a mass <= 1; at
 * 36 x 511 x 511, Q = 38 and the first term is 3.4e-5 / Z with Z >= 1, and Z is of the order of the number of cells
 * that matter).  The masses that are RETURNED (mass, gt_stats)
 * do not pass through the fixed point: they are float64 sums of the float64 weights, exact to float64 summation error
 * (far inside EPS).
 * PASSES over the volume, for every L: 1 (vmax and the counts) + 4 (one per digit) + 1 final pass that writes the
 * level maps and accumulates the masses, the tables' partials and the ground-truth tail masses = 6.  Eleven launches
 * (max, which also zeroes the global bins; 4 x (bins, select); levels; one workgroup that folds the partial rows).
 * No floating-point atomics anywhere (the only atomics are the integer ones above and the level pass's LDS minima,
 * maxima and counts); per-workgroup float64 partials are folded in an order fixed by (R, Ho, Wo), so
 * two calls with the same arguments give the same bytes.  Every element of every output is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, else SNAP_ERR_BAD_SHAPE; a NULL pointer other than gt_index and
 * level_cell SNAP_ERR_NULL; a scale that is not a finite number > 0, an L outside 1..8, or levels that are not strictly
 * increasing inside (0, 1) SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE; all before
 * any launch, in that order.  workspace: snap_vote_credible_workspace_bytes() bytes (0 = unsupported shape or L); it
 * needs no initialisation and no launch touches a byte beyond that size.  Asynchronous on `stream`, no host
 * synchronisation; the caller owns every buffer. */
size_t snap_vote_credible_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t L);
int snap_vote_credible_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale, const float* levels,
                           int32_t L, const float* gt_index, float* threshold, float* mass, int32_t* table,
                           uint8_t* level_xy, uint8_t* level_r, uint8_t* level_cell, float* gt_stats, int32_t* count,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The MODES of a vote volume: for each of K peaks the mass, mean and covariance of the cells around it, i.e. the
 * weight, mean and 3 x 3 covariance of one component of a Gaussian mixture over (rotation, a, b).  votes[R,Ho,Wo] f32:
 * unnormalised log-scores in the flat order of the other vote ops; peaks[K,3] i32: a DEVICE table of (r, a, b) rows,
 * exactly what snap_vote_peaks_f32 writes (unsorted tables are legal), read by the kernels, no host synchronisation;
 * gt_index: NULL, or a DEVICE pointer to f32 [3] = (k, i, j) as exhaustive_tfm_to_index returns it; stats[K,16] f32;
 * count[K,2] i32.
 *   CONTRIBUTING CELLS.  x = (double)scale * (double)v; a cell contributes iff v is finite (snap_vote_posterior_f32's
 *   rule): -inf cells are silently excluded, NaN and +inf cells are excluded and counted.
 *   EMPTY ROWS.  Row k is empty iff any component lies outside [0,R) x [0,Ho) x [0,Wo) (the -1 rows of
 *   snap_vote_peaks_f32 are the normal case).  An empty row owns nothing and no address is formed from it.
 *   WINDOW of a non-empty peak k: |dr| <= win_r, |da| <= win_xy, |db| <= win_xy with dr = (r - r_k) wrapped into its
 *   nearest representative (the rotation axis is circular; 2 win_r + 1 <= R makes it unique inside a window),
 *   da = a - a_k, db = b - b_k; clipped at the borders in a and b.
 *   OWNERSHIP, a partition: a cell inside at least one window belongs to the peak that minimises the integer
 *   D = wr^2 (da^2 + db^2) + win_xy^2 dr^2, wr = max(win_r, 1) (the distance normalised by the window half-widths,
 *   exact in int32), ties to the lowest k; a cell inside no window belongs to nobody.  A duplicate of an earlier peak
 *   therefore owns nothing.
 *   SUMS over O_k, the owned contributing cells, with offsets (dr, da, db) from the peak itself: m_k = max x,
 *   S0 = sum exp(x - m_k), and the three first and six second offset moments under those weights; the offsets are small
 *   integers, so the central moments E[d d'] - E[d] E[d'] cancel at most win_xy^2 against float64.
 *   stats[k] = { log_mass = m_k + log S0 (unnormalised: the mode's part of log_z); m_k; the mean rotation index
 *   r_k + E[dr] wrapped into [0, R) (a value that rounds to R in f32 is stored as 0); a_k + E[da]; b_k + E[db];
 *   Var r; Cov ra; Cov rb; Var a; Cov ab; Var b (index units); nees_gt; 0; 0; 0; 0 }.
 *   nees_gt = e^T (Sigma_k + I/12)^-1 e, the normalised estimation error squared of the ground truth under the mode:
 *   e = gt - mean in index units (the float64 means, the rotation's after its wrap), its rotation component taken to
 *   the nearest representative (IEEE remainder by R); I/12 is the variance of a uniform distribution over one lattice
 *   cell, below which the lattice cannot resolve, and keeps the matrix positive definite for a mode of one rotation
 *   or one cell; a float64 closed-form (cofactor) inverse.  NaN when gt_index is NULL or not finite.
 *   count[k] = { owned contributing cells; owned NaN or +inf cells }.
 *   An empty row, or O_k empty: log_mass = m_k = -inf, stats[2..11] = NaN (0x7fc00000), stats[12..15] = 0.
 * All arithmetic above the load is float64 and every output is a float64 expression rounded to f32 once.  No atomics:
 * K (2 win_r + 1) workgroups each reduce one rotation of one window in an order fixed by (win_xy), one thread per mode
 * merges its planes in the order dr = -win_r .. win_r; two calls with the same arguments give the same bytes.  Every
 * element of stats and count is written by every call; nothing beyond them and the workspace is touched.
 * Supported: R, Ho, Wo >= 1, R*Ho*Wo < 2^31, 1 <= K <= 64, 0 <= win_r <= 4 with 2 win_r + 1 <= R, 1 <= win_xy <= 32,
 * else SNAP_ERR_BAD_SHAPE; a NULL pointer other than gt_index SNAP_ERR_NULL; a scale that is not a finite number > 0
 * SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE; all before any launch.  workspace:
 * snap_vote_modes_workspace_bytes() bytes (0 = unsupported arguments); it needs no initialisation.  Asynchronous on
 * `stream`, no host synchronisation; the caller owns every buffer. */
size_t snap_vote_modes_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t K, int32_t win_r, int32_t win_xy);
int snap_vote_modes_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale, const int32_t* peaks,
                        int32_t K, int32_t win_r, int32_t win_xy, const float* gt_index, float* stats, int32_t* count,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The EXPECTED RECALL of a vote volume: how much posterior mass lies within (rho cells, half_r rotation bins) of a
 * pose.  The reference scores the localizer by hit / miss at thresholds (snap/models/bev_localizer.py:268-270,
 * loc/recall_max_{t}m and loc/recall_max_{t}deg: dt < t, dr < t; :274-277, the joint pairs (0.5 m, 1 deg), (1 m, 2 deg),
 * (2 m, 4 deg)); under the posterior of the votes the probability of such a hit for a candidate pose is the mass of
 * the threshold ball around it, and the cell whose ball carries the most mass maximises the expected recall.
 * votes[R,Ho,Wo] f32: unnormalised log-scores in the flat order of the other vote ops; rho2[L], half_r[L] i32: HOST
 * arrays, read before the call returns; centres[K,3] i32: a DEVICE table of (r, a, b) rows, exactly what
 * snap_vote_peaks_f32 writes, or NULL with K = 0; gt_index: NULL, or a DEVICE pointer to f32 [3] = (k, i, j) as
 * exhaustive_tfm_to_index returns it; maps[L,R,Ho,Wo] f32 or NULL.
 *   CONTRIBUTING CELLS.  x = (double)scale * (double)v; a cell contributes iff v is finite (snap_vote_posterior_f32's
 *   rule): -inf cells are silently excluded, NaN and +inf cells are excluded and counted.  m = max x, e = exp(x - m),
 *   S = sum e, all float64; a cell that does not contribute has e = 0.
 *   BALL of level l around (r, a, b): the cells (r', a', b') with |r' - r| <= half_r[l] on the circle of R rotations and
 *   (a' - a)^2 + (b' - b)^2 <= rho2[l], clipped to the volume in a and b (there is no mass outside it).  The thresholds
 *   are integers so that membership is exact everywhere (pose_exhaustive_voting.recall_thresholds turns metres and
 *   degrees into them with the reference's strict <).
 *   log_mass_l(r, a, b) = fl32(min(0, log(sum over the ball of e) - log S)), float64 above the cell and rounded once;
 *   -inf where the sum is 0 (no contributing cell in the ball).
 *   best_index[L,3] i32, best_log_mass[L] f32: the maximum of log_mass_l over ALL cells, compared as the stored f32
 *   values, the greater value first and then the lower flat index (r*Ho + a)*Wo + b; (-1, -1, -1) and -inf when no
 *   cell has a log mass above -inf.
 *   centre_log_mass[K,L] f32: log_mass_l at row k's cell; a row with a component outside [0,R) x [0,Ho) x [0,Wo) (the
 *   -1 rows of snap_vote_peaks_f32) is EMPTY: -inf, and no address is formed from it.
 *   gt_log_mass[L] f32: log_mass_l at the ground-truth cell (rintf(k) mod R, rint(i), rint(j)) (round half to even,
 *   mathematical modulo: snap_vote_credible_f32's rounding); the ground truth is valid iff k, i, j are finite,
 *   |k| <= 2^20, 0 <= i <= Ho-1 and 0 <= j <= Wo-1 (the cell itself need not contribute: the mass near a masked truth
 *   is a legitimate answer); NaN (0x7fc00000) when gt_index is NULL or invalid.
 *   stats[4] f32 = { log_z = m + log S; m; 0; 0 } (both -inf when no cell contributes).
 *   count[4] i32 = { contributing cells; NaN or +inf cells; 1 if the ground truth is valid, else 0; 0 }.
 *   maps, when not NULL: log_mass_l at every cell.  Every other output holds the same bytes with and without maps.
 * METHOD.  Every ball mass is a sum of NON-NEGATIVE float64 terms: no prefix sums and no sliding-window differences,
 * which lose a low-mass ball against its row total and can go negative.  E = e as a float64 volume; per level one
 * launch in which a wave owns 64 columns and marches down the rows: the row of sum_{|dr| <= half_r} E[r + dr] goes to
 * LDS, a thread grows the centred spans of its column S_h = (S_{h-1} + e(b-h)) + e(b+h), h = 0 .. rho, and adds
 * S_{isqrt(rho2 - d^2)} into the pending output rows at distance d, a ring of 2 rho + 1 rows in LDS; about 4 rho + 1
 * additions per cell and level instead of pi rho^2.  An output row receives its spans in ascending input-row order
 * whatever the tiling.  The centres' and the ground truth's masses are summed directly over their balls.  Values at
 * the same cell in maps and in centre_log_mass come from different summation orders of the same non-negative terms:
 * equal to float64 rounding before the single f32 rounding.  No atomics; per-workgroup partials are folded in an order
 * fixed by the shape, so two calls with the same arguments give the same bytes.  Every element of every output is
 * written by every call; the workspace needs no initialisation.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, 0 <= K <= 64, 1 <= L <= 8, 0 <= rho2[l] <= 1024,
 * 0 <= half_r[l] <= 4 with 2 half_r[l] + 1 <= R, else SNAP_ERR_BAD_SHAPE; a NULL pointer other than gt_index, maps and
 * (with K = 0) centres / centre_log_mass SNAP_ERR_NULL (checked first: the thresholds are read); a scale that is not a
 * finite number > 0 SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE; all before any
 * launch.  workspace: snap_vote_recall_workspace_bytes() bytes (0 = unsupported shape, K or L): ONE float64 volume
 * plus per-workgroup partials (75 MB at 36 x 511 x 511, L = 8), independent of the thresholds.  Asynchronous on
 * `stream`, no host synchronisation; the caller owns every buffer. */
size_t snap_vote_recall_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t K, int32_t L);
int snap_vote_recall_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale, const int32_t* rho2,
                         const int32_t* half_r, int32_t L, const int32_t* centres, int32_t K, const float* gt_index,
                         int32_t* best_index, float* best_log_mass, float* centre_log_mass, float* gt_log_mass,
                         float* stats, int32_t* count, float* maps, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The MOTION BETWEEN TWO FRAMES from their votes: the joint posterior over the integer index shift between the previous
 * frame's pose distribution and the current frame's votes, the one input every sequence operator above takes from
 * outside.  prev[R,Ho,Wo] f32: the previous frame's log-space distribution (a belief of snap_vote_filter_f32 with
 * scale_prev = 1, or a vote volume with its temperature); cur[R,Ho,Wo] f32: the current frame's votes; shifts[U,R,3]
 * i32 on the DEVICE or NULL with U = 0: row (u, r) = (k, i, j), candidate increment u seen from rotation r
 * (pose_exhaustive_voting.increment_lattice); log_table[2Kr+1,R,2S+1,2S+1] f32; log_evidence[U] f32 (may be NULL with
 * U = 0); best[1] i32; stats[4] f32; count[6] i32.
 *   MASSES (snap_vote_filter_f32's PREDICT rule, with a scale).  For a volume v with scale s: M = the largest finite
 *   cell; d = v - M, ONE f32 subtraction; the cell has mass fl32(exp((double)s * (double)d)) iff v is finite and
 *   (double)s * (double)d >= -40, else exactly 0.  NaN and +-inf cells have no mass; NaN and +inf cells are counted.
 *   p = the masses of prev, q = those of cur, zp and zq their float64 sums.
 *   TABLE.  For k in [-Kr, Kr], r in [0, R), i, j in [-S, S]:
 *     T[k][r][i][j] = sum over (a, b) of q[r, a, b] * p[(r + k) mod R, a + i, b + j]   (float64; a source cell outside
 *   the plane contributes nothing), motion_taps' indexing: the current pose (r, a, b) has its previous pose at
 *   (r + dk, a + da(r), b + db(r)).  Both factors are f32, so every product is exact in float64 and T is a sum of
 *   exact non-negative terms: only the order of the sum can change a bit.
 *   log_table[k + Kr][r][i + S][j + S] = fl32((log T - log zp) - log zq); -inf where T == 0.
 *   CANDIDATES.  A row (k, i, j) is INSIDE the window iff -Kr <= k <= Kr, -S <= i <= S and -S <= j <= S (as given: k is
 *   not wrapped).  E[u] = sum over r = 0 .. R-1, in that order, of T[k][r][i][j] at row (u, r); a row outside the window
 *   adds 0, is counted, and no address is formed from it.  log_evidence[u] = fl32((log E[u] - log zp) - log zq), -inf
 *   where E[u] == 0.
 *   best[0] = the lowest u with the largest log_evidence (compared as stored), -1 when none is finite.
 *   stats[4] = { log zp + scale_prev * M_prev; log zq + scale_cur * M_cur (the log-sum-exp of the scaled volume over its
 *   cells with mass); log sum over the finite u of exp((double)log_evidence[u]), as m + log sum exp(. - m) with m the
 *   largest; log_evidence[best] }, float64 rounded once; -inf where empty.
 *   count[6] = { cells of prev with mass; NaN or +inf cells of prev; cells of cur with mass; NaN or +inf cells of cur;
 *   shift rows outside the window; candidates with a finite log_evidence }.
 * METHOD.  The masses are written once as two f32 volumes.  The hot launch: a workgroup owns one (k, r) and a band of
 * rows; per tile it stages the q tile and the (tile + 2 S) halo of p in LDS as f32; a thread keeps the accumulators of
 * one column shift j and a block of consecutive row shifts i in float64 registers and walks the tile column by column,
 * the p values it needs being a sliding window down one LDS column (one LDS read of p and one broadcast read of q per
 * block of fmas); tiles whose q or p is all zero, and cells whose q is zero, are skipped (they add exact zeros).  Band
 * partials are folded in band order by a second launch.  No atomics; every float64 sum's order is a function of
 * (R, Ho, Wo, Kr, S, U) alone, so two calls with the same arguments give the same bytes.  Every element of every output
 * is written by every call; the workspace needs no initialisation.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, 0 <= Kr with 2 Kr + 1 <= R, 0 <= S <= 32, U >= 0 (with U == 0
 * only the table is produced: best = -1, stats[2] = stats[3] = -inf), else SNAP_ERR_BAD_SHAPE; a NULL pointer other than
 * (with U = 0) shifts / log_evidence SNAP_ERR_NULL; a scale that is not a finite number > 0 SNAP_ERR_UNSUPPORTED; a short
 * or not 8-byte aligned workspace SNAP_ERR_WORKSPACE; all before any launch.  workspace:
 * snap_vote_odometry_workspace_bytes() bytes (0 = unsupported arguments): the two mass volumes, the band partials and
 * the float64 table, 105.1 MB at R = 36, 511 x 511, Kr = 2, S = 16.  Asynchronous on `stream`, no host synchronisation;
 * the caller owns every buffer. */
size_t snap_vote_odometry_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Kr, int32_t S, int32_t U);
int snap_vote_odometry_f32(const float* prev, const float* cur, float scale_prev, float scale_cur,
                           const int32_t* shifts, int32_t R, int32_t Ho, int32_t Wo, int32_t Kr, int32_t S, int32_t U,
                           float* log_table, float* log_evidence, int32_t* best, float* stats, int32_t* count,
                           void* workspace, size_t workspace_bytes, void* stream);

/* A vote volume or belief carried into ANOTHER MAP FRAME.  Every transporting operator above composes a motion on the
 * query side (m_t_prev = m_t_cur @ cur_t_prev: a shift per rotation); a change of map frame composes on the left,
 * n_t_q = n_t_m @ m_t_q, which in index space is a constant circular shift in the rotation and ONE affine map of every
 * plane (pose_exhaustive_voting.rebase_table).  The operator gathers.  src[R,Ho,Wo] f32: a log-space vote volume or
 * belief (-inf = impossible pose); scale > 0 (the temperature); dk in [0, R) and A00, A01, A10, A11, oa, ob: the table,
 * float64 by value; dst[R,Ho,Wo] f32 (must not overlap src); stats[4] FLOAT64; count[4] i32.
 *   MASSES.  M = the largest finite value of src (exact).  A source cell v has the mass p = fl32(exp((double)scale *
 *   ((double)v - (double)M))), exactly 0 for v = -inf; a NaN or +inf cell is a caller error, counted, and poisons the
 *   cells that read it.
 *   GATHER, float64 per destination cell (r, a, b), the expressions exactly as written (no contraction):
 *     k = (double)r - dk, k0 = floor(k), fk = k - k0: the planes k0 mod R (mathematical modulo) and its circular successor;
 *     sa = (A00 * a + A01 * b) + oa, sb = (A10 * a + A11 * b) + ob, each with its floor and fraction;
 *   the axis weights are (1 - f, f) and the weight of a tap is (wk * wa) * wb.  A tap is SKIPPED when its weight is
 *   exactly 0 or it lies outside [0, Ho) x [0, Wo): an identity or a whole-cell shift reads exactly one cell.  The cell's
 *   mass is the float64 sum of weight * p over its taps in the order k, then a, then b, from 0, rounded to f32 once; NaN
 *   when one of its taps is a NaN or +inf cell.  S = the float64 sum of the f32 cell masses that are not NaN.
 *   dst = fl32(log((double)mass) - log(S)); -inf where the mass is 0; NaN stays NaN (0x7fc00000).  With S == 0 every
 *   cell that is not NaN is -inf.
 *   stats = { (double)scale * M + log(sum p): the log-sum-exp of scale * src over its finite cells (-inf without one);
 *   S / sum p, the share of the mass that arrived (0 when sum p == 0); M (-inf without a finite cell); the largest dst
 *   (NaN cells aside; -inf when there is none) }; sum p is the float64 sum of the f32 masses of the cells that are not
 *   NaN or +inf.
 *   count = { finite cells of dst; NaN cells of dst; NaN or +inf cells of src; cells of dst with no tap of non-zero
 *   weight inside the volume (what the old frame did not cover) }.
 * Four launches of 256 threads: the peak; the gather, a tile = 16 x 16 cells of one rotation's plane whose footprint in
 * both source planes (at most 24 x 24 cells each for a rotation) is staged in LDS as masses, so exp runs once per
 * staged cell and the 8-tap blend reads LDS (a table whose footprint is larger reads the source directly: same
 * expressions, same result); the normalisation in place; the statistics.  No atomics: everything above the cell is
 * float64 (counts int32) in an order fixed by (R, Ho, Wo), so two calls give the same bits.  Every element of dst, stats
 * and count is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31; anything else returns SNAP_ERR_BAD_SHAPE before any launch (a
 * NULL pointer SNAP_ERR_NULL, checked first; a scale that is not a finite number > 0, a dk outside [0, R) or a table
 * entry that is not finite SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE).
 * workspace: snap_vote_rebase_workspace_bytes() bytes (0 = unsupported shape): the per-workgroup partials only; it needs
 * no initialisation and no launch touches a byte beyond that size.  Asynchronous on `stream`; the caller owns every
 * buffer. */
size_t snap_vote_rebase_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo);
int snap_vote_rebase_f32(const float* src, int32_t R, int32_t Ho, int32_t Wo, float scale, double dk, double A00,
                         double A01, double A10, double A11, double oa, double ob, float* dst, double* stats,
                         int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* A vote volume's statistics over a TEMPERATURE LADDER: everything a one-parameter fit of p = softmax(s * votes) needs
 * (the temperature that minimises the ground-truth NLL over a validation set), at S scales from ONE visit of the frame.
 * For x = s * v: log_z(s), d log_z / d s = E_s[v], d2 log_z / d s2 = Var_s[v], and the ground-truth sample v_gt, which
 * does not depend on s (the trilinear interpolation is linear).
 * votes[R,Ho,Wo] f32 unnormalised log-scores, flat(r,a,b) = (r*Ho + a)*Wo + b; scales: a HOST pointer to S f32, every
 * one finite and > 0, strictly increasing; table[S,8] FLOAT64; stats[4] FLOAT64; count[4] i32.
 *   A cell CONTRIBUTES iff its vote is finite (snap_vote_posterior_f32's rule: -inf cells are masked silently, NaN and
 *   +inf cells are excluded and counted).  F = the contributing set, m = max_F v (exact; the same for every scale, as
 *   scales are > 0), d = fl32(v - m) <= 0.
 *   Level l, s = scales[l]: x = fl32(s * d), e = expf(x) and, over F, S0 = sum e, S1 = sum fl32(e x), S2 = sum
 *   fl32(fl32(e x) x) (the moments are summed in x: a term with e > 0 has |x| < 104, so no sum overflows);
 *   A = log S0, mu = S1 / S0 / s (= sum e d / sum e), q = S2 / S0 / s^2 (= sum e d^2 / sum e), all float64.
 *   table[l] = { 0: log_z = s m + A, 1: E[v] = m + mu, 2: Var[v] = max(q - mu^2, 0), 3: entropy = A - s mu,
 *                4: log p_max = -A, 5: log_prob_gt = s v_gt - log_z, 6: dnll = E[v] - v_gt (the derivative of the
 *                ground truth's NLL in s), 7: written as 0 }.
 *   stats = { m, v_gt, 0, 0 }.  count = { contributing cells; NaN or +inf cells; 1 if the ground-truth sample is valid,
 *   else 0; 0 }.
 *   gt_index: NULL, or a DEVICE pointer to f32 [3] = (k, i, j), read by the kernel.  v_gt = the trilinear interpolation
 *   of v (not of s v) at (k, i, j) in float64 by exactly snap_vote_posterior_f32's rule: circular in k, a tap of weight
 *   exactly 0 is not read, valid iff k, i, j are finite, 0 <= i <= Ho-1, 0 <= j <= Wo-1 and every tap of non-zero weight
 *   contributes.  Otherwise (and with NULL) v_gt, log_prob_gt and dnll are NaN and count[2] = 0.
 *   F empty: m = log_z = -inf, every other column of table[l][1..6] NaN.
 *   NO OVERFLOW CAVEAT: s * v is never formed in f32, only s * d with d <= 0 (it underflows to e = 0, which is the right
 *   weight), and s * m is formed in float64; snap_vote_posterior_f32's condition "|scale * v| below the f32 maximum"
 *   does not exist here, and neither does one on the spread of the votes.
 * f32 is used for the expf and for the sums of one pixel's <= R terms (each of one sign: e >= 0, e x <= 0, e x^2 >= 0);
 * everything above is float64 and every output is a float64 expression.  Three launches: the maximum and the counts;
 * the tile walk, one pixel per thread with its 3 S sums in registers, ONE partial row per workgroup; the fold, one
 * workgroup per level.  The volume is read twice (the second read follows the first through the cache), not S times.
 * No atomics and no hand-off between workgroups: every reduction order is fixed by (R, Ho, Wo, S), so two calls give
 * the same bits.  Every element of table, stats and count is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, 1 <= S <= 16; anything else returns SNAP_ERR_BAD_SHAPE before
 * any launch (a NULL pointer other than gt_index SNAP_ERR_NULL; a ladder that is not finite, > 0 and strictly increasing
 * SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE).  workspace:
 * snap_vote_temper_workspace_bytes() bytes (0 = unsupported shape); it needs no initialisation and no launch touches a
 * byte beyond that size.  Asynchronous on `stream`; the caller owns every buffer. */
size_t snap_vote_temper_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t S);
int snap_vote_temper_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, const float* scales, int32_t S,
                         const float* gt_index, double* table, double* stats, int32_t* count, void* workspace,
                         size_t workspace_bytes, void* stream);

/* A position / heading PRIOR fused into a vote volume or belief: the measurement update for a GNSS fix and a compass.
 * The prior is a mixture of M components, each a Gaussian in the plane times a von Mises factor per rotation.  The map
 * position of a sensor that does not sit at the query grid's centre depends on the rotation, so the Gaussian's centre
 * is a table entry per (component, rotation); pose_exhaustive_voting.pose_prior builds the tables in float64.
 * votes[R,Ho,Wo] f32 log-scores, flat(r,a,b) = (r*Ho + a)*Wo + b, or NULL (every cell then contributes with v = 0 and
 * scale is ignored: the prior itself as a belief); scale: a finite float > 0 with |scale * v| below the f32 maximum for
 * every finite v (not checked); on the DEVICE: centres[M,R,2] i32 = (n_a, n_b), planes[M,R,3] f32 = (f_a, f_b, y) and
 * comps[M,4] f32 = (Pxx, Pxy, Pyy, log w): component m in plane k is centred at the index n + f, |f| <= 0.5, has the
 * precision P in cells^-2 and the heading term y <= 0; log w <= 0.  PRECONDITION (not checked): every entry is finite,
 * P is positive semi-definite and |P| times the squared distance of any cell from any centre stays below 2^120.
 * out[R,Ho,Wo] f32 (must not overlap votes); resp[M] FLOAT64; stats[8] FLOAT64; count[4] i32.
 *   THE LOG-PRIOR u of the cell (k, a, b), every operation ONE IEEE f32 operation (no contraction), in this order:
 *     da = fl(float(a - n_a) - f_a), db = fl(float(b - n_b) - f_b)   (the integer difference is exact, its conversion
 *       exact below 2^24);
 *     q = fl(fl(fl(fl(Pxx da) da) + fl(fl(fl(2 Pxy) da) db)) + fl(fl(Pyy db) db))   (2 Pxy is exact);
 *     term_m = fl(fl(log w_m + y_mk) - fl(0.5 q))   (0.5 q is exact);
 *     M = 1: u = term_0, no exponential and no logarithm;
 *     M > 1: mx = max_m term_m, s = the f32 sum over m = 0 .. M-1, in that order from 0, of expf(fl(term_m - mx)),
 *       u = fl(mx + logf(s)).
 *   A cell CONTRIBUTES iff its vote is finite (snap_vote_posterior_f32's rule: -inf cells are masked silently, NaN and
 *   +inf cells are excluded and counted).  F = the contributing set.  On F: x = fl(scale v) (0 without votes),
 *   t = fl(x + u); tmax = max_F t, xmax = max_F x, umax = the largest u of ALL R Ho Wo cells (maxima: exact).
 *   With e = expf(fl(t - tmax)), eu = expf(fl(u - umax)), ev = expf(fl(x - xmax)) and S0 = sum_F e:
 *   stats = { 0: log_z = tmax + log S0,
 *             1: log_z_votes = xmax + log sum_F ev: the log-sum-exp of scale * votes over F,
 *             2: log_z_prior = umax + log (sum of eu over ALL cells),
 *             3: log_z_prior_F = umax + log sum_F eu (-inf where no cell of F has prior mass in f32),
 *             4: expected_log_prior = (sum_F (double)e (double)u) / S0 = E_post[u],
 *             5-7: written as 0 };
 *   resp[m] = (sum_F fl(e expf(fl(term_m - u)))) / S0: the posterior responsibility of component m (M = 1: exactly 1);
 *   out = fl32((double)t - log_z) on F, -inf elsewhere;
 *   count = { contributing cells; NaN or +inf cells; cells of F with e == 0 (their mass underflowed); 0 }.
 *   F empty: stats = { -inf, -inf, log_z_prior, -inf, NaN, 0, 0, 0 }, resp NaN, out all -inf.
 *   The caller's figures: log_evidence = log_z - log_z_prior (the frame under the prior normalised on the lattice);
 *   log_overlap = log_evidence - log_z_votes <= 0; information_gain = expected_log_prior - log_z + log_z_votes =
 *   KL(post || votes alone) >= 0.
 * f32 is used for the cell's expressions above and for the sums of one pixel's <= R terms of e, eu, ev and
 * fl(e expf(..)) (each >= 0); e u enters its sum in float64 cell by cell, and everything above the pixel is float64.
 * Four launches of 256 threads: t into out, the maxima and the counts (one pixel per thread walks its R cells; the
 * tables sit in LDS); the sums, ONE partial row per workgroup; the fold, one workgroup; the normalisation of out in
 * place.  The votes are read twice (the second read follows the first through the cache), out is written and then
 * updated.  No atomics and no hand-off between workgroups: every reduction order is fixed by (R, Ho, Wo, M), so two
 * calls give the same bits.  Every element of out, resp[0..M), stats and count is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, 1 <= M <= 8; anything else returns SNAP_ERR_BAD_SHAPE before
 * any launch (a NULL pointer other than votes SNAP_ERR_NULL, checked first; with votes, a scale that is not a finite
 * number > 0 SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE).  workspace:
 * snap_vote_prior_workspace_bytes() bytes (0 = unsupported shape); it needs no initialisation and no launch touches a
 * byte beyond that size.  Asynchronous on `stream`; the caller owns every buffer. */
size_t snap_vote_prior_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t M);
int snap_vote_prior_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale, int32_t M,
                        const int32_t* centres, const float* planes, const float* comps, float* out, double* resp,
                        double* stats, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* A road / lane RASTER prior fused into a vote volume or belief: the map's own constraint (the vehicle is on a drivable
 * area and heads along the lane) as a measurement update, evaluated over a ladder of S prior strengths in one visit.
 * votes[R,Ho,Wo] f32 log-scores, flat(r,a,b) = (r*Ho + a)*Wo + b, or NULL (every cell then has v = 0 and scale is
 * ignored: the raster prior itself as a belief); scale: a finite float > 0 with |scale * v| below the f32 maximum for
 * every finite v (not checked).  On the DEVICE: raster[X,Y,4] f32 = (A, C, S, valid), 16-byte aligned: the log-prior of
 * position, kappa cos(h phi), kappa sin(h phi) of the lane heading phi, and valid = 0.0 for a cell that holds no data
 * (any other value: valid); offsets[R,2] i32 = (n_a, n_b) and planes[R,4] f32 = (f_a, f_b, c_k, s_k): in raster index
 * units the lattice cell (k, a, b) sits at (a, b) + n_k + f_k, 0 <= f < 1, and c_k, s_k are cos and sin of h theta_k,
 * theta_k = -2 pi k / R (models/votes/raster.raster_prior builds them in float64).  On the HOST: strengths[S], each a
 * finite float > 0.  outside: a float that is finite or -inf.  write: the ladder index w whose posterior is written to
 * out; gt_index: a flat cell index, or -1.  PRECONDITION (not checked): A, C, S are finite on valid cells, and
 * |lambda_s| (|A| + |C| + |S|) stays below the f32 maximum.
 * out[R,Ho,Wo] f32 (must not overlap votes); table[S,4] FLOAT64; stats[4] FLOAT64; count[4] i32.
 *   THE RASTER LOG-PRIOR g of the cell (k, a, b), every operation ONE IEEE f32 operation (no contraction), in this order:
 *     ga = fl(1 - f_a), gb = fl(1 - f_b); the weights of the taps (0,0), (0,1), (1,0), (1,1) are fl(ga gb), fl(ga f_b),
 *       fl(f_a gb), fl(f_a f_b): constants of the plane k.  Tap (i, j) is the raster cell (a + n_a + i, b + n_b + j)
 *       (integer arithmetic, exact for any int32 n).
 *     A tap whose weight is exactly 0 is neither read nor tested nor summed.  If any other tap lies off the raster or
 *     has valid == 0, g = outside.  Otherwise, for each plane Q of A, C, S: bQ = the sum from 0 over the taps present,
 *     in the order above, bQ = fl(bQ + fl(w Q_tap)) (one tap of weight 1: bQ = Q_tap exactly), and
 *     g = fl(fl(bA + fl(c_k bC)) + fl(s_k bS)).
 *   A cell CONTRIBUTES iff its vote is finite (snap_vote_posterior_f32's rule: -inf cells are masked silently, NaN and
 *   +inf cells are excluded and counted) AND g > -inf.  F = the contributing set; V = the cells with a finite vote.
 *   x = fl(scale v) (0 without votes); for level s, lg_s = fl(lambda_s g) and t_s = fl(x + lg_s) on F.
 *   tmax_s = max_F t_s, gmax = the largest g of ALL R Ho Wo cells, xmax = max_V x (maxima: exact).  With
 *   e_s = expf(fl(t_s - tmax_s)) and S0 = sum_F e_s:
 *   table[s] = { 0: log_z_s = tmax_s + log S0,
 *                1: log_z_prior_s = fl(lambda_s gmax) + log (sum of expf(fl(lg_s - fl(lambda_s gmax))) over ALL cells with
 *                   g > -inf): the normaliser of the prior alone on the lattice (-inf where no cell has g > -inf),
 *                2: E_s[g] = (sum_F (double)e_s (double)g) / S0,
 *                3: Var_s[g] = max(0, (sum_F ((double)e_s (double)g) (double)g) / S0 - E_s[g]^2) };
 *   stats = { 0: log_z_votes = xmax + log sum_V expf(fl(x - xmax)) (-inf where V is empty),
 *             1: x_gt = fl(scale v) of the cell gt_index as float64 (0 without votes; -inf for a -inf vote; NaN for a NaN
 *                or +inf vote or gt_index == -1),
 *             2: g_gt = g of that cell (-inf for a cell the raster excludes; NaN with gt_index == -1),
 *             3: written as 0 };
 *   out = fl32((double)t_w - log_z_w) on F, -inf elsewhere;
 *   count = { |V|; NaN or +inf cells; cells of V with g == -inf; cells of F with e_w == 0 (their mass underflowed) }.
 *   F empty: log_z_s = -inf, E_s and Var_s NaN, out all -inf.
 *   The caller's figures: log p_s(gt) = x_gt + lambda_s g_gt - log_z_s and its derivative in lambda, g_gt - E_s[g];
 *   log_evidence_s = log_z_s - log_z_prior_s; log_overlap_s = log_evidence_s - log_z_votes; information_gain_s =
 *   lambda_s E_s[g] - log_z_s + log_z_votes = KL(post_s || votes alone) >= 0; d log_z_s / d lambda = E_s[g] and
 *   d2 log_z_s / d lambda^2 = Var_s[g].
 * f32 is used for the cell's expressions above and for the sums of one pixel's <= R terms of e_s, of the prior's
 * exponentials and of the votes' (each >= 0); e g and (e g) g enter their sums in float64 cell by cell, and everything
 * above the pixel is float64.  Four launches of 256 threads: g into out, the maxima and the counts (one pixel per thread
 * walks its R cells; the per-rotation table sits in LDS); the sums, ONE partial row per workgroup (g is read back from
 * out: nothing is interpolated twice); the fold, one workgroup; out from (votes, g) in place.  No atomics and no hand-off
 * between workgroups: every reduction order is fixed by (R, Ho, Wo, S), so two calls give the same bits.  Every element
 * of out, table[0..S), stats and count is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, X, Y >= 1, X*Y < 2^29, 1 <= S <= 8, 0 <= write < S, -1 <=
 * gt_index < R*Ho*Wo; anything else returns SNAP_ERR_BAD_SHAPE before any launch (a NULL pointer other than votes
 * SNAP_ERR_NULL, checked first; a raster that is not 16-byte aligned, with votes a scale that is not a finite number > 0,
 * an outside that is NaN or +inf, a strength that is not a finite number > 0: SNAP_ERR_UNSUPPORTED; a short or not 8-byte
 * aligned workspace SNAP_ERR_WORKSPACE).  workspace: snap_vote_raster_workspace_bytes() bytes (0 = unsupported shape); it
 * needs no initialisation and no launch touches a byte beyond that size.  Asynchronous on `stream`; the caller owns
 * every buffer. */
size_t snap_vote_raster_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t X, int32_t Y, int32_t S);
int snap_vote_raster_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale, const float* raster,
                         int32_t X, int32_t Y, const int32_t* offsets, const float* planes, float outside,
                         const float* strengths, int32_t S, int32_t write, int64_t gt_index, float* out, double* table,
                         double* stats, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* Most likely pose TRACK over vote volumes: one forward step of the max-product (Viterbi) recursion that goes with the
 * filter above, with back-pointers.  score_prev[R,Ho,Wo] f32 is the log score of the best path into every pose of the
 * previous frame (-inf = no path), or NULL (the first frame of a track); votes[R,Ho,Wo] f32; on the DEVICE:
 * ltaps_k[Tk] f32 with first offset lk, ltaps_a[R,Ta] / ltaps_b[R,Tb] f32 and offsets[R,2] i32 = (la, lb), the layout of
 * snap_vote_filter_f32's tables with every tap replaced by its LOGARITHM (pose_exhaustive_voting.motion_log_taps);
 * score_out[R,Ho,Wo] f32 and back[R,Ho,Wo] i32 (neither may overlap an input: score_out holds intermediates during
 * the call); stats[2] f32; count[6] i32.  n = R*Ho*Wo; a linear index is (r*Ho + a)*Wo + b.
 *   LOG-TAPS (precondition, not checked): every entry is -inf (a zero tap) or a finite f32 <= 0.  They are inputs so
 *   that no launch evaluates a transcendental function.
 *   Every operation below is ONE IEEE f32 operation (no contraction into fma).
 *   PEAK.  M = the largest finite value of score_prev (exact); J = the lowest linear index at which it is attained, -1
 *   when no cell is finite.  A NaN or +inf cell is a caller error: it counts as -inf, and is counted.
 *   d = score_prev - M; a cell that is not finite has d = -inf.  (Subtracting M at every step keeps the scores bounded
 *   over a long track; M is returned so the caller can sum the path's total.)
 *   MAX-PLUS PASSES, in the filter's order and with the filter's indexing (the rotation pass circular, at the source
 *   cell; the xy passes with the OUTPUT rotation's tables; a source row / column outside the volume is -inf), the
 *   intermediate volumes stored as f32:
 *     m0[r,a,b] = max_tk ( ltaps_k[tk]   + d [(r + lk + tk) mod R, a, b] )    (mathematical modulo);
 *     m1[r,a,b] = max_ta ( ltaps_a[r,ta] + m0[r, a + la[r] + ta, b] );
 *     m2[r,a,b] = max_tb ( ltaps_b[r,tb] + m1[r, a, b + lb[r] + tb] ).
 *   Each maximum runs over its taps ASCENDING from -inf and is replaced on a strict > only: among equal candidates the
 *   LOWEST tap index is the chosen one.  (f32 addition is monotone, so m2 is exactly the joint maximum over all
 *   (tk, ta, tb) of fl32(ltaps_b + fl32(ltaps_a + fl32(ltaps_k + d))).)
 *   UPDATE.  stay = log_stay + m2; jump = log_jump if J >= 0, else -inf (the jump's predecessor is cell J, where d = 0).
 *   best = stay if stay >= jump (the transported predecessor wins a tie), else jump.
 *   score_out = fl32(scale * votes) + best; -inf for a -inf vote or best = -inf; -inf, and counted, for a NaN or +inf
 *   vote.  back[x] = the linear index of the predecessor: for a transported predecessor the source reached through the
 *   three chosen taps -- the column tap chosen at (r, a, b) gives b' = b + lb[r] + tb, the row tap chosen at (r, a, b')
 *   gives a' = a + la[r] + ta, the rotation tap chosen at (r, a', b') gives k' = (r + lk + tk) mod R, and the
 *   predecessor is (k', a', b') --; for a jump J; -1 wherever score_out is -inf.
 *   With score_prev == NULL: best = 0 and back = -1 everywhere, M = -inf, J = -1; the tables are not read.
 *   stats = { M; the largest score_out (-inf when every cell is -inf) }.
 *   count = { finite cells of score_out; NaN or +inf cells of score_prev; NaN or +inf cells of votes; cells whose
 *   predecessor is the jump (score_out above -inf and back = J by the jump); J; the lowest linear index of the largest
 *   score_out, or -1 }.
 *   Statistically this is the max-product recursion under the transition K_max(x|x') = max((1 - eps) T(x|x'), eps / n)
 *   with log_stay = log(1 - eps), log_jump = log(eps / n) and T the filter's three tap passes; K_max lies within a
 *   factor 2 (log 2 per step) of the filter's (1 - eps) T + eps / n.  The filter's renormalisation of the transported
 *   mass (sum p / S) is constant over the lattice, cannot change an argmax, and is left out.
 * Five launches of min(R * ceil(Ho*Wo/256), 2048) workgroups of 256 threads (the last: one workgroup; two with
 * score_prev == NULL), a tile = one rotation and 256 consecutive pixels: the peak; the rotation pass with the
 * subtraction fused; the row pass; the column pass with the update and the composition of back; the statistics.  m0
 * lives in score_out, m1 and the rotation and row passes' chosen taps (one byte per cell each) in the workspace.  10
 * passes over the volume in 4-byte cells (reads: score_prev 2, m0, m1, votes, the two byte volumes 1/2; writes: m0,
 * m1, score_out, back, the two byte volumes 1/2), 3 with score_prev == NULL, against the filter's 12; no float64 and no
 * transcendental function.  No atomics: maxima are exact and every fold keeps "the larger value, then the lower
 * index", a total order, so two calls give the same bits whatever the fold order.  Every element of score_out, back,
 * stats and count is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, 1 <= Tk <= 16, 1 <= Ta, Tb <= 32; anything else returns
 * SNAP_ERR_BAD_SHAPE before any launch (a NULL pointer other than score_prev SNAP_ERR_NULL, checked first; a scale that
 * is not a finite number > 0, or a log_stay / log_jump that is not <= 0 (-inf allowed; NaN is not) SNAP_ERR_UNSUPPORTED;
 * a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE).  workspace: snap_vote_viterbi_workspace_bytes() bytes
 * (0 = unsupported shape): m1, the two byte volumes and the per-workgroup partials; it needs no initialisation and no
 * launch touches a byte beyond that size.  Asynchronous on `stream`; the caller owns every buffer. */
size_t snap_vote_viterbi_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb);
int snap_vote_viterbi_f32(const float* score_prev, const float* votes, const float* ltaps_k, int32_t lk,
                          const float* ltaps_a, const float* ltaps_b, const int32_t* offsets, int32_t R, int32_t Ho,
                          int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb, float scale, float log_stay, float log_jump,
                          float* score_out, int32_t* back, float* stats, int32_t* count, void* workspace,
                          size_t workspace_bytes, void* stream);

/* One step BACK along snap_vote_viterbi_f32's back-pointers, for B independent chains at once: back[n] i32 (a step's
 * `back`, n = R*Ho*Wo), cur[B] i32 linear indices at frame t, prev[B] i32: prev[i] = back[cur[i]] if 0 <= cur[i] < n,
 * else -1 (a chain that has ended stays ended).  prev must not overlap back or cur.  n, B >= 1, else
 * SNAP_ERR_BAD_SHAPE; a NULL pointer SNAP_ERR_NULL, checked first.  One launch of ceil(B / 256) workgroups, asynchronous
 * on `stream`, no host read. */
int snap_vote_backstep_i32(const int32_t* back, int32_t n, const int32_t* cur, int32_t* prev, int32_t B, void* stream);

/* DRAWS from a vote volume: B independent cells of p = softmax(scale * votes) over the lattice, by the project's keyed
 * Philox.  votes[R,Ho,Wo] f32 (log-space; -inf = impossible); uniforms: NULL or float64 [B,2] on the DEVICE; index[B]
 * i32; log_prob[B] f32; stats[2] f32; count[2] i32.  n = R*Ho*Wo; a linear index is (r*Ho + a)*Wo + b.
 *   MASS.  s = fl32(scale * v) (one f32 product); M = the largest finite s (exact); d = fl32(s - M); the cell has the
 *   mass p = fl32(exp((double)d)) iff s is finite and d >= -40, else exactly 0 (snap_vote_filter_f32's rule).  A NaN or
 *   +inf s carries no mass and is counted.
 *   UNIFORMS.  With uniforms == NULL draw i takes (x0, x1, x2, x3) = Philox4x32-10(counter = (i, stream_id, 0, 0),
 *   key = (seed low word, seed high word)) and u0 = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53, u1 likewise from x2, x3:
 *   float64 in [0, 1).  Otherwise (u0, u1) = uniforms[i] (precondition: in [0, 1)).  This entry point uses u0.
 *   DRAW.  The inverse CDF in lattice order (linear index ascending): the first cell whose inclusive prefix of p
 *   exceeds u0 * Z, Z = sum p.  Evaluated as a descent over three levels of float64 sums -- the R plane sums, the Ho
 *   row sums of the chosen plane, the Wo cells of the chosen row with their masses recomputed -- each level by ONE
 *   routine: chunks of 64 entries in ascending order; inside a chunk the inclusive prefixes are a Kogge-Stone scan
 *   (lane i: a fixed tree over entries 0 .. i of the chunk) added to the carry, the inclusive prefix of the chunk
 *   before at its last lane; the level takes the first entry WITH MASS whose inclusive prefix exceeds the target t and
 *   hands max(t - its exclusive prefix, 0) to the next level as its target; when no prefix exceeds t (the levels' sums
 *   are rounded differently) it takes its LAST entry with mass.  A row sum is a chain per lane over b = lane, lane + 64,
 *   .. and an xor butterfly over the 64 lanes; a plane sum the same over its rows; Z is the plane level's carry after
 *   its scan, and the first target is u0 * Z.  So a cell with p == 0 is never returned, the result is a function of the
 *   inputs alone, and it differs from the dense float64 CDF's answer only where u0 * Z lies within rounding (2^-22 Z
 *   covers the masses' last f32 bit and every float64 sum) of a prefix.
 *   index = the linear index; -1 for every draw when no cell has mass.  log_prob = fl32(((double)s - M) - log Z) of the
 *   drawn cell; -inf where index is -1.
 *   stats = { fl32(M + log Z) (the log normaliser of scale * votes; -inf without mass); M (-inf without a finite cell) }.
 *   count = { cells with mass; NaN or +inf cells }.
 * Four launches: the peak on min(R * ceil(Ho*Wo/256), 2048) workgroups of 256 threads; the row sums, one wave per
 * (r, a) row; one workgroup for the plane sums, Z, stats and count; the draws, one wave per draw.  Two reads of the
 * volume; a draw reads R plane sums, Ho row sums and Wo cells.  No atomics; two calls give the same bytes; every
 * element of index, log_prob, stats and count is written by every call.
 * Supported: 1 <= R <= 64, Ho, Wo >= 1, R*Ho*Wo < 2^31, 1 <= B <= 2^20; anything else returns SNAP_ERR_BAD_SHAPE
 * before any launch (a NULL pointer other than uniforms SNAP_ERR_NULL, checked first; a scale that is not a finite
 * number > 0 SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE).  workspace:
 * snap_vote_sample_workspace_bytes() bytes (0 = unsupported shape): the row sums and counts, the plane sums and the
 * per-workgroup partials; it needs no initialisation and no launch touches a byte beyond that size.  Asynchronous on
 * `stream`; the caller owns every buffer. */
size_t snap_vote_sample_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo);
int snap_vote_sample_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale, int32_t B, uint64_t seed,
                         int32_t stream_id, const double* uniforms, int32_t* index, float* log_prob, float* stats,
                         int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* One BACKWARD step of forward-filter / backward-sample for B chains: from the chains' cells at frame t+1 to cells at
 * frame t drawn from p(x_t | x_{t+1}, frames 0 .. t), the exact conditional of snap_vote_filter_f32's own transition.
 * Run from a draw of the last belief (snap_vote_sample_f32) down to frame 0, it yields joint tracks from
 * p(x_0 .. x_{N-1} | all frames).  belief[R,Ho,Wo] f32 = the filter's belief_out at frame t (required); taps_k, lk,
 * taps_a, taps_b, offsets and uniform_mix = eps: what snap_vote_filter_f32 was given for the step t -> t+1 (same
 * layout, same precondition); next[B] i32 linear indices at frame t+1; uniforms: NULL or float64 [B,2] on the DEVICE;
 * prev[B] i32; jumped[B] i32; stats[2] f32; count[3] i32.
 *   PREDICT, exactly as snap_vote_filter_f32 does it with `belief` (one set of device code): M, the masses p, sum p and
 *   S = sum t2 are the filter's bits.  The row sums, plane sums and Z of p are formed as in snap_vote_sample_f32 (scale
 *   1).  (u0, u1) as there, with the counter (i, stream_id, 1, 0).
 *   WINDOW of a chain at x = (r, a, b): entry (tk, ta, tb), in ascending lexicographic order, has the cell
 *   x' = ((r + lk + tk) mod R, a + la[r] + ta, b + lb[r] + tb) and the float64 weight
 *   (((double)taps_k[tk] * taps_a[r,ta]) * taps_b[r,tb]) * p[x'], 0 outside the volume.  The (tk, ta) row sums are
 *   chains over tb ascending; W = the carry after the scan (the routine above) over the Tk*Ta row sums.
 *   A = ((1 - eps) * W) / S (0 when S == 0); J = eps / n (0 when sum p == 0).
 *   u0 * (A + J) < J selects the JUMP: prev = a draw as in snap_vote_sample_f32 from p with u1.  Otherwise prev = the
 *   cell of the window entry found by the routine above over the row sums with the target u1 * W, then over the chosen
 *   row's Tb entries recomputed.  Several entries may name one cell (Tk > R).
 *   prev = -1 where next is outside [0, n) (a chain that has ended stays ended) or A + J == 0; jumped = 1 for the jump,
 *   0 for a transported step, -1 where prev is -1.
 *   stats = { S / sum p (0 when sum p == 0: the filter's stats[1] of that step, bit for bit); M }.
 *   count = { chains with a predecessor; chains that jumped; NaN or +inf cells of belief }.
 *   This is p(x' | x) proportional to (1 - eps) K(x, x') p(x') / S + (eps / n) p(x') / sum p, the filter's prior
 *   ((1 - eps) * t2) / S + eps / n taken apart by source cell.
 * Eight launches: the filter's peak, rotation, row and column passes on its grid; the row sums; one workgroup for the
 * plane sums and totals; one 256-thread workgroup per chain (the row sums of the window in LDS, then one wave); the
 * counts.  No atomics; two calls give the same bytes; every element of prev, jumped, stats and count is written by
 * every call.
 * Supported: the shapes of snap_vote_filter_f32 (1 <= Tk <= 16, 1 <= Ta, Tb <= 32) and 1 <= B <= 2^20; anything else
 * returns SNAP_ERR_BAD_SHAPE before any launch (a NULL pointer other than uniforms SNAP_ERR_NULL, checked first; a
 * uniform_mix outside [0, 1] SNAP_ERR_UNSUPPORTED; a short or not 8-byte aligned workspace SNAP_ERR_WORKSPACE).
 * workspace: snap_vote_sample_back_workspace_bytes() bytes (0 = unsupported shape): two volumes (t0 / t2 and t1), the
 * row and plane sums and the per-workgroup partials; it needs no initialisation and no launch touches a byte beyond
 * that size.  Asynchronous on `stream`; the caller owns every buffer. */
size_t snap_vote_sample_back_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb);
int snap_vote_sample_back_f32(const float* belief, const float* taps_k, int32_t lk, const float* taps_a,
                              const float* taps_b, const int32_t* offsets, int32_t R, int32_t Ho, int32_t Wo, int32_t Tk,
                              int32_t Ta, int32_t Tb, float uniform_mix, const int32_t* next, int32_t B, uint64_t seed,
                              int32_t stream_id, const double* uniforms, int32_t* prev, int32_t* jumped, float* stats,
                              int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* Dense plane ALIGNMENT SCORE at continuous poses: what a vote of the exhaustive voting measures (the correlation of
 * the query plane with the map plane, normalised by the number of valid query cells), evaluated at poses that need
 * not lie on the vote lattice (pose_exhaustive_voting.refine_poses: a lattice of sub-bin / sub-cell poses around
 * every peak of ops.vote_peaks).
 * fq[Hq,Wq,D] f32 / vq[Hq,Wq] u8: the query plane; fm[Hm,Wm,D] f32 / vm[Hm,Wm] u8: the map plane; poses[P,4] f32 on
 * the DEVICE = (cos, sin, tx, ty), the map <- query transform in corner frames with tx, ty in CELL units;
 * score[P] f32; overlap[P] i32.
 *   SAMPLE.  For pose p and query cell (i, j) with vq[i,j] != 0, in f32 and in this order:
 *   u = (cos*(i+0.5) - sin*(j+0.5)) + tx, v = (sin*(i+0.5) + cos*(j+0.5)) + ty (no contraction into fma).  The rest
 *   is snap_rot_geom / snap_rot_sample of csrc/rotate_sample.h with cell = 1 on the map plane: the sample is inside iff
 *   0 <= u < Hm and 0 <= v < Wm; with cu = u - 0.5, fu = floor(cu) the taps are rows clamp(fu), clamp(fu + 1) into
 *   [0, Hm-1] with factors (1 - wu1, wu1), wu1 = cu - fu, columns alike, and the four weights are the f32 products of a
 *   row and a column factor.  The cell COUNTS iff the sample is inside and all four taps are valid in vm, those of
 *   weight zero included.
 *   VALUE.  raw(p) = sum over the counted cells of sum_d fq[i,j,d] * mix_d, mix_d = ((w00 m00 + w01 m01) + w10 m10) +
 *   w11 m11 of the taps' channel d; overlap(p) = the number of counted cells; tcount = the number of cells with
 *   vq != 0; score(p) = raw(p) / tcount if overlap(p) > threshold (compared as f32), else -inf: the normaliser and the
 *   rule of snap_template_finalize_f32, so a score compares with a vote.  (tcount = 0 with a negative threshold: NaN.)
 *   A pose row with a non-finite entry gives score -inf and overlap 0.  A NaN / Inf feature reaches exactly the poses
 *   one of whose counted cells has it as a tap (a zero-weight tap included: 0 * NaN) or as its own feature.
 *   SUMMATION.  A cell's channel sum is f32: lane l of the cell's 8 lanes adds its products a_d * mix_d over the
 *   channels d = 32 k + 4 l .. 32 k + 4 l + 3, k ascending, in one chain from 0, and the 8 lanes fold as a binary tree
 *   (lane distance 1, 2, 4).  Everything above the cell is float64 in an order fixed by (Hq, Wq) alone (16 x 16 cell
 *   tiles, row-major, 16 tiles per workgroup), and the score is the float64 quotient rounded to f32 once.
 * No atomics: two calls give the same bits, and a pose's result does not depend on P or on the other rows.
 * Every element of score and overlap is written by every call.
 * Supported: 1 <= Hq, Wq, Hm, Wm <= 1024, D % 4 == 0 with 4 <= D <= 128, 1 <= P < 2^20, fq and fm 16-byte aligned;
 * anything else returns SNAP_ERR_UNSUPPORTED before any launch (a NULL pointer SNAP_ERR_NULL, checked first; a short or
 * not 8-byte aligned workspace SNAP_ERR_WORKSPACE).  workspace: snap_plane_align_score_workspace_bytes() bytes (0 =
 * unsupported geometry): one 16-byte partial per (pose, workgroup) and tcount; it needs no initialisation and no
 * launch touches a byte beyond that size.  Three launches, asynchronous on `stream`; the caller owns every buffer. */
size_t snap_plane_align_score_workspace_bytes(int32_t Hq, int32_t Wq, int32_t Hm, int32_t Wm, int32_t D, int32_t P);
int snap_plane_align_score_f32(const float* fq, const uint8_t* vq, const float* fm, const uint8_t* vm,
                               const float* poses, int32_t Hq, int32_t Wq, int32_t Hm, int32_t Wm, int32_t D,
                               int32_t P, float threshold, float* score, int32_t* overlap, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Confidence-weighted vertical pooling: the 'softmax' / 'weighted' modes of VerticalPooling
 * (bev_mapper.py:63-78).  score_z = vol[m,z,:] . w + bias[0] (log_sigmoid of it when
 * log_sigmoid_scores != 0, i.e. 'weighted'); weights = softmax over the valid levels (all
 * levels if none is valid, then zeroed), plane = sum_z weights_z vol[m,z,:], zero where no
 * level is valid.  scores / weights: [M, Z] (pred['scores'], pred['weights']).  Z <= 64,
 * D <= 128.  Backward: d vol from d plane (scores / weights outputs carry no gradient here),
 * plus per-workgroup partial rows [rows, D + 4] of (d w | d bias at column D) whose column
 * sums (snap_colsum_f32) are d w and d bias; rows = snap_vertical_pool_conf_bwd_partial_rows(M). */
int snap_vertical_pool_conf_f32(const float* vol, const uint8_t* vvalid, const float* w,
                                const float* bias, int64_t M, int32_t Z, int32_t D,
                                int32_t log_sigmoid_scores, float* plane, uint8_t* pvalid,
                                float* scores, float* weights, void* stream);
size_t snap_vertical_pool_conf_bwd_partial_rows(int64_t M);
int snap_vertical_pool_conf_bwd_f32(const float* vol, const uint8_t* vvalid, const float* w,
                                    const float* bias, const float* weights, const float* dplane,
                                    int64_t M, int32_t Z, int32_t D, int32_t log_sigmoid_scores,
                                    float* dvol, float* dw_partial, void* stream);

/* ------------------------------------------------------------------------- *
 * Training path: vector-Jacobian products of the kernels above.
 * The reference obtains these from jax.grad over the same call sites
 * (snap/trainer.py:223-234).  Data-gradients of convs reuse snap_conv2d_nhwc_f32
 * with the rotated / transposed kernel (host side, snap_amd/autograd.py).
 * ------------------------------------------------------------------------- */
/* dw[KH*KW*Cin, Cout] (+)= im2col(prologue(x))^T dy   on f32 MFMA; dy [N,Ho,Wo,Cout]. */
/* The maximum over the loader plans the launch may take (the plan depends on the pointer alignment seen at launch):
 * an upper bound, and no launch touches a byte beyond it. */
size_t snap_conv2d_wgrad_workspace_bytes(const SnapConvDesc* desc);
/* Per-call A/B switches (tools, tests) of the half-precision engines' plans, OR-ed into
 * desc->tile_hint of a snap_conv2d_wgrad_* call (no process-wide state):
 *   SNAP_WGRAD_NO_WIDE   flat kernel gradients (1 x 1, Cin >= 192, >= 65 536 rows) stay on the per-tap
 *                        128 x 128 tiles instead of the 512-thread 256-wide tiles;
 *   SNAP_WGRAD_NO_FUSED3 3 x 3 / stride 1 / pad 1 kernel gradients with a half-precision dy stay on the
 *                        per-tap kernel instead of the fused-tap kernel (all nine taps per workgroup,
 *                        patch-ordered reduction).
 * Same rounded operands, another summation order.  Default (0): both plans where they apply. */
enum { SNAP_WGRAD_NO_WIDE = 1 << 8, SNAP_WGRAD_NO_FUSED3 = 1 << 9 };
int snap_conv2d_wgrad_f32(const SnapConvDesc* desc, const float* x, const float* dy,
                          float* dw, const float* gn_mu, const float* gn_sc,
                          const float* gn_beta, int32_t accumulate, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Row-list variant for the masked fusion MLP (flat [1,1,M,C] Dense layout only): reduction
 * row m reads x row rows_z[m] and dy row rows_dy[m]; only the first *row_count (device
 * scalar) rows exist.  Any of the three may be NULL. */
int snap_conv2d_wgrad_rows_f32(const SnapConvDesc* desc, const float* x, const float* dy,
                               float* dw, const float* gn_mu, const float* gn_sc,
                               const float* gn_beta, int32_t accumulate, void* workspace,
                               size_t workspace_bytes, const int32_t* rows_z,
                               const int32_t* rows_dy, const int32_t* row_count, void* stream);
/* The same with a choice of arithmetic: SNAP_MATH_F32 (exact f32 matrix cores) or
 * SNAP_MATH_BF16 (both operands rounded to bf16 after the f32 prologue, f32 accumulate: the
 * training-precision engine, see snap_conv2d_pack_weights_bf16).  Shapes the bf16 engine does
 * not carry (Cin < 4, unaligned channel rows) run in f32. */
#define SNAP_MATH_F32 0
#define SNAP_MATH_BF16 1
#define SNAP_MATH_F16 2   /* operands rounded to IEEE half (the reference's float16 train config) */
int snap_conv2d_wgrad_ex_f32(const SnapConvDesc* desc, const float* x, const float* dy,
                             float* dw, const float* gn_mu, const float* gn_sc,
                             const float* gn_beta, int32_t accumulate, void* workspace,
                             size_t workspace_bytes, const int32_t* rows_z,
                             const int32_t* rows_dy, const int32_t* row_count, int32_t math,
                             void* stream);

/* ... with ONE of the operands already in the engine's 2-byte element type (math BF16 / F16):
 * x_is_half -- x [rows, Cin_stride] (prologue NONE), dy_is_half -- dy [rows, Cout_stride]; the other
 * operand stays f32.  The hidden activations and inter-layer gradients of the masked MLP, written in
 * that type by SnapConvExtras.y_half / snap_epilogue_bwd_colsum_half: half the bytes, no rounding
 * work, same bits as rounding an f32 copy in the loop. */
int snap_conv2d_wgrad_half_f32(const SnapConvDesc* desc, const void* x, const void* dy, float* dw,
                               const float* gn_mu, const float* gn_sc, const float* gn_beta,
                               int32_t accumulate, void* workspace, size_t workspace_bytes,
                               const int32_t* rows_z, const int32_t* rows_dy,
                               const int32_t* row_count, int32_t math, int32_t x_is_half,
                               int32_t dy_is_half, void* stream);

/* Adam over every parameter tensor in ONE launch (optax.adam as train_step applies it,
 * snap/trainer.py:236-243: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
 * p -= lr / (1 - b1^step) * m / (sqrt(v / (1 - b2^step)) + eps); `step` counts from 1).
 * `items`: DEVICE table sorted by block_begin; item i owns snap_adam_multi_blocks(n) workgroups
 * of 1024 elements.  p, m, v are updated in place; g is read.  apply_flag (optional DEVICE scalar):
 * the whole update is skipped unless *apply_flag > 0 -- the non-finite step skip of
 * trainer.py:269-276 without a host round trip between the finite check and the update. */
typedef struct SnapAdamItem {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  int64_t block_begin;
} SnapAdamItem;
int64_t snap_adam_multi_blocks(int64_t n);
int snap_adam_multi_f32(const SnapAdamItem* items, int32_t n_items, int64_t total_blocks, float lr,
                        float b1, float b2, float eps, int32_t step, const float* apply_flag,
                        void* stream);

/* GroupNorm(+ReLU) backward.  dz: grad w.r.t. the prologue output; add: optional extra
 * gradient summed into dx (identity-residual branch).  mode: SNAP_PRO_GN_RELU /
 * SNAP_PRO_RELU_GN.  dgamma/dbeta [C] (+)=. */
/* Exact: no launch touches a byte beyond this size. */
size_t snap_group_norm_bwd_workspace_bytes(int32_t N, int32_t HW, int32_t C, int32_t groups);
/* ... _ex: dx_half (optional, [N, HW, C] 2-byte elements) also receives dx rounded to bf16
 * (half_kind = 1) or IEEE half (half_kind = 2), RNE -- the operand image the producing layer's
 * data-gradient convolution (SnapConvExtras.x_half) and kernel-gradient GEMM read instead of the
 * f32 tensor. */
int snap_group_norm_bwd_ex_f32(const float* x, const float* dz, const float* add, float* dx,
                               int32_t N, int32_t HW, int32_t C, int32_t groups,
                               const float* mu, const float* rstd, const float* gamma,
                               const float* beta, int32_t mode, float* dgamma, float* dbeta,
                               int32_t accumulate, void* workspace, size_t workspace_bytes,
                               void* dx_half, int32_t half_kind, void* stream);
/* ... with the statistics pass already done by the convolution that wrote dz (SnapConvExtras.gnb_*):
 * stats = that launch's gn_partial ([N][HW / tile_rows + 2][C][2]), tile_rows = snap_conv2d_tile_rows_ex of
 * its descriptor.  stats == NULL: exactly snap_group_norm_bwd_ex_f32. */
int snap_group_norm_bwd_stats_f32(const float* x, const float* dz, const float* add, float* dx,
                                  int32_t N, int32_t HW, int32_t C, int32_t groups,
                                  const float* mu, const float* rstd, const float* gamma,
                                  const float* beta, int32_t mode, float* dgamma, float* dbeta,
                                  int32_t accumulate, void* workspace, size_t workspace_bytes,
                                  void* dx_half, int32_t half_kind, const float* stats, int32_t tile_rows,
                                  void* stream);
int snap_group_norm_bwd_f32(const float* x, const float* dz, const float* add, float* dx,
                            int32_t N, int32_t HW, int32_t C, int32_t groups,
                            const float* mu, const float* rstd, const float* gamma,
                            const float* beta, int32_t mode, float* dgamma, float* dbeta,
                            int32_t accumulate, void* workspace, size_t workspace_bytes,
                            void* stream);

int snap_weight_standardize_bwd_f32(const float* w, const float* dws, float* dw, int32_t K,
                                    int32_t Cout, float eps, void* stream);
int snap_max_pool_3x3s2_bwd_f32(const float* x, const float* dy, float* dx, int32_t N,
                                int32_t H, int32_t W, int32_t C, void* stream);
/* dprev[N,Hp,Wp,C] = transpose of the bilinear x2 up-sampling applied to dy[N,2Hp,2Wp,C]. */
int snap_upsample2x_bwd_f32(const float* dy, float* dprev, int32_t N, int32_t Hp, int32_t Wp,
                            int32_t C, void* stream);
/* out = dy * [y > 0 iff relu] * row_mask  (epilogue gating; y, row_mask optional). */
int snap_epilogue_bwd_f32(const float* dy, const float* y, const uint8_t* row_mask, float* out,
                          int64_t M, int32_t C, int32_t relu, void* stream);
/* out[C] (+)= column sums of a[M,C]  (bias gradients). */
/* Exact: no launch touches a byte beyond this size. */
size_t snap_colsum_workspace_bytes(int64_t M, int32_t C);
/* snap_epilogue_bwd_f32 and the column sums of ITS OUTPUT over the first *row_count rows (all M if
 * NULL) in one pass: the gradient of a bias that sits in front of a ReLU / row mask (layers.py:55-78
 * under jax.grad).  workspace: snap_colsum_workspace_bytes(M, C). */
int snap_epilogue_bwd_colsum_f32(const float* dy, const float* y, const uint8_t* row_mask, float* out,
                                 int64_t M, int32_t C, int32_t relu, const int32_t* row_count,
                                 float* colsum, void* workspace, size_t workspace_bytes, void* stream);
/* ... on 2-byte tensors of the training engine's element type (half_kind 1 = bf16, 2 = IEEE half):
 * dy, y, out [rows, C]; the column sums stay f32.  Rows beyond *row_count are neither read nor
 * written (compact row buffers of the masked MLP). */
int snap_epilogue_bwd_colsum_half(const void* dy, const void* y, void* out, int64_t M, int32_t C,
                                  int32_t relu, const int32_t* row_count, float* colsum,
                                  void* workspace, size_t workspace_bytes, int32_t half_kind,
                                  void* stream);
/* ... plus wsum[C] = sum_r w(r) * out[r, :], w(r) = round_to_element_type(relu?(wsrc[wrows[r] * wstride]))
 * (wrows may be NULL: r itself): the kernel-gradient row of ONE extra input channel of the layer in
 * front -- the 257th channel of the fusion MLP (streetview_encoder.py:277-283) -- taken in the gate
 * pass.  workspace: 2 x snap_colsum_workspace_bytes(M, C). */
int snap_epilogue_bwd_colsum_wsum_half(const void* dy, const void* y, void* out, int64_t M, int32_t C,
                                       int32_t relu, const int32_t* row_count, float* colsum,
                                       void* workspace, size_t workspace_bytes, int32_t half_kind,
                                       const float* wsrc, const int32_t* wrows, int64_t wstride,
                                       int32_t wrelu, float* wsum, void* stream);
/* ... plus (C == 256) the DATA gradient of that channel: dtail[wrows[r] * dstride .. + 3] =
 * (sum_c out[r, c] * round_to_element_type(wtail[c]), 0, 0, 0) -- dtail points at the channel's column of
 * the layer-0 input gradient (f32 rows of dstride floats, 16-byte aligned): with it the data-gradient GEMM
 * in front writes only the whole 128-column tiles (snap_conv2d with Cout_stride > Cout). */
int snap_epilogue_bwd_colsum_wsum_tail_half(const void* dy, const void* y, void* out, int64_t M, int32_t C,
                                            int32_t relu, const int32_t* row_count, float* colsum,
                                            void* workspace, size_t workspace_bytes, int32_t half_kind,
                                            const float* wsrc, const int32_t* wrows, int64_t wstride,
                                            int32_t wrelu, float* wsum, const float* wtail, float* dtail,
                                            int64_t dstride, void* stream);
int snap_colsum_f32(const float* a, int64_t M, int32_t C, float* out, int32_t accumulate,
                    void* workspace, size_t workspace_bytes, void* stream);
/* ... over the listed rows only: sum_{m < *row_count} a[rows[m], :]  (rows / row_count may be NULL). */
int snap_colsum_rows_f32(const float* a, int64_t M, int32_t C, const int32_t* rows,
                         const int32_t* row_count, float* out, int32_t accumulate,
                         void* workspace, size_t workspace_bytes, void* stream);

/* d f_images[B,V,h,w,C] = VJP of snap_lift_pool_f32 w.r.t. f_images (zeroed inside).  The
 * bilinear taps are scatter-added with hardware float atomics: order-dependent sums. */
int snap_lift_pool_bwd_f32(const SnapLiftDesc* desc, const float* f_images, const float* cam,
                           const float* Rt, const float* points, const float* dpooled,
                           float* df_images, void* stream);
/* The same VJP, DETERMINISTIC (bitwise reproducible) and atomic-free: every (voxel, selected
 * view) observation becomes a record, the records are sorted by image pixel (stable radix sort)
 * and one half-wave per pixel gathers the records that touch it in that order; every element of
 * df_images is written exactly once.  workspace: snap_lift_pool_bwd_det_workspace_bytes(desc)
 * bytes (0 = unsupported shape), 256-byte aligned; num_bins <= 32, <= 8 selected views.  Every
 * fusion option of pool_multiview_features (desc->weighted / use_variance / add_minmax; the
 * max / min cotangents are split equally among tied views, as jnp.max's VJP does). */
size_t snap_lift_pool_bwd_det_workspace_bytes(const SnapLiftDesc* desc);
int snap_lift_pool_bwd_det_f32(const SnapLiftDesc* desc, const float* f_images, const float* cam,
                               const float* Rt, const float* points, const float* dpooled,
                               float* df_images, void* workspace, size_t workspace_bytes,
                               void* stream);
/* depth_mlp fusion (streetview_encoder.py:263-267), the VJPs of its two lift passes:
 *   snap_lift_pool_observations_bwd_f32: d pooled -> d obs_feat' [B, N, S, fd] (zero for views that
 *     do not see the point), the pooling VJP on the given (corrected) observations;
 *   snap_lift_observations_bwd_f32: d obs [B, N, S, fd] (the caller's sum of the gradient of
 *     obs[..., :fd] and of obs_feat; depth and ray carry none) -> d f_images, by the deterministic
 *     records / sort / gather machinery with the rows of d obs as the record vectors. */
int snap_lift_pool_observations_bwd_f32(const SnapLiftDesc* desc, const float* cam, const float* Rt,
                                        const float* points, const float* obs_feat,
                                        const float* dpooled, float* dobs, void* stream);
size_t snap_lift_observations_bwd_workspace_bytes(const SnapLiftDesc* desc);
int snap_lift_observations_bwd_f32(const SnapLiftDesc* desc, const float* cam, const float* Rt,
                                   const float* points, const float* dobs, float* df_images,
                                   void* workspace, size_t workspace_bytes, void* stream);
int snap_vertical_pool_bwd_f32(const float* vol, const uint8_t* vvalid, const float* dplane,
                               float* dvol, int64_t M, int32_t Z, int32_t D, int32_t pooling,
                               void* stream);
/* The same VJP for pooling = max from the forward's record (snap_vertical_pool_max_arg_f32): dvol
 * [M, Z, D] is written once and the volume is read only for channels whose maximum is shared by
 * several levels (ties > 1: the gradient is divided between them, as jnp.max's VJP does).  Same
 * values as snap_vertical_pool_bwd_f32, bit for bit. */
int snap_vertical_pool_max_bwd_arg_f32(const float* vol, const uint8_t* vvalid, const uint8_t* argz,
                                       const uint8_t* ties, const float* dplane, float* dvol,
                                       int64_t M, int32_t Z, int32_t D, void* stream);
/* VJP of snap_plane_fuse_match_f32: dplanes[i][M,D] and dy[M,Dm] (gradient w.r.t. the
 * Dense output, for the kernel / bias gradients via wgrad / colsum). */
int snap_plane_fuse_match_bwd_f32(const float* const* planes, const uint8_t* const* valids,
                                  float* const* dplanes, int32_t num_planes, int64_t M,
                                  int32_t D, int32_t pooling, const float* Wm, const float* bm,
                                  int32_t Dm, int32_t normalize, float eps,
                                  const float* dmatching, const float* dfused, float* dy,
                                  void* stream);

/* VJP of snap_pose_score_f32 w.r.t. sim: dsim[B,Nq,X,Y] (planes <= 96 KiB). */
/* Exact: no launch touches a byte beyond this size. */
size_t snap_pose_score_bwd_workspace_bytes(int32_t B, int32_t P);
int snap_pose_score_bwd_f32(const float* dscores, const float* poses, const float* q_xy,
                            const uint8_t* valid_q, const uint8_t* map_valid, int32_t B,
                            int32_t Nq, int32_t X, int32_t Y, int32_t P, float cell_size,
                            int32_t mask_oob, float* dsim, void* workspace,
                            size_t workspace_bytes, void* stream);
/* ... with flags: bit 0 = accumulate the score planes with float LDS atomics (order-dependent sums;
 * A/B timing).  Default (0): where the 8-byte plane fits the LDS (X * Y <= 19 456 cells, no
 * out-of-bounds mask, P <= 10 240) the plane is accumulated in 64-bit fixed point -- exactly
 * associative, so d sim is bitwise reproducible. */
int snap_pose_score_bwd_ex_f32(const float* dscores, const float* poses, const float* q_xy,
                               const uint8_t* valid_q, const uint8_t* map_valid, int32_t B,
                               int32_t Nq, int32_t X, int32_t Y, int32_t P, float cell_size,
                               int32_t mask_oob, int32_t flags, float* dsim, void* workspace,
                               size_t workspace_bytes, void* stream);
/* In place: dsim <- dsim * [sim > 0 iff clip] * coef[b]; partial[B,num_partial] <- partial
 * sums of dsim*sim (temperature gradient). */
int snap_sim_bwd_prepare_f32(float* dsim, const float* sim, int32_t B, int64_t per_scene,
                             int32_t clip_negative, const float* coef, float* partial,
                             int32_t num_partial, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* SNAP_HIP_H_ */
