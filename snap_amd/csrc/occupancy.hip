// OccupancyNet query path (snap/models/occupancy_net.py:34-60,84-116): lidar-ray sample points ->
// trilinear gather of the StreetView feature volume -> occupancy MLP -> logits.
//
//   snap_occupancy_ray_features_f32   producer: sample points (+ labels, ray validity), the
//                                     interpolated feature rows [B*P, D] and their validity.  The
//                                     fallback / training path (its rows feed ops.dense / ag.dense).
//   snap_occupancy_head_f32           the whole chain in ONE launch: no feature row and no hidden
//                                     activation reaches memory; only logits + validity leave.
//
// Point arithmetic (sample_queries_from_rays, :34-60), in f32 with no contraction:
//   dir = hit - origin; dist = sqrt((dx*dx + dy*dy) + dz*dz);
//   dir *= (dist - margin) / clip(dist, min=1)      (the reference's clip, not dist: kept)
//   sample k = 0 is the hit; k = 1..S-1 is (t * dir) + origin, t = (k - 1) / (S - 2) (0 for S = 2),
//   jnp.linspace(0, 1, S - 1) as jax evaluates it (iota / div).  Element order k * N + n.
// The trilinear sample is grid_ops.hip's interpolate_nd_kernel<3> verbatim (grids.py:116-137): the
// same f32 expressions on p = point / cell_size, the same tap order (first axis slowest), the same
// acc = c0 + c1 + ... chain and the zero-weight-invalid-tap rule -- the features are bitwise
// those of snap_interpolate_nd_f32 on the same index-space points.
//
// Fused head layout: one workgroup (8 waves) = 64 consecutive sample rows.
//   gather   D/4 lanes per point, 16-byte tap loads (a voxel row is D floats; the z neighbour is the
//            next row), the blended row goes to LDS as the A operand ([64][D + 2]: the +2 pad makes
//            the MFMA operand fetch A[i = l & 31][k = l >> 5] hit 64 distinct banks).
//   hidden   each hidden layer is a [64 x K] x [K x N] product on v_mfma_f32_32x32x2_f32, one
//            32 x 32 tile per wave at a time, k ascending: the exact f32 MFMA is a k-ordered fmaf
//            chain from zero with a bias-then-ReLU epilogue: the arithmetic class of the f32 Dense
//            engine (conv_igemm.hip), whose results it matches to the last bits (<= 2e-6 relative;
//            not bitwise: the engine's slab staging orders some products differently).  The B
//            operand (weights, [in, out] row-major: lane reads W[k][col], 128 contiguous bytes per
//            half-wave; the next slab's requested before this one's MFMAs) streams from L1 / L2: the
//            train config's weights (64 + 128 KB) do not fit the LDS next to the A and H tiles,
//            and every workgroup of the launch reads the same few hundred KB, so they stay
//            cache-resident.  The first hidden layer's activations go to a second LDS buffer.
//   output   width-1 layer, a fixed-order dot product.  One hidden layer: one lane per row,
//            acc = fmaf(h[k], w[k], acc) for k = 0..K-1 from zero, then + bias.  Two hidden layers:
//            the second is never stored whole -- each 32 x 32 tile is folded into per-row partial
//            dots (an fmaf chain over its 32 columns) in the epilogue, the partials are added in
//            column-tile order: the LDS image stays at 68.6 KB (two workgroups per CU) for the
//            train config.  No atomics: the logits are bitwise repeatable.
// Supported: D, hidden widths multiples of 32 up to 256; one or two hidden layers; last width 1
// (snap_occupancy_head_supported).  Everything else is the producer + ops.dense.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"

namespace {

struct OccArgs {
  const float* hits;         // [B, N, 3]  rays (hits != nullptr) ...
  const float* origins;      // [B, N, 3]
  const uint8_t* ray_mask;   // [B, N]
  const float* points;       // [B, P, 3]  ... or explicit query points
  int64_t N;                 // rays per scene
  int S;                     // samples per ray
  float margin;
  int64_t P;                 // points per scene (S * N, or the query count)
  int64_t B;
  float cell;
  const float* vol;          // [B, X, Y, Z, D]
  const uint8_t* vvalid;     // [B, X, Y, Z] or nullptr
  int X, Y, Z, D;
  float* out_points;         // [B, P, 3]  optional
  uint8_t* out_labels;       // [B, P]     optional
  uint8_t* out_ray_valid;    // [B, P]     optional
};

__device__ __forceinline__ void occ_point(const OccArgs& a, int64_t b, int64_t p, float xyz[3],
                                          bool& label, bool& rvalid) {
  if (a.hits) {
    const int64_t k = p / a.N;
    const int64_t r = b * a.N + (p - k * a.N);
    const float* h = a.hits + r * 3;
    label = k == 0;
    rvalid = a.ray_mask[r] != 0;
    if (k == 0) {
      xyz[0] = h[0]; xyz[1] = h[1]; xyz[2] = h[2];
      return;
    }
    const float* o = a.origins + r * 3;
    float d0 = h[0] - o[0], d1 = h[1] - o[1], d2 = h[2] - o[2];
    const float dist = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    const float s = (dist - a.margin) / (dist < 1.f ? 1.f : dist);   // clip(min=1); NaN passes
    d0 = d0 * s; d1 = d1 * s; d2 = d2 * s;
    const float t = a.S > 2 ? (float)(k - 1) / (float)(a.S - 2) : 0.f;
    xyz[0] = t * d0 + o[0];
    xyz[1] = t * d1 + o[1];
    xyz[2] = t * d2 + o[2];
  } else {
    const float* q = a.points + (b * a.P + p) * 3;
    xyz[0] = q[0]; xyz[1] = q[1]; xyz[2] = q[2];
    label = false;
    rvalid = true;
  }
}

// interpolate_nd_kernel<3>'s set-up: voxel index of each tap (product order) and its weight
__device__ __forceinline__ void occ_taps(const OccArgs& a, const float xyz[3], int off[8], float ww[8],
                                         bool& inb) {
  const int size[3] = {a.X, a.Y, a.Z};
  int idx[3][2];
  float w[3][2];
  inb = true;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const float p = xyz[t] / a.cell;
    inb = inb && (p >= 0.f) && (p < (float)size[t]);
    const float c = p - 0.5f;
    const float lo = floorf(c);
    const float whi = c - lo;
    w[t][0] = 1.f - whi;
    w[t][1] = whi;
    // lo is clamped to [-1, size] BEFORE the conversion: a float-to-int conversion out of range is
    // undefined, and with il = INT_MAX (lo = +inf, 1e30) the compiler's rewrite of the clamp below,
    // min(max(il, -1) + 1, size - 1), wrapped to INT_MIN: an out-of-bounds tap.  NaN -> -1 (fmaxf).
    const int il = (int)fminf(fmaxf(lo, -1.f), (float)size[t]);
    idx[t][0] = min(max(il, 0), size[t] - 1);
    idx[t][1] = min(max(il + 1, 0), size[t] - 1);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int o = 0;
    float wc = 1.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int bit = (c >> (2 - t)) & 1;
      o = o * size[t] + idx[t][bit];
      wc = t == 0 ? w[t][bit] : wc * w[t][bit];
    }
    off[c] = o;
    ww[c] = wc;
  }
}

__device__ __forceinline__ bool occ_taps_ok(const OccArgs& a, int64_t b, const int off[8]) {
  if (!a.vvalid) return true;
  const uint8_t* v = a.vvalid + b * ((int64_t)a.X * a.Y * a.Z);
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) ok = ok && v[off[c]] != 0;
  return ok;
}

__device__ __forceinline__ void occ_write_sample(const OccArgs& a, int64_t row, const float xyz[3], bool label,
                                                 bool rvalid) {
  if (a.out_points) {
    a.out_points[row * 3 + 0] = xyz[0];
    a.out_points[row * 3 + 1] = xyz[1];
    a.out_points[row * 3 + 2] = xyz[2];
  }
  if (a.out_labels) a.out_labels[row] = label ? 1 : 0;
  if (a.out_ray_valid) a.out_ray_valid[row] = rvalid ? 1 : 0;
}

// the blend of channels [ch, ch + 4) of one point: acc = w0 v0 + w1 v1 + ... (product order)
__device__ __forceinline__ f32x4 occ_blend4(const float* __restrict__ base, int D, int ch, const int off[8],
                                            const float ww[8]) {
  f32x4 v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const f32x4*>(base + (int64_t)off[c] * D + ch);
  f32x4 acc;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float contrib = ww[c] * v[c][e];
      acc[e] = c == 0 ? contrib : acc[e] + contrib;
    }
  }
  return acc;
}

__device__ __forceinline__ float occ_blend1(const float* __restrict__ base, int D, int ch, const int off[8],
                                            const float ww[8]) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float contrib = ww[c] * base[(int64_t)off[c] * D + ch];
    acc = c == 0 ? contrib : acc + contrib;
  }
  return acc;
}

// ---- producer: one thread per (point, 4 channels) [VW = 4] or (point, channel) [VW = 1] ----------
template <int VW>
__global__ __launch_bounds__(256) void occ_features_kernel(const OccArgs a, float* __restrict__ feat,
                                                           uint8_t* __restrict__ valid) {
  const int Q = a.D / VW;
  const int64_t total = a.B * a.P * Q;
  const int64_t XYZ = (int64_t)a.X * a.Y * a.Z;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / Q;
    const int q = (int)(i - row * Q);
    const int64_t b = row / a.P;
    const int64_t p = row - b * a.P;
    float xyz[3];
    bool label, rvalid, inb;
    occ_point(a, b, p, xyz, label, rvalid);
    int off[8];
    float ww[8];
    occ_taps(a, xyz, off, ww, inb);
    const float* base = a.vol + b * XYZ * a.D;
    if constexpr (VW == 4) {
      *reinterpret_cast<f32x4*>(feat + row * a.D + 4 * q) = occ_blend4(base, a.D, 4 * q, off, ww);
    } else {
      feat[row * a.D + q] = occ_blend1(base, a.D, q, off, ww);
    }
    if (q == 0) {
      valid[row] = (inb && occ_taps_ok(a, b, off)) ? 1 : 0;
      occ_write_sample(a, row, xyz, label, rvalid);
    }
  }
}

// ---- fused head --------------------------------------------------------------------------------
constexpr int kHeadRows = 64;
constexpr int kHeadThreads = 512;

struct HeadArgs {
  OccArgs a;
  const float* w0;
  const float* b0;
  int h1;
  const float* w1;           // nullptr: one hidden layer
  const float* b1;
  int h2;
  const float* wo;           // [h_last]
  const float* bo;           // [1]
  float* logits;             // [B * P]
  uint8_t* valid;            // [B * P]
};

// Y[64][N] = relu(X[64][K] W[K][N] + bias) on the exact f32 MFMA (LDS in, LDS out)
__device__ __forceinline__ void head_layer(const float* X, int sx, int K, const float* __restrict__ W,
                                           const float* __restrict__ bias, int N, float* Y, int sy, int wave,
                                           int lane) {
  const int ntiles = (kHeadRows / 32) * (N / 32);
  const int i = lane & 31, hk = lane >> 5;
  for (int t = wave; t < ntiles; t += kHeadThreads / 64) {
    const int rt = t & 1, ct = t >> 1;
    const float* xa = X + (rt * 32 + i) * sx + hk;
    const float* wb = W + (int64_t)hk * N + ct * 32 + i;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // the weights of the next 16-deep k slab are requested before the MFMAs of this one
    float bv[8], bn[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) bn[u] = wb[(int64_t)(2 * u) * N];
    for (int k = 0; k < K; k += 16) {
      float av[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        bv[u] = bn[u];
        av[u] = xa[k + 2 * u];
      }
      if (k + 16 < K) {
#pragma unroll
        for (int u = 0; u < 8; ++u) bn[u] = wb[(int64_t)(k + 16 + 2 * u) * N];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    }
    const int col = ct * 32 + i;
    const float bb = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
      Y[row * sy + col] = snap_relu(acc[r] + bb);
    }
  }
}

// The last hidden layer fused with the width-1 output: relu(X W + b) is never stored whole.  Each
// 32 x 32 tile goes to the wave's own scratch ([32][33]), and lane i (< 32) folds its row into
// partial[ct][row] = fmaf chain over the tile's 32 columns (c ascending); the caller sums the
// column tiles in ct order.  A fixed-order dot product: bitwise repeatable.
constexpr int kScratchFloats = (kHeadThreads / 64) * 32 * 33;
constexpr int kDotFloats = kScratchFloats + 8 * kHeadRows;      // + partial[8][64]

__device__ __forceinline__ void head_layer_dot(const float* X, int sx, int K, const float* __restrict__ W,
                                               const float* __restrict__ bias, int N, const float* __restrict__ wo,
                                               float* scratch, float* partial, int wave, int lane) {
  const int ntiles = (kHeadRows / 32) * (N / 32);
  const int i = lane & 31, hk = lane >> 5;
  float* sw = scratch + wave * (32 * 33);
  for (int t = wave; t < ntiles; t += kHeadThreads / 64) {
    const int rt = t & 1, ct = t >> 1;
    const float* xa = X + (rt * 32 + i) * sx + hk;
    const float* wb = W + (int64_t)hk * N + ct * 32 + i;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bv[8], bn[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) bn[u] = wb[(int64_t)(2 * u) * N];
    for (int k = 0; k < K; k += 16) {
      float av[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        bv[u] = bn[u];
        av[u] = xa[k + 2 * u];
      }
      if (k + 16 < K) {
#pragma unroll
        for (int u = 0; u < 8; ++u) bn[u] = wb[(int64_t)(k + 16 + 2 * u) * N];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    }
    const float bb = bias[ct * 32 + i];
#pragma unroll
    for (int r = 0; r < 16; ++r) sw[((r & 3) + 8 * (r >> 2) + 4 * hk) * 33 + i] = snap_relu(acc[r] + bb);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (hk == 0) {
      const float* w = wo + ct * 32;
      float p = 0.f;
#pragma unroll
      for (int c = 0; c < 32; ++c) p = fmaf(sw[i * 33 + c], w[c], p);
      partial[ct * kHeadRows + rt * 32 + i] = p;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// BUF0: floats of the A / second-hidden buffer, BUF1: of the first-hidden buffer (64 rows each)
template <int BUF0, int BUF1>
__global__ __launch_bounds__(kHeadThreads) void occ_head_kernel(const HeadArgs h) {
  __shared__ __attribute__((aligned(16))) float smem[BUF0 + BUF1];
  float* const buf0 = smem;
  float* const buf1 = smem + BUF0;
  const OccArgs& a = h.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t rows = a.B * a.P;
  const int64_t row0 = (int64_t)blockIdx.x * kHeadRows;
  const int64_t XYZ = (int64_t)a.X * a.Y * a.Z;

  // 1. sample points + trilinear gather -> buf0 [64][D + 2]
  const int Q = a.D >> 2;
  const int ppp = kHeadThreads / Q;
  const int slot = tid / Q;
  const int q = tid - slot * Q;
  const int sx = a.D + 2;
  if (slot < ppp) {
    for (int r = slot; r < kHeadRows; r += ppp) {
      const int64_t row = row0 + r;
      float* dst = buf0 + r * sx + 4 * q;
      f32x4 f = {0.f, 0.f, 0.f, 0.f};
      if (row < rows) {
        const int64_t b = row / a.P;
        const int64_t p = row - b * a.P;
        float xyz[3];
        bool label, rvalid, inb;
        occ_point(a, b, p, xyz, label, rvalid);
        int off[8];
        float ww[8];
        occ_taps(a, xyz, off, ww, inb);
        f = occ_blend4(a.vol + b * XYZ * a.D, a.D, 4 * q, off, ww);
        if (q == 0) {
          h.valid[row] = (inb && occ_taps_ok(a, b, off)) ? 1 : 0;
          occ_write_sample(a, row, xyz, label, rvalid);
        }
      }
      dst[0] = f[0]; dst[1] = f[1]; dst[2] = f[2]; dst[3] = f[3];
    }
  }
  __syncthreads();

  // 2. hidden layers (bias + ReLU epilogue)
  head_layer(buf0, sx, a.D, h.w0, h.b0, h.h1, buf1, h.h1 + 2, wave, lane);
  __syncthreads();
  if (h.w1) {
    // 3'. second hidden layer + width-1 output (buf0, the dead A tile, becomes the scratch)
    float* partial = buf0 + kScratchFloats;
    head_layer_dot(buf1, h.h1 + 2, h.h1, h.w1, h.b1, h.h2, h.wo, buf0, partial, wave, lane);
    __syncthreads();
    if (tid < kHeadRows) {
      const int64_t row = row0 + tid;
      if (row < rows) {
        float acc = partial[tid];
        for (int ct = 1; ct < h.h2 / 32; ++ct) acc = acc + partial[ct * kHeadRows + tid];
        h.logits[row] = acc + h.bo[0];
      }
    }
    return;
  }
  const float* last = buf1;
  const int K = h.h1;

  // 3. width-1 output layer: one k-ordered fmaf chain per row
  if (tid < kHeadRows) {
    const int64_t row = row0 + tid;
    if (row < rows) {
      const float* x = last + tid * (K + 2);
      float acc = 0.f;
      for (int k = 0; k < K; k += 16) {        // (loads of 16 steps in flight, then the chain)
        float xv[16], wv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          xv[u] = x[k + u];
          wv[u] = h.wo[k + u];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = fmaf(xv[u], wv[u], acc);
      }
      h.logits[row] = acc + h.bo[0];
    }
  }
}

// the point source and the grid (everything but the volume and the optional outputs)
int occ_setup_source(OccArgs& a, const float* hits, const float* origins, const uint8_t* ray_mask, int64_t num_rays,
                     int32_t num_samples, float margin, const float* points, int64_t num_points, int32_t B, int32_t X,
                     int32_t Y, int32_t Z, int32_t D, float cell_size) {
  if (B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || D <= 0 || !(cell_size > 0.f)) return SNAP_ERR_BAD_SHAPE;
  if ((int64_t)X * Y * Z >= ((int64_t)1 << 31)) return SNAP_ERR_BAD_SHAPE;     // (tap offsets are int)
  a = OccArgs{};
  if (hits) {
    if (!origins || !ray_mask) return SNAP_ERR_NULL;
    if (num_rays <= 0 || num_samples <= 0) return SNAP_ERR_BAD_SHAPE;
    a.hits = hits; a.origins = origins; a.ray_mask = ray_mask;
    a.N = num_rays; a.S = num_samples; a.margin = margin;
    a.P = num_rays * num_samples;
  } else {
    if (!points) return SNAP_ERR_NULL;
    if (num_points <= 0) return SNAP_ERR_BAD_SHAPE;
    a.points = points;
    a.N = 1; a.S = 1;
    a.P = num_points;
  }
  a.B = B;
  a.cell = cell_size;
  a.X = X; a.Y = Y; a.Z = Z; a.D = D;
  return SNAP_OK;
}

int occ_setup(OccArgs& a, const float* hits, const float* origins, const uint8_t* ray_mask, int64_t num_rays,
              int32_t num_samples, float margin, const float* points, int64_t num_points, int32_t B,
              const float* volume, const uint8_t* volume_valid, int32_t X, int32_t Y, int32_t Z, int32_t D,
              float cell_size, float* out_points, uint8_t* out_labels, uint8_t* out_ray_valid) {
  if (!volume) return SNAP_ERR_NULL;
  const int st = occ_setup_source(a, hits, origins, ray_mask, num_rays, num_samples, margin, points, num_points, B,
                                  X, Y, Z, D, cell_size);
  if (st != SNAP_OK) return st;
  a.vol = volume; a.vvalid = volume_valid;
  a.out_points = out_points; a.out_labels = out_labels; a.out_ray_valid = out_ray_valid;
  return SNAP_OK;
}

}  // namespace

extern "C" int snap_occupancy_ray_features_f32(
    const float* hits, const float* origins, const uint8_t* ray_mask, int64_t num_rays, int32_t num_samples,
    float margin, const float* points, int64_t num_points, int32_t B, const float* volume,
    const uint8_t* volume_valid, int32_t X, int32_t Y, int32_t Z, int32_t D, float cell_size, float* out_points,
    uint8_t* out_labels, uint8_t* out_ray_valid, float* features, uint8_t* valid, void* stream) {
  if (!features || !valid) return SNAP_ERR_NULL;
  OccArgs a;
  const int st = occ_setup(a, hits, origins, ray_mask, num_rays, num_samples, margin, points, num_points, B, volume,
                           volume_valid, X, Y, Z, D, cell_size, out_points, out_labels, out_ray_valid);
  if (st != SNAP_OK) return st;
  const bool vec = (D % 4) == 0 && (reinterpret_cast<uintptr_t>(volume) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(features) & 15) == 0;
  const int64_t total = a.B * a.P * (vec ? D / 4 : D);
  const int64_t blocks = snap_cdiv(total, 256);
  const dim3 grid((unsigned)(blocks < (1 << 22) ? blocks : (1 << 22)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(occ_features_kernel<4>, grid, dim3(256), 0, s, a, features, valid);
  else hipLaunchKernelGGL(occ_features_kernel<1>, grid, dim3(256), 0, s, a, features, valid);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

extern "C" int32_t snap_occupancy_head_supported(int32_t D, int32_t h1, int32_t h2) {
  auto ok = [](int32_t w) { return w > 0 && w % 32 == 0 && w <= 256; };
  return (ok(D) && ok(h1) && (h2 == 0 || ok(h2))) ? 1 : 0;
}

extern "C" int snap_occupancy_head_f32(
    const float* hits, const float* origins, const uint8_t* ray_mask, int64_t num_rays, int32_t num_samples,
    float margin, const float* points, int64_t num_points, int32_t B, const float* volume,
    const uint8_t* volume_valid, int32_t X, int32_t Y, int32_t Z, int32_t D, float cell_size, const float* w0,
    const float* b0, int32_t h1, const float* w1, const float* b1, int32_t h2, const float* w_out,
    const float* b_out, float* out_points, uint8_t* out_labels, uint8_t* out_ray_valid, float* logits,
    uint8_t* valid, void* stream) {
  if (!w0 || !b0 || !w_out || !b_out || !logits || !valid) return SNAP_ERR_NULL;
  if (h2 && (!w1 || !b1)) return SNAP_ERR_NULL;
  if (!snap_occupancy_head_supported(D, h1, h2)) return SNAP_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(volume) & 15) return SNAP_ERR_UNSUPPORTED;
  HeadArgs h{};
  const int st = occ_setup(h.a, hits, origins, ray_mask, num_rays, num_samples, margin, points, num_points, B,
                           volume, volume_valid, X, Y, Z, D, cell_size, out_points, out_labels, out_ray_valid);
  if (st != SNAP_OK) return st;
  h.w0 = w0; h.b0 = b0; h.h1 = h1;
  h.w1 = h2 ? w1 : nullptr; h.b1 = h2 ? b1 : nullptr; h.h2 = h2;
  h.wo = w_out; h.bo = b_out;
  h.logits = logits; h.valid = valid;
  const int64_t rows = h.a.B * h.a.P;
  const dim3 grid((unsigned)snap_cdiv(rows, kHeadRows));
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the LDS image of the launch: buf0 = the A tile [64][D + 2] (then, with two hidden layers, the
  // per-wave scratch + partial sums of the fused output layer), buf1 = [64][h1 + 2]; the small form
  // (68.6 KB: D, h1 <= 128, both reference configs) leaves room for two workgroups per CU
  static_assert(kDotFloats <= kHeadRows * 258, "scratch fits the large A tile");
  if (D <= 128 && h1 <= 128)
    hipLaunchKernelGGL((occ_head_kernel<kDotFloats, kHeadRows * 130>), grid, dim3(kHeadThreads), 0, s, h);
  else if (h1 <= 128)
    hipLaunchKernelGGL((occ_head_kernel<kHeadRows * 258, kHeadRows * 130>), grid, dim3(kHeadThreads), 0, s, h);
  else
    hipLaunchKernelGGL((occ_head_kernel<kHeadRows * 258, kHeadRows * 258>), grid, dim3(kHeadThreads), 0, s, h);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

// ---- VJP of the producer into the volume (grids.py:116-137 differentiated, occupancy_net.py:106-111) ----
// d_volume = (d features / d volume)^T d_features.  Every point is re-derived with occ_point / occ_taps (the
// forward's f32 expressions, tap order and clamps) into 8 records (voxel, p, c) of weight ww[c]; the
// contribution of a record to channel ch is ww[c] * d_features[b * P + p, ch] (one f32 multiply).
// Summation order, per voxel of each scene (bitwise contract):
//   its records in ascending (p, c), cut into consecutive chunks of kVjpChunk records; each chunk sum starts
//   from its first contribution and adds the rest in order; the voxel starts from its first chunk sum and
//   adds the others in chunk order; a voxel with no record is +0.
// Passes (no float atomics, every d_volume element written once):
//   1. records: key = b * XYZ + voxel (u32), weight by record id (b * P + p) * 8 + c
//   2. stable radix sort of the record ids by key (only the key bits in use): ties keep (p, c) order
//   3. segment bounds of every touched key (start / end in the sorted order)
//   4. per key: chunk count and, for keys of more than one chunk, partial-sum slots (one packed u64 scan)
//   5. chunk heads: sorted position of the first record of every chunk
//   6. chunk pass: one group of D/4 lanes (x float4) per chunk; a key of one chunk writes d_volume directly,
//      a longer key writes its chunk's partial row
//   7. combine: per key, zero rows and the in-order sum of the partial rows of multi-chunk keys
// kVjpChunk follows the split rule of a skewed gather (lists longer than a quarter of one wave's share of
// the records are cut): ~8 M records over ~8 K resident waves -> ~1000 per wave -> 256.
namespace {

constexpr int kVjpChunk = 256;

struct VjpLayout {
  size_t R, nkeys, max_chunks, max_partials;
  int bits;
  size_t off_keys, off_keys_out, off_vals_out, off_w, off_seg, off_cval, off_cbase, off_pos, off_part, off_tmp;
  size_t tmp_bytes, total;
};

inline size_t vjp_align(size_t v) { return (v + 255) & ~(size_t)255; }

int vjp_layout(int64_t P, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t D, VjpLayout* L) {
  if (P <= 0 || B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || D <= 0) return SNAP_ERR_BAD_SHAPE;
  const int64_t XYZ = (int64_t)X * Y * Z;
  if (XYZ >= ((int64_t)1 << 31)) return SNAP_ERR_BAD_SHAPE;
  if (P >= ((int64_t)1 << 32) || (int64_t)B * P >= ((int64_t)1 << 29)) return SNAP_ERR_BAD_SHAPE;  // B P 8 < 2^32
  if ((int64_t)B * XYZ >= ((int64_t)1 << 32) - 1) return SNAP_ERR_BAD_SHAPE;                       // keys in u32
  L->R = (size_t)B * P * 8;
  L->nkeys = (size_t)B * XYZ;
  L->bits = 1;
  while (((size_t)1 << L->bits) < L->nkeys) ++L->bits;
  // every chunk holds >= 1 record and all but the last of a key hold kVjpChunk: <= touched keys + R / L;
  // a key of more than one chunk has > L records and ceil(n / L) < 2 n / L partial slots
  L->max_chunks = (L->nkeys < L->R ? L->nkeys : L->R) + L->R / kVjpChunk + 1;
  L->max_partials = 2 * L->R / kVjpChunk + 1;
  size_t sort_tmp = 0, scan_tmp = 0;
  unsigned* nul = nullptr;
  unsigned long long* nul64 = nullptr;
  if (rocprim::radix_sort_pairs(nullptr, sort_tmp, nul, nul, rocprim::counting_iterator<unsigned>(0), nul, L->R, 0,
                                L->bits, (hipStream_t)0) != hipSuccess)
    return SNAP_ERR_LAUNCH;
  if (rocprim::exclusive_scan(nullptr, scan_tmp, nul64, nul64, 0ull, L->nkeys + 1,
                              rocprim::plus<unsigned long long>(), (hipStream_t)0) != hipSuccess)
    return SNAP_ERR_LAUNCH;
  L->tmp_bytes = sort_tmp > scan_tmp ? sort_tmp : scan_tmp;
  size_t o = 0;
  L->off_keys = o;     o += vjp_align(L->R * sizeof(unsigned));
  L->off_keys_out = o; o += vjp_align(L->R * sizeof(unsigned));
  L->off_vals_out = o; o += vjp_align(L->R * sizeof(unsigned));
  L->off_w = o;        o += vjp_align(L->R * sizeof(float));
  L->off_seg = o;      o += vjp_align(2 * L->nkeys * sizeof(unsigned));             // start [nkeys] | end [nkeys]
  L->off_cval = o;     o += vjp_align((L->nkeys + 1) * sizeof(unsigned long long));
  L->off_cbase = o;    o += vjp_align((L->nkeys + 1) * sizeof(unsigned long long));
  L->off_pos = o;      o += vjp_align(L->max_chunks * sizeof(unsigned));
  L->off_part = o;     o += vjp_align(L->max_partials * (size_t)D * sizeof(float));
  L->off_tmp = o;      o += vjp_align(L->tmp_bytes);
  L->total = o;
  return SNAP_OK;
}

struct VjpArgs {
  OccArgs a;
  const float* dfeat;        // [B * P, D]
  float* dvol;               // [B, X, Y, Z, D]
  unsigned* keys;            // [R] by record id
  float* w;                  // [R] by record id
  const unsigned* skeys;     // [R] sorted keys
  const unsigned* svals;     // [R] record ids in sorted order
  unsigned* seg_start;       // [nkeys]
  unsigned* seg_end;         // [nkeys]  (both 0 for an untouched key)
  unsigned long long* cval;  // [nkeys + 1] chunks << 32 | partial slots
  const unsigned long long* cbase;   // exclusive scan of cval
  unsigned* chunk_pos;       // [chunks] sorted position of every chunk's first record
  float* part;               // [partial slots, D]
  int64_t R, nkeys;
};

__global__ __launch_bounds__(256) void occ_vjp_records_kernel(const VjpArgs v) {
  const OccArgs& a = v.a;
  const int64_t XYZ = (int64_t)a.X * a.Y * a.Z;
  const int64_t rows = a.B * a.P;
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < rows; row += (int64_t)gridDim.x * 256) {
    const int64_t b = row / a.P;
    const int64_t p = row - b * a.P;
    float xyz[3];
    bool label, rvalid, inb;
    occ_point(a, b, p, xyz, label, rvalid);
    int off[8];
    float ww[8];
    occ_taps(a, xyz, off, ww, inb);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      v.keys[row * 8 + c] = (unsigned)(b * XYZ + off[c]);
      v.w[row * 8 + c] = ww[c];
    }
  }
}

__global__ __launch_bounds__(256) void occ_vjp_bounds_kernel(const VjpArgs v) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < v.R; i += (int64_t)gridDim.x * 256) {
    const unsigned k = v.skeys[i];
    if (i == 0 || v.skeys[i - 1] != k) v.seg_start[k] = (unsigned)i;
    if (i == v.R - 1 || v.skeys[i + 1] != k) v.seg_end[k] = (unsigned)(i + 1);
  }
}

__global__ __launch_bounds__(256) void occ_vjp_count_kernel(const VjpArgs v) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k <= v.nkeys; k += (int64_t)gridDim.x * 256) {
    unsigned long long c = 0;
    if (k < v.nkeys) {
      const unsigned n = v.seg_end[k] - v.seg_start[k];
      const unsigned long long nch = (n + kVjpChunk - 1) / kVjpChunk;
      c = (nch << 32) | (nch > 1 ? nch : 0ull);
    }
    v.cval[k] = c;
  }
}

__global__ __launch_bounds__(256) void occ_vjp_heads_kernel(const VjpArgs v) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < v.R; i += (int64_t)gridDim.x * 256) {
    const unsigned k = v.skeys[i];
    const unsigned rank = (unsigned)i - v.seg_start[k];
    if (rank % kVjpChunk == 0) v.chunk_pos[(v.cbase[k] >> 32) + rank / kVjpChunk] = (unsigned)i;
  }
}

template <int VW>
__device__ __forceinline__ void vjp_load(const float* p, float (&x)[VW]) {
  if constexpr (VW == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
  } else {
    x[0] = *p;
  }
}

template <int VW>
__device__ __forceinline__ void vjp_store(float* p, const float (&x)[VW]) {
  if constexpr (VW == 4) *reinterpret_cast<f32x4*>(p) = f32x4{x[0], x[1], x[2], x[3]};
  else *p = x[0];
}

// one group of G lanes per chunk (grid-stride over the chunks); lane l owns the VW-channel slices
// q = l, l + G, ... < D / VW.  Record ids and weights of up to G entries by one load (lane = entry),
// handed round by shuffles; 8 feature rows in flight, added in list order.
template <int VW, int G>
__global__ __launch_bounds__(256) void occ_vjp_chunks_kernel(const VjpArgs v) {
  constexpr int U = 8;
  const int D = v.a.D;
  const int Q = D / VW;
  const int lane = threadIdx.x & (G - 1);
  const int64_t group = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const int64_t ngroups = (int64_t)gridDim.x * (256 / G);
  const int64_t nchunks = (int64_t)(v.cbase[v.nkeys] >> 32);
  for (int64_t ch = group; ch < nchunks; ch += ngroups) {
    const unsigned i0 = v.chunk_pos[ch];
    const unsigned k = v.skeys[i0];
    const unsigned st = v.seg_start[k], en = v.seg_end[k];
    const unsigned i1 = min(i0 + (unsigned)kVjpChunk, en);
    const bool multi = en - st > (unsigned)kVjpChunk;
    float* out = multi ? v.part + ((int64_t)(v.cbase[k] & 0xffffffffull) + (i0 - st) / kVjpChunk) * D
                       : v.dvol + (int64_t)k * D;
    for (int q0 = 0; q0 < Q; q0 += G) {
      const int q = q0 + lane;
      const bool on = q < Q;
      float acc[VW];
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[e] = 0.f;
      bool first = true;
      for (unsigned base = i0; base < i1; base += G) {
        const unsigned nb = min((unsigned)G, i1 - base);
        const unsigned my_rec = v.svals[min(base + (unsigned)lane, i1 - 1u)];
        const float my_w = v.w[my_rec];
        for (unsigned u0 = 0; u0 < nb; u0 += U) {
          float x[U][VW], w[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int src = (int)min(u0 + u, nb - 1u);
            const unsigned rec = (unsigned)__shfl((int)my_rec, src, G);
            w[u] = __shfl(my_w, src, G);
            if (on) vjp_load<VW>(v.dfeat + (int64_t)(rec >> 3) * D + VW * q, x[u]);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (u0 + u >= nb) break;
#pragma unroll
            for (int e = 0; e < VW; ++e) {
              const float contrib = w[u] * x[u][e];
              acc[e] = first ? contrib : acc[e] + contrib;
            }
            first = false;
          }
        }
      }
      if (on) vjp_store<VW>(out + VW * q, acc);
    }
  }
}

// one thread per (key, VW-channel slice): +0 rows for untouched keys, the in-order sum of the partial rows
// for multi-chunk keys (16 rows in flight); single-chunk keys were written by the chunk pass
template <int VW>
__global__ __launch_bounds__(256) void occ_vjp_combine_kernel(const VjpArgs v) {
  constexpr int U = 16;
  const int D = v.a.D;
  const int Q = D / VW;
  const int64_t total = v.nkeys * Q;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t k = t / Q;
    const int q = (int)(t - k * Q);
    const unsigned n = v.seg_end[k] - v.seg_start[k];
    float acc[VW];
    if (n == 0) {
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[e] = 0.f;
    } else if (n <= (unsigned)kVjpChunk) {
      continue;
    } else {
      const int64_t nch = (n + kVjpChunk - 1) / kVjpChunk;
      const float* p = v.part + (int64_t)(v.cbase[k] & 0xffffffffull) * D + VW * q;
      vjp_load<VW>(p, acc);
      int64_t j = 1;
      for (; j + U <= nch; j += U) {
        float x[U][VW];
#pragma unroll
        for (int u = 0; u < U; ++u) vjp_load<VW>(p + (j + u) * D, x[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int e = 0; e < VW; ++e) acc[e] = acc[e] + x[u][e];
        }
      }
      for (; j < nch; ++j) {
        float x[VW];
        vjp_load<VW>(p + j * D, x);
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = acc[e] + x[e];
      }
    }
    vjp_store<VW>(v.dvol + k * D + VW * q, acc);
  }
}

inline dim3 vjp_grid(int64_t items) {
  const int64_t blocks = snap_cdiv(items, 256);
  return dim3((unsigned)(blocks < (1 << 20) ? (blocks > 0 ? blocks : 1) : (1 << 20)));
}

}  // namespace

extern "C" int32_t snap_occupancy_features_vjp_chunk(void) { return kVjpChunk; }

extern "C" size_t snap_occupancy_features_vjp_workspace_bytes(int64_t num_points, int32_t B, int32_t X, int32_t Y,
                                                              int32_t Z, int32_t D) {
  VjpLayout L;
  if (vjp_layout(num_points, B, X, Y, Z, D, &L) != SNAP_OK) return 0;
  return L.total;
}

extern "C" int snap_occupancy_ray_features_vjp_f32(
    const float* hits, const float* origins, const uint8_t* ray_mask, int64_t num_rays, int32_t num_samples,
    float margin, const float* points, int64_t num_points, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t D,
    float cell_size, const float* d_features, float* d_volume, void* workspace, size_t workspace_bytes,
    void* stream) {
  if (!d_features || !d_volume || !workspace) return SNAP_ERR_NULL;
  VjpArgs v{};
  const int st = occ_setup_source(v.a, hits, origins, ray_mask, num_rays, num_samples, margin, points, num_points, B,
                                  X, Y, Z, D, cell_size);
  if (st != SNAP_OK) return st;
  VjpLayout L;
  const int lst = vjp_layout(v.a.P, B, X, Y, Z, D, &L);
  if (lst != SNAP_OK) return lst;
  if (workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) return SNAP_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  v.dfeat = d_features;
  v.dvol = d_volume;
  v.keys = reinterpret_cast<unsigned*>(ws + L.off_keys);
  v.w = reinterpret_cast<float*>(ws + L.off_w);
  unsigned* skeys = reinterpret_cast<unsigned*>(ws + L.off_keys_out);
  unsigned* svals = reinterpret_cast<unsigned*>(ws + L.off_vals_out);
  v.skeys = skeys;
  v.svals = svals;
  v.seg_start = reinterpret_cast<unsigned*>(ws + L.off_seg);
  v.seg_end = v.seg_start + L.nkeys;
  v.cval = reinterpret_cast<unsigned long long*>(ws + L.off_cval);
  unsigned long long* cbase = reinterpret_cast<unsigned long long*>(ws + L.off_cbase);
  v.cbase = cbase;
  v.chunk_pos = reinterpret_cast<unsigned*>(ws + L.off_pos);
  v.part = reinterpret_cast<float*>(ws + L.off_part);
  v.R = (int64_t)L.R;
  v.nkeys = (int64_t)L.nkeys;
  if (hipMemsetAsync(v.seg_start, 0, 2 * L.nkeys * sizeof(unsigned), s) != hipSuccess) return SNAP_ERR_LAUNCH;
  // 1. records
  hipLaunchKernelGGL(occ_vjp_records_kernel, vjp_grid(v.a.B * v.a.P), dim3(256), 0, s, v);
  SNAP_CHECK_LAUNCH();
  // 2. stable sort of the record ids by key
  size_t tmp = L.tmp_bytes;
  if (rocprim::radix_sort_pairs(ws + L.off_tmp, tmp, v.keys, skeys, rocprim::counting_iterator<unsigned>(0), svals,
                                L.R, 0, L.bits, s) != hipSuccess)
    return SNAP_ERR_LAUNCH;
  // 3. segment bounds, 4. chunk counts + their scan, 5. chunk heads
  hipLaunchKernelGGL(occ_vjp_bounds_kernel, vjp_grid(v.R), dim3(256), 0, s, v);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(occ_vjp_count_kernel, vjp_grid(v.nkeys + 1), dim3(256), 0, s, v);
  SNAP_CHECK_LAUNCH();
  tmp = L.tmp_bytes;
  if (rocprim::exclusive_scan(ws + L.off_tmp, tmp, v.cval, cbase, 0ull, L.nkeys + 1,
                              rocprim::plus<unsigned long long>(), s) != hipSuccess)
    return SNAP_ERR_LAUNCH;
  hipLaunchKernelGGL(occ_vjp_heads_kernel, vjp_grid(v.R), dim3(256), 0, s, v);
  SNAP_CHECK_LAUNCH();
  // 6. chunk pass (grid-stride over the chunks: their count is known on the device only), 7. combine
  const bool vec = (D % 4) == 0 && (reinterpret_cast<uintptr_t>(d_features) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_volume) & 15) == 0;
  const int64_t chunk_blocks = snap_cdiv((int64_t)L.max_chunks, 4);
  const dim3 cgrid((unsigned)(chunk_blocks < 8192 ? chunk_blocks : 8192));
  if (vec && D / 4 <= 32) hipLaunchKernelGGL((occ_vjp_chunks_kernel<4, 32>), cgrid, dim3(256), 0, s, v);
  else if (vec) hipLaunchKernelGGL((occ_vjp_chunks_kernel<4, 64>), cgrid, dim3(256), 0, s, v);
  else hipLaunchKernelGGL((occ_vjp_chunks_kernel<1, 64>), cgrid, dim3(256), 0, s, v);
  SNAP_CHECK_LAUNCH();
  if (vec) hipLaunchKernelGGL(occ_vjp_combine_kernel<4>, vjp_grid(v.nkeys * (D / 4)), dim3(256), 0, s, v);
  else hipLaunchKernelGGL(occ_vjp_combine_kernel<1>, vjp_grid(v.nkeys * D), dim3(256), 0, s, v);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
