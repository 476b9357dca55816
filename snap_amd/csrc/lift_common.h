// Device and host pieces shared by the camera-ray lift's forward kernels (lift.hip), its backward
// kernels (bev_bwd.hip) and the consumer of the forward's tap records (mlp_pool.hip, GATHER).  The
// backward recomputes the forward's geometry and must agree with it on every bit of visibility,
// selection order, tap index, tap weight and depth bin: each of those bodies exists once, here.
// No kernels.  -ffp-contract=off is in force, so one expression gives one set of bits wherever it
// is inlined.
#ifndef SNAP_CSRC_LIFT_COMMON_H_
#define SNAP_CSRC_LIFT_COMMON_H_

#include <type_traits>

#include "common.h"

// ------------------------------- projection ---------------------------------------------------
struct LiftProj {
  float pi, pj;   // (row, col) coordinates in the feature map, corner origin
  float depth;
  float dist;     // distance voxel -> camera centre
  bool vis;
  float vx, vy;   // camera-frame x, y (z = depth): the viewing ray of the observation
};

// One (voxel, view) projection.  cam = wh f c k(3) max_fov pad; Rt = R(9) t(3).
__device__ __forceinline__ LiftProj lift_project(const float* __restrict__ cam,
                                                 const float* __restrict__ Rt, float px, float py,
                                                 float pz, int fisheye) {
  const float eps = 1e-3f;
  // Transform3D.inv: R_inv = R^T, t_inv = -(R^T t); then t_inv + R_inv p.
  float pv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float r0 = Rt[0 * 3 + i], r1 = Rt[1 * 3 + i], r2 = Rt[2 * 3 + i];
    const float tinv = -((r0 * Rt[9] + r1 * Rt[10]) + r2 * Rt[11]);
    pv[i] = tinv + ((r0 * px + r1 * py) + r2 * pz);
  }
  LiftProj o;
  o.vx = pv[0];
  o.vy = pv[1];
  o.depth = pv[2];
  bool valid = pv[2] >= eps;
  const float z = fmaxf(pv[2], eps);
  float x = pv[0] / z, y = pv[1] / z;
  if (fisheye) {
    const float radius2 = x * x + y * y;
    const bool in_center = radius2 < eps * eps;
    const float radius = sqrtf(in_center ? eps * eps : radius2);
    const float theta = atanf(radius);
    const float t2 = theta * theta;
    const float offset = (cam[6] * t2 + cam[7] * (t2 * t2)) + cam[8] * (t2 * t2 * t2);
    float dist = (offset + 1.f) * theta / radius;
    dist = in_center ? 1.f : dist;
    x *= dist;
    y *= dist;
    valid = valid && (in_center || ((radius < cam[10]) && (dist > 0.f)));
  }
  x = x * cam[2] + cam[4];
  y = y * cam[3] + cam[5];
  valid = valid && (x >= 0.f) && (x < cam[0]) && (y >= 0.f) && (y < cam[1]);
  o.pi = y;  // xy -> ij
  o.pj = x;
  o.vis = valid;
  const float dx = px - Rt[9], dy = py - Rt[10], dz = pz - Rt[11];
  o.dist = sqrtf((dx * dx + dy * dy) + dz * dz);
  return o;
}

// ------------------------------- bilinear taps ------------------------------------------------
struct LiftTaps {
  int i0, i1, j0, j1;
  float w00, w01, w10, w11;
  float wi1, wj1;   // the 1-D weights the four products are built from
};

// selective != 0: streetview_encoder.py:93-105 (clip the point, floor, +1);
// selective == 0: grids.interpolate_nd / map_coordinates (clip each tap index).
__device__ __forceinline__ LiftTaps lift_taps(float pi, float pj, int h, int w, int selective) {
  LiftTaps t;
  float ci = pi - 0.5f, cj = pj - 0.5f;
  if (selective) {
    ci = fmaxf(fminf(ci, (float)(h - 1)), 0.f);
    cj = fmaxf(fminf(cj, (float)(w - 1)), 0.f);
  }
  const float fi = floorf(ci), fj = floorf(cj);
  const float wi1 = ci - fi, wj1 = cj - fj;
  const float wi0 = 1.f - wi1, wj0 = 1.f - wj1;
  t.i0 = (int)fminf(fmaxf(fi, 0.f), (float)(h - 1));
  t.i1 = (int)fminf(fmaxf(fi + 1.f, 0.f), (float)(h - 1));
  t.j0 = (int)fminf(fmaxf(fj, 0.f), (float)(w - 1));
  t.j1 = (int)fminf(fmaxf(fj + 1.f, 0.f), (float)(w - 1));
  t.w00 = wi0 * wj0;
  t.w01 = wi0 * wj1;
  t.w10 = wi1 * wj0;
  t.w11 = wi1 * wj1;
  t.wi1 = wi1;
  t.wj1 = wj1;
  return t;
}

// ------------------------------- depth bins ---------------------------------------------------
// The depth score interpolates two neighbouring log-depth bins: bins b0, b1, weight wb1 of b1.
struct LiftBins {
  int b0, b1;
  float wb1;
};

// log(depth_max / depth_min): uniform, taken once per kernel and handed to lift_depth_bins
__device__ __forceinline__ float lift_depth_span(const SnapLiftDesc& d) { return logf(d.depth_max / d.depth_min); }

__device__ __forceinline__ LiftBins lift_depth_bins(float depth, const SnapLiftDesc& d, float log_range) {
  const float dc = fminf(fmaxf(depth, d.depth_min), d.depth_max);
  const float tt = logf(dc / d.depth_min) / log_range;
  const float index = 0.5f + tt * (float)(d.num_bins - 1);
  const float c = index - 0.5f;
  const float fl = floorf(c);
  LiftBins o;
  o.wb1 = c - fl;
  o.b0 = (int)fminf(fmaxf(fl, 0.f), (float)(d.num_bins - 1));
  o.b1 = (int)fminf(fmaxf(fl + 1.f, 0.f), (float)(d.num_bins - 1));
  return o;
}

// ------------------------------- selection ----------------------------------------------------
// Half-wave per voxel, lane v holds view v's projection: sel[r] = the r-th nearest visible view by
// K argmin rounds over the half-wave with xor-shuffles, ties towards the lowest view index
// (== jax.lax.top_k(-dist)); with all views, sel[r] = r.  min_dist = the nearest visible distance.
template <int KMAX>
__device__ __forceinline__ void lift_select_halfwave(float dist, bool vis, int hl, int V, int nsel, bool all_views,
                                                     int (&sel)[KMAX], float& min_dist) {
  float key_d = (hl < V && vis) ? dist : INFINITY;
  int key_i = (hl < V) ? hl : 1000 + hl;
  min_dist = INFINITY;
#pragma unroll
  for (int r = 0; r < KMAX; ++r) {
    if (r >= nsel) { sel[r] = 0; continue; }
    if (all_views) {
      sel[r] = r;
      continue;
    }
    float bd = key_d;
    int bi = key_i;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float od = __shfl_xor(bd, o, 32);
      const int oi = __shfl_xor(bi, o, 32);
      if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if (r == 0) min_dist = bd;
    sel[r] = bi;            // bi < V always while r < nsel <= V
    if (hl == bi) { key_d = INFINITY; key_i = 1000 + hl; }
  }
  if (all_views) {
    float md = key_d;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) md = fminf(md, __shfl_xor(md, o, 32));
    min_dist = md;
  }
}

// ------------------------------- tap records --------------------------------------------------
// A (voxel, slot) record, four dwords: word 0 (the caller's: the forward stores the byte offset of
// tap (i0, j0) in f_images, the backward its pixel id, which is also the sort key) | packed =
// view | (i1 != i0) << 8 | (j1 != j0) << 9 | bin0 << 10 | bin1 << 18 | wi1 | wj1.  The forward's
// 32-byte tap_recs row (lift.hip -> mlp_pool.hip) opens with the same four dwords.
__device__ __forceinline__ void lift_rec_pack(int* rec, int word0, int view, const LiftTaps& t, const LiftBins& bn) {
  rec[0] = word0;
  rec[1] = view | ((t.i1 != t.i0) << 8) | ((t.j1 != t.j0) << 9) | (bn.b0 << 10) | (bn.b1 << 18);
  rec[2] = __float_as_int(t.wi1);
  rec[3] = __float_as_int(t.wj1);
}
__device__ __forceinline__ uint32_t lift_rec_ei(uint32_t pk) { return (pk >> 8) & 1u; }
__device__ __forceinline__ uint32_t lift_rec_ej(uint32_t pk) { return (pk >> 9) & 1u; }
__device__ __forceinline__ uint32_t lift_rec_bin0(uint32_t pk) { return (pk >> 10) & 0xff; }
__device__ __forceinline__ uint32_t lift_rec_bin1(uint32_t pk) { return (pk >> 18) & 0xff; }

// The four tap weights (the products lift_taps builds, rebuilt from the stored 1-D weights) and the
// four tap byte offsets of a record.  o00 = the byte offset of tap (i0, j0), plus whatever lane
// offset the caller folds in; Cb / Wb = bytes per pixel / per image row.
struct LiftRecTaps {
  float w00, w01, w10, w11;
  uint32_t o00, o01, o10, o11;
};
__device__ __forceinline__ LiftRecTaps lift_rec_decode(uint32_t o00, uint32_t pk, float wi1, float wj1,
                                                       uint32_t Cb, uint32_t Wb) {
  LiftRecTaps q;
  const float wi0 = 1.f - wi1, wj0 = 1.f - wj1;
  q.w00 = wi0 * wj0; q.w01 = wi0 * wj1; q.w10 = wi1 * wj0; q.w11 = wi1 * wj1;
  q.o00 = o00;
  q.o01 = o00 + (lift_rec_ej(pk) ? Cb : 0u);
  q.o10 = o00 + (lift_rec_ei(pk) ? Wb : 0u);
  q.o11 = q.o10 + (q.o01 - o00);
  return q;
}

// ------------------------------- depth score --------------------------------------------------
// The eight depth-score values of an observation (two bins at each of the four taps), loaded by
// 32-bit byte offsets from the base of f_images (c0, c1: byte offsets of the bins in a pixel) or
// through the four tap pointers (c0, c1: channel indices), and their blend.
struct LiftScoreTaps {
  float t00, t01, t10, t11;   // bin 0
  float u00, u01, u10, u11;   // bin 1
};
__device__ __forceinline__ LiftScoreTaps lift_score_load(const char* fb, const LiftRecTaps& q, uint32_t c0,
                                                         uint32_t c1) {
  LiftScoreTaps s;
  s.t00 = *reinterpret_cast<const float*>(fb + (q.o00 + c0));
  s.t01 = *reinterpret_cast<const float*>(fb + (q.o01 + c0));
  s.t10 = *reinterpret_cast<const float*>(fb + (q.o10 + c0));
  s.t11 = *reinterpret_cast<const float*>(fb + (q.o11 + c0));
  s.u00 = *reinterpret_cast<const float*>(fb + (q.o00 + c1));
  s.u01 = *reinterpret_cast<const float*>(fb + (q.o01 + c1));
  s.u10 = *reinterpret_cast<const float*>(fb + (q.o10 + c1));
  s.u11 = *reinterpret_cast<const float*>(fb + (q.o11 + c1));
  return s;
}
__device__ __forceinline__ LiftScoreTaps lift_score_load(const float* r00, const float* r01, const float* r10,
                                                         const float* r11, int c0, int c1) {
  return LiftScoreTaps{r00[c0], r01[c0], r10[c0], r11[c0], r00[c1], r01[c1], r10[c1], r11[c1]};
}
__device__ __forceinline__ float lift_score_blend(float w00, float w01, float w10, float w11,
                                                  const LiftScoreTaps& s, float wb1) {
  const float wb0 = 1.f - wb1;
  const float s0 = ((w00 * s.t00 + w01 * s.t01) + w10 * s.t10) + w11 * s.t11;
  const float s1 = ((w00 * s.u00 + w01 * s.u01) + w10 * s.u10) + w11 * s.u11;
  return wb0 * s0 + wb1 * s1;
}

// ------------------------------- pooling weights ----------------------------------------------
// jax.nn.softmax(scores, where = ok, initial = 0), up to the division its callers place themselves:
// shift = max(0, max valid score); e[r] = exp(score - shift), 0 where !ok[r] (those terms add +0 to
// the denominator); the weight of slot r is e[r] / den.  smax = the largest valid score (-inf: none).
template <int KMAX>
__device__ __forceinline__ void lift_softmax_weights(const float (&score)[KMAX], const bool (&ok)[KMAX],
                                                     float (&e)[KMAX], float& den, float& smax) {
  float m = 0.f;
  smax = -INFINITY;
#pragma unroll
  for (int r = 0; r < KMAX; ++r)
    if (ok[r]) { m = fmaxf(m, score[r]); smax = fmaxf(smax, score[r]); }
  den = 0.f;
#pragma unroll
  for (int r = 0; r < KMAX; ++r) {
    e[r] = ok[r] ? expf(score[r] - m) : 0.f;
    den += e[r];
  }
}

// ------------------------------- host ---------------------------------------------------------
static inline int lift_nsel(const SnapLiftDesc& d) { return d.K == 0 ? d.V : d.K; }

// channels of a pooled row: mean | var? | max, min? | score_max?
static inline int lift_pool_chans(const SnapLiftDesc& d) {
  return d.feature_dim * (1 + (d.use_variance ? 1 : 0) + (d.add_minmax ? 2 : 0)) + (d.weighted ? 1 : 0);
}

// What an entry point asks of its descriptor beyond the checks all of them share.  Callers set the
// fields by name.
struct LiftDescChecks {
  bool image = true;             // h, w are read
  bool unsupported = false;      // the entry point's own refusal, reported with the view / width limits
  bool read_C = false;           // C must be feature_dim + bins and a multiple of 4
  int bins = 0;
  bool read_out_stride = false;  // out_stride must hold chans channels and be a multiple of 4
  int chans = 0;
  bool selection = true;         // K (lift_pool_launch places this check itself)
  bool max8 = true;              // ... and at most 8 selected views, refused here, before any work
};

// The shared checks, in the order every lift entry point makes them (the first failure decides the
// return code).
static int lift_desc_validate(const SnapLiftDesc& d, const LiftDescChecks& what) {
  if (d.B <= 0 || d.V <= 0 || d.N <= 0 || (what.image && (d.h <= 0 || d.w <= 0))) return SNAP_ERR_BAD_SHAPE;
  if (d.V > 32 || d.feature_dim % 4 != 0 || d.feature_dim > 128 || d.feature_dim <= 0 || what.unsupported)
    return SNAP_ERR_UNSUPPORTED;
  if (what.read_C && (d.C != d.feature_dim + what.bins || d.C % 4 != 0)) return SNAP_ERR_BAD_SHAPE;
  if (what.read_out_stride && (d.out_stride < what.chans || d.out_stride % 4 != 0)) return SNAP_ERR_BAD_SHAPE;
  if (what.selection) {
    if (d.K < 0 || (d.K > 0 && d.K >= d.V)) return SNAP_ERR_BAD_SHAPE;  // K > 0 means V > K
    if (what.max8 && lift_nsel(d) > 8) return SNAP_ERR_UNSUPPORTED;
  }
  return SNAP_OK;
}

// launch(std::integral_constant<int, KMAX>) with the smallest KMAX of 1 / 4 / 8 that holds nsel; more than
// 8 selected views launch nothing and are SNAP_ERR_UNSUPPORTED
template <class F>
static inline int lift_nsel_ladder(int nsel, F&& launch) {
  if (nsel <= 1) launch(std::integral_constant<int, 1>{});
  else if (nsel <= 4) launch(std::integral_constant<int, 4>{});
  else if (nsel <= 8) launch(std::integral_constant<int, 8>{});
  else return SNAP_ERR_UNSUPPORTED;
  return SNAP_OK;
}

#endif  // SNAP_CSRC_LIFT_COMMON_H_
