// Device and host pieces shared by the BEV plane kernels: vertical pooling, modality fusion + matching head and
// the confidence head (bev_ops.hip), their VJPs (bev_bwd.hip, below the lift) and the confidence-weighted
// pooling (bev_conf_pool.hip).  Every kernel of the family has one layout -- a 32-lane half-wave owns a BEV cell,
// lane q holds the channel quad 4q..4q+3 as one f32x4 -- and the variants of a kernel (per-cell / persistent,
// forward / the VJP's recompute) are tested against each other bit for bit: the reductions, the head product,
// the normalisation and the gradient routing those comparisons rest on exist once, here.  No kernels.
// -ffp-contract=off is in force, so one expression gives one set of bits wherever it is inlined.
#ifndef SNAP_CSRC_BEV_COMMON_H_
#define SNAP_CSRC_BEV_COMMON_H_

#include "common.h"

constexpr int BEV_MAXQ = 2;  // channel quads per lane: up to D = 256 channels (BEV_MAXQ * 32 lanes * 4)

__device__ __forceinline__ f32x4 bev_quad(float v) { return f32x4{v, v, v, v}; }

// ------------------------------- half-wave butterflies ----------------------------------------
// xor butterflies over the 32 lanes of a cell: the same bits in every lane.
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}
__device__ __forceinline__ float half_max(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 32));
  return v;
}
__device__ __forceinline__ int half_or(int v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v |= __shfl_xor(v, o, 32);
  return v;
}

// ------------------------------- scalar pieces ------------------------------------------------
// A lane's four terms of a dot product over the channels, associated left to right.
__device__ __forceinline__ float bev_dot4(f32x4 x, f32x4 w) {
  return ((x[0] * w[0] + x[1] * w[1]) + x[2] * w[2]) + x[3] * w[3];
}
// jax.nn.log_sigmoid = -softplus(-x) = min(x, 0) - log1p(exp(-|x|))  (stable)
__device__ __forceinline__ float bev_log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

// ------------------------------- masked reduce ------------------------------------------------
// max / sum / mean over the valid planes or levels of a cell: init, one step per valid entry, finish.
// NAN_WINS is deliberate, not an oversight: the forward kernels step with snap_max_nan (the NaN of an
// observed voxel reaches the plane, as jnp.max gives it); the two fuse VJP kernels recompute the fused vector
// with fmaxf (a NaN is skipped: it then equals no plane's value and receives no gradient).
__device__ __forceinline__ float bev_reduce_init(int pooling) { return pooling == SNAP_POOL_MAX ? -INFINITY : 0.f; }

template <bool NAN_WINS>
__device__ __forceinline__ float bev_reduce_step(float acc, float v, int pooling) {
  if (NAN_WINS) return pooling == SNAP_POOL_MAX ? snap_max_nan(acc, v) : acc + v;
  return pooling == SNAP_POOL_MAX ? fmaxf(acc, v) : acc + v;
}
template <bool NAN_WINS>
__device__ __forceinline__ f32x4 bev_reduce_step(f32x4 acc, f32x4 v, int pooling) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = bev_reduce_step<NAN_WINS>(acc[e], v[e], pooling);
  return acc;
}

// zero for a cell nothing covers (count == 0), the sum divided by the count for mean
__device__ __forceinline__ f32x4 bev_reduce_finish(f32x4 acc, int pooling, int count) {
  const bool any = count > 0;
  if (!any) acc = bev_quad(0.f);
  if (any && pooling == SNAP_POOL_MEAN) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = acc[e] / (float)count;
  }
  return acc;
}

// ------------------------------- wave-per-column level walk -----------------------------------
// Z <= 64: the validity bytes of column m as a wave-uniform 64-bit mask (one ballot), so the walk over the
// valid levels has no data-dependent branches.
__device__ __forceinline__ unsigned long long bev_level_mask(const uint8_t* __restrict__ vvalid, int64_t m, int Z,
                                                             int lane) {
  return __ballot(lane < Z && vvalid[m * Z + lane] != 0);
}
// One trip: the next four valid levels leave the mask, z[0], z[2] -> half 0 and z[1], z[3] -> half 1 (the two
// half-waves take alternate valid levels, two row loads in flight each); -1 when the mask ran out.
__device__ __forceinline__ void bev_next_levels(unsigned long long& mask, int half, int& za, int& zb) {
  int z[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    z[k] = mask ? (int)__builtin_ctzll(mask) : -1;
    mask &= mask - 1;                    // (0 stays 0)
  }
  za = half ? z[1] : z[0];
  zb = half ? z[3] : z[2];
}

// ------------------------------- max VJP: ties share the gradient -----------------------------
// Pass 1 over the valid levels of channel quad q of a column (base = the column's address): the column maximum
// by `>` then `==` in ascending order (a NaN never wins) and the number of levels that hold it.
struct BevColumnMax {
  f32x4 best, cnt;   // per channel: the maximum, the number of valid levels that hold it
  int nvalid;        // valid levels of the column
};
__device__ __forceinline__ BevColumnMax bev_column_max_ties(const float* __restrict__ base,
                                                            const uint8_t* __restrict__ vv, int Z, int D, int q) {
  f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  f32x4 cnt = {0.f, 0.f, 0.f, 0.f};
  int nvalid = 0;
  for (int z = 0; z < Z; ++z) {
    if (!vv[z]) continue;
    ++nvalid;
    const f32x4 v = *reinterpret_cast<const f32x4*>(base + (int64_t)z * D + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (v[e] > best[e]) { best[e] = v[e]; cnt[e] = 1.f; }
      else if (v[e] == best[e]) cnt[e] += 1.f;
    }
  }
  return BevColumnMax{best, cnt, nvalid};
}
// Pass 2, one entry: g / cnt to every holder of the maximum (as jnp.max's VJP does), zero to the others.
__device__ __forceinline__ f32x4 bev_share_among_holders(f32x4 v, f32x4 best, f32x4 g, f32x4 cnt) {
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (v[e] == best[e]) ? g[e] / cnt[e] : 0.f;
  return o;
}

// ------------------------------- matching head ------------------------------------------------
// y_j = bm_j + sum_c x_c Wm[c, j] in ascending channel order, lane j computing output channel j (Dm <= 32).
// Shuffle form (any D): the cell's vector stays in its lanes' registers and every term costs a lane exchange
// and a load of Wm.
__device__ __forceinline__ float bev_head_shfl(const f32x4 (&x)[BEV_MAXQ], int nq, const float* __restrict__ Wm,
                                               const float* __restrict__ bm, int Dm, int j) {
  float y = (j < Dm) ? bm[j] : 0.f;
#pragma unroll
  for (int i = 0; i < BEV_MAXQ; ++i) {
    for (int q = 0; q < 32; ++q) {
      const int cq = q + 32 * i;
      if (cq >= nq) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xv = __shfl(x[i][e], q, 32);
        if (j < Dm) y += xv * Wm[(int64_t)(4 * cq + e) * Dm + j];
      }
    }
  }
  return y;
}

// What one half-wave wrote to its LDS row becomes readable by its other lanes (a wave-level publish: the row
// belongs to the wave, no workgroup barrier).
__device__ __forceinline__ void bev_wave_publish() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Register-column form (D = 128, persistent kernels): lane j keeps column j of Wm in registers for all the cells
// its half-wave visits ...
__device__ __forceinline__ void bev_head_load_column(float (&wreg)[128], const float* __restrict__ Wm, int Dm, int j) {
#pragma unroll
  for (int k = 0; k < 128; ++k) wreg[k] = j < Dm ? Wm[(int64_t)k * Dm + j] : 0.f;
}
// ... and the cell's vector comes back from the half-wave's LDS row as 32 broadcast 16-byte reads.  The caller
// puts a wave_barrier between this and the next write of the row.
__device__ __forceinline__ float bev_head_column(float* __restrict__ row, int hl, f32x4 x, const float (&wreg)[128],
                                                 float bj) {
  *reinterpret_cast<f32x4*>(row + 4 * hl) = x;
  bev_wave_publish();
  float y = bj;
#pragma unroll
  for (int q = 0; q < 32; ++q) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(row + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) y += xv[e] * wreg[4 * q + e];
  }
  return y;
}

// ------------------------------- L2 normalisation over the Dm head channels -------------------
// layers.normalize: y_safe = where(invalid, eps, y); z = y / ||y_safe||, zero where invalid (the invalid
// branch's denominator sqrt(Dm) * eps is ||y_safe||; it is computed and unused, as the reference has it).
__device__ __forceinline__ float bev_l2_normalize(float y, int j, int Dm, float eps) {
  const float nrm = sqrtf(half_sum((j < Dm) ? y * y : 0.f));
  const bool invalid = nrm < eps;
  const float denom = invalid ? sqrtf((float)Dm) * eps : nrm;
  return invalid ? 0.f : y / denom;
}
// Its VJP: dy = (dz - z <z, dz>) / ||y||, zero below eps (nrm is half-wave uniform, so is the branch).
__device__ __forceinline__ float bev_l2_normalize_vjp(float y, float dz, int j, int Dm, float eps) {
  float dy = 0.f;
  const float nrm = sqrtf(half_sum((j < Dm) ? y * y : 0.f));
  if (nrm >= eps) {
    const float z = y / nrm;
    const float zdz = half_sum((j < Dm) ? z * dz : 0.f);
    dy = (dz - z * zdz) / nrm;
  }
  return dy;
}

// ------------------------------- d fused -> d planes ------------------------------------------
// One channel quad of one cell: x[p] the planes' values (pv[p]: plane p covers the cell), fused their reduce,
// df the gradient of it.  max: shared equally among the planes that hold the maximum; sum: to every covering
// plane; mean: divided by their count.  A plane that does not cover the cell gets zero; a plane without a
// gradient buffer is skipped.  off = the quad's offset in a plane.
__device__ __forceinline__ void bev_route_to_planes(const f32x4 (&x)[4], const bool (&pv)[4], f32x4 fused, f32x4 df,
                                                    int pooling, int count, int num_planes,
                                                    float* const (&dplanes)[4], int64_t off) {
  f32x4 ties = bev_quad(0.f);
  if (pooling == SNAP_POOL_MAX) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (pv[p]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ties[e] += (x[p][e] == fused[e]) ? 1.f : 0.f;
      }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (p >= num_planes || !dplanes[p]) continue;
    f32x4 o = bev_quad(0.f);
    if (pv[p]) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (pooling == SNAP_POOL_MAX) o[e] = (x[p][e] == fused[e]) ? df[e] / ties[e] : 0.f;
        else if (pooling == SNAP_POOL_SUM) o[e] = df[e];
        else o[e] = df[e] / (float)count;
      }
    }
    *reinterpret_cast<f32x4*>(dplanes[p] + off) = o;
  }
}

// ------------------------------- host side ----------------------------------------------------
// What the fuse + matching-head launch and its VJP both take.
struct BevFuseHead {
  const float* planes[4];
  const uint8_t* valids[4];
  int num_planes;
  int64_t M;
  int D, pooling;
  const float* Wm;
  const float* bm;
  int Dm, normalize;
  float eps;
};

// The checks of snap_plane_fuse_match_f32 and snap_plane_fuse_match_bwd_f32, in their order, and the fill.
// head: the call has a matching head (an output or a gradient of it was given); head_ok: every pointer the
// head needs was given too.
static inline int bev_fuse_head_fill(BevFuseHead& h, const float* const* planes, const uint8_t* const* valids,
                                     int32_t num_planes, int64_t M, int32_t D, int32_t pooling, const float* Wm,
                                     const float* bm, int32_t Dm, int32_t normalize, float eps, bool head,
                                     bool head_ok) {
  if (!planes) return SNAP_ERR_NULL;
  if (num_planes < 1 || num_planes > 4) return SNAP_ERR_UNSUPPORTED;
  if (M <= 0 || D <= 0 || D % 4 != 0 || D > BEV_MAXQ * 128) return SNAP_ERR_BAD_SHAPE;
  if (pooling < SNAP_POOL_MAX || pooling > SNAP_POOL_MEAN) return SNAP_ERR_UNSUPPORTED;
  if (head && !head_ok) return SNAP_ERR_NULL;
  if (head && (Dm < 1 || Dm > 32)) return SNAP_ERR_UNSUPPORTED;
  for (int i = 0; i < 4; ++i) {
    h.planes[i] = i < num_planes ? planes[i] : nullptr;
    h.valids[i] = (i < num_planes && valids) ? valids[i] : nullptr;
    if (i < num_planes && !h.planes[i]) return SNAP_ERR_NULL;
  }
  h.num_planes = num_planes;
  h.M = M; h.D = D; h.pooling = pooling;
  h.Wm = Wm; h.bm = bm; h.Dm = Dm; h.normalize = normalize; h.eps = eps;
  return SNAP_OK;
}

// The persistent register-column kernels take the launch from here (forward and VJP alike).
static inline bool bev_fuse_persistent(const BevFuseHead& h, bool head) { return head && h.D == 128 && h.M >= 8192; }

#endif  // SNAP_CSRC_BEV_COMMON_H_
