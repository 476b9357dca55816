// Device and host pieces shared by the operators on the exhaustive vote volume (vote_peaks.hip, vote_posterior.hip,
// vote_fuse.hip, vote_filter.hip, vote_smooth.hip, vote_pairs.hip, vote_viterbi.hip, vote_sample.hip, vote_refine.hip,
// vote_credible.hip, vote_modes.hip, vote_recall.hip, vote_odometry.hip, vote_rebase.hip, vote_temper.hip, vote_prior.hip, vote_raster.hip).  The family's
// contract is
// "no floating-point atomics; every floating-point sum's order is a function of the shape alone; two calls give the
// same bits"
// (vote_credible.hip alone uses atomics, INTEGER ones: uint64 adds of fixed-point mass and int minima / maxima /
// counts, exact in any order), and vote_filter is tested against vote_fuse and vote_posterior bit for bit: the
// predicates, reductions, tile walk and circular indices those comparisons rest on exist once, here.  So do the two
// pieces vote_credible.hip and vote_recall.hip share: the scan for the largest finite vote and the counts
// (vote_scan_max) and the rounding of a ground-truth index to its cell (vote_gt_cell).  No kernels in this file
// (vote_predict.h and vote_ratio.h, built on it, hold the kernels several operators launch).  -ffp-contract=off is in
// force, so one expression gives one set of bits wherever it is inlined.
#ifndef SNAP_CSRC_VOTE_COMMON_H_
#define SNAP_CSRC_VOTE_COMMON_H_

#include "common.h"

__device__ __forceinline__ bool vote_finite(float v) { return fabsf(v) < INFINITY; }   // false for NaN and +-inf

// ------------------------------- wave butterflies ---------------------------------------------
// xor butterflies: the same bits in every lane.  (Not common.h's DPP wave_sum: another order, another instruction mix.)
__device__ __forceinline__ double vote_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int vote_wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ------------------------------- workgroup reductions -----------------------------------------
// The waves' partials combined in the order that is part of a float64 result: the four waves of a 256-thread
// workgroup pairwise, (w0 + w1) + (w2 + w3); the 16 of a 1024-thread workgroup in sequence from 0.
template <int WAVES, typename T>
__device__ __forceinline__ T vote_waves_sum(const T* sh) {
  if constexpr (WAVES == 4) {
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
  } else {
    T s = 0;
    for (int w = 0; w < WAVES; ++w) s += sh[w];
    return s;
  }
}

// A wave tree (lane 0's value is used), then the waves: the same bits in every thread.  `sh` [WAVES] is free again on
// return.
template <int WAVES, typename T>
__device__ __forceinline__ T vote_block_sum(T v, T* sh) {
  v = vote_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const T s = vote_waves_sum<WAVES>(sh);
  __syncthreads();
  return s;
}
template <int WAVES>
__device__ __forceinline__ float vote_block_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  static_assert(WAVES == 4, "the 1024-thread kernels use their staging arrays once and keep their own fold");
  const float m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  return m;
}
// Two counts at once behind ONE barrier: thread 0 returns the workgroup's sum of c0, thread 1 that of c1 (the other
// threads 0).  `sh` is not free again before the caller's next barrier.
template <int WAVES>
__device__ __forceinline__ int vote_block_count_pair(int c0, int c1, int (*sh)[2]) {
  c0 = vote_wave_sum(c0);
  c1 = vote_wave_sum(c1);
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = c0;
    sh[threadIdx.x >> 6][1] = c1;
  }
  __syncthreads();
  int s = 0;
  if (threadIdx.x < 2)
    for (int w = 0; w < WAVES; ++w) s += sh[w][threadIdx.x];
  return s;
}

// The fold of column `col` of [groups][STRIDE] per-workgroup partials by a whole workgroup: a strided chain per
// thread, then the workgroup reduction.
template <int WAVES, int STRIDE, typename T>
__device__ __forceinline__ T vote_fold_sum(const T* __restrict__ part, int col, int groups, T* sh) {
  T v = 0;
  for (int g = threadIdx.x; g < groups; g += WAVES * SNAP_WAVE) v += part[(size_t)g * STRIDE + col];
  return vote_block_sum<WAVES>(v, sh);
}
template <int WAVES, int STRIDE>
__device__ __forceinline__ float vote_fold_max(const float* __restrict__ part, int col, int groups, float* sh) {
  float v = -INFINITY;
  for (int g = threadIdx.x; g < groups; g += WAVES * SNAP_WAVE) v = fmaxf(v, part[(size_t)g * STRIDE + col]);
  return vote_block_max<WAVES>(v, sh);
}

// ------------------------------- (maximum, lowest index) pairs --------------------------------
// (m, i) = (the largest value of a set, the lowest index at which it is attained); the empty set is
// (-inf, VOTE_NO_INDEX).  No value is NaN.  "Larger value, then lower index" is a total order, so the merge is
// associative and commutative: every fold order gives the same pair.
constexpr int VOTE_NO_INDEX = 0x7fffffff;
__device__ __forceinline__ void vote_argmax_merge(float* m, int* i, float m2, int i2) {
  if (m2 > *m || (m2 == *m && i2 < *i)) {
    *m = m2;
    *i = i2;
  }
}
// A wave butterfly, then the waves: the same pair in every thread.  `shm` / `shi` [WAVES] are free again on return.
template <int WAVES>
__device__ __forceinline__ void vote_block_argmax(float* m, int* i, float* shm, int* shi) {
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(*m, o);
    const int i2 = __shfl_xor(*i, o);
    vote_argmax_merge(m, i, m2, i2);
  }
  if ((threadIdx.x & 63) == 0) {
    shm[threadIdx.x >> 6] = *m;
    shi[threadIdx.x >> 6] = *i;
  }
  __syncthreads();
  float mm = shm[0];
  int ii = shi[0];
  for (int w = 1; w < WAVES; ++w) vote_argmax_merge(&mm, &ii, shm[w], shi[w]);
  __syncthreads();
  *m = mm;
  *i = ii;
}
// The fold of the pairs in column fcol of [groups][FSTRIDE] float and column icol of [groups][ISTRIDE] int32 partials.
template <int WAVES, int FSTRIDE, int ISTRIDE>
__device__ __forceinline__ void vote_fold_argmax(const float* __restrict__ fpart, int fcol,
                                                 const int32_t* __restrict__ ipart, int icol, int groups, float* m,
                                                 int* i, float* shm, int* shi) {
  *m = -INFINITY;
  *i = VOTE_NO_INDEX;
  for (int g = threadIdx.x; g < groups; g += WAVES * SNAP_WAVE)
    vote_argmax_merge(m, i, fpart[(size_t)g * FSTRIDE + fcol], ipart[(size_t)g * ISTRIDE + icol]);
  vote_block_argmax<WAVES>(m, i, shm, shi);
}

// ------------------------------- log-sum-exp pairs --------------------------------------------
// (m, s) = (maximum, sum of exp(u - m)) of a set of finite u; the empty set is (-inf, 0).  Merge another set in.
__device__ __forceinline__ void vote_lse_merge(double* m, double* s, double m2, double s2) {
  if (m2 == -(double)INFINITY) return;
  if (*m == -(double)INFINITY) {
    *m = m2;
    *s = s2;
  } else if (m2 > *m) {
    *s = *s * exp(*m - m2) + s2;
    *m = m2;
  } else {
    *s += s2 * exp(m2 - *m);
  }
}
// One more finite u into a thread's running pair.
__device__ __forceinline__ void vote_lse_add(double* m, double* s, double u) {
  if (u > *m) {
    *s = *s * exp(*m - u) + 1.0;            // (m = -inf at the first cell: exp gives 0)
    *m = u;
  } else {
    *s += exp(u - *m);
  }
}
template <int WAVES>
__device__ __forceinline__ void vote_block_lse(double* m, double* s, double (*sh)[2]) {
  for (int o = 32; o > 0; o >>= 1) {        // (lane 0 ends with the tree over all 64 lanes; only it is used)
    const double m2 = __shfl_xor(*m, o), s2 = __shfl_xor(*s, o);
    vote_lse_merge(m, s, m2, s2);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = *m;
    sh[threadIdx.x >> 6][1] = *s;
  }
  __syncthreads();
  double mm = sh[0][0], ss = sh[0][1];
  for (int w = 1; w < WAVES; ++w) vote_lse_merge(&mm, &ss, sh[w][0], sh[w][1]);
  __syncthreads();
  *m = mm;
  *s = ss;
}
// The fold of the pairs in columns (col_m, col_s) of [groups][STRIDE] partials -> log sum exp (-inf for the empty set).
template <int WAVES, int STRIDE>
__device__ __forceinline__ double vote_fold_lse(const double* __restrict__ part, int col_m, int col_s, int groups,
                                                double (*sh)[2]) {
  double m = -(double)INFINITY, s = 0.0;
  for (int g = threadIdx.x; g < groups; g += WAVES * SNAP_WAVE)
    vote_lse_merge(&m, &s, part[(size_t)g * STRIDE + col_m], part[(size_t)g * STRIDE + col_s]);
  vote_block_lse<WAVES>(&m, &s, sh);
  return m == -(double)INFINITY ? m : m + log(s);
}
// A float64 log-value against the log-sum-exp of its set, as the f32 that is stored: NaN -> NaN, -inf -> -inf, else
// fl32(w - log_norm).
__device__ __forceinline__ float vote_normalised(double w, double log_norm) {
  if (w != w) return __int_as_float(0x7fc00000);
  if (w == -(double)INFINITY) return -INFINITY;
  return (float)(w - log_norm);
}

// ------------------------------- the tile walk ------------------------------------------------
// A tile is one rotation and NT consecutive pixels p = a * Wo + b of its plane, one per thread; workgroups stride over
// the tiles.  This thread's pixel of tile `tile_in_plane`: false (and p = 0) past the plane's end, in the ragged last
// tile.
template <int NT>
__device__ __forceinline__ bool vote_tile_pixel(int tile_in_plane, int P, int* p) {
  const int64_t p64 = (int64_t)tile_in_plane * NT + threadIdx.x;
  const bool in = p64 < P;
  *p = in ? (int)p64 : 0;
  return in;
}
template <int NT>
__device__ __forceinline__ bool vote_tile_cell(int tile, int tiles_per_plane, int P, int* r, int* p) {
  *r = tile / tiles_per_plane;
  return vote_tile_pixel<NT>(tile - *r * tiles_per_plane, P, p);
}
__device__ __forceinline__ void vote_row_col(int p, int Wo, int* a, int* b) {
  *a = p / Wo;
  *b = p - *a * Wo;
}

// ------------------------------- circular rotation index --------------------------------------
__device__ __forceinline__ int vote_wrap(int r, int R) { return r < 0 ? r + R : (r >= R ? r - R : r); }   // -R <= r < 2 R
__device__ __forceinline__ int vote_next(int k, int R) { return k + 1 == R ? 0 : k + 1; }
__device__ __forceinline__ int vote_mod(int v, int R) {   // v mod R in [0, R), mathematically, for any v
  const int k = (int)((int64_t)v % R);
  return k < 0 ? k + R : k;
}

// ------------------------------- the contributing-cell scan -----------------------------------
// This thread's share of the tile walk over a volume: the largest finite vote (-inf when none), the count of finite
// votes and the count of NaN / +inf ones (-inf is a masked cell: neither).  The caller reduces the three over its
// workgroup (vote_block_max, vote_block_count_pair).
template <int NT>
__device__ __forceinline__ void vote_scan_max(const float* __restrict__ votes, int P, int tpp, int tiles, float* m,
                                              int* n_ok, int* n_bad) {
  float vmax = -INFINITY;                   // (locals, handed out once: accumulators behind the pointers end in scratch)
  int ok = 0, bad = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p;
    if (vote_tile_cell<NT>(tile, tpp, P, &r, &p)) {
      const float v = votes[(size_t)r * P + p];
      if (vote_finite(v)) {
        vmax = fmaxf(vmax, v);
        ++ok;
      } else if (!(v == -INFINITY)) {
        ++bad;                              // NaN or +inf
      }
    }
  }
  *m = vmax;
  *n_ok = ok;
  *n_bad = bad;
}

// ------------------------------- the ground-truth cell ----------------------------------------
// The cell nearest to a ground-truth index gt = (k, i, j) (f32 [3] on the device, or NULL): rintf on k (half to even)
// and the mathematical modulo in the rotation, rint in double on i and j.  False when gt is NULL, not finite,
// |k| > 2^20 or (i, j) outside [0, Ho - 1] x [0, Wo - 1]; (r, a, b) are written only with true.
__device__ __forceinline__ bool vote_gt_cell(const float* __restrict__ gt, int R, int Ho, int Wo, int* r, int* a,
                                             int* b) {
  if (gt == nullptr) return false;
  const float k = gt[0], i = gt[1], j = gt[2];
  if (!(vote_finite(k) && vote_finite(i) && vote_finite(j))) return false;
  if (!(fabsf(k) <= 1048576.f && (double)i >= 0.0 && (double)i <= (double)(Ho - 1) && (double)j >= 0.0 &&
        (double)j <= (double)(Wo - 1)))
    return false;
  *r = vote_mod((int)rintf(k), R);
  *a = (int)rint((double)i);                // in range: no overflow
  *b = (int)rint((double)j);
  return true;
}

// ------------------------------- host: the launch plan ----------------------------------------
struct VotePlan {
  int P, tiles_per_plane, tiles, groups;
};

// Every flat index of the volume(s) is an int: false at 2^31 cells and beyond.
inline bool vote_cells_fit(int64_t cells) { return cells < ((int64_t)1 << 31); }

// `planes` planes of Ho x Wo cut into tiles of `nt` pixels, at most `max_groups` workgroups striding over them.
inline bool vote_plan(int64_t cells, int planes, int Ho, int Wo, int nt, int max_groups, VotePlan* plan) {
  if (!vote_cells_fit(cells)) return false;
  plan->P = Ho * Wo;
  plan->tiles_per_plane = (int)snap_cdiv(plan->P, nt);
  plan->tiles = planes * plan->tiles_per_plane;   // < 2^31 / nt + planes
  plan->groups = plan->tiles < max_groups ? plan->tiles : max_groups;
  return true;
}

// ------------------------------- host: the workspace layout -----------------------------------
// A running offset over the sections of a workspace, each rounded up to whole 8-byte words.  An operator describes its
// layout ONCE, as a function of its plan that take()s the sections in order (inside one braced list: evaluated left
// to right): with base == nullptr it yields the size (`bytes`, and null sections), with the caller's workspace the
// pointers.
struct VoteLayout {
  void* base;
  size_t bytes = 0;
  template <typename T>
  T* take(size_t count) {
    T* section = base != nullptr ? reinterpret_cast<T*>(static_cast<unsigned char*>(base) + bytes) : nullptr;
    bytes += (count * sizeof(T) + 7) / 8 * 8;
    return section;
  }
};

inline bool vote_workspace_ok(const void* workspace, size_t workspace_bytes, size_t need) {
  return workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 8 == 0;
}

#endif  // SNAP_CSRC_VOTE_COMMON_H_
