// Highest-density credible regions of a vote volume: snap_vote_credible_f32 (include/snap_hip.h).
//
// votes [R, Ho, Wo] f32 are unnormalised log-scores; over the FINITE cells F (vote_posterior's rule) a cell weighs
// w = exp(scale (v - vmax)) in float64.  For L levels q_l the op finds the thresholds tau_l (the largest vote value t
// with mass{v >= t} >= q_l Z), and for the nested regions {v >= tau_l}: their masses, cell / pixel / rotation counts,
// bounding boxes, one u8 level map per pixel, per rotation and (optionally) per cell, and the tail masses above a
// ground-truth cell.
//
// SELECTION: a most-significant-digit radix select over the monotone 32-bit key of the vote (-0 = +0), 8 bits a pass,
// for all L levels at once.  A pass bins the FIXED-POINT weight wfix = rint(w 2^Q) (uint64, Q = 62 - bit length of
// R Ho Wo, so no sum overflows) of every cell whose key starts with one of the levels' prefixes into that prefix's 256
// bins; levels that share a prefix share the bins, so a cell is binned once however many levels there are.  Integer
// sums are exact and order-free: the LDS atomics (ds_add_u64, a wave that agrees on the bin adds its sum once) give the
// same bits in any order, and the same cell has the same wfix in every pass, so a digit's bins sum exactly to their
// parent's bin.  Selection is therefore EXACT for the quantised weights; against the float64 weights it is decided
// whenever q_l is further than eps = R Ho Wo 2^-Q / Z from the normalised mass at a vote value.
//
// SIX passes over the volume for every L:
//   launch 1   vote_credible_max_kernel     vmax, the counts                              (1 pass)
//   launch 2-9 vote_credible_hist_kernel    bins of digit d = 0 .. 3: in LDS per workgroup, the non-empty ones then
//                                           added to the pass's global bins (zeroed by launch 1)  (4 passes)
//              vote_credible_select_kernel  L workgroups of 256: one bin per thread, pick the level's digit
//   launch 10  vote_credible_levels_kernel  the level maps, and per workgroup: float64 masses per level and around the
//                                           ground-truth value, counts, boxes, rotation levels (1 pass)
//   launch 11  vote_credible_finish_kernel  one workgroup folds the partial rows and writes the small outputs
// The masses that are RETURNED are float64 sums of the float64 weights in a fixed order (vote_common.h's reductions),
// not the fixed-point ones.  No floating-point atomics; integer atomics only (uint64 adds on the fixed-point bins, in
// LDS and from there into the global bins; LDS minima, maxima and counts of the level pass): order-free, exact.
// Measured split at [36, 511, 511], L = 3 (kernel trace): max 22 us, bins 4 x ~35, levels 50; with per-workgroup bin
// rows folded by the select launches (4 x 42 us) and a finish that reduced column after column from memory (163 us)
// the folds were 60 % of the call: hence the global bins and a finish that holds a row per thread.
#include "vote_common.h"

namespace {

constexpr int CR_NT = 256;                  // threads of the volume launches = pixels of a tile = bins of a digit
constexpr int CR_WAVES = CR_NT / SNAP_WAVE;
constexpr int CR_MAX_R = 64;
constexpr int CR_MAX_L = 8;
constexpr int CR_MAX_GROUPS = 1024;
constexpr int CR_BINS = 256;
constexpr int CR_DIGITS = 4;
constexpr int CR_NS = 1024;                 // select / finish threads
constexpr int CR_NS_WAVES = CR_NS / SNAP_WAVE;
constexpr int CR_DCOLS = 12;                // float64 partial row: mass of level 0 .. 8 (exclusive) | above gt | at gt | 0
constexpr int CR_I_PIX = 8, CR_I_BOX = 16, CR_I_LR = 48;
constexpr int CR_ICOLS = CR_I_LR + CR_MAX_R;   // int partial row: cells[8] | pixels[8] | box[8][4] | level_r[64]
constexpr int CR_NO_MIN = 0x7fffffff;
static_assert(CR_BINS == CR_NT, "one thread per bin");

typedef unsigned long long u64;

struct CrLevels {
  float q[CR_MAX_L];
};

// The monotone key: a < b (f32, -0 = +0) iff key(a) < key(b), for all non-NaN a, b.
__device__ __forceinline__ uint32_t cr_key(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;               // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cr_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ double cr_weight(float v, float vmax, double scale) {
  return exp(scale * ((double)v - (double)vmax));
}
__device__ __forceinline__ u64 cr_wave_sum(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The ground-truth cell's vote (vote_gt_cell), NaN when the index is invalid (or the pointer NULL) or the vote is not
// finite.
__device__ __forceinline__ float cr_gt_vote(const float* __restrict__ votes, const float* __restrict__ gt, int R, int Ho,
                                            int Wo) {
  const float nan = __int_as_float(0x7fc00000);
  int r, a, b;
  if (!vote_gt_cell(gt, R, Ho, Wo, &r, &a, &b)) return nan;
  const float v = votes[((size_t)r * Ho + (size_t)a) * Wo + (size_t)b];
  return vote_finite(v) ? v : nan;
}

// ---- launch 1: the largest contributing vote and the counts, per workgroup
__global__ __launch_bounds__(CR_NT) void vote_credible_max_kernel(const float* __restrict__ votes, int P, int tpp,
                                                                  int tiles, float* __restrict__ fpart,
                                                                  int32_t* __restrict__ cpart,
                                                                  u64* __restrict__ gbins) {
  __shared__ float shm[CR_WAVES];
  __shared__ int shc[CR_WAVES][2];
  for (int i = blockIdx.x * CR_NT + threadIdx.x; i < CR_DIGITS * CR_MAX_L * CR_BINS; i += gridDim.x * CR_NT)
    gbins[i] = 0;                           // the digit passes add into them
  float m;
  int n_ok, n_bad;
  vote_scan_max<CR_NT>(votes, P, tpp, tiles, &m, &n_ok, &n_bad);
  m = vote_block_max<CR_WAVES>(m, shm);
  const int c = vote_block_count_pair<CR_WAVES>(n_ok, n_bad, shc);
  if (threadIdx.x == 0) fpart[blockIdx.x] = m;
  if (threadIdx.x < 2) cpart[(size_t)blockIdx.x * 2 + threadIdx.x] = c;
}

// ---- digit pass `pass`: this workgroup's bins in LDS, one row of 256 per DISTINCT prefix, then added to the pass's
// global row of the first level that has the prefix (integer atomics: the sum is exact whatever the order);
// prefix == nullptr in pass 0 (every level's prefix is empty)
__global__ __launch_bounds__(CR_NT) void vote_credible_hist_kernel(const float* __restrict__ votes, int P, int tpp,
                                                                   int tiles, int groups, float scale, double two_q,
                                                                   int L, int pass, const float* __restrict__ fpart,
                                                                   const uint32_t* __restrict__ prefix,
                                                                   u64* __restrict__ gbins) {
  __shared__ u64 hist[CR_MAX_L * CR_BINS];
  __shared__ float shm[CR_WAVES];
  __shared__ uint32_t s_prefix[CR_MAX_L];
  __shared__ int s_owner[CR_MAX_L];
  __shared__ int s_rows;
  const int t = threadIdx.x, lane = t & 63;
  const float vmax = vote_fold_max<CR_WAVES, 1>(fpart, 0, groups, shm);
  if (t == 0) {
    int n = 0;
    for (int l = 0; l < L; ++l) {
      const uint32_t pf = pass == 0 ? 0u : prefix[l];
      bool seen = false;
      for (int k = 0; k < n; ++k) seen = seen || s_prefix[k] == pf;
      if (!seen) {
        s_prefix[n] = pf;
        s_owner[n] = l;
        ++n;
      }
    }
    s_rows = n;
  }
  __syncthreads();
  const int rows = s_rows;
  for (int k = 0; k < rows; ++k) hist[k * CR_BINS + t] = 0;
  __syncthreads();
  const int hi_shift = 32 - 8 * pass, digit_shift = 24 - 8 * pass;
  const double ds = (double)scale;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p;
    const bool in = vote_tile_cell<CR_NT>(tile, tpp, P, &r, &p);
    int code = -1;
    u64 wf = 0;
    if (in) {
      const float v = votes[(size_t)r * P + p];
      if (vote_finite(v)) {
        const uint32_t key = cr_key(v);
        const uint32_t hi = pass == 0 ? 0u : key >> hi_shift;
        int row = -1;
        for (int k = 0; k < rows; ++k)
          if (s_prefix[k] == hi) row = k;
        if (row >= 0) {
          wf = (u64)__double2ll_rn(cr_weight(v, vmax, ds) * two_q);
          if (wf != 0) code = row * CR_BINS + (int)((key >> digit_shift) & 255u);
        }
      }
    }
    const u64 act = __ballot(code >= 0);
    if (act != 0) {                          // (uniform)
      const int lead = __ffsll((long long)act) - 1;
      const int c0 = __shfl(code, lead);
      if (__all(code < 0 || code == c0)) {   // (uniform) the wave agrees on the bin: one add of its integer sum
        const u64 s = cr_wave_sum(code >= 0 ? wf : (u64)0);
        if (lane == lead) atomicAdd(&hist[c0], s);
      } else if (code >= 0) {
        atomicAdd(&hist[code], wf);
      }
    }
  }
  __syncthreads();
  for (int k = 0; k < rows; ++k) {          // (a workgroup fills few bins: most threads add nothing)
    const u64 v = hist[k * CR_BINS + t];
    if (v != 0) atomicAdd(&gbins[((size_t)pass * CR_MAX_L + s_owner[k]) * CR_BINS + t], v);
  }
}

// ---- digit pass `pass`, workgroup l: level l's row of bins, then the next digit of tau_l: the largest b with
// above + sum_{b' >= b} bins >= q_l Z.  Reads state `pass`, writes state `pass + 1`.
__global__ __launch_bounds__(CR_BINS) void vote_credible_select_kernel(CrLevels lv, int L, int pass,
                                                                       const u64* __restrict__ gbins,
                                                                       const uint32_t* __restrict__ prefix_in,
                                                                       const u64* __restrict__ above_in, u64* zfix,
                                                                       uint32_t* __restrict__ prefix_out,
                                                                       u64* __restrict__ above_out) {
  __shared__ u64 hist[CR_BINS];
  __shared__ u64 s_z;
  const int l = blockIdx.x, t = threadIdx.x;
  const uint32_t pf = pass == 0 ? 0u : prefix_in[l];
  int owner = l;
  for (int k = l - 1; k >= 0; --k)
    if ((pass == 0 ? 0u : prefix_in[k]) == pf) owner = k;
  hist[t] = gbins[((size_t)pass * CR_MAX_L + owner) * CR_BINS + t];
  __syncthreads();
  u64 cum = 0;                              // sum_{k >= t} hist[k]: integer, any order (broadcast reads, 16 in flight)
#pragma unroll 16
  for (int k = 0; k < CR_BINS; ++k) cum += k >= t ? hist[k] : (u64)0;
  if (pass == 0 && t == 0) s_z = cum;
  __syncthreads();
  {
    const u64 Z = pass == 0 ? s_z : *zfix;
    const u64 ab = pass == 0 ? (u64)0 : above_in[l];
    const double target = (double)lv.q[l] * (double)Z;
    const u64 next = cum - hist[t];
    const bool here = (double)(ab + cum) >= target || t == 0;
    const bool beyond = t < CR_BINS - 1 && (double)(ab + next) >= target;
    if (here && !beyond) {                  // exactly one thread
      prefix_out[l] = (pf << 8) | (uint32_t)t;
      above_out[l] = ab + next;
      if (pass == 0 && l == 0) *zfix = Z;
    }
  }
}

// ---- launch 10: levels.  Tiles of 256 pixels of ONE plane; a thread walks its pixel's R cells.
__global__ __launch_bounds__(CR_NT) void vote_credible_levels_kernel(
    const float* __restrict__ votes, int R, int Ho, int Wo, int P, int tiles, float scale, int L,
    const float* __restrict__ gt, int hgroups, const float* __restrict__ fpart, const uint32_t* __restrict__ prefix,
    uint8_t* __restrict__ level_xy, uint8_t* __restrict__ level_cell, double* __restrict__ dpart,
    int32_t* __restrict__ ipart) {
  __shared__ float shm[CR_WAVES];
  __shared__ double shd[CR_WAVES];
  __shared__ int shi[CR_WAVES];
  __shared__ int s_lr[CR_MAX_R];
  __shared__ int s_box[CR_MAX_L * 4];
  __shared__ int s_pix[CR_MAX_L];
  const int t = threadIdx.x;
  const float nan = __int_as_float(0x7fc00000);
  const float vmax = vote_fold_max<CR_WAVES, 1>(fpart, 0, hgroups, shm);
  const bool empty = !(vmax > -INFINITY);
  float tau[CR_MAX_L];
#pragma unroll
  for (int l = 0; l < CR_MAX_L; ++l) tau[l] = (l < L && !empty) ? cr_unkey(prefix[l]) : nan;
  const float vgt = empty ? nan : cr_gt_vote(votes, gt, R, Ho, Wo);
  if (t < CR_MAX_R) s_lr[t] = L;
  if (t < CR_MAX_L * 4) s_box[t] = (t & 1) ? -1 : CR_NO_MIN;   // { a_min, a_max, b_min, b_max }
  if (t < CR_MAX_L) s_pix[t] = 0;
  __syncthreads();
  const double ds = (double)scale;
  double m[CR_MAX_L + 1], ga = 0.0, ge = 0.0;
  int c[CR_MAX_L];
#pragma unroll
  for (int k = 0; k <= CR_MAX_L; ++k) m[k] = 0.0;
#pragma unroll
  for (int k = 0; k < CR_MAX_L; ++k) c[k] = 0;

  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int p;
    if (!vote_tile_pixel<CR_NT>(tile, P, &p)) continue;   // (no barrier in this loop)
    int lxy = L;
    for (int r = 0; r < R; ++r) {
      const float v = votes[(size_t)r * P + p];
      int lev = L;
      if (vote_finite(v)) {
        lev = 0;
#pragma unroll
        for (int l = 0; l < CR_MAX_L; ++l) lev += v < tau[l] ? 1 : 0;   // (tau descends; NaN past L: never counted)
        const double w = cr_weight(v, vmax, ds);
#pragma unroll
        for (int k = 0; k <= CR_MAX_L; ++k) m[k] += lev == k ? w : 0.0;
#pragma unroll
        for (int k = 0; k < CR_MAX_L; ++k) c[k] += lev == k ? 1 : 0;
        if (v > vgt)
          ga += w;
        else if (v == vgt)
          ge += w;
      }
      if (level_cell != nullptr) level_cell[(size_t)r * P + p] = (uint8_t)lev;
      if (lev < L) {
        lxy = min(lxy, lev);
        // (the plain read may be stale, and a stale value is only ever larger: then the atomic is merely redundant)
        if (lev < *(volatile int*)&s_lr[r]) atomicMin(&s_lr[r], lev);
      }
    }
    level_xy[p] = (uint8_t)lxy;
    if (lxy < L) {
      int a, b;
      vote_row_col(p, Wo, &a, &b);
      atomicAdd(&s_pix[lxy], 1);
      volatile int* box = &s_box[lxy * 4];
      if (a < box[0]) atomicMin(&s_box[lxy * 4 + 0], a);
      if (a > box[1]) atomicMax(&s_box[lxy * 4 + 1], a);
      if (b < box[2]) atomicMin(&s_box[lxy * 4 + 2], b);
      if (b > box[3]) atomicMax(&s_box[lxy * 4 + 3], b);
    }
  }
  __syncthreads();
  double* drow = dpart + (size_t)blockIdx.x * CR_DCOLS;
  int32_t* irow = ipart + (size_t)blockIdx.x * CR_ICOLS;
#pragma unroll
  for (int k = 0; k <= CR_MAX_L; ++k) {
    const double s = vote_block_sum<CR_WAVES>(m[k], shd);
    if (t == 0) drow[k] = s;
  }
  ga = vote_block_sum<CR_WAVES>(ga, shd);
  ge = vote_block_sum<CR_WAVES>(ge, shd);
  if (t == 0) {
    drow[CR_MAX_L + 1] = ga;
    drow[CR_MAX_L + 2] = ge;
    drow[CR_MAX_L + 3] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < CR_MAX_L; ++k) {
    const int s = vote_block_sum<CR_WAVES>(c[k], shi);
    if (t == 0) irow[k] = s;
  }
  if (t < CR_MAX_L) irow[CR_I_PIX + t] = s_pix[t];
  if (t < CR_MAX_L * 4) irow[CR_I_BOX + t] = s_box[t];
  if (t < CR_MAX_R) irow[CR_I_LR + t] = s_lr[t];
}

// ---- launch 11: one workgroup folds the partial rows
__global__ __launch_bounds__(CR_NS) void vote_credible_finish_kernel(
    const float* __restrict__ votes, int R, int Ho, int Wo, int L, const float* __restrict__ gt, int hgroups,
    int fgroups, const float* __restrict__ fpart, const int32_t* __restrict__ cpart,
    const uint32_t* __restrict__ prefix, const double* __restrict__ dpart, const int32_t* __restrict__ ipart,
    float* __restrict__ threshold, float* __restrict__ mass, int32_t* __restrict__ table,
    uint8_t* __restrict__ level_r, float* __restrict__ gt_stats, int32_t* __restrict__ count) {
  __shared__ float shm[CR_NS_WAVES];
  __shared__ double shd[CR_NS_WAVES];
  __shared__ int shi[CR_NS_WAVES];
  __shared__ int s_box[CR_NS / 32][32];
  __shared__ int s_lrp[CR_NS / CR_MAX_R][CR_MAX_R];
  __shared__ int s_lr[CR_MAX_R];
  __shared__ int s_boxf[32];
  const int t = threadIdx.x;
  const float nan = __int_as_float(0x7fc00000);
  // vmax: the same fold value as the other launches' (a maximum has no order)
  float vm = -INFINITY;
  for (int g = t; g < hgroups; g += CR_NS) vm = fmaxf(vm, fpart[g]);
  vm = wave_max(vm);
  if ((t & 63) == 0) shm[t >> 6] = vm;
  __syncthreads();
  float vmax = -INFINITY;
  for (int w = 0; w < CR_NS_WAVES; ++w) vmax = fmaxf(vmax, shm[w]);
  const bool empty = !(vmax > -INFINITY);

  // thread g holds workgroup g's partial rows (fgroups, hgroups <= CR_NS): every load is in flight before the first
  // reduction, and the reductions (vote_block_sum: a wave tree, then the 16 waves in sequence) wait for no memory
  static_assert(CR_MAX_GROUPS <= CR_NS, "one thread per partial row");
  double tot[CR_MAX_L + 3];
  int cells[CR_MAX_L], pix[CR_MAX_L];
  const bool frow = t < fgroups, hrow = t < hgroups;
#pragma unroll
  for (int k = 0; k < CR_MAX_L + 3; ++k) tot[k] = frow ? dpart[(size_t)t * CR_DCOLS + k] : 0.0;
#pragma unroll
  for (int k = 0; k < CR_MAX_L; ++k) {
    cells[k] = frow ? ipart[(size_t)t * CR_ICOLS + k] : 0;
    pix[k] = frow ? ipart[(size_t)t * CR_ICOLS + CR_I_PIX + k] : 0;
  }
  int n_ok = hrow ? cpart[(size_t)t * 2] : 0, n_bad = hrow ? cpart[(size_t)t * 2 + 1] : 0;
#pragma unroll
  for (int k = 0; k < CR_MAX_L + 3; ++k) tot[k] = vote_block_sum<CR_NS_WAVES>(tot[k], shd);
#pragma unroll
  for (int k = 0; k < CR_MAX_L; ++k) {
    cells[k] = vote_block_sum<CR_NS_WAVES>(cells[k], shi);
    pix[k] = vote_block_sum<CR_NS_WAVES>(pix[k], shi);
  }
  n_ok = vote_block_sum<CR_NS_WAVES>(n_ok, shi);
  n_bad = vote_block_sum<CR_NS_WAVES>(n_bad, shi);
  {
    const int col = t & 31, slice = t >> 5;
    const bool is_max = col & 1;
    int v = is_max ? -1 : CR_NO_MIN;
#pragma unroll 8
    for (int g = slice; g < fgroups; g += CR_NS / 32) {
      const int x = ipart[(size_t)g * CR_ICOLS + CR_I_BOX + col];
      v = is_max ? max(v, x) : min(v, x);
    }
    s_box[slice][col] = v;
  }
  {
    const int col = t & (CR_MAX_R - 1), slice = t / CR_MAX_R;
    int v = L;
#pragma unroll 8
    for (int g = slice; g < fgroups; g += CR_NS / CR_MAX_R) v = min(v, ipart[(size_t)g * CR_ICOLS + CR_I_LR + col]);
    s_lrp[slice][col] = v;
  }
  __syncthreads();
  if (t < CR_MAX_R) {
    int v = L;
    for (int s = 0; s < CR_NS / CR_MAX_R; ++s) v = min(v, s_lrp[s][t]);
    s_lr[t] = v;
    if (t < R) level_r[t] = (uint8_t)v;
  }
  __syncthreads();
  if (t >= CR_MAX_R && t < CR_MAX_R + 32) {   // the box columns over the slices
    const int col = t - CR_MAX_R;
    const bool is_max = col & 1;
    int v = is_max ? -1 : CR_NO_MIN;
    for (int s = 0; s < CR_NS / 32; ++s) v = is_max ? max(v, s_box[s][col]) : min(v, s_box[s][col]);
    s_boxf[col] = v;
  }
  __syncthreads();
  if (t >= L) return;

  // thread l writes level l's outputs (the sums are in every thread's registers: static indices, in order)
  const int l = t;
  const float vgt = empty ? nan : cr_gt_vote(votes, gt, R, Ho, Wo);
  const bool gt_valid = vgt == vgt;
  const float tau = empty ? nan : cr_unkey(prefix[l]);
  double Z = 0.0, cum = 0.0;
  int ccum = 0, pcum = 0, a0 = CR_NO_MIN, a1 = -1, b0 = CR_NO_MIN, b1 = -1;
#pragma unroll
  for (int k = 0; k <= CR_MAX_L; ++k) Z += tot[k];
#pragma unroll
  for (int k = 0; k < CR_MAX_L; ++k) {
    if (k <= l) {
      cum += tot[k];
      ccum += cells[k];
      pcum += pix[k];
      a0 = min(a0, s_boxf[k * 4 + 0]);
      a1 = max(a1, s_boxf[k * 4 + 1]);
      b0 = min(b0, s_boxf[k * 4 + 2]);
      b1 = max(b1, s_boxf[k * 4 + 3]);
    }
  }
  int rot = 0;
  for (int r = 0; r < R; ++r) rot += s_lr[r] <= l ? 1 : 0;
  threshold[l] = tau;
  mass[l] = empty ? nan : (float)(cum / Z);
  int32_t* row = table + l * 8;
  const bool none = ccum == 0;
  row[0] = ccum;
  row[1] = pcum;
  row[2] = rot;
  row[3] = none ? -1 : a0;
  row[4] = none ? -1 : a1;
  row[5] = none ? -1 : b0;
  row[6] = none ? -1 : b1;
  row[7] = 0;
  if (l != 0) return;
  int gt_level = 0;
  for (int k = 0; k < L; ++k) gt_level += (gt_valid && vgt < cr_unkey(prefix[k])) ? 1 : 0;
  gt_stats[0] = vgt;
  gt_stats[1] = gt_valid ? (float)(tot[CR_MAX_L + 1] / Z) : nan;
  gt_stats[2] = gt_valid ? (float)((tot[CR_MAX_L + 1] + tot[CR_MAX_L + 2]) / Z) : nan;
  gt_stats[3] = 0.f;
  count[0] = n_ok;
  count[1] = n_bad;
  count[2] = gt_valid ? 1 : 0;
  count[3] = gt_valid ? gt_level : -1;
}

struct CrPlan {
  VotePlan cell;     // the max and digit passes: tiles of every rotation's plane
  VotePlan pixel;    // the level pass: tiles of one plane
  int q_bits;        // Q: a weight is held in units of 2^-Q
};

bool cr_plan(int R, int Ho, int Wo, CrPlan* plan) {
  if (R < 1 || R > CR_MAX_R || Ho < 1 || Wo < 1) return false;
  const int64_t cells = (int64_t)R * Ho * Wo;
  if (!vote_plan(cells, R, Ho, Wo, CR_NT, CR_MAX_GROUPS, &plan->cell)) return false;
  if (!vote_plan(cells, 1, Ho, Wo, CR_NT, CR_MAX_GROUPS, &plan->pixel)) return false;
  int bits = 0;
  while ((cells >> bits) != 0) ++bits;      // cells < 2^bits, bits <= 31
  plan->q_bits = 62 - bits;
  return true;
}

// [hg] f32 maxima | [hg][2] counts | prefix state [5][8] | above state [5][8] | Z | [4][8][256] bins |
// [fg][12] float64 rows | [fg][112] int rows
struct CrWorkspace {
  float* fpart;
  int32_t* cpart;
  uint32_t* prefix;
  u64* above;
  u64* zfix;
  u64* gbins;
  double* dpart;
  int32_t* ipart;
  size_t bytes;
};

CrWorkspace cr_workspace(const CrPlan& plan, int L, void* workspace) {
  VoteLayout l{workspace};
  const size_t hg = plan.cell.groups, fg = plan.pixel.groups;
  return {l.take<float>(hg),
          l.take<int32_t>(hg * 2),
          l.take<uint32_t>((CR_DIGITS + 1) * CR_MAX_L),
          l.take<u64>((CR_DIGITS + 1) * CR_MAX_L),
          l.take<u64>(1),
          l.take<u64>((size_t)CR_DIGITS * CR_MAX_L * CR_BINS),
          l.take<double>(fg * CR_DCOLS),
          l.take<int32_t>(fg * CR_ICOLS),
          l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_credible_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t L) {
  CrPlan plan;
  if (L < 1 || L > CR_MAX_L || !cr_plan(R, Ho, Wo, &plan)) return 0;
  return cr_workspace(plan, L, nullptr).bytes;
}

extern "C" int snap_vote_credible_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale,
                                      const float* levels, int32_t L, const float* gt_index, float* threshold,
                                      float* mass, int32_t* table, uint8_t* level_xy, uint8_t* level_r,
                                      uint8_t* level_cell, float* gt_stats, int32_t* count, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!votes || !levels || !threshold || !mass || !table || !level_xy || !level_r || !gt_stats || !count || !workspace)
    return SNAP_ERR_NULL;
  CrPlan plan;
  if (!cr_plan(R, Ho, Wo, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale > 0.f) || !(scale < INFINITY)) return SNAP_ERR_UNSUPPORTED;
  if (L < 1 || L > CR_MAX_L) return SNAP_ERR_UNSUPPORTED;
  CrLevels lv;
  for (int l = 0; l < CR_MAX_L; ++l) lv.q[l] = 0.f;
  for (int l = 0; l < L; ++l) {
    const float q = levels[l];
    if (!(q > 0.f && q < 1.f) || (l > 0 && !(q > levels[l - 1]))) return SNAP_ERR_UNSUPPORTED;
    lv.q[l] = q;
  }
  if (!vote_workspace_ok(workspace, workspace_bytes, cr_workspace(plan, L, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const CrWorkspace w = cr_workspace(plan, L, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const VotePlan& c = plan.cell;
  const double two_q = ldexp(1.0, plan.q_bits);
  hipLaunchKernelGGL(vote_credible_max_kernel, dim3(c.groups), dim3(CR_NT), 0, s, votes, c.P, c.tiles_per_plane,
                     c.tiles, w.fpart, w.cpart, w.gbins);
  SNAP_CHECK_LAUNCH();
  for (int pass = 0; pass < CR_DIGITS; ++pass) {
    const uint32_t* pin = pass == 0 ? nullptr : w.prefix + pass * CR_MAX_L;
    const u64* ain = pass == 0 ? nullptr : w.above + pass * CR_MAX_L;
    hipLaunchKernelGGL(vote_credible_hist_kernel, dim3(c.groups), dim3(CR_NT), 0, s, votes, c.P, c.tiles_per_plane,
                       c.tiles, c.groups, scale, two_q, L, pass, w.fpart, pin, w.gbins);
    SNAP_CHECK_LAUNCH();
    hipLaunchKernelGGL(vote_credible_select_kernel, dim3(L), dim3(CR_BINS), 0, s, lv, L, pass, w.gbins, pin,
                       ain, w.zfix, w.prefix + (pass + 1) * CR_MAX_L, w.above + (pass + 1) * CR_MAX_L);
    SNAP_CHECK_LAUNCH();
  }
  const uint32_t* keys = w.prefix + CR_DIGITS * CR_MAX_L;
  hipLaunchKernelGGL(vote_credible_levels_kernel, dim3(plan.pixel.groups), dim3(CR_NT), 0, s, votes, R, Ho, Wo,
                     plan.pixel.P, plan.pixel.tiles, scale, L, gt_index, c.groups, w.fpart, keys, level_xy, level_cell,
                     w.dpart, w.ipart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_credible_finish_kernel, dim3(1), dim3(CR_NS), 0, s, votes, R, Ho, Wo, L, gt_index, c.groups,
                     plan.pixel.groups, w.fpart, w.cpart, keys, w.dpart, w.ipart, threshold, mass, table, level_r,
                     gt_stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
