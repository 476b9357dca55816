// The PREDICT step of the vote-volume filter (snap_vote_filter_f32): its four kernels and the one function that
// launches them, shared by vote_filter.hip, vote_smooth.hip, vote_pairs.hip and vote_sample.hip.  The smoother's ratio,
// the tap posteriors and the backward sampler's conditional are taken against the prior the filter used, so M, the
// masses, t0, t1, t2, S and the prior have to be the filter's bits.  They are, because all four files run the kernels
// below through vp_launch_predict (and -ffp-contract=off is in force).  A tile is one rotation and VP_NT consecutive
// pixels p = a * Wo + b, one cell per thread, on min(tiles, VP_MAX_GROUPS) workgroups of VP_NT threads striding over
// the tiles; the tap rows of a tile are uniform (scalar loads).
//
// Per-workgroup partials are rows of FS floats, DS doubles and IS int32 (VpParts); the predict step owns the first
// columns (VP_F_PEAK; VP_D_SUMP, VP_D_SUMT2; VP_I_BAD, VP_I_MASS), the including file the others.
//
// The row and column kernels also run as the ADJOINT of themselves (ADJ = true: vp_launch_rows<true> and
// vp_launch_cols<true>, vote_smooth.hip and vote_pairs.hip): the same tables read backwards,
// out[x] = sum_t taps[t] * src[x - l - t], by index arithmetic: the first source is x - l - (T - 1) and source i takes
// taps[T - 1 - i], so the chain still runs over the source cell ascending.
//
// LINKAGE: the kernels and their launchers are in an unnamed namespace, so every including file keeps its own copy of
// the instantiations it uses (vp_rows_kernel<false> exists four times in the library), exactly as when each file
// declared forwarding kernels of its own name.  With external linkage the four code objects would each carry a kernel
// of one name behind one merged host stub, registered with the HIP runtime four times; that is left untried, since the
// copies cost a few KiB of code and nothing at run time.
#ifndef SNAP_CSRC_VOTE_PREDICT_H_
#define SNAP_CSRC_VOTE_PREDICT_H_

#include "vote_common.h"

constexpr int VP_NT = 256;                  // threads = cells of a tile
constexpr int VP_WAVES = VP_NT / SNAP_WAVE;
constexpr int VP_MAX_R = 64;
constexpr int VP_MAX_TK = 16;
constexpr int VP_MAX_TXY = 32;
constexpr int VP_MAX_GROUPS = 2048;
constexpr float VP_CUT = -40.f;             // a cell carries mass iff value - peak >= VP_CUT

enum { VP_F_PEAK = 0 };
enum { VP_D_SUMP = 0, VP_D_SUMT2 = 1 };
enum { VP_I_BAD = 0, VP_I_MASS = 1 };

// The mass of a belief cell relative to the peak M: one f32 subtraction, the cut, exp in float64 rounded once.
__device__ __forceinline__ float vp_mass(float v, float M) {
  const float d = v - M;
  return (vote_finite(v) && d >= VP_CUT) ? (float)exp((double)d) : 0.f;
}

// The first source index of output index x and the tap source i takes.
template <bool ADJ>
__device__ __forceinline__ int64_t vp_first(int x, int l, int T) {
  return ADJ ? (int64_t)x - l - (T - 1) : (int64_t)x + l;
}
template <bool ADJ>
__device__ __forceinline__ int vp_tap(int i, int T) {
  return ADJ ? T - 1 - i : i;
}

// ---- per workgroup the largest finite belief and the count of NaN / +inf cells
template <int FS, int IS>
__device__ __forceinline__ void vp_peak(const float* __restrict__ belief, int n, float* __restrict__ fpart,
                                        int32_t* __restrict__ ipart) {
  __shared__ float shf[VP_WAVES];
  __shared__ int shi[VP_WAVES];
  float m = -INFINITY;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * VP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * VP_NT) {
    const float v = belief[i];
    if (vote_finite(v))
      m = fmaxf(m, v);
    else if (!(v == -INFINITY))
      ++bad;                                // NaN or +inf
  }
  m = vote_block_max<VP_WAVES>(m, shf);
  bad = vote_block_sum<VP_WAVES>(bad, shi);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * FS + VP_F_PEAK] = m;
    ipart[(size_t)blockIdx.x * IS + VP_I_BAD] = bad;
  }
}

// ---- t0[r, a, b] = sum_tk taps_k[tk] * p[(r + lk + tk) mod R, a, b], exp fused; sum p and the cells with mass
template <int FS, int DS, int IS>
__device__ __forceinline__ void vp_rotate(const float* __restrict__ belief, const float* __restrict__ taps_k, int lk,
                                          int R, int P, int Tk, int tiles_per_plane, int tiles,
                                          const float* __restrict__ fpart, float* __restrict__ t0,
                                          double* __restrict__ dpart, int32_t* __restrict__ ipart) {
  __shared__ float shf[VP_WAVES];
  __shared__ double shd[VP_WAVES];
  __shared__ int shi[VP_WAVES];
  const float M = vote_fold_max<VP_WAVES, FS>(fpart, VP_F_PEAK, gridDim.x, shf);
  const int kfirst = vote_mod(lk, R);       // (r + lk) mod R, mathematically: lk mod R in [0, R) first
  double sum_p = 0.0;
  int n_mass = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // (vote_tile_cell written out: through it this kernel takes 42 VGPRs / 58 SGPRs for 40 / 56)
    const int r = tile / tiles_per_plane;
    const int64_t p64 = (int64_t)(tile - r * tiles_per_plane) * VP_NT + threadIdx.x;
    if (p64 >= P) continue;
    const int p = (int)p64;
    const float own = vp_mass(belief[(int64_t)r * P + p], M);
    sum_p += (double)own;
    n_mass += own > 0.f ? 1 : 0;
    int k = r + kfirst;                     // (>= 0: one side of vote_wrap)
    if (k >= R) k -= R;
    float acc = 0.f;
    for (int i = 0; i < Tk; ++i) {
      acc = fmaf(taps_k[i], vp_mass(belief[(int64_t)k * P + p], M), acc);
      k = vote_next(k, R);
    }
    t0[(int64_t)r * P + p] = acc;
  }
  sum_p = vote_block_sum<VP_WAVES>(sum_p, shd);
  n_mass = vote_block_sum<VP_WAVES>(n_mass, shi);
  if (threadIdx.x == 0) {
    dpart[(size_t)blockIdx.x * DS + VP_D_SUMP] = sum_p;
    ipart[(size_t)blockIdx.x * IS + VP_I_MASS] = n_mass;
  }
}

// ---- t1[r, a, b] = sum_ta taps_a[r, ta] * t0[r, a + la[r] + ta, b]      (ADJ: ... * t0[r, a - la[r] - ta, b])
template <bool ADJ>
__device__ __forceinline__ void vp_rows(const float* __restrict__ t0, const float* __restrict__ taps_a,
                                        const int32_t* __restrict__ offsets, int Ho, int Wo, int P, int Ta,
                                        int tiles_per_plane, int tiles, float* __restrict__ t1) {
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p, a, b;
    if (!vote_tile_cell<VP_NT>(tile, tiles_per_plane, P, &r, &p)) continue;
    vote_row_col(p, Wo, &a, &b);
    const float* w = taps_a + (size_t)r * Ta;                     // uniform over the workgroup
    const int64_t first = vp_first<ADJ>(a, offsets[(size_t)r * 2], Ta);   // the source row of the chain's first link
    const float* src = t0 + (int64_t)r * P + b;
    float acc = 0.f;
    for (int i = 0; i < Ta; ++i) {
      const int64_t sa = first + i;
      if (sa >= 0 && sa < Ho) acc = fmaf(w[vp_tap<ADJ>(i, Ta)], src[sa * Wo], acc);   // (outside: + 0, the chain is unchanged)
    }
    t1[(int64_t)r * P + p] = acc;
  }
}

// ---- t2[r, a, b] = sum_tb taps_b[r, tb] * t1[r, a, b + lb[r] + tb]      (ADJ: ... * t1[r, a, b - lb[r] - tb]);
// with SUM, per workgroup sum t2 (float64) into column VP_D_SUMT2
template <bool ADJ, bool SUM, int DS>
__device__ __forceinline__ void vp_cols(const float* __restrict__ t1, const float* __restrict__ taps_b,
                                        const int32_t* __restrict__ offsets, int Wo, int P, int Tb,
                                        int tiles_per_plane, int tiles, float* __restrict__ t2,
                                        double* __restrict__ dpart) {
  __shared__ double shd[VP_WAVES];
  double sum = 0.0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p, a, b;
    if (!vote_tile_cell<VP_NT>(tile, tiles_per_plane, P, &r, &p)) continue;
    vote_row_col(p, Wo, &a, &b);
    const float* w = taps_b + (size_t)r * Tb;
    const int64_t first = vp_first<ADJ>(b, offsets[(size_t)r * 2 + 1], Tb);
    const float* src = t1 + (int64_t)r * P + (int64_t)a * Wo;
    float acc = 0.f;
    for (int i = 0; i < Tb; ++i) {
      const int64_t sb = first + i;
      if (sb >= 0 && sb < Wo) acc = fmaf(w[vp_tap<ADJ>(i, Tb)], src[sb], acc);
    }
    t2[(int64_t)r * P + p] = acc;
    if (SUM) sum += (double)acc;
  }
  if (SUM) {
    sum = vote_block_sum<VP_WAVES>(sum, shd);
    if (threadIdx.x == 0) dpart[(size_t)blockIdx.x * DS + VP_D_SUMT2] = sum;
  }
}

// The predicted prior of one cell, float64: ((1 - eps) * t2) / S + eps / n, the first term 0 without a belief or with
// S == 0.  `transported` = (1 - eps) / S is NOT folded into one factor: the expression is the contract's.
struct VpPrior {
  double one_minus_eps, S, eps_over_n;
  bool has_prior;                           // a belief was given and S > 0
};
__device__ __forceinline__ double vp_prior(const VpPrior& c, float t2) {
  double prior = c.eps_over_n;
  if (c.has_prior) prior = (c.one_minus_eps * (double)t2) / c.S + c.eps_over_n;
  return prior;
}
// (`S` is the fold of the VP_D_SUMT2 column, 0 without a belief.)  belief == NULL is the uniform prior: eps = 1.
__device__ __forceinline__ VpPrior vp_prior_setup(double S, bool with_belief, float eps, int n) {
  VpPrior c;
  c.S = S;
  c.has_prior = with_belief && S > 0.0;
  c.one_minus_eps = with_belief ? 1.0 - (double)eps : 0.0;
  c.eps_over_n = (with_belief ? (double)eps : 1.0) / (double)n;
  return c;
}

// ------------------------------- host: limits and the plan ------------------------------------
struct VpPlan : VotePlan {
  int R, Ho, Wo, n;
};

inline bool vp_plan(int R, int Ho, int Wo, int Tk, int Ta, int Tb, VpPlan* plan) {
  if (R < 1 || R > VP_MAX_R || Ho < 1 || Wo < 1) return false;
  if (Tk < 1 || Tk > VP_MAX_TK || Ta < 1 || Ta > VP_MAX_TXY || Tb < 1 || Tb > VP_MAX_TXY) return false;
  if (!vote_plan((int64_t)R * Ho * Wo, R, Ho, Wo, VP_NT, VP_MAX_GROUPS, plan)) return false;
  plan->R = R, plan->Ho = Ho, plan->Wo = Wo;
  plan->n = R * Ho * Wo;
  return true;
}

// ------------------------------- host: the launches -------------------------------------------
// The tap tuple of a filter step, as the entry points take it.
struct VpTaps {
  const float* taps_k;
  int lk;
  const float *taps_a, *taps_b;
  const int32_t* offsets;
  int Tk, Ta, Tb;
};
// The three per-workgroup partial arrays; their row strides are part of the type, so a launch cannot take one file's
// arrays with another's strides.
template <int FS, int DS, int IS>
struct VpParts {
  float* f;
  double* d;
  int32_t* i;
};

// An entry point's call of a launcher below: a status other than SNAP_OK is the entry point's.
#define VP_CHECK(call)                 \
  do {                                 \
    const int e_ = (call);             \
    if (e_ != SNAP_OK) return e_;      \
  } while (0)

namespace {   // (LINKAGE, above)

// The kernels: each is one body above (the body inlined into a kernel is the shape whose assembly is the forwarding
// kernels' that every file used to declare, instruction for instruction).
template <int FS, int IS>
__global__ __launch_bounds__(VP_NT) void vp_peak_kernel(const float* __restrict__ belief, int n,
                                                        float* __restrict__ fpart, int32_t* __restrict__ ipart) {
  vp_peak<FS, IS>(belief, n, fpart, ipart);
}
template <int FS, int DS, int IS>
__global__ __launch_bounds__(VP_NT) void vp_rotate_kernel(const float* __restrict__ belief,
                                                          const float* __restrict__ taps_k, int lk, int R, int P, int Tk,
                                                          int tiles_per_plane, int tiles, const float* __restrict__ fpart,
                                                          float* __restrict__ t0, double* __restrict__ dpart,
                                                          int32_t* __restrict__ ipart) {
  vp_rotate<FS, DS, IS>(belief, taps_k, lk, R, P, Tk, tiles_per_plane, tiles, fpart, t0, dpart, ipart);
}
template <bool ADJ>
__global__ __launch_bounds__(VP_NT) void vp_rows_kernel(const float* __restrict__ src, const float* __restrict__ taps_a,
                                                        const int32_t* __restrict__ offsets, int Ho, int Wo, int P,
                                                        int Ta, int tiles_per_plane, int tiles,
                                                        float* __restrict__ dst) {
  vp_rows<ADJ>(src, taps_a, offsets, Ho, Wo, P, Ta, tiles_per_plane, tiles, dst);
}
template <bool ADJ, bool SUM, int DS>
__global__ __launch_bounds__(VP_NT) void vp_cols_kernel(const float* __restrict__ src, const float* __restrict__ taps_b,
                                                        const int32_t* __restrict__ offsets, int Wo, int P, int Tb,
                                                        int tiles_per_plane, int tiles, float* __restrict__ dst,
                                                        double* __restrict__ dpart) {
  vp_cols<ADJ, SUM, DS>(src, taps_b, offsets, Wo, P, Tb, tiles_per_plane, tiles, dst, dpart);
}

// One launch each: the row pass and the column pass, src -> dst (two volumes).  ADJ = false is the predict step's pass
// (the columns with SUM: sum t2 into the partials), ADJ = true the adjoint pass the smoother and the tap posteriors
// interleave with kernels of their own (no sum).  Templates, so a file that never asks for the adjoint carries none.
template <bool ADJ>
int vp_launch_rows(const VpPlan& plan, const VpTaps& t, const float* src, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(vp_rows_kernel<ADJ>, dim3(plan.groups), dim3(VP_NT), 0, s, src, t.taps_a, t.offsets, plan.Ho,
                     plan.Wo, plan.P, t.Ta, plan.tiles_per_plane, plan.tiles, dst);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
template <bool ADJ, int FS, int DS, int IS>
int vp_launch_cols(const VpPlan& plan, const VpTaps& t, const float* src, float* dst, const VpParts<FS, DS, IS>& part,
                   hipStream_t s) {
  hipLaunchKernelGGL((vp_cols_kernel<ADJ, !ADJ, DS>), dim3(plan.groups), dim3(VP_NT), 0, s, src, t.taps_b, t.offsets,
                     plan.Wo, plan.P, t.Tb, plan.tiles_per_plane, plan.tiles, dst, part.d);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

// Launches 1-4 of every operator with a predict step, in this order: peak, rotate (belief -> t0), rows (t0 -> t1),
// cols with SUM (t1 -> t2).  t0 and t2 MAY be the same volume: t0's last reader (rows) is done before cols writes t2
// (the filter and the smoother keep both in their output, the sampler in `t02`); t1 is a volume of its own.  Returns
// SNAP_OK or SNAP_ERR_LAUNCH.
template <int FS, int DS, int IS>
int vp_launch_predict(const VpPlan& plan, const VpTaps& t, const float* belief, float* t0, float* t1, float* t2,
                      const VpParts<FS, DS, IS>& part, hipStream_t s) {
  const dim3 grid(plan.groups), block(VP_NT);
  hipLaunchKernelGGL((vp_peak_kernel<FS, IS>), grid, block, 0, s, belief, plan.n, part.f, part.i);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL((vp_rotate_kernel<FS, DS, IS>), grid, block, 0, s, belief, t.taps_k, t.lk, plan.R, plan.P, t.Tk,
                     plan.tiles_per_plane, plan.tiles, part.f, t0, part.d, part.i);
  SNAP_CHECK_LAUNCH();
  VP_CHECK(vp_launch_rows<false>(plan, t, t0, t1, s));
  VP_CHECK(vp_launch_cols<false>(plan, t, t1, t2, part, s));
  return SNAP_OK;
}

}  // namespace

#endif  // SNAP_CSRC_VOTE_PREDICT_H_
