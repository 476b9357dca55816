// Tap posteriors of one step of the vote-volume filter: snap_vote_pairs_f32 (include/snap_hip.h).
//
// belief [R, Ho, Wo] f32 = log alpha_t, the filter's output at frame t; next [R, Ho, Wo] f32 = log gamma_{t+1}, the
// smoothed belief of frame t + 1; the taps the filter used from t to t + 1; eps = uniform_mix; n = R Ho Wo.  The
// pairwise posterior of the step, xi(x, x') = alpha(x) K(x' | x) gamma_{t+1}(x') / prior(x'), splits into the JUMP
// branch (the uniform share eps / n of the prior) and the STAY branch by tap triple; this file gives the three per-axis
// marginals of the stay branch and the two masses, never the joint.
// PREDICT, the filter's own code (vote_predict.h): M, the masses p, t0, t1, t2, S = sum t2, sum p and the prior: the
// filter's bits.  RATIO, the smoother's own code (vote_ratio.h): G, q = fl32(exp(lg - G)), Q = sum q: the smoother's
// bits.  ADJOINT, vote_predict.h's kernels with ADJ (the smoother's first two gathers; its c1 is c0 here and its c0 is c1:
// the names below count the passes):
//   c0[r, a, b] = sum_tb taps_b[r, tb] q [r, a, b - lb[r] - tb];
//   c1[r, a, b] = sum_ta taps_a[r, ta] c0[r, a - la[r] - ta, b];
// HISTOGRAMS, raw (in units of e^G S / (1 - eps)), sources outside the volume skipped as the passes skip them:
//   Hb[r, tb] = sum_{a, b} fl32(fl32(taps_b[r, tb] * t1[r, a, b + lb[r] + tb]) * q [r, a, b]);
//   Ha[r, ta] = sum_{a, b} fl32(fl32(taps_a[r, ta] * t0[r, a + la[r] + ta, b]) * c0[r, a, b]);
//   Hk[tk]    = sum_{r, a, b} fl32(fl32(taps_k[tk] * p[(r + lk + tk) mod R, a, b]) * c1[r, a, b]);
// every term two f32 products (no fma: -ffp-contract=off), every sum float64.  FINISH, float64: H = sum_tk Hk (index
// order), c = (1 - eps) / S (0 when S == 0), stay_raw = c H, jump_raw = (eps / n) Q, total = stay_raw + jump_raw;
// stay = stay_raw / total, jump = jump_raw / total, hist = (c Hraw) / total, log_norm = G + log(total); all 0 and
// log_norm = -inf when total == 0 (no ratio mass).
//
// The predict, ratio and adjoint launches have the family's shape: a tile = one rotation and 256 consecutive pixels,
// min(tiles, 2048) workgroups of 256 threads striding over the tiles.  The three REDUCTION launches keep the tile and
// the 256 threads but hand the tiles out PER ROTATION: gpr = min(tiles per plane, 2048 / R) workgroups per rotation,
// R gpr <= 2048 in all, workgroup (r, g) striding over the tiles g, g + gpr, ... of plane r.  That is the choice
// between flushing and indexing partials per rotation: a workgroup never changes rotation, so its tap row is one
// scalar-loaded row for its whole life, it accumulates in registers over all its tiles and writes ONE partial row of T
// float64 at its end, and the partials are [R gpr][T] (<= 2048 x 32 x 8 bytes = 512 KiB per histogram) instead of
// [2048][R][T].  Per thread: <= 32 (k: 16) float64 accumulators in registers (the tap loop is unrolled to the table's
// limit and predicated on the uniform T, so the array is never indexed dynamically), one chain per tap over the
// thread's tiles in order.  Per workgroup: each tap's xor butterfly over the wave, lane 0 into LDS [4 waves][32]
// float64 = 1 KiB (k: [4][16] = 512 bytes), then (w0 + w1) + (w2 + w3) by thread t.  The finish launch, one workgroup,
// folds a histogram's partial rows with 256 threads = 32 columns x 8 slices (k: 16 x 16): a strided chain per thread,
// the slices in index order through 2 KiB of LDS; hist_k first (it gives the total), then hist_a and hist_b row by
// row, scaled as they are written.  No atomics, no inter-workgroup hand-off inside a launch: every order is fixed by
// (R, Ho, Wo, Tk, Ta, Tb) alone.
// Launches: 1-4 the filter's (vp_launch_predict, kernels in vote_predict.h: t0 -> A, t1 -> B, t2 -> C); 5-6 the
// smoother's ratio (vr_launch_ratio, kernels in vote_ratio.h: q -> D); 7 Hb (vote_pairs_hist_b_kernel; reads q, t1);
// 8 c0 = adjoint columns of q -> C (vp_launch_cols<true>); 9 Ha (vote_pairs_hist_a_kernel; reads c0, t0); 10 c1 = adjoint
// rows of c0 -> B (vp_launch_rows<true>); 11 Hk (vote_pairs_hist_k_kernel; reads c1, belief); 12 finish
// (vote_pairs_finish_kernel).  A-D are the workspace's four volumes.
// HBM traffic (n cells of 4 bytes): reads belief 3 (+ L2 re-reads in k, twice), next 2, t0 2, t1 2, t2 2, q 2, c0 2,
// c1 1; writes t0, t1, t2, q, c0, c1: 22 n cells, the smoother's figure.
#include "vote_ratio.h"

namespace {

constexpr int PR_NT = VP_NT;
constexpr int PR_WAVES = VP_WAVES;

// per-workgroup partials of the predict / ratio launches: double [groups][4], int32 [groups][4], float [groups][1]
constexpr int PR_DS = 4, PR_IS = 4, PR_FS = 1;

// The workgroup's accumulators -> its partial row [T]: per tap a wave butterfly, the four waves pairwise.
template <int MAXT>
__device__ __forceinline__ void pr_flush(const double (&acc)[MAXT], int T, double* __restrict__ row) {
  __shared__ double sh[PR_WAVES][MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    if (t < T) {                            // (uniform)
      const double s = vote_wave_sum(acc[t]);
      if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][t] = s;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < T) row[t] = (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]);
}

// ---- launch 7: Hb[r, tb] = sum_{a, b} (taps_b[r, tb] * t1[r, a, b + lb[r] + tb]) * q[r, a, b]
__global__ __launch_bounds__(PR_NT) void vote_pairs_hist_b_kernel(const float* __restrict__ q,
                                                                  const float* __restrict__ t1,
                                                                  const float* __restrict__ taps_b,
                                                                  const int32_t* __restrict__ offsets, int Wo, int P,
                                                                  int Tb, int tiles_per_plane, int gpr,
                                                                  double* __restrict__ part) {
  const int r = blockIdx.x / gpr, g = blockIdx.x - r * gpr;
  const float* w = taps_b + (size_t)r * Tb;                       // uniform over the workgroup, for all its tiles
  const int lb = offsets[(size_t)r * 2 + 1];
  double acc[VP_MAX_TXY];
#pragma unroll
  for (int t = 0; t < VP_MAX_TXY; ++t) acc[t] = 0.0;
  for (int tile = g; tile < tiles_per_plane; tile += gpr) {
    int p, a, b;
    if (!vote_tile_pixel<PR_NT>(tile, P, &p)) continue;
    vote_row_col(p, Wo, &a, &b);
    const float c = q[(int64_t)r * P + p];
    const float* src = t1 + (int64_t)r * P + (int64_t)a * Wo;
    const int64_t first = (int64_t)b + lb;
#pragma unroll
    for (int t = 0; t < VP_MAX_TXY; ++t) {
      if (t < Tb) {
        const int64_t sb = first + t;
        if (sb >= 0 && sb < Wo) acc[t] += (double)((w[t] * src[sb]) * c);
      }
    }
  }
  pr_flush<VP_MAX_TXY>(acc, Tb, part + (size_t)blockIdx.x * Tb);
}

// ---- launch 9: Ha[r, ta] = sum_{a, b} (taps_a[r, ta] * t0[r, a + la[r] + ta, b]) * c0[r, a, b]
__global__ __launch_bounds__(PR_NT) void vote_pairs_hist_a_kernel(const float* __restrict__ c0,
                                                                  const float* __restrict__ t0,
                                                                  const float* __restrict__ taps_a,
                                                                  const int32_t* __restrict__ offsets, int Ho, int Wo,
                                                                  int P, int Ta, int tiles_per_plane, int gpr,
                                                                  double* __restrict__ part) {
  const int r = blockIdx.x / gpr, g = blockIdx.x - r * gpr;
  const float* w = taps_a + (size_t)r * Ta;
  const int la = offsets[(size_t)r * 2];
  double acc[VP_MAX_TXY];
#pragma unroll
  for (int t = 0; t < VP_MAX_TXY; ++t) acc[t] = 0.0;
  for (int tile = g; tile < tiles_per_plane; tile += gpr) {
    int p, a, b;
    if (!vote_tile_pixel<PR_NT>(tile, P, &p)) continue;
    vote_row_col(p, Wo, &a, &b);
    const float c = c0[(int64_t)r * P + p];
    const float* src = t0 + (int64_t)r * P + b;
    const int64_t first = (int64_t)a + la;
#pragma unroll
    for (int t = 0; t < VP_MAX_TXY; ++t) {
      if (t < Ta) {
        const int64_t sa = first + t;
        if (sa >= 0 && sa < Ho) acc[t] += (double)((w[t] * src[sa * Wo]) * c);
      }
    }
  }
  pr_flush<VP_MAX_TXY>(acc, Ta, part + (size_t)blockIdx.x * Ta);
}

// ---- launch 11: Hk[tk] = sum_{r, a, b} (taps_k[tk] * p[(r + lk + tk) mod R, a, b]) * c1[r, a, b], per workgroup; the
// masses are vp_mass of the belief against the fold of the peak launch's maxima, as vp_rotate_kernel forms them
__global__ __launch_bounds__(PR_NT) void vote_pairs_hist_k_kernel(const float* __restrict__ c1,
                                                                  const float* __restrict__ belief,
                                                                  const float* __restrict__ taps_k, int lk, int R, int P,
                                                                  int Tk, int tiles_per_plane, int gpr,
                                                                  const float* __restrict__ fpart, int groups,
                                                                  double* __restrict__ part) {
  __shared__ float shf[PR_WAVES];
  const float M = vote_fold_max<PR_WAVES, PR_FS>(fpart, VP_F_PEAK, groups, shf);
  const int r = blockIdx.x / gpr, g = blockIdx.x - r * gpr;
  int kfirst = r + vote_mod(lk, R);         // (r + lk) mod R
  if (kfirst >= R) kfirst -= R;
  double acc[VP_MAX_TK];
#pragma unroll
  for (int t = 0; t < VP_MAX_TK; ++t) acc[t] = 0.0;
  for (int tile = g; tile < tiles_per_plane; tile += gpr) {
    int p;
    if (!vote_tile_pixel<PR_NT>(tile, P, &p)) continue;
    const float c = c1[(int64_t)r * P + p];
    int k = kfirst;
#pragma unroll
    for (int t = 0; t < VP_MAX_TK; ++t) {
      if (t < Tk) {
        acc[t] += (double)((taps_k[t] * vp_mass(belief[(int64_t)k * P + p], M)) * c);
        k = vote_next(k, R);
      }
    }
  }
  pr_flush<VP_MAX_TK>(acc, Tk, part + (size_t)blockIdx.x * Tk);
}

// The fold of `rows` partial rows [T] by the whole workgroup, COLS columns x (256 / COLS) slices: a strided chain per
// thread, then the slices in index order.  The sum of column t in thread t (< T; the other threads 0).  `sh` [256] is
// free again on return.
template <int COLS>
__device__ __forceinline__ double pr_fold_rows(const double* __restrict__ part, int rows, int T, double* sh) {
  constexpr int SLICES = PR_NT / COLS;
  const int col = threadIdx.x % COLS, slice = threadIdx.x / COLS;
  double v = 0.0;
  if (col < T)
    for (int row = slice; row < rows; row += SLICES) v += part[(size_t)row * T + col];
  sh[threadIdx.x] = v;
  __syncthreads();
  double s = 0.0;
  if (slice == 0 && col < T)
    for (int i = 0; i < SLICES; ++i) s += sh[i * COLS + col];
  __syncthreads();
  return s;
}

// ---- launch 12, one workgroup
__global__ __launch_bounds__(PR_NT) void vote_pairs_finish_kernel(int groups, int R, int gpr, int Tk, int Ta, int Tb,
                                                                  float eps, int n, const double* __restrict__ dpart,
                                                                  const int32_t* __restrict__ ipart,
                                                                  const double* __restrict__ part_k,
                                                                  const double* __restrict__ part_a,
                                                                  const double* __restrict__ part_b,
                                                                  double* __restrict__ hist_k, double* __restrict__ hist_a,
                                                                  double* __restrict__ hist_b, double* __restrict__ stats,
                                                                  int32_t* __restrict__ count) {
  __shared__ double shd[PR_WAVES];
  __shared__ int shi[PR_WAVES];
  __shared__ double sh[PR_NT];
  __shared__ double shk[VP_MAX_TK];
  const int n_mass = vote_fold_sum<PR_WAVES, PR_IS>(ipart, VP_I_MASS, groups, shi);
  const int n_bad = vote_fold_sum<PR_WAVES, PR_IS>(ipart, VP_I_BAD, groups, shi);
  const int n_badnext = vote_fold_sum<PR_WAVES, PR_IS>(ipart, VR_I_BADNEXT, groups, shi);
  const int n_ratio = vote_fold_sum<PR_WAVES, PR_IS>(ipart, VR_I_RATIO, groups, shi);
  const double sum_p = vote_fold_sum<PR_WAVES, PR_DS>(dpart, VP_D_SUMP, groups, shd);
  const double S = vote_fold_sum<PR_WAVES, PR_DS>(dpart, VP_D_SUMT2, groups, shd);
  const double Q = vote_fold_sum<PR_WAVES, PR_DS>(dpart, VR_D_Q, groups, shd);
  const double G = vr_fold_max<PR_DS>(dpart, VR_D_G, groups, shd);
  const double hk = pr_fold_rows<VP_MAX_TK>(part_k, R * gpr, Tk, sh);
  if ((int)threadIdx.x < Tk) shk[threadIdx.x] = hk;
  __syncthreads();
  double H = 0.0;
  for (int t = 0; t < Tk; ++t) H += shk[t];
  const double c = S > 0.0 ? (1.0 - (double)eps) / S : 0.0;
  const double stay_raw = c * H, jump_raw = ((double)eps / (double)n) * Q;
  const double total = stay_raw + jump_raw;
  const bool has = total > 0.0;
  if ((int)threadIdx.x < Tk) hist_k[threadIdx.x] = has ? (c * hk) / total : 0.0;
  for (int r = 0; r < R; ++r) {
    const double ha = pr_fold_rows<VP_MAX_TXY>(part_a + (size_t)r * gpr * Ta, gpr, Ta, sh);
    if ((int)threadIdx.x < Ta) hist_a[(size_t)r * Ta + threadIdx.x] = has ? (c * ha) / total : 0.0;
    const double hb = pr_fold_rows<VP_MAX_TXY>(part_b + (size_t)r * gpr * Tb, gpr, Tb, sh);
    if ((int)threadIdx.x < Tb) hist_b[(size_t)r * Tb + threadIdx.x] = has ? (c * hb) / total : 0.0;
  }
  if (threadIdx.x == 0) {
    stats[0] = has ? stay_raw / total : 0.0;
    stats[1] = has ? jump_raw / total : 0.0;
    stats[2] = has ? G + log(total) : -(double)INFINITY;
    stats[3] = sum_p > 0.0 ? (double)(float)(S / sum_p) : 0.0;   // (the filter's mass_kept: the same expression)
    count[0] = n_mass;
    count[1] = n_bad;
    count[2] = n_badnext;
    count[3] = n_ratio;
  }
}

struct PrPlan : VpPlan {
  int gpr;                                  // workgroups per rotation of the reduction launches
};

bool pr_plan(int R, int Ho, int Wo, int Tk, int Ta, int Tb, PrPlan* plan) {
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, plan)) return false;
  const int per = VP_MAX_GROUPS / R;        // >= 32
  plan->gpr = plan->tiles_per_plane < per ? plan->tiles_per_plane : per;
  return true;
}

// 4 x [R Ho Wo] f32 (A: t0; B: t1, c1; C: t2, c0; D: q) | [groups][4] float64 | [groups][4] int32 | [groups][1] f32 |
// [R gpr][Tk] | [R gpr][Ta] | [R gpr][Tb] float64
struct PrWorkspace {
  float *A, *B, *C, *D;
  double* dpart;
  int32_t* ipart;
  float* fpart;
  double *part_k, *part_a, *part_b;
  size_t bytes;
};

PrWorkspace pr_workspace(const PrPlan& plan, int R, int Tk, int Ta, int Tb, void* workspace) {
  VoteLayout l{workspace};
  const size_t rows = (size_t)R * plan.gpr;
  return {l.take<float>(plan.n), l.take<float>(plan.n), l.take<float>(plan.n), l.take<float>(plan.n),
          l.take<double>((size_t)plan.groups * PR_DS), l.take<int32_t>((size_t)plan.groups * PR_IS),
          l.take<float>((size_t)plan.groups * PR_FS), l.take<double>(rows * Tk), l.take<double>(rows * Ta),
          l.take<double>(rows * Tb), l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_pairs_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta,
                                                  int32_t Tb) {
  PrPlan plan;
  if (!pr_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return 0;
  return pr_workspace(plan, R, Tk, Ta, Tb, nullptr).bytes;
}

extern "C" int snap_vote_pairs_f32(const float* belief, const float* next, const float* taps_k, int32_t lk,
                                   const float* taps_a, const float* taps_b, const int32_t* offsets, int32_t R,
                                   int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb, float uniform_mix,
                                   double* hist_k, double* hist_a, double* hist_b, double* stats, int32_t* count,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!belief || !next || !taps_k || !taps_a || !taps_b || !offsets || !hist_k || !hist_a || !hist_b || !stats ||
      !count || !workspace)
    return SNAP_ERR_NULL;
  PrPlan plan;
  if (!pr_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!(uniform_mix >= 0.f && uniform_mix <= 1.f)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, pr_workspace(plan, R, Tk, Ta, Tb, nullptr).bytes))
    return SNAP_ERR_WORKSPACE;
  const PrWorkspace w = pr_workspace(plan, R, Tk, Ta, Tb, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 rgrid(R * plan.gpr), block(PR_NT);
  const int P = plan.P, tpp = plan.tiles_per_plane, gpr = plan.gpr;
  const VpTaps taps = {taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb};
  const VpParts<PR_FS, PR_DS, PR_IS> part = {w.fpart, w.dpart, w.ipart};
  VP_CHECK(vp_launch_predict(plan, taps, belief, w.A, w.B, w.C, part, s));   // t0, t1, t2
  VP_CHECK(vr_launch_ratio(plan, w.C, next, uniform_mix, w.D, part, s));     // q
  hipLaunchKernelGGL(vote_pairs_hist_b_kernel, rgrid, block, 0, s, w.D, w.B, taps_b, offsets, Wo, P, Tb, tpp, gpr,
                     w.part_b);
  SNAP_CHECK_LAUNCH();
  VP_CHECK(vp_launch_cols<true>(plan, taps, w.D, w.C, part, s));               // c0
  hipLaunchKernelGGL(vote_pairs_hist_a_kernel, rgrid, block, 0, s, w.C, w.A, taps_a, offsets, Ho, Wo, P, Ta, tpp, gpr,
                     w.part_a);
  SNAP_CHECK_LAUNCH();
  VP_CHECK(vp_launch_rows<true>(plan, taps, w.C, w.B, s));                     // c1
  hipLaunchKernelGGL(vote_pairs_hist_k_kernel, rgrid, block, 0, s, w.B, belief, taps_k, lk, R, P, Tk, tpp, gpr, w.fpart,
                     plan.groups, w.part_k);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_pairs_finish_kernel, dim3(1), block, 0, s, plan.groups, R, gpr, Tk, Ta, Tb, uniform_mix,
                     plan.n, w.dpart, w.ipart, w.part_k, w.part_a, w.part_b, hist_k, hist_a, hist_b, stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
