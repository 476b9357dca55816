// Recursive pose filter over exhaustive vote volumes: snap_vote_filter_f32 (include/snap_hip.h).
//
// belief [R, Ho, Wo] f32 is the log-space belief after the previous frame (-inf = impossible pose), votes [R, Ho, Wo]
// the new frame's vote volume.  PREDICT: the belief's masses p = exp(belief - M) are transported and diffused by three
// separable tap passes (rotation, circular; rows and columns with the OUTPUT rotation's tables, as in vote_fuse) into
// t2, S = sum t2.  UPDATE: u = scale * votes + log((1 - eps) t2 / S + eps / n), belief_out = u - logsumexp(u).
//
// A tile is one rotation and 256 consecutive pixels p = a * Wo + b, one cell per thread; every launch has
// min(tiles, 2048) workgroups of 256 threads striding over the tiles (the tap rows of a tile are uniform: scalar loads).
// Launches 1-4 are the predict step, vp_launch_predict; its kernels live in vote_predict.h:
// Launch 1 (vp_peak_kernel):   per workgroup the largest finite belief and the count of NaN / +inf cells.
// Launch 2 (vp_rotate_kernel): every workgroup folds the partial maxima into M (a maximum: exact, the same
//   bits everywhere); t0 = the k-tap chain over p, exp fused (a source cell's exp is recomputed by each of its <= Tk
//   readers: the re-reads of the belief are L2 hits, t0 is the only store); sum p (float64) and the count of cells
//   with mass from each thread's own cell.  t0 lives in belief_out.
// Launch 3 (vp_rows_kernel):   t1 = the a-tap chain over t0 (each tap a wave-contiguous run of a source row),
//   into the workspace.
// Launch 4 (vp_cols_kernel):   t2 = the b-tap chain over t1, into belief_out; per workgroup sum t2 (float64).
// Launch 5 (vote_filter_evidence_kernel): every workgroup folds the partial sums into S; per cell u (float64), folded
//   into a running (maximum, sum of exp relative to it) pair per thread, then per workgroup.
// Launch 6 (vote_filter_normalise_kernel): every workgroup folds the pairs into log_z, recomputes u (the same
//   expression: the same bits) and writes belief_out = fl32(u - log_z) over t2 in place; per workgroup the counts of
//   finite / NaN cells written and their maximum.  Workgroup 0 writes stats[0].
// Launch 7 (vote_filter_finish_kernel, one workgroup): the remaining stats and count.
// With belief == NULL launches 1-4 are skipped (uniform prior).  No atomics and no inter-workgroup hand-off inside a
// launch: every sum is a per-thread chain over its tiles, a wave tree, the four waves, then the workgroups in a strided
// chain per thread and the same tree -- an order fixed by (R, Ho, Wo) alone.
// HBM traffic (n = R Ho Wo cells of 4 bytes): reads belief 2 (+ L2 re-reads), t0, t1, t2 twice, votes twice; writes
// t0, t1, t2, belief_out: 12 n cells with a belief, 3 n without.
#include "vote_predict.h"

namespace {

constexpr int FL_NT = VP_NT;                // threads = cells of a tile
constexpr int FL_WAVES = VP_WAVES;

// per-workgroup partials: double [groups][4], int32 [groups][4], float [groups][2]; the predict step's columns first
constexpr int FL_DS = 4, FL_IS = 4, FL_FS = 2;
enum { FL_D_SUMP = VP_D_SUMP, FL_D_SUMT2 = VP_D_SUMT2, FL_D_LSE_M = 2, FL_D_LSE_S = 3 };
enum { FL_I_BAD = VP_I_BAD, FL_I_MASS = VP_I_MASS, FL_I_FIN = 2, FL_I_NAN = 3 };
enum { FL_F_PEAK = VP_F_PEAK, FL_F_OUTMAX = 1 };

// The update of one cell, float64: u = scale * vote + log(prior), prior = (1 - eps) t2 / S + eps / n.  NaN for a NaN
// or +inf vote, -inf for a -inf vote or a prior of 0.  `transported` = (1 - eps) / S is NOT folded into one factor:
// the expression is ((1 - eps) * t2) / S + eps / n as the contract writes it.
struct FlUpdate {
  double scale;
  VpPrior prior;
};
__device__ __forceinline__ double fl_update(const FlUpdate& c, float t2, float vote) {
  if (!(vote < INFINITY)) return (double)__int_as_float(0x7fc00000);   // NaN or +inf
  if (vote == -INFINITY) return -(double)INFINITY;
  const double prior = vp_prior(c.prior, t2);
  if (!(prior > 0.0)) return -(double)INFINITY;
  return c.scale * (double)vote + log(prior);
}
__device__ __forceinline__ FlUpdate fl_update_setup(const double* dpart, int groups, bool with_belief, float scale,
                                                    float eps, int n, double* sh) {
  FlUpdate c;
  c.scale = (double)scale;
  c.prior = vp_prior_setup(with_belief ? vote_fold_sum<FL_WAVES, FL_DS>(dpart, FL_D_SUMT2, groups, sh) : 0.0,
                           with_belief, eps, n);
  return c;
}

// ---- launch 5
__global__ __launch_bounds__(FL_NT) void vote_filter_evidence_kernel(const float* __restrict__ t2,
                                                                     const float* __restrict__ votes, int n,
                                                                     int with_belief, float scale, float eps,
                                                                     double* __restrict__ dpart) {
  __shared__ double shd[FL_WAVES];
  __shared__ double shl[FL_WAVES][2];
  const FlUpdate c = fl_update_setup(dpart, gridDim.x, with_belief != 0, scale, eps, n, shd);
  double m = -(double)INFINITY, s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * FL_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * FL_NT) {
    const double u = fl_update(c, with_belief ? t2[i] : 0.f, votes[i]);
    if (fabs(u) < (double)INFINITY) vote_lse_add(&m, &s, u);
  }
  vote_block_lse<FL_WAVES>(&m, &s, shl);
  if (threadIdx.x == 0) {
    dpart[(size_t)blockIdx.x * FL_DS + FL_D_LSE_M] = m;
    dpart[(size_t)blockIdx.x * FL_DS + FL_D_LSE_S] = s;
  }
}

// ---- launch 6
__global__ __launch_bounds__(FL_NT) void vote_filter_normalise_kernel(const float* __restrict__ votes, int n,
                                                                      int with_belief, float scale, float eps,
                                                                      const double* __restrict__ dpart,
                                                                      float* __restrict__ belief_out,
                                                                      float* __restrict__ fpart, int32_t* __restrict__ ipart,
                                                                      float* __restrict__ stats) {
  __shared__ double shd[FL_WAVES];
  __shared__ double shl[FL_WAVES][2];
  __shared__ float shf[FL_WAVES];
  __shared__ int shi[FL_WAVES];
  const FlUpdate c = fl_update_setup(dpart, gridDim.x, with_belief != 0, scale, eps, n, shd);
  const double log_z = vote_fold_lse<FL_WAVES, FL_DS>(dpart, FL_D_LSE_M, FL_D_LSE_S, gridDim.x, shl);
  float top = -INFINITY;
  int n_fin = 0, n_nan = 0;
  for (int64_t i = (int64_t)blockIdx.x * FL_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * FL_NT) {
    const double u = fl_update(c, with_belief ? belief_out[i] : 0.f, votes[i]);   // (t2 lives in belief_out)
    const float out = vote_normalised(u, log_z);
    belief_out[i] = out;
    n_fin += vote_finite(out) ? 1 : 0;
    n_nan += out != out ? 1 : 0;
    top = fmaxf(top, out);                  // (fmaxf drops a NaN)
  }
  top = vote_block_max<FL_WAVES>(top, shf);
  n_fin = vote_block_sum<FL_WAVES>(n_fin, shi);
  n_nan = vote_block_sum<FL_WAVES>(n_nan, shi);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * FL_FS + FL_F_OUTMAX] = top;
    ipart[(size_t)blockIdx.x * FL_IS + FL_I_FIN] = n_fin;
    ipart[(size_t)blockIdx.x * FL_IS + FL_I_NAN] = n_nan;
    if (blockIdx.x == 0) stats[0] = (float)log_z;
  }
}

// ---- launch 7
__global__ __launch_bounds__(FL_NT) void vote_filter_finish_kernel(int groups, int with_belief,
                                                                   const double* __restrict__ dpart,
                                                                   const float* __restrict__ fpart,
                                                                   const int32_t* __restrict__ ipart,
                                                                   float* __restrict__ stats, int32_t* __restrict__ count) {
  __shared__ double shd[FL_WAVES];
  __shared__ float shf[FL_WAVES];
  __shared__ int shi[FL_WAVES];
  const int n_fin = vote_fold_sum<FL_WAVES, FL_IS>(ipart, FL_I_FIN, groups, shi);
  const int n_nan = vote_fold_sum<FL_WAVES, FL_IS>(ipart, FL_I_NAN, groups, shi);
  const float top = vote_fold_max<FL_WAVES, FL_FS>(fpart, FL_F_OUTMAX, groups, shf);
  int n_bad = 0, n_mass = 0;
  float M = -INFINITY, kept = 1.f;
  if (with_belief) {
    n_bad = vote_fold_sum<FL_WAVES, FL_IS>(ipart, FL_I_BAD, groups, shi);
    n_mass = vote_fold_sum<FL_WAVES, FL_IS>(ipart, FL_I_MASS, groups, shi);
    M = vote_fold_max<FL_WAVES, FL_FS>(fpart, FL_F_PEAK, groups, shf);
    const double sum_p = vote_fold_sum<FL_WAVES, FL_DS>(dpart, FL_D_SUMP, groups, shd);
    const double S = vote_fold_sum<FL_WAVES, FL_DS>(dpart, FL_D_SUMT2, groups, shd);
    kept = sum_p > 0.0 ? (float)(S / sum_p) : 0.f;
  }
  if (threadIdx.x == 0) {
    stats[1] = kept;
    stats[2] = M;
    stats[3] = top;
    count[0] = n_fin;
    count[1] = n_bad;
    count[2] = n_nan;
    count[3] = n_mass;
  }
}

// [R Ho Wo] f32 t1 | [groups][4] float64 | [groups][4] int32 | [groups][2] f32
struct FlWorkspace {
  float* t1;
  double* dpart;
  int32_t* ipart;
  float* fpart;
  size_t bytes;
};

FlWorkspace fl_workspace(const VpPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<float>(plan.n), l.take<double>((size_t)plan.groups * FL_DS),
          l.take<int32_t>((size_t)plan.groups * FL_IS), l.take<float>((size_t)plan.groups * FL_FS), l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_filter_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta,
                                                   int32_t Tb) {
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return 0;
  return fl_workspace(plan, nullptr).bytes;
}

extern "C" int snap_vote_filter_f32(const float* belief, const float* votes, const float* taps_k, int32_t lk,
                                    const float* taps_a, const float* taps_b, const int32_t* offsets, int32_t R,
                                    int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb, float scale,
                                    float uniform_mix, float* belief_out, float* stats, int32_t* count, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (!votes || !taps_k || !taps_a || !taps_b || !offsets || !belief_out || !stats || !count || !workspace)
    return SNAP_ERR_NULL;
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale > 0.f) || !(scale < INFINITY)) return SNAP_ERR_UNSUPPORTED;
  if (!(uniform_mix >= 0.f && uniform_mix <= 1.f)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, fl_workspace(plan, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const FlWorkspace w = fl_workspace(plan, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(plan.groups), block(FL_NT);
  const int with_belief = belief != nullptr ? 1 : 0;
  if (with_belief) {
    const VpTaps taps = {taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb};
    const VpParts<FL_FS, FL_DS, FL_IS> part = {w.fpart, w.dpart, w.ipart};
    VP_CHECK(vp_launch_predict(plan, taps, belief, belief_out, w.t1, belief_out, part, s));   // t0, t1, t2
  }
  hipLaunchKernelGGL(vote_filter_evidence_kernel, grid, block, 0, s, belief_out, votes, plan.n, with_belief, scale,
                     uniform_mix, w.dpart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_filter_normalise_kernel, grid, block, 0, s, votes, plan.n, with_belief, scale, uniform_mix,
                     w.dpart, belief_out, w.fpart, w.ipart, stats);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_filter_finish_kernel, dim3(1), block, 0, s, plan.groups, with_belief, w.dpart, w.fpart,
                     w.ipart, stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
