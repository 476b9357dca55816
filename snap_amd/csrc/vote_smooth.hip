// Backward smoothing step of the vote-volume filter: snap_vote_smooth_f32 (include/snap_hip.h).
//
// belief [R, Ho, Wo] f32 = log alpha_t, the filter's output at frame t; next [R, Ho, Wo] f32 = log gamma_{t+1}, the
// smoothed belief of frame t + 1; the taps the filter used from t to t + 1; eps = uniform_mix; n = R Ho Wo.
// PREDICT, the filter's own code (vote_predict.h): M, the masses p, t0, t1, t2, S = sum t2, sum p, and per cell
// prior = ((1 - eps) t2) / S + eps / n: the filter's bits.  RATIO, float64 (vote_ratio.h, shared with vote_pairs.hip):
// lg = next - log(prior) where next is finite and prior > 0, G = max lg, q = fl32(exp(lg - G)) where
// fl32(lg - G) >= -40, else 0, Q = sum q.  ADJOINT transport,
// three gathers, the xy passes first with their own rotation's tables, the rotation pass last:
//   c1[r, a, b] = sum_tb taps_b[r, tb] q [r, a, b - lb[r] - tb];
//   c0[r, a, b] = sum_ta taps_a[r, ta] c1[r, a - la[r] - ta, b];
//   u [k, a, b] = sum_tk taps_k[tk] c0[(k - lk - tk) mod R, a, b];
// each an f32 fma chain from 0 over the SOURCE cell ascending (a - la - (Ta - 1), ..., a - la: the tap index descends;
// in k: (k - lk - (Tk - 1) + i) mod R for i = 0 .. Tk - 1, ascending before the modulo), sources outside the volume
// skipped, the intermediates stored as f32.  COMBINE, float64: h = ((1 - eps) (sum p / S)) u + (eps / n) Q,
// w = (belief + G) + log(h), smoothed = fl32(w - log_norm), log_norm = log sum exp(w) over the finite cells.
//
// A tile is one rotation and 256 consecutive pixels p = a * Wo + b, one cell per thread; every launch has
// min(tiles, 2048) workgroups of 256 threads striding over the tiles (the tap rows of a tile are uniform: scalar loads).
// Launches 1-4 (vp_launch_predict: vp_peak / rotate / rows / cols_kernel of vote_predict.h): the filter's launches
//   1-4.  t0 and t2 live in `smoothed`, t1 in the workspace.
// Launches 5-6 are vr_launch_ratio; its kernels live in vote_ratio.h:
// Launch 5 (vr_max_kernel):   every workgroup folds the partial sums into S; per cell lg; per workgroup the
//   largest lg (float64), the count of NaN / +inf cells of `next` and of cells with ratio mass.
// Launch 6 (vr_mass_kernel):  every workgroup folds the maxima into G (a maximum: exact), recomputes lg (the
//   same expression: the same bits) and writes q into the workspace, ONCE: the float64 log and exp sit on this pass, not
//   on the taps; per workgroup sum q (float64).
// Launch 7 (vp_launch_cols<true>: vp_cols_kernel with ADJ): c1 = the adjoint b chain over q, into `smoothed`.
// Launch 8 (vp_launch_rows<true>: vp_rows_kernel with ADJ): c0 = the adjoint a chain over c1, into the workspace.
// Launch 9 (vote_smooth_gather_kernel):  every workgroup folds sum p, S, Q and G; u = the adjoint k chain over c0 (the
//   re-reads of c0 by a cell's <= Tk readers are L2 hits), into `smoothed`; per cell w (float64), folded into a running
//   (maximum, sum of exp relative to it) pair per thread, then per workgroup.
// Launch 10 (vote_smooth_normalise_kernel): every workgroup folds the pairs into log_norm, recomputes w (the same
//   expression: the same bits) and writes smoothed = fl32(w - log_norm) over u in place; per workgroup the count of
//   finite cells written and their maximum.  Workgroup 0 writes stats[0].
// Launch 11 (vote_smooth_finish_kernel, one workgroup): the remaining stats and count.
// No atomics and no inter-workgroup hand-off inside a launch: every sum is a per-thread chain over its tiles, a wave
// tree, the four waves, then the workgroups in a strided chain per thread and the same tree -- an order fixed by
// (R, Ho, Wo) alone.
// HBM traffic (n = R Ho Wo cells of 4 bytes): reads belief 4 (+ L2 re-reads), next 2, t0, t1, t2 twice, q, c1, c0
// (+ L2 re-reads), u; writes t0, t1, t2, q, c1, c0, u, smoothed: 22 n cells (the filter: 12).
#include "vote_ratio.h"

namespace {

constexpr int SM_NT = VP_NT;
constexpr int SM_WAVES = VP_WAVES;

// per-workgroup partials: double [groups][6], int32 [groups][5], float [groups][2]; the predict step's columns first
constexpr int SM_DS = 6, SM_IS = 5, SM_FS = 2;
enum { SM_D_SUMP = VP_D_SUMP, SM_D_SUMT2 = VP_D_SUMT2, SM_D_G = VR_D_G, SM_D_Q = VR_D_Q, SM_D_LSE_M = 4, SM_D_LSE_S = 5 };
enum { SM_I_BAD = VP_I_BAD, SM_I_MASS = VP_I_MASS, SM_I_BADNEXT = VR_I_BADNEXT, SM_I_RATIO = VR_I_RATIO, SM_I_FIN = 4 };
enum { SM_F_PEAK = VP_F_PEAK, SM_F_OUTMAX = 1 };

// The combination of one cell, float64: w = (belief + G) + log(h), h = ((1 - eps) (sum p / S)) u + (eps / n) Q.  NaN
// for a NaN or +inf belief, -inf for a -inf belief or h == 0 (then G, which may be -inf, is not read).
struct SmCombine {
  double carried, uniform, G;               // (1 - eps) (sum p / S), 0 when S == 0; (eps / n) Q
};
__device__ __forceinline__ double sm_combine(const SmCombine& c, float u, float belief) {
  if (!(belief < INFINITY)) return (double)__int_as_float(0x7fc00000);   // NaN or +inf
  if (belief == -INFINITY) return -(double)INFINITY;
  const double h = c.carried * (double)u + c.uniform;
  if (!(h > 0.0)) return -(double)INFINITY;
  return ((double)belief + c.G) + log(h);
}
__device__ __forceinline__ SmCombine sm_combine_setup(const double* __restrict__ dpart, int groups, float eps, int n,
                                                      double* sh) {
  const double sum_p = vote_fold_sum<SM_WAVES, SM_DS>(dpart, SM_D_SUMP, groups, sh);
  const double S = vote_fold_sum<SM_WAVES, SM_DS>(dpart, SM_D_SUMT2, groups, sh);
  const double Q = vote_fold_sum<SM_WAVES, SM_DS>(dpart, SM_D_Q, groups, sh);
  SmCombine c;
  c.carried = S > 0.0 ? (1.0 - (double)eps) * (sum_p / S) : 0.0;
  c.uniform = ((double)eps / (double)n) * Q;
  c.G = vr_fold_max<SM_DS>(dpart, SM_D_G, groups, sh);
  return c;
}

// ---- launch 9: u[k, a, b] = sum_tk taps_k[tk] * c0[(k - lk - tk) mod R, a, b]; the pairs of w
__global__ __launch_bounds__(SM_NT) void vote_smooth_gather_kernel(const float* __restrict__ c0,
                                                                   const float* __restrict__ belief,
                                                                   const float* __restrict__ taps_k, int lk, int R, int P,
                                                                   int Tk, int tiles_per_plane, int tiles, float eps, int n,
                                                                   float* __restrict__ u, double* __restrict__ dpart) {
  __shared__ double shd[SM_WAVES];
  __shared__ double shl[SM_WAVES][2];
  const SmCombine c = sm_combine_setup(dpart, gridDim.x, eps, n, shd);
  // (k - lk - (Tk - 1)) mod R, mathematically, in 64 bits: lk is any int32
  const int kfirst = (int)(((-(int64_t)lk - (Tk - 1)) % R + R) % R);
  double m = -(double)INFINITY, s = 0.0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p;
    if (!vote_tile_cell<SM_NT>(tile, tiles_per_plane, P, &r, &p)) continue;
    int k = r + kfirst;                     // (>= 0: one side of vote_wrap)
    if (k >= R) k -= R;
    float acc = 0.f;
    for (int i = 0; i < Tk; ++i) {
      acc = fmaf(taps_k[Tk - 1 - i], c0[(int64_t)k * P + p], acc);
      k = vote_next(k, R);
    }
    u[(int64_t)r * P + p] = acc;
    const double w = sm_combine(c, acc, belief[(int64_t)r * P + p]);
    if (fabs(w) < (double)INFINITY) vote_lse_add(&m, &s, w);
  }
  vote_block_lse<SM_WAVES>(&m, &s, shl);
  if (threadIdx.x == 0) {
    dpart[(size_t)blockIdx.x * SM_DS + SM_D_LSE_M] = m;
    dpart[(size_t)blockIdx.x * SM_DS + SM_D_LSE_S] = s;
  }
}

// ---- launch 10
__global__ __launch_bounds__(SM_NT) void vote_smooth_normalise_kernel(const float* __restrict__ belief, int n, float eps,
                                                                      const double* __restrict__ dpart,
                                                                      float* __restrict__ smoothed,
                                                                      float* __restrict__ fpart, int32_t* __restrict__ ipart,
                                                                      float* __restrict__ stats) {
  __shared__ double shd[SM_WAVES];
  __shared__ double shl[SM_WAVES][2];
  __shared__ float shf[SM_WAVES];
  __shared__ int shi[SM_WAVES];
  const SmCombine c = sm_combine_setup(dpart, gridDim.x, eps, n, shd);
  const double log_norm = vote_fold_lse<SM_WAVES, SM_DS>(dpart, SM_D_LSE_M, SM_D_LSE_S, gridDim.x, shl);
  float top = -INFINITY;
  int n_fin = 0;
  for (int64_t i = (int64_t)blockIdx.x * SM_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * SM_NT) {
    const double w = sm_combine(c, smoothed[i], belief[i]);   // (u lives in smoothed)
    const float out = vote_normalised(w, log_norm);
    smoothed[i] = out;
    n_fin += vote_finite(out) ? 1 : 0;
    top = fmaxf(top, out);                  // (fmaxf drops a NaN)
  }
  top = vote_block_max<SM_WAVES>(top, shf);
  n_fin = vote_block_sum<SM_WAVES>(n_fin, shi);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * SM_FS + SM_F_OUTMAX] = top;
    ipart[(size_t)blockIdx.x * SM_IS + SM_I_FIN] = n_fin;
    if (blockIdx.x == 0) stats[0] = (float)log_norm;
  }
}

// ---- launch 11
__global__ __launch_bounds__(SM_NT) void vote_smooth_finish_kernel(int groups, const double* __restrict__ dpart,
                                                                   const float* __restrict__ fpart,
                                                                   const int32_t* __restrict__ ipart,
                                                                   float* __restrict__ stats, int32_t* __restrict__ count) {
  __shared__ double shd[SM_WAVES];
  __shared__ float shf[SM_WAVES];
  __shared__ int shi[SM_WAVES];
  const int n_fin = vote_fold_sum<SM_WAVES, SM_IS>(ipart, SM_I_FIN, groups, shi);
  const int n_bad = vote_fold_sum<SM_WAVES, SM_IS>(ipart, SM_I_BAD, groups, shi);
  const int n_badnext = vote_fold_sum<SM_WAVES, SM_IS>(ipart, SM_I_BADNEXT, groups, shi);
  const int n_ratio = vote_fold_sum<SM_WAVES, SM_IS>(ipart, SM_I_RATIO, groups, shi);
  const float top = vote_fold_max<SM_WAVES, SM_FS>(fpart, SM_F_OUTMAX, groups, shf);
  const double sum_p = vote_fold_sum<SM_WAVES, SM_DS>(dpart, SM_D_SUMP, groups, shd);
  const double S = vote_fold_sum<SM_WAVES, SM_DS>(dpart, SM_D_SUMT2, groups, shd);
  const double G = vr_fold_max<SM_DS>(dpart, SM_D_G, groups, shd);
  if (threadIdx.x == 0) {
    stats[1] = sum_p > 0.0 ? (float)(S / sum_p) : 0.f;   // (the filter's mass_kept: the same expression)
    stats[2] = (float)G;
    stats[3] = top;
    count[0] = n_fin;
    count[1] = n_bad;
    count[2] = n_badnext;
    count[3] = n_ratio;
  }
}

// [R Ho Wo] f32 (t1, q, c0) | [groups][6] float64 | [groups][5] int32 | [groups][2] f32
struct SmWorkspace {
  float* vol;
  double* dpart;
  int32_t* ipart;
  float* fpart;
  size_t bytes;
};

SmWorkspace sm_workspace(const VpPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<float>(plan.n), l.take<double>((size_t)plan.groups * SM_DS),
          l.take<int32_t>((size_t)plan.groups * SM_IS), l.take<float>((size_t)plan.groups * SM_FS), l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_smooth_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta,
                                                   int32_t Tb) {
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return 0;
  return sm_workspace(plan, nullptr).bytes;
}

extern "C" int snap_vote_smooth_f32(const float* belief, const float* next, const float* taps_k, int32_t lk,
                                    const float* taps_a, const float* taps_b, const int32_t* offsets, int32_t R,
                                    int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb, float uniform_mix,
                                    float* smoothed, float* stats, int32_t* count, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (!belief || !next || !taps_k || !taps_a || !taps_b || !offsets || !smoothed || !stats || !count || !workspace)
    return SNAP_ERR_NULL;
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!(uniform_mix >= 0.f && uniform_mix <= 1.f)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, sm_workspace(plan, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const SmWorkspace w = sm_workspace(plan, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(plan.groups), block(SM_NT);
  const VpTaps taps = {taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb};
  const VpParts<SM_FS, SM_DS, SM_IS> part = {w.fpart, w.dpart, w.ipart};
  VP_CHECK(vp_launch_predict(plan, taps, belief, smoothed, w.vol, smoothed, part, s));   // t0, t1, t2
  VP_CHECK(vr_launch_ratio(plan, smoothed, next, uniform_mix, w.vol, part, s));          // q
  VP_CHECK(vp_launch_cols<true>(plan, taps, w.vol, smoothed, part, s));                    // c1
  VP_CHECK(vp_launch_rows<true>(plan, taps, smoothed, w.vol, s));                          // c0
  hipLaunchKernelGGL(vote_smooth_gather_kernel, grid, block, 0, s, w.vol, belief, taps_k, lk, R, plan.P, Tk,
                     plan.tiles_per_plane, plan.tiles, uniform_mix, plan.n, smoothed, w.dpart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_smooth_normalise_kernel, grid, block, 0, s, belief, plan.n, uniform_mix, w.dpart, smoothed,
                     w.fpart, w.ipart, stats);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_smooth_finish_kernel, dim3(1), block, 0, s, plan.groups, w.dpart, w.fpart, w.ipart, stats,
                     count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
