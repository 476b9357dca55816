// The motion between two frames from their votes: snap_vote_odometry_f32 (include/snap_hip.h).
//
// prev [R, Ho, Wo] f32 is the pose distribution of the previous frame in log space (a filter belief, or a vote volume
// with its temperature as scale_prev), cur [R, Ho, Wo] f32 the current frame's votes.  With the masses p of prev and q
// of cur (the filter's PREDICT rule with a scale: M = the largest finite cell, d = v - M one f32 subtraction, mass =
// fl32(exp((double)scale * (double)d)) iff that product is >= -40 and v is finite, else 0), the TABLE
//   T[k][r][i][j] = sum over (a, b) of q[r, a, b] * p[(r + k) mod R, a + i, b + j],  |k| <= Kr, |i|, |j| <= S,
// is the agreement of the two distributions as a function of the integer index shift between them (motion_taps'
// indexing: the current pose (r, a, b) has its previous pose at (r + dk, a + da(r), b + db(r))).  Both factors are f32,
// so every product is exact in float64 and T is a sum of exact non-negative terms: only its order can move a bit.
//
//   launch 1  vote_odometry_max_kernel    grid (groups, 2): the largest finite cell and the NaN / +inf count of each
//                                         volume, per workgroup
//   launch 2  vote_odometry_mass_kernel   grid (groups, 2): the masses as f32 volumes in the workspace, the float64 sum
//             and the count of cells with mass per workgroup.  The masses are materialised ONCE: staged from the inputs,
//             a cell's float64 exp would be evaluated again by every one of the (2 Kr + 1) x (overlapping halos)
//             workgroups that read it, which at S = 16 costs half as much again as the products themselves.
//   launch 3  vote_odometry_corr_kernel   THE HOT KERNEL.  A workgroup of 256 threads owns one (k, r) and a band of
//             2 TH rows, and walks the band's tiles of TH x 64 cells.  Per tile the q tile and the (TH + 2 S) x
//             (64 + 2 S) halo of p go to LDS as f32 (zeros outside the plane); a tile whose q or p is all zero is
//             skipped (it adds exact zeros).  Thread t = ib * W + jx (W = 2 S + 1) keeps the NACC accumulators
//             (i = ib * NACC + m - S, j = jx - S), m < NACC, in float64 registers.  It walks the tile's columns b and,
//             per column, the rows a: the NACC values p[a + i_m, b + j] it needs are a sliding window down one LDS
//             column, so a step costs ONE LDS read of p (lanes = consecutive j: consecutive banks), one broadcast read
//             of q[a, b] and NACC fmas; the window lives in registers that rotate by unrolling (no moves).  A q of 0
//             skips the step's fmas (a scalar branch).  NACC is the smallest of {1, 2, 3, 5, 7, 10, 13, 17, 22} with
//             W * ceil(W / NACC) <= 256, TH = NACC * max(1, 16 / NACC).  Band partials go to the workspace.
//   launch 4  vote_odometry_table_kernel  one thread per table entry folds its partials in band order: T (float64, kept
//             for launch 5) and log_table = fl32((log T - log zp) - log zq).
//   launch 5  vote_odometry_cand_kernel   (U > 0) one thread per candidate: E[u] = sum over r = 0 .. R-1 of
//             T[shifts[u, r]]; log_evidence; per workgroup the (maximum, lowest u), a log-sum-exp pair and counts.
//   launch 6  vote_odometry_finish_kernel one workgroup: best, stats, count.
// LDS of a hot workgroup (TH x 64 + (TH + IB NACC - 1) x (64 + 2 S) f32, IB = ceil(W / NACC)): 8.1 KB at S = 1, 22.7 KB
// at S = 16 (7 workgroups = 28 waves per 160 KiB CU), 50.2 KB at S = 32 (3 workgroups = 12 waves).  Registers: the
// accumulators are 2 NACC VGPRs, the window stays f32 until it is used: 42 VGPRs at S = 16 (8 waves per SIMD), 108 at
// S = 32 (4).  The float64 fma issues at 16 lanes per clock and SIMD, the LDS serves 32 lanes per clock and CU for
// ds_read_b32: with NACC >= 3 the reads (1 + 1 per NACC fmas) are under the fma time.
// Measured at R = 36, 511 x 511, Kr = 2, S = 16, every unmasked cell with mass: 3.6 ms per call, 29 % of the float64
// vector rate (profiles/vote_odometry_bench.json); untuned.
// Workspace at R = 36, 511 x 511, Kr = 2, S = 16 (TH = 15, 18 bands): two f32 mass volumes 75.2 MB + 18 x 180 x 1089
// float64 band partials 28.2 MB + T 1.6 MB + partials = 105.1 MB.
// No atomics; every float64 sum's order is a function of the shape arguments alone (a thread's chain over its tiles,
// columns and rows; the bands in order; r = 0 .. R-1), so two calls give the same bytes.
#include "vote_common.h"

namespace {

constexpr int OD_NT = 256;
constexpr int OD_WAVES = OD_NT / SNAP_WAVE;
constexpr int OD_MAX_R = 64;
constexpr int OD_MAX_S = 32;
constexpr int OD_MAX_GROUPS = 1024;         // workgroups per volume of launches 1, 2 and of launch 5
constexpr int OD_TW = 64;                   // columns of a tile
constexpr int OD_BAND_TILES = 2;            // row tiles of a band
constexpr double OD_CUT = -40.0;            // a cell carries mass iff scale * (value - peak) >= OD_CUT

// The mass of a cell relative to the peak M (vote_predict.h's vp_mass with a scale).
__device__ __forceinline__ float od_mass(float v, float M, double scale) {
  const float d = v - M;
  const double x = scale * (double)d;
  return (vote_finite(v) && x >= OD_CUT) ? (float)exp(x) : 0.f;
}

// ---- launch 1: blockIdx.y = volume (0 prev, 1 cur): the largest finite cell, the NaN / +inf count
__global__ __launch_bounds__(OD_NT) void vote_odometry_max_kernel(const float* __restrict__ prev,
                                                                  const float* __restrict__ cur, int P, int tpp,
                                                                  int tiles, float* __restrict__ fpart,
                                                                  int32_t* __restrict__ cbad) {
  __shared__ float shm[OD_WAVES];
  __shared__ int shi[OD_WAVES];
  const float* __restrict__ v0 = blockIdx.y == 0 ? prev : cur;
  float m = -INFINITY;
  int n_bad = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p;
    if (vote_tile_cell<OD_NT>(tile, tpp, P, &r, &p)) {
      const float v = v0[(size_t)r * P + p];
      if (vote_finite(v)) {
        m = fmaxf(m, v);
      } else if (!(v == -INFINITY)) {
        ++n_bad;                            // NaN or +inf
      }
    }
  }
  m = vote_block_max<OD_WAVES>(m, shm);
  n_bad = vote_block_sum<OD_WAVES>(n_bad, shi);
  if (threadIdx.x == 0) {
    fpart[blockIdx.y * OD_MAX_GROUPS + blockIdx.x] = m;
    cbad[blockIdx.y * OD_MAX_GROUPS + blockIdx.x] = n_bad;
  }
}

// ---- launch 2: the mass volumes, their sums and the counts of cells with mass
__global__ __launch_bounds__(OD_NT) void vote_odometry_mass_kernel(const float* __restrict__ prev,
                                                                   const float* __restrict__ cur, int P, int tpp,
                                                                   int tiles, float scale_prev, float scale_cur,
                                                                   const float* __restrict__ fpart,
                                                                   float* __restrict__ mass, size_t cells,
                                                                   double* __restrict__ dpart,
                                                                   int32_t* __restrict__ cmass) {
  __shared__ float shm[OD_WAVES];
  __shared__ double shd[OD_WAVES];
  __shared__ int shi[OD_WAVES];
  const int which = blockIdx.y;
  const float* __restrict__ v0 = which == 0 ? prev : cur;
  float* __restrict__ out = mass + (size_t)which * cells;
  const double scale = (double)(which == 0 ? scale_prev : scale_cur);
  const float M = vote_fold_max<OD_WAVES, 1>(fpart + which * OD_MAX_GROUPS, 0, gridDim.x, shm);
  double s = 0.0;
  int n_mass = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p;
    if (vote_tile_cell<OD_NT>(tile, tpp, P, &r, &p)) {
      const float e = od_mass(v0[(size_t)r * P + p], M, scale);   // (M = -inf: no cell is finite, every mass is 0)
      out[(size_t)r * P + p] = e;
      s += (double)e;
      n_mass += e > 0.f ? 1 : 0;
    }
  }
  s = vote_block_sum<OD_WAVES>(s, shd);
  n_mass = vote_block_sum<OD_WAVES>(n_mass, shi);
  if (threadIdx.x == 0) {
    dpart[which * OD_MAX_GROUPS + blockIdx.x] = s;
    cmass[which * OD_MAX_GROUPS + blockIdx.x] = n_mass;
  }
}

// ---- launch 3: the hot kernel (the file comment).  Dynamic LDS: q tile [TH][64] | p halo [PH][64 + 2 S], f32.
// grid = bands * (2 Kr + 1) * R, the band slowest; part [bands][2 Kr + 1][R][W][W] float64.
template <int NACC, int STEPS>
__global__ __launch_bounds__(OD_NT) void vote_odometry_corr_kernel(const float* __restrict__ pmass,
                                                                   const float* __restrict__ qmass, int R, int Ho,
                                                                   int Wo, int Kr, int S, double* __restrict__ part) {
  extern __shared__ float od_smem[];
  constexpr int TH = NACC * STEPS;
  const int W = 2 * S + 1, IB = (W + NACC - 1) / NACC;
  const int PW = OD_TW + 2 * S, PH = TH + IB * NACC - 1;
  float* qs = od_smem;
  float* ps = od_smem + TH * OD_TW;
  const int t = threadIdx.x;
  const bool owner = t < IB * W;            // the other threads only stage
  const int ib = owner ? t / W : 0, jx = owner ? t - ib * W : 0;
  int g = blockIdx.x;
  const int r = g % R;
  g /= R;
  const int kk = g % (2 * Kr + 1), band = g / (2 * Kr + 1);
  const int rk = vote_mod(r + kk - Kr, R);
  const size_t P = (size_t)Ho * Wo;
  const float* __restrict__ qp = qmass + (size_t)r * P;
  const float* __restrict__ pp = pmass + (size_t)rk * P;
  const int row_end = min(Ho, (band + 1) * OD_BAND_TILES * TH);
  double acc[NACC];
#pragma unroll
  for (int m = 0; m < NACC; ++m) acc[m] = 0.0;
  for (int a0 = band * OD_BAND_TILES * TH; a0 < row_end; a0 += TH) {
    for (int b0 = 0; b0 < Wo; b0 += OD_TW) {
      __syncthreads();                      // the previous tile's readers are done
      int any = 0;
      for (int i = t; i < TH * OD_TW; i += OD_NT) {
        const int a = a0 + i / OD_TW, b = b0 + i % OD_TW;
        const float v = (a < row_end && b < Wo) ? qp[(size_t)a * Wo + b] : 0.f;
        qs[i] = v;
        any |= v > 0.f ? 1 : 0;
      }
      if (!__syncthreads_or(any)) continue;   // (uniform) no mass in the q tile
      any = 0;
      for (int i = t; i < PH * PW; i += OD_NT) {
        const int row = i / PW, col = i - row * PW;
        const int a = a0 - S + row, b = b0 - S + col;
        const float v = (row < TH + 2 * S && a >= 0 && a < Ho && b >= 0 && b < Wo) ? pp[(size_t)a * Wo + b] : 0.f;
        ps[i] = v;
        any |= v > 0.f ? 1 : 0;
      }
      if (!__syncthreads_or(any)) continue;   // (uniform) no mass in the p halo
      const float* pc0 = ps + ib * NACC * PW + jx;
      for (int b = 0; b < OD_TW; ++b) {
        const float* pc = pc0 + b;
        const float* qc = qs + b;
        double win[NACC];                   // row rho of the column lives in slot rho % NACC
#pragma unroll
        for (int m = 0; m < NACC - 1; ++m) win[m] = (double)pc[m * PW];
        for (int a = 0; a < TH; a += NACC) {
#pragma unroll
          for (int s = 0; s < NACC; ++s) {
            win[(s + NACC - 1) % NACC] = (double)pc[(a + s + NACC - 1) * PW];
            const float qv = qc[(a + s) * OD_TW];
            if (__builtin_amdgcn_readfirstlane(__float_as_int(qv)) != 0) {   // (the same value in every lane)
              const double qd = (double)qv;
#pragma unroll
              for (int m = 0; m < NACC; ++m) acc[m] = fma(qd, win[(s + m) % NACC], acc[m]);   // (exact product)
            }
          }
        }
      }
    }
  }
  if (owner) {
    double* out = part + (size_t)blockIdx.x * W * W;   // blockIdx.x = (band (2 Kr + 1) + kk) R + r
#pragma unroll
    for (int m = 0; m < NACC; ++m) {
      const int ix = ib * NACC + m;
      if (ix < W) out[ix * W + jx] = acc[m];
    }
  }
}

// log zp, log zq (-inf for an empty volume) from the per-workgroup sums of launch 2.
__device__ __forceinline__ void od_log_sums(const double* __restrict__ dpart, int groups, double* sh, double* lzp,
                                            double* lzq) {
  const double zp = vote_fold_sum<OD_WAVES, 1>(dpart, 0, groups, sh);
  const double zq = vote_fold_sum<OD_WAVES, 1>(dpart + OD_MAX_GROUPS, 0, groups, sh);
  *lzp = zp > 0.0 ? log(zp) : -(double)INFINITY;
  *lzq = zq > 0.0 ? log(zq) : -(double)INFINITY;
}
__device__ __forceinline__ float od_log_ratio(double T, double lzp, double lzq) {
  return T > 0.0 ? (float)((log(T) - lzp) - lzq) : -INFINITY;
}

// ---- launch 4: one thread per table entry
__global__ __launch_bounds__(OD_NT) void vote_odometry_table_kernel(const double* __restrict__ part, int bands,
                                                                    int entries, const double* __restrict__ dpart,
                                                                    int groups, double* __restrict__ T,
                                                                    float* __restrict__ log_table) {
  __shared__ double shd[OD_WAVES];
  double lzp, lzq;
  od_log_sums(dpart, groups, shd, &lzp, &lzq);
  const int e = blockIdx.x * OD_NT + threadIdx.x;
  if (e >= entries) return;
  double s = 0.0;
  for (int band = 0; band < bands; ++band) s += part[(size_t)band * entries + e];
  T[e] = s;
  log_table[e] = od_log_ratio(s, lzp, lzq);
}

// per-workgroup partials of launch 5: double [groups][2] = the log-sum-exp pair, float [groups] / int32 [groups][3] =
// the maximum | its lowest u, rows outside the window, finite candidates
constexpr int OD_CI = 3;

// ---- launch 5: one thread per candidate, workgroups striding
__global__ __launch_bounds__(OD_NT) void vote_odometry_cand_kernel(const int32_t* __restrict__ shifts, int R, int Kr,
                                                                   int S, int U, const double* __restrict__ T,
                                                                   const double* __restrict__ dpart, int groups,
                                                                   float* __restrict__ log_evidence,
                                                                   double* __restrict__ lpart, float* __restrict__ mpart,
                                                                   int32_t* __restrict__ ipart) {
  __shared__ double shd[OD_WAVES];
  __shared__ double shl[OD_WAVES][2];
  __shared__ float shm[OD_WAVES];
  __shared__ int shi[OD_WAVES];
  double lzp, lzq;
  od_log_sums(dpart, groups, shd, &lzp, &lzq);
  const int W = 2 * S + 1;
  float bm = -INFINITY;
  int bi = VOTE_NO_INDEX, n_out = 0, n_fin = 0;
  double lm = -(double)INFINITY, ls = 0.0;
  for (int64_t u = (int64_t)blockIdx.x * OD_NT + threadIdx.x; u < U; u += (int64_t)gridDim.x * OD_NT) {
    const int32_t* row = shifts + (size_t)u * R * 3;
    double E = 0.0;
    for (int r = 0; r < R; ++r) {
      const int k = row[r * 3], i = row[r * 3 + 1], j = row[r * 3 + 2];
      if (k < -Kr || k > Kr || i < -S || i > S || j < -S || j > S) {
        ++n_out;                            // adds 0; no address is formed from it
      } else {
        E += T[(((size_t)(k + Kr) * R + r) * W + (i + S)) * W + (j + S)];
      }
    }
    const float le = od_log_ratio(E, lzp, lzq);
    log_evidence[u] = le;
    if (le > -INFINITY) {
      ++n_fin;
      vote_argmax_merge(&bm, &bi, le, (int)u);
      vote_lse_add(&lm, &ls, (double)le);
    }
  }
  vote_block_argmax<OD_WAVES>(&bm, &bi, shm, shi);
  vote_block_lse<OD_WAVES>(&lm, &ls, shl);
  n_out = vote_block_sum<OD_WAVES>(n_out, shi);
  n_fin = vote_block_sum<OD_WAVES>(n_fin, shi);
  if (threadIdx.x == 0) {
    lpart[(size_t)blockIdx.x * 2] = lm;
    lpart[(size_t)blockIdx.x * 2 + 1] = ls;
    mpart[blockIdx.x] = bm;
    ipart[(size_t)blockIdx.x * OD_CI] = bi;
    ipart[(size_t)blockIdx.x * OD_CI + 1] = n_out;
    ipart[(size_t)blockIdx.x * OD_CI + 2] = n_fin;
  }
}

// ---- launch 6: one workgroup.  cgroups = the workgroups of launch 5 (0 with U = 0)
__global__ __launch_bounds__(OD_NT) void vote_odometry_finish_kernel(int groups, int cgroups, float scale_prev,
                                                                     float scale_cur, const float* __restrict__ fpart,
                                                                     const int32_t* __restrict__ cbad,
                                                                     const int32_t* __restrict__ cmass,
                                                                     const double* __restrict__ dpart,
                                                                     const double* __restrict__ lpart,
                                                                     const float* __restrict__ mpart,
                                                                     const int32_t* __restrict__ ipart,
                                                                     int32_t* __restrict__ best,
                                                                     float* __restrict__ stats,
                                                                     int32_t* __restrict__ count) {
  __shared__ double shd[OD_WAVES];
  __shared__ double shl[OD_WAVES][2];
  __shared__ float shm[OD_WAVES];
  __shared__ int shi[OD_WAVES];
  double lzp, lzq;
  od_log_sums(dpart, groups, shd, &lzp, &lzq);
  const float Mp = vote_fold_max<OD_WAVES, 1>(fpart, 0, groups, shm);
  const float Mq = vote_fold_max<OD_WAVES, 1>(fpart + OD_MAX_GROUPS, 0, groups, shm);
  const int c0 = vote_fold_sum<OD_WAVES, 1>(cmass, 0, groups, shi);
  const int c1 = vote_fold_sum<OD_WAVES, 1>(cbad, 0, groups, shi);
  const int c2 = vote_fold_sum<OD_WAVES, 1>(cmass + OD_MAX_GROUPS, 0, groups, shi);
  const int c3 = vote_fold_sum<OD_WAVES, 1>(cbad + OD_MAX_GROUPS, 0, groups, shi);
  const int c4 = vote_fold_sum<OD_WAVES, OD_CI>(ipart, 1, cgroups, shi);
  const int c5 = vote_fold_sum<OD_WAVES, OD_CI>(ipart, 2, cgroups, shi);
  float bm;
  int bi;
  vote_fold_argmax<OD_WAVES, 1, OD_CI>(mpart, 0, ipart, 0, cgroups, &bm, &bi, shm, shi);
  const double lse = vote_fold_lse<OD_WAVES, 2>(lpart, 0, 1, cgroups, shl);
  if (threadIdx.x == 0) {
    const bool any = bi != VOTE_NO_INDEX;
    best[0] = any ? bi : -1;
    stats[0] = lzp > -(double)INFINITY ? (float)(lzp + (double)scale_prev * (double)Mp) : -INFINITY;
    stats[1] = lzq > -(double)INFINITY ? (float)(lzq + (double)scale_cur * (double)Mq) : -INFINITY;
    stats[2] = (float)lse;
    stats[3] = any ? bm : -INFINITY;
    count[0] = c0;
    count[1] = c1;
    count[2] = c2;
    count[3] = c3;
    count[4] = c4;
    count[5] = c5;
  }
}

struct OdPlan {
  VotePlan cell;                            // launches 1, 2
  int nacc, th, bands, entries, cgroups;    // the hot kernel's accumulators per thread and tile rows; table entries
  size_t lds;
};

constexpr int OD_NACC[] = {1, 2, 3, 5, 7, 10, 13, 17, 22};
constexpr int od_steps(int nacc) { return 16 / nacc > 1 ? 16 / nacc : 1; }

bool od_plan(int R, int Ho, int Wo, int Kr, int S, int U, OdPlan* plan) {
  if (R < 1 || R > OD_MAX_R || Ho < 1 || Wo < 1 || Kr < 0 || 2 * (int64_t)Kr + 1 > R || S < 0 || S > OD_MAX_S || U < 0)
    return false;
  if (!vote_plan((int64_t)R * Ho * Wo, R, Ho, Wo, OD_NT, OD_MAX_GROUPS, &plan->cell)) return false;
  const int W = 2 * S + 1, need = (int)snap_cdiv(W, OD_NT / W);
  plan->nacc = 0;
  for (int n : OD_NACC)
    if (plan->nacc == 0 && n >= need) plan->nacc = n;   // (need <= 22 at S = 32)
  plan->th = plan->nacc * od_steps(plan->nacc);
  plan->bands = (int)snap_cdiv(Ho, OD_BAND_TILES * plan->th);
  plan->entries = (2 * Kr + 1) * R * W * W;             // <= 64 * 65 * 65
  const int ib = (int)snap_cdiv(W, plan->nacc);
  plan->lds = ((size_t)plan->th * OD_TW + (size_t)(plan->th + ib * plan->nacc - 1) * (OD_TW + 2 * S)) * sizeof(float);
  const int64_t cg = snap_cdiv(U, OD_NT);
  plan->cgroups = (int)(cg < OD_MAX_GROUPS ? cg : OD_MAX_GROUPS);
  return true;
}

// mass [2][R Ho Wo] f32 | band partials [bands][entries] float64 | T [entries] float64 | sums [2][1024] float64 |
// lse pairs [1024][2] float64 | maxima [2][1024] f32 | candidate maxima [1024] f32 | counts [2][1024] x 2, [1024][3] i32
struct OdWorkspace {
  float* mass;
  double* part;
  double* T;
  double* dpart;
  double* lpart;
  float* fpart;
  float* mpart;
  int32_t* cbad;
  int32_t* cmass;
  int32_t* ipart;
  size_t bytes;
};

OdWorkspace od_workspace(int R, const OdPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<float>(2 * (size_t)R * plan.cell.P),
          l.take<double>((size_t)plan.bands * plan.entries),
          l.take<double>(plan.entries),
          l.take<double>(2 * OD_MAX_GROUPS),
          l.take<double>(2 * OD_MAX_GROUPS),
          l.take<float>(2 * OD_MAX_GROUPS),
          l.take<float>(OD_MAX_GROUPS),
          l.take<int32_t>(2 * OD_MAX_GROUPS),
          l.take<int32_t>(2 * OD_MAX_GROUPS),
          l.take<int32_t>(OD_CI * OD_MAX_GROUPS),
          l.bytes};
}

template <int NACC>
void od_launch_corr(const OdPlan& plan, const OdWorkspace& w, int R, int Ho, int Wo, int Kr, int S, hipStream_t s) {
  const size_t cells = (size_t)R * plan.cell.P;
  hipLaunchKernelGGL((vote_odometry_corr_kernel<NACC, od_steps(NACC)>), dim3(plan.bands * (2 * Kr + 1) * R),
                     dim3(OD_NT), plan.lds, s, w.mass, w.mass + cells, R, Ho, Wo, Kr, S, w.part);
}

}  // namespace

extern "C" size_t snap_vote_odometry_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Kr, int32_t S,
                                                     int32_t U) {
  OdPlan plan;
  if (!od_plan(R, Ho, Wo, Kr, S, U, &plan)) return 0;
  return od_workspace(R, plan, nullptr).bytes;
}

extern "C" int snap_vote_odometry_f32(const float* prev, const float* cur, float scale_prev, float scale_cur,
                                      const int32_t* shifts, int32_t R, int32_t Ho, int32_t Wo, int32_t Kr, int32_t S,
                                      int32_t U, float* log_table, float* log_evidence, int32_t* best, float* stats,
                                      int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  if (!prev || !cur || !log_table || !best || !stats || !count || !workspace) return SNAP_ERR_NULL;
  if (U > 0 && (!shifts || !log_evidence)) return SNAP_ERR_NULL;
  OdPlan plan;
  if (!od_plan(R, Ho, Wo, Kr, S, U, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale_prev > 0.f) || !(scale_prev < INFINITY) || !(scale_cur > 0.f) || !(scale_cur < INFINITY))
    return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, od_workspace(R, plan, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const OdWorkspace w = od_workspace(R, plan, workspace);
  const VotePlan& c = plan.cell;
  const size_t cells = (size_t)R * c.P;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vote_odometry_max_kernel, dim3(c.groups, 2), dim3(OD_NT), 0, s, prev, cur, c.P, c.tiles_per_plane,
                     c.tiles, w.fpart, w.cbad);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_odometry_mass_kernel, dim3(c.groups, 2), dim3(OD_NT), 0, s, prev, cur, c.P, c.tiles_per_plane,
                     c.tiles, scale_prev, scale_cur, w.fpart, w.mass, cells, w.dpart, w.cmass);
  SNAP_CHECK_LAUNCH();
  switch (plan.nacc) {
    case 1: od_launch_corr<1>(plan, w, R, Ho, Wo, Kr, S, s); break;
    case 2: od_launch_corr<2>(plan, w, R, Ho, Wo, Kr, S, s); break;
    case 3: od_launch_corr<3>(plan, w, R, Ho, Wo, Kr, S, s); break;
    case 5: od_launch_corr<5>(plan, w, R, Ho, Wo, Kr, S, s); break;
    case 7: od_launch_corr<7>(plan, w, R, Ho, Wo, Kr, S, s); break;
    case 10: od_launch_corr<10>(plan, w, R, Ho, Wo, Kr, S, s); break;
    case 13: od_launch_corr<13>(plan, w, R, Ho, Wo, Kr, S, s); break;
    case 17: od_launch_corr<17>(plan, w, R, Ho, Wo, Kr, S, s); break;
    default: od_launch_corr<22>(plan, w, R, Ho, Wo, Kr, S, s); break;
  }
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_odometry_table_kernel, dim3((unsigned)snap_cdiv(plan.entries, OD_NT)), dim3(OD_NT), 0, s,
                     w.part, plan.bands, plan.entries, w.dpart, c.groups, w.T, log_table);
  SNAP_CHECK_LAUNCH();
  if (U > 0) {
    hipLaunchKernelGGL(vote_odometry_cand_kernel, dim3(plan.cgroups), dim3(OD_NT), 0, s, shifts, R, Kr, S, U, w.T,
                       w.dpart, c.groups, log_evidence, w.lpart, w.mpart, w.ipart);
    SNAP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(vote_odometry_finish_kernel, dim3(1), dim3(OD_NT), 0, s, c.groups, plan.cgroups, scale_prev,
                     scale_cur, w.fpart, w.cbad, w.cmass, w.dpart, w.lpart, w.mpart, w.ipart, best, stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
