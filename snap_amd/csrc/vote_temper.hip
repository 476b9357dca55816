// A vote volume's statistics over a temperature ladder: snap_vote_temper_f32 (include/snap_hip.h).
//
// votes [R, Ho, Wo] f32 are unnormalised log-scores; over the FINITE cells F (vote_posterior's rule) m = max v and
// d = fl32(v - m) <= 0.  For each of the S scales s of the ladder, with x = fl32(s * d) and e = expf(x), the op returns
// the float64 row built from S0 = sum e, S1 = sum e x (<= 0) and S2 = sum (e x) x (>= 0): log_z = s m + log S0,
// E[v] = m + mu, mu = S1 / S0 / s, Var[v] = S2 / S0 / s^2 - mu^2, the entropy, log p_max, and the log-probability and
// NLL slope of a ground-truth index whose sample v_gt (of v, not of s v) does not depend on s.  s * v is never formed,
// and the moments are summed in x, not in d: a term with e > 0 has |x| < 104, so no f32 sum can overflow whatever the
// votes' range (the division by s and s^2 is float64).
//
//   launch 1  vote_temper_max_kernel     the largest finite vote and the counts, per workgroup (vote_scan_max; tiles of
//                                        256 consecutive cells of one rotation)
//   launch 2  vote_temper_tiles_kernel   <S>: every workgroup folds the maxima into m (a maximum: exact); workgroups
//             stride over tiles of 256 consecutive pixels, one pixel per thread (vote_posterior's plan: a wave's loads
//             of one rotation are 256 contiguous bytes).  A thread walks its pixel's R cells ONCE and feeds 3 S f32
//             sums (<= R terms of one sign each), then adds them into its 3 S float64 accumulators; they live in
//             registers (the ladder is a by-value kernel argument indexed by unrolled loops, S a template parameter).
//             After the last tile one wave tree per column and the four waves pairwise: ONE partial row of 3 S float64
//             per workgroup.  The volume is read a second time here; launch 1 has just pulled it through the cache.
//   launch 3  vote_temper_finish_kernel  workgroup l folds level l's three columns (vote_fold_sum) and writes row l of
//             the table; every workgroup samples the ground truth (8 taps, one thread), workgroup 0 writes stats / count.
// No atomics, no hand-off between workgroups inside a launch: every sum's order is a function of (R, Ho, Wo, S) alone.
#include "vote_common.h"

namespace {

constexpr int TP_NT = 256;                  // threads of every launch; launch 2: pixels of a tile
constexpr int TP_WAVES = TP_NT / SNAP_WAVE;
constexpr int TP_MAX_R = 64;
constexpr int TP_MAX_S = 16;
constexpr int TP_MAX_GROUPS = 1024;         // workgroups of launches 1 and 2
constexpr int TP_COLS = 3 * TP_MAX_S;       // the stride of a partial row: level l owns columns 3 l .. 3 l + 2
constexpr float TP_X_FLOOR = -128.f;        // expf is exactly 0 from -104 down: no weight changes, and e * x stays 0

struct TpScales {
  float s[TP_MAX_S];
};
// Entry l of the by-value ladder (a select chain: no dynamically indexed copy of the kernel argument).
__device__ __forceinline__ float tp_pick(const TpScales& sc, int l) {
  float x = sc.s[0];
#pragma unroll
  for (int i = 1; i < TP_MAX_S; ++i) x = i == l ? sc.s[i] : x;
  return x;
}

// ---- launch 1: the largest contributing vote and the counts, per workgroup
__global__ __launch_bounds__(TP_NT) void vote_temper_max_kernel(const float* __restrict__ votes, int P, int tpp,
                                                                int tiles, float* __restrict__ fpart,
                                                                int32_t* __restrict__ cpart) {
  __shared__ float shm[TP_WAVES];
  __shared__ int shc[TP_WAVES][2];
  float m;
  int n_ok, n_bad;
  vote_scan_max<TP_NT>(votes, P, tpp, tiles, &m, &n_ok, &n_bad);
  m = vote_block_max<TP_WAVES>(m, shm);
  const int c = vote_block_count_pair<TP_WAVES>(n_ok, n_bad, shc);
  if (threadIdx.x == 0) fpart[blockIdx.x] = m;
  if (threadIdx.x < 2) cpart[(size_t)blockIdx.x * 2 + threadIdx.x] = c;
}

// ---- launch 2: the 3 S sums of this workgroup's pixels
template <int S>
__global__ __launch_bounds__(TP_NT) void vote_temper_tiles_kernel(const float* __restrict__ votes, int R, int P,
                                                                  int tiles, int groups1, TpScales sc,
                                                                  const float* __restrict__ fpart,
                                                                  double* __restrict__ part) {
  __shared__ float shm[TP_WAVES];
  __shared__ double wred[TP_WAVES][3 * S];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const float vmax = vote_fold_max<TP_WAVES, 1>(fpart, 0, groups1, shm);
  double a0[S], a1[S], a2[S];
#pragma unroll
  for (int l = 0; l < S; ++l) a0[l] = a1[l] = a2[l] = 0.0;
  if (vmax > -INFINITY) {                   // (uniform) without a contributing cell every sum is exactly 0
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
      int p;
      if (!vote_tile_pixel<TP_NT>(tile, P, &p)) continue;
      const float* src = votes + p;
      float s0[S], s1[S], s2[S];
#pragma unroll
      for (int l = 0; l < S; ++l) s0[l] = s1[l] = s2[l] = 0.f;
      for (int r = 0; r < R; ++r) {
        const float v = src[(size_t)r * P];
        if (vote_finite(v)) {
          const float d = v - vmax;
#pragma unroll
          for (int l = 0; l < S; ++l) {
            const float x = fmaxf(sc.s[l] * d, TP_X_FLOOR);
            const float e = expf(x);
            const float ex = e * x;
            s0[l] += e;
            s1[l] += ex;
            s2[l] += ex * x;
          }
        }
      }
#pragma unroll
      for (int l = 0; l < S; ++l) {
        a0[l] += (double)s0[l];
        a1[l] += (double)s1[l];
        a2[l] += (double)s2[l];
      }
    }
  }
#pragma unroll
  for (int l = 0; l < S; ++l) {
    const double w0 = vote_wave_sum(a0[l]), w1 = vote_wave_sum(a1[l]), w2 = vote_wave_sum(a2[l]);
    if (lane == 0) {
      wred[wave][3 * l] = w0;
      wred[wave][3 * l + 1] = w1;
      wred[wave][3 * l + 2] = w2;
    }
  }
  __syncthreads();
  if (t < 3 * S) part[(size_t)blockIdx.x * TP_COLS + t] = (wred[0][t] + wred[1][t]) + (wred[2][t] + wred[3][t]);
}

// The trilinear sample of v at gt = (k, i, j), by vote_posterior's rule (a copy of its finish kernel's, without the
// scale): circular in k, a tap of weight exactly 0 is not read, valid iff k, i, j are finite, i and j in range and
// every tap of non-zero weight is finite.
__device__ __forceinline__ bool tp_gt_sample(const float* __restrict__ votes, int R, int Ho, int Wo,
                                             const float* __restrict__ gt, double* out) {
  if (gt == nullptr) return false;
  const float k = gt[0], i = gt[1], j = gt[2];
  if (!(vote_finite(k) && vote_finite(i) && vote_finite(j) && i >= 0.f && i <= (float)(Ho - 1) && j >= 0.f &&
        j <= (float)(Wo - 1)))
    return false;
  const double kfl = floor((double)k), ifl = floor((double)i), jfl = floor((double)j);
  const double wk = (double)k - kfl, wi = (double)i - ifl, wj = (double)j - jfl;
  double km = fmod(kfl, (double)R);
  if (km < 0.0) km += (double)R;
  int k0 = (int)km;
  if (k0 >= R) k0 = 0;
  const int k1 = vote_next(k0, R);
  const int i0 = (int)ifl, j0 = (int)jfl;
  double sum = 0.0;
  bool ok = true;
  for (int tap = 0; tap < 8; ++tap) {
    const int dk = tap >> 2, di = (tap >> 1) & 1, dj = tap & 1;
    const double w = (dk ? wk : 1.0 - wk) * (di ? wi : 1.0 - wi) * (dj ? wj : 1.0 - wj);
    if (w == 0.0) continue;                 // a tap of weight 0 is not read
    const int rr = dk ? k1 : k0, aa = i0 + di, bb = j0 + dj;
    if (aa >= Ho || bb >= Wo) {             // (unreachable: the upper tap's weight is 0 on the last row / column)
      ok = false;
      continue;
    }
    const float v = votes[((size_t)rr * Ho + aa) * Wo + bb];
    if (vote_finite(v))
      sum += w * (double)v;
    else
      ok = false;
  }
  *out = sum;
  return ok;
}

// ---- launch 3: workgroup l writes row l of the table; workgroup 0 stats and count as well
__global__ __launch_bounds__(TP_NT) void vote_temper_finish_kernel(const float* __restrict__ votes, int R, int Ho,
                                                                   int Wo, TpScales sc, const float* __restrict__ gt,
                                                                   int groups1, int groups2,
                                                                   const float* __restrict__ fpart,
                                                                   const int32_t* __restrict__ cpart,
                                                                   const double* __restrict__ part,
                                                                   double* __restrict__ table,
                                                                   double* __restrict__ stats,
                                                                   int32_t* __restrict__ count) {
  __shared__ float shm[TP_WAVES];
  __shared__ double shd[TP_WAVES];
  __shared__ int32_t shc[TP_WAVES];
  const int l = blockIdx.x;
  const float vmax = vote_fold_max<TP_WAVES, 1>(fpart, 0, groups1, shm);
  const double S0 = vote_fold_sum<TP_WAVES, TP_COLS>(part, 3 * l, groups2, shd);
  const double S1 = vote_fold_sum<TP_WAVES, TP_COLS>(part, 3 * l + 1, groups2, shd);
  const double S2 = vote_fold_sum<TP_WAVES, TP_COLS>(part, 3 * l + 2, groups2, shd);
  int32_t c0 = 0, c1 = 0;
  if (l == 0) {                             // (uniform)
    c0 = vote_fold_sum<TP_WAVES, 2>(cpart, 0, groups1, shc);
    c1 = vote_fold_sum<TP_WAVES, 2>(cpart, 1, groups1, shc);
  }
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool empty = !(vmax > -INFINITY);
  double v_gt = nan;
  const bool valid = tp_gt_sample(votes, R, Ho, Wo, gt, &v_gt) && !empty;
  if (!valid) v_gt = nan;
  double* row = table + (size_t)l * 8;
  if (empty) {
    row[0] = -(double)INFINITY;
    for (int i = 1; i < 7; ++i) row[i] = nan;
  } else {
    const double s = (double)tp_pick(sc, l), m = (double)vmax;
    const double A = log(S0), smu = S1 / S0;   // (smu = s mu, as summed)
    const double mu = smu / s, q = (S2 / S0) / (s * s);
    const double var = q - mu * mu;
    const double log_z = s * m + A, mean = m + mu;
    row[0] = log_z;
    row[1] = mean;
    row[2] = var > 0.0 ? var : 0.0;
    row[3] = A - smu;
    row[4] = -A;
    row[5] = s * v_gt - log_z;              // (NaN with an invalid ground truth)
    row[6] = mean - v_gt;
  }
  row[7] = 0.0;
  if (l == 0) {
    stats[0] = (double)vmax;
    stats[1] = v_gt;
    stats[2] = 0.0;
    stats[3] = 0.0;
    count[0] = c0;
    count[1] = c1;
    count[2] = valid ? 1 : 0;
    count[3] = 0;
  }
}

struct TpPlan {
  VotePlan cell;                            // launch 1: one tile = 256 consecutive cells of one rotation
  VotePlan pixel;                           // launch 2: one tile = 256 consecutive pixels, every rotation of them
};

bool tp_plan(int R, int Ho, int Wo, int S, TpPlan* plan) {
  if (R < 1 || R > TP_MAX_R || Ho < 1 || Wo < 1 || S < 1 || S > TP_MAX_S) return false;
  const int64_t cells = (int64_t)R * Ho * Wo;
  return vote_plan(cells, R, Ho, Wo, TP_NT, TP_MAX_GROUPS, &plan->cell) &&
         vote_plan(cells, 1, Ho, Wo, TP_NT, TP_MAX_GROUPS, &plan->pixel);
}

// [groups2][48] float64 partial rows | the maxima and counts of launch 1
struct TpWorkspace {
  double* part;
  float* fpart;
  int32_t* cpart;
  size_t bytes;
};

TpWorkspace tp_workspace(const TpPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<double>((size_t)plan.pixel.groups * TP_COLS), l.take<float>(plan.cell.groups),
          l.take<int32_t>((size_t)plan.cell.groups * 2), l.bytes};
}

template <int S>
void tp_launch_tiles(const TpPlan& plan, const float* votes, int R, const TpScales& sc, const TpWorkspace& w,
                     hipStream_t s) {
  hipLaunchKernelGGL(vote_temper_tiles_kernel<S>, dim3(plan.pixel.groups), dim3(TP_NT), 0, s, votes, R, plan.pixel.P,
                     plan.pixel.tiles, plan.cell.groups, sc, w.fpart, w.part);
}

}  // namespace

extern "C" size_t snap_vote_temper_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t S) {
  TpPlan plan;
  if (!tp_plan(R, Ho, Wo, S, &plan)) return 0;
  return tp_workspace(plan, nullptr).bytes;
}

extern "C" int snap_vote_temper_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, const float* scales,
                                    int32_t S, const float* gt_index, double* table, double* stats, int32_t* count,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!votes || !scales || !table || !stats || !count || !workspace) return SNAP_ERR_NULL;
  TpPlan plan;
  if (!tp_plan(R, Ho, Wo, S, &plan)) return SNAP_ERR_BAD_SHAPE;
  TpScales sc = {};
  for (int l = 0; l < S; ++l) {
    const float x = scales[l];
    if (!(x > 0.f) || !(x < INFINITY) || (l > 0 && !(x > scales[l - 1]))) return SNAP_ERR_UNSUPPORTED;
    sc.s[l] = x;
  }
  if (!vote_workspace_ok(workspace, workspace_bytes, tp_workspace(plan, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const TpWorkspace w = tp_workspace(plan, workspace);
  const VotePlan& c = plan.cell;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vote_temper_max_kernel, dim3(c.groups), dim3(TP_NT), 0, s, votes, c.P, c.tiles_per_plane, c.tiles,
                     w.fpart, w.cpart);
  SNAP_CHECK_LAUNCH();
  switch (S) {
#define TP_CASE(N) \
  case N: tp_launch_tiles<N>(plan, votes, R, sc, w, s); break;
    TP_CASE(1) TP_CASE(2) TP_CASE(3) TP_CASE(4) TP_CASE(5) TP_CASE(6) TP_CASE(7) TP_CASE(8)
    TP_CASE(9) TP_CASE(10) TP_CASE(11) TP_CASE(12) TP_CASE(13) TP_CASE(14) TP_CASE(15) TP_CASE(16)
#undef TP_CASE
  }
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_temper_finish_kernel, dim3(S), dim3(TP_NT), 0, s, votes, R, Ho, Wo, sc, gt_index, c.groups,
                     plan.pixel.groups, w.fpart, w.cpart, w.part, table, stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
