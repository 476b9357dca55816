// Expected recall of a vote volume: snap_vote_recall_f32 (include/snap_hip.h).
//
// votes [R, Ho, Wo] f32 are unnormalised log-scores; over the FINITE cells (vote_posterior's rule) x = (double)scale *
// (double)v, m = max x, e = exp(x - m), S = sum e.  For L threshold pairs (rho2_l, half_r_l) the BALL of a cell
// (r, a, b) holds the cells (r', a', b') with circular |r' - r| <= half_r_l and (a' - a)^2 + (b' - b)^2 <= rho2_l
// (clipped to the volume in a, b), and log_mass_l = fl32(min(0, log sum_ball e - log S)): the logarithm of the
// probability that the pose lies within the metric's threshold of that cell.  The op returns, per level, the cell with
// the largest log mass (the maximum-expected-recall pose), the log masses at K given centres and at a ground-truth
// cell, and optionally the whole map.
//
// EVERY BALL MASS IS A SUM OF NON-NEGATIVE TERMS: no prefix sums, no sliding-window differences (a difference loses a
// low-mass ball against its row total and can go negative).  A disc is cut into its rows: the row at distance da from
// the centre is the centred span of half-width h(da) = isqrt(rho2 - da^2), and the spans of one centre column grow out
// of each other, S_h = (S_{h-1} + e(b - h)) + e(b + h).
//
//   launch 1  vote_recall_max_kernel      the largest finite vote and the counts, per workgroup
//   launch 2  vote_recall_exp_kernel      E = e as a float64 volume (0 for a cell that does not contribute), sum per
//                                         workgroup
//   launch 3  vote_recall_norm_kernel     one workgroup: log S, stats, count[0, 1, 3]
//   launch 4  vote_recall_disc_kernel     ONE PER LEVEL.  A workgroup is one wave: 64 columns b of one rotation r and a
//             chunk of 128 output rows.  It marches over the input rows a' of its chunk and the rho rows either side.
//             Per row: the row of W = sum_{|dr| <= half_r} E[r + dr] (dr ascending, circular) with rho columns of halo
//             goes to LDS (zeros outside the volume); a thread grows the spans of its column, h = 0 .. rho, and adds
//             S_{h(d)} to the pending output rows a' + d and a' - d, d = rho .. 0, kept as a ring of 2 rho + 1 rows in
//             LDS (a thread touches its own column of the ring only).  Output row a' - rho is then complete: the
//             logarithm, the optional map store, the thread's running (maximum, lowest flat index); its ring slot is
//             zeroed for row a' + rho + 1.  An output row receives its 2 rho + 1 spans in the order a' ascending
//             whatever the chunk, so the tiling is not part of the result.  ~4 rho + 1 LDS additions per cell.
//   launch 5  vote_recall_centres_kernel  (K + 1) x L workgroups: the ball of one centre (row K: the ground truth) at
//             one level summed directly from E, 256 threads striding over the bounding box, dr = -half_r .. half_r.
//   launch 6  vote_recall_finish_kernel   L workgroups fold the disc workgroups' (maximum, index) pairs.
// LDS of a disc workgroup: ring (2 rho + 1) x 64 x 8 B + two row buffers (64 + 2 rho) x 8 B + 33 ints: 2.6 KB at
// rho = 1, 9.9 KB at rho = 7, 27.6 KB at rho = 25, 35.4 KB at rho = 32, i.e. 4 to 60 one-wave workgroups per 160 KiB
// CU.  No atomics; every sum's order is a function of the shape and the thresholds, so two calls give the same bytes.
#include "vote_common.h"

namespace {

constexpr int RC_NT = 256;                  // threads of the volume, centre and finish launches
constexpr int RC_WAVES = RC_NT / SNAP_WAVE;
constexpr int RC_MAX_R = 64;
constexpr int RC_MAX_L = 8;
constexpr int RC_MAX_K = 64;
constexpr int RC_MAX_RHO2 = 1024;
constexpr int RC_MAX_RHO = 32;
constexpr int RC_MAX_HALF_R = 4;
constexpr int RC_MAX_GROUPS = 1024;         // workgroups of launches 1 and 2
constexpr int RC_TW = SNAP_WAVE;            // disc launch: columns of a tile = threads (one wave)
constexpr int RC_CH = 128;                  // disc launch: output rows of a chunk
static_assert(RC_MAX_RHO * RC_MAX_RHO == RC_MAX_RHO2, "the span table holds rho + 1 entries");

struct RcLevels {
  int32_t rho2[RC_MAX_L];
  int32_t half_r[RC_MAX_L];
};
// Entry l of a by-value table (a select chain: no dynamically indexed copy of the kernel argument).
__device__ __forceinline__ int rc_pick(const int32_t (&v)[RC_MAX_L], int l) {
  int x = v[0];
#pragma unroll
  for (int i = 1; i < RC_MAX_L; ++i) x = i == l ? v[i] : x;
  return x;
}

// floor(sqrt(x)), 0 <= x <= 1024, exactly (host and device).
__host__ __device__ __forceinline__ int rc_isqrt(int x) {
  int h = (int)sqrtf((float)x);
  while (h * h > x) --h;
  while ((h + 1) * (h + 1) <= x) ++h;
  return h;
}

// fl32(min(0, log(mass) - log S)); -inf for an empty ball.
__device__ __forceinline__ float rc_log_mass(double mass, double log_s) {
  if (!(mass > 0.0)) return -INFINITY;
  const double q = log(mass) - log_s;
  return (float)(q > 0.0 ? 0.0 : q);
}

// ---- launch 1: the largest contributing vote and the counts, per workgroup
__global__ __launch_bounds__(RC_NT) void vote_recall_max_kernel(const float* __restrict__ votes, int P, int tpp,
                                                                int tiles, float* __restrict__ fpart,
                                                                int32_t* __restrict__ cpart) {
  __shared__ float shm[RC_WAVES];
  __shared__ int shc[RC_WAVES][2];
  float m;
  int n_ok, n_bad;
  vote_scan_max<RC_NT>(votes, P, tpp, tiles, &m, &n_ok, &n_bad);
  m = vote_block_max<RC_WAVES>(m, shm);
  const int c = vote_block_count_pair<RC_WAVES>(n_ok, n_bad, shc);
  if (threadIdx.x == 0) fpart[blockIdx.x] = m;
  if (threadIdx.x < 2) cpart[(size_t)blockIdx.x * 2 + threadIdx.x] = c;
}

// ---- launch 2: E = exp(x - m), 0 where the cell does not contribute; the workgroup's sum
// (scale > 0 and a float64 product rounds monotonically: the largest x is the x of the largest v)
__global__ __launch_bounds__(RC_NT) void vote_recall_exp_kernel(const float* __restrict__ votes, int P, int tpp,
                                                                int tiles, int groups, float scale,
                                                                const float* __restrict__ fpart,
                                                                double* __restrict__ E, double* __restrict__ dpart) {
  __shared__ float shm[RC_WAVES];
  __shared__ double shd[RC_WAVES];
  const float vmax = vote_fold_max<RC_WAVES, 1>(fpart, 0, groups, shm);
  const double ds = (double)scale, m = ds * (double)vmax;   // (vmax = -inf: no cell is finite, m is not used)
  double s = 0.0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p;
    if (vote_tile_cell<RC_NT>(tile, tpp, P, &r, &p)) {
      const float v = votes[(size_t)r * P + p];
      const double e = vote_finite(v) ? exp(ds * (double)v - m) : 0.0;
      E[(size_t)r * P + p] = e;
      s += e;
    }
  }
  s = vote_block_sum<RC_WAVES>(s, shd);
  if (threadIdx.x == 0) dpart[blockIdx.x] = s;
}

// ---- launch 3: one workgroup: norm = (log S, m), stats, count[0, 1, 3]
__global__ __launch_bounds__(RC_NT) void vote_recall_norm_kernel(int groups, float scale,
                                                                 const float* __restrict__ fpart,
                                                                 const double* __restrict__ dpart,
                                                                 const int32_t* __restrict__ cpart,
                                                                 double* __restrict__ norm, float* __restrict__ stats,
                                                                 int32_t* __restrict__ count) {
  __shared__ float shm[RC_WAVES];
  __shared__ double shd[RC_WAVES];
  __shared__ int32_t shc[RC_WAVES];
  const float vmax = vote_fold_max<RC_WAVES, 1>(fpart, 0, groups, shm);
  const double S = vote_fold_sum<RC_WAVES, 1>(dpart, 0, groups, shd);
  const int32_t c0 = vote_fold_sum<RC_WAVES, 2>(cpart, 0, groups, shc);
  const int32_t c1 = vote_fold_sum<RC_WAVES, 2>(cpart, 1, groups, shc);
  if (threadIdx.x == 0) {
    const double ninf = -(double)INFINITY;
    const double m = vmax > -INFINITY ? (double)scale * (double)vmax : ninf;
    const double log_s = S > 0.0 ? log(S) : ninf;
    norm[0] = log_s;
    norm[1] = m;
    stats[0] = (float)(m + log_s);
    stats[1] = (float)m;
    stats[2] = 0.f;
    stats[3] = 0.f;
    count[0] = c0;
    count[1] = c1;
    count[3] = 0;
  }
}

// ---- launch 4, one per level: the disc pass (the file comment).  Dynamic LDS: ring [2 rho + 1][64] | rows [2][64 + 2 rho]
__global__ __launch_bounds__(RC_TW) void vote_recall_disc_kernel(const double* __restrict__ E, int R, int Ho, int Wo,
                                                                 int ctiles, int chunks, int rho2, int rho, int half_r,
                                                                 const double* __restrict__ norm,
                                                                 float* __restrict__ map, float* __restrict__ bpart,
                                                                 int32_t* __restrict__ ipart) {
  extern __shared__ double rc_smem[];
  __shared__ int s_span[RC_MAX_RHO + 1];    // h(d) = isqrt(rho2 - d^2), d = 0 .. rho
  __shared__ float shm[1];
  __shared__ int shi[1];
  const int t = threadIdx.x;
  const int n = 2 * rho + 1, roww = RC_TW + 2 * rho;
  double* ring = rc_smem;
  double* rows = rc_smem + n * RC_TW;
  int g = blockIdx.x;
  const int ct = g % ctiles;
  g /= ctiles;
  const int ch = g % chunks, r = g / chunks;
  const int b0 = ct * RC_TW, b = b0 + t;
  const int c0 = ch * RC_CH, c1 = c0 + RC_CH < Ho ? c0 + RC_CH : Ho;
  const int c = t + rho;                    // this thread's column in a row buffer
  const size_t P = (size_t)Ho * Wo;
  for (int i = 0; i < n; ++i) ring[i * RC_TW + t] = 0.0;
  if (t <= rho) s_span[t] = rc_isqrt(rho2 - t * t);
  const double log_s = norm[0];
  float bm = -INFINITY;
  int bi = VOTE_NO_INDEX;
  int s0 = vote_mod(c0 - 2 * rho, n);       // the ring slot of output row ap - rho
  __syncthreads();
  for (int ap = c0 - rho; ap < c1 + rho; ++ap) {
    if (ap >= 0 && ap < Ho) {               // (uniform) an input row inside the volume
      double* row = rows + (ap & 1) * roww;
      for (int i = t; i < roww; i += RC_TW) {
        const int col = b0 - rho + i;
        double w = 0.0;
        if (col >= 0 && col < Wo) {
          const size_t at = (size_t)ap * Wo + col;
          for (int dr = -half_r; dr <= half_r; ++dr) w += E[(size_t)vote_wrap(r + dr, R) * P + at];
        }
        row[i] = w;
      }
      __syncthreads();                      // (one barrier a row: the other buffer is written next)
      double S = row[c];
      int h = 0;
      for (int d = rho; d >= 0; --d) {
        const int target = s_span[d];
        while (h < target) {
          ++h;
          S = (S + row[c - h]) + row[c + h];
        }
        int s = s0 + rho + d;               // output row ap + d
        if (s >= n) s -= n;
        ring[s * RC_TW + t] += S;
        if (d > 0) {
          s = s0 + rho - d;                 // output row ap - d
          if (s >= n) s -= n;
          ring[s * RC_TW + t] += S;
        }
      }
    }
    const int ao = ap - rho;                // complete: every input row up to ao + rho is in
    if (ao >= c0 && b < Wo) {
      const float lm = rc_log_mass(ring[s0 * RC_TW + t], log_s);
      const int flat = (r * Ho + ao) * Wo + b;
      if (map != nullptr) map[flat] = lm;
      if (lm > -INFINITY) vote_argmax_merge(&bm, &bi, lm, flat);
    }
    ring[s0 * RC_TW + t] = 0.0;
    s0 = s0 + 1 == n ? 0 : s0 + 1;
  }
  vote_block_argmax<1>(&bm, &bi, shm, shi);
  if (t == 0) {
    bpart[blockIdx.x] = bm;
    ipart[blockIdx.x] = bi;
  }
}

// ---- launch 5: workgroup (k, l): the ball of centre k (k = K: the ground truth) at level l, directly from E
__global__ __launch_bounds__(RC_NT) void vote_recall_centres_kernel(
    const double* __restrict__ E, int R, int Ho, int Wo, RcLevels lv, int L, const int32_t* __restrict__ centres, int K,
    const float* __restrict__ gt, const double* __restrict__ norm, float* __restrict__ centre_lm,
    float* __restrict__ gt_lm, int32_t* __restrict__ count) {
  __shared__ double shd[RC_WAVES];
  const int t = threadIdx.x, k = blockIdx.x, l = blockIdx.y;
  int r = 0, a = 0, b = 0;
  bool ok;
  float* out;
  float none;
  if (k < K) {
    r = centres[k * 3], a = centres[k * 3 + 1], b = centres[k * 3 + 2];
    ok = r >= 0 && r < R && a >= 0 && a < Ho && b >= 0 && b < Wo;
    out = centre_lm + (size_t)k * L + l;
    none = -INFINITY;
  } else {
    ok = vote_gt_cell(gt, R, Ho, Wo, &r, &a, &b);   // (vote_credible's cell: one rule)
    out = gt_lm + l;
    none = __int_as_float(0x7fc00000);
    if (l == 0 && t == 0) count[2] = ok ? 1 : 0;
  }
  if (!ok) {                                // (uniform) no address is formed from an empty row
    if (t == 0) *out = none;
    return;
  }
  const int rho2 = rc_pick(lv.rho2, l), half_r = rc_pick(lv.half_r, l);
  const int rho = rc_isqrt(rho2), side = 2 * rho + 1, cells = side * side;
  const size_t P = (size_t)Ho * Wo;
  double s = 0.0;
  for (int dr = -half_r; dr <= half_r; ++dr) {
    const double* plane = E + (size_t)vote_wrap(r + dr, R) * P;
    for (int i = t; i < cells; i += RC_NT) {
      const int ia = i / side;
      const int da = ia - rho, db = i - ia * side - rho;
      const int aa = a + da, bb = b + db;
      if (da * da + db * db <= rho2 && aa >= 0 && aa < Ho && bb >= 0 && bb < Wo) s += plane[(size_t)aa * Wo + bb];
    }
  }
  s = vote_block_sum<RC_WAVES>(s, shd);
  if (t == 0) *out = rc_log_mass(s, norm[0]);
}

// ---- launch 6: workgroup l folds level l's pairs
__global__ __launch_bounds__(RC_NT) void vote_recall_finish_kernel(int Ho, int Wo, int groups,
                                                                   const float* __restrict__ bpart,
                                                                   const int32_t* __restrict__ ipart,
                                                                   int32_t* __restrict__ best_index,
                                                                   float* __restrict__ best_lm) {
  __shared__ float shm[RC_WAVES];
  __shared__ int shi[RC_WAVES];
  const int l = blockIdx.x;
  float m;
  int i;
  vote_fold_argmax<RC_WAVES, 1, 1>(bpart + (size_t)l * groups, 0, ipart + (size_t)l * groups, 0, groups, &m, &i, shm,
                                   shi);
  if (threadIdx.x == 0) {
    const int P = Ho * Wo;
    const bool any = i != VOTE_NO_INDEX;
    const int r = any ? i / P : -1;
    const int p = any ? i - r * P : 0;
    const int a = any ? p / Wo : -1;
    best_index[l * 3] = r;
    best_index[l * 3 + 1] = a;
    best_index[l * 3 + 2] = any ? p - a * Wo : -1;
    best_lm[l] = any ? m : -INFINITY;
  }
}

struct RcPlan {
  VotePlan cell;                            // launches 1, 2: one tile = 256 consecutive pixels of one rotation
  int ctiles, chunks, groups;               // launch 4: column tiles, row chunks, workgroups = R * chunks * ctiles
};

bool rc_plan(int R, int Ho, int Wo, int K, int L, RcPlan* plan) {
  if (R < 1 || R > RC_MAX_R || Ho < 1 || Wo < 1 || K < 0 || K > RC_MAX_K || L < 1 || L > RC_MAX_L) return false;
  if (!vote_plan((int64_t)R * Ho * Wo, R, Ho, Wo, RC_NT, RC_MAX_GROUPS, &plan->cell)) return false;
  plan->ctiles = (int)snap_cdiv(Wo, RC_TW);
  plan->chunks = (int)snap_cdiv(Ho, RC_CH);
  plan->groups = R * plan->chunks * plan->ctiles;   // <= R Ho Wo
  return true;
}

bool rc_levels_ok(int R, const int32_t* rho2, const int32_t* half_r, int L) {
  for (int l = 0; l < L; ++l) {
    if (rho2[l] < 0 || rho2[l] > RC_MAX_RHO2) return false;
    if (half_r[l] < 0 || half_r[l] > RC_MAX_HALF_R || 2 * half_r[l] + 1 > R) return false;
  }
  return true;
}

// E [R Ho Wo] float64 | the sums of launch 2 | norm | the maxima and counts of launch 1 | [L][groups] pairs of launch 4
struct RcWorkspace {
  double* E;
  double* dpart;
  double* norm;
  float* fpart;
  int32_t* cpart;
  float* bpart;
  int32_t* ipart;
  size_t bytes;
};

RcWorkspace rc_workspace(int R, int L, const RcPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  const size_t pairs = (size_t)L * plan.groups;
  return {l.take<double>((size_t)R * plan.cell.P), l.take<double>(RC_MAX_GROUPS), l.take<double>(2),
          l.take<float>(RC_MAX_GROUPS),            l.take<int32_t>(RC_MAX_GROUPS * 2), l.take<float>(pairs),
          l.take<int32_t>(pairs),                  l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_recall_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t K, int32_t L) {
  RcPlan plan;
  if (!rc_plan(R, Ho, Wo, K, L, &plan)) return 0;
  return rc_workspace(R, L, plan, nullptr).bytes;
}

extern "C" int snap_vote_recall_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale,
                                    const int32_t* rho2, const int32_t* half_r, int32_t L, const int32_t* centres,
                                    int32_t K, const float* gt_index, int32_t* best_index, float* best_log_mass,
                                    float* centre_log_mass, float* gt_log_mass, float* stats, int32_t* count,
                                    float* maps, void* workspace, size_t workspace_bytes, void* stream) {
  if (!votes || !rho2 || !half_r || !best_index || !best_log_mass || !gt_log_mass || !stats || !count || !workspace)
    return SNAP_ERR_NULL;
  if (K > 0 && (!centres || !centre_log_mass)) return SNAP_ERR_NULL;
  RcPlan plan;
  if (!rc_plan(R, Ho, Wo, K, L, &plan) || !rc_levels_ok(R, rho2, half_r, L)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale > 0.f) || !(scale < INFINITY)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, rc_workspace(R, L, plan, nullptr).bytes))
    return SNAP_ERR_WORKSPACE;
  const RcWorkspace w = rc_workspace(R, L, plan, workspace);
  const VotePlan& c = plan.cell;
  RcLevels lv = {};
  for (int l = 0; l < L; ++l) {
    lv.rho2[l] = rho2[l];
    lv.half_r[l] = half_r[l];
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vote_recall_max_kernel, dim3(c.groups), dim3(RC_NT), 0, s, votes, c.P, c.tiles_per_plane, c.tiles,
                     w.fpart, w.cpart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_recall_exp_kernel, dim3(c.groups), dim3(RC_NT), 0, s, votes, c.P, c.tiles_per_plane, c.tiles,
                     c.groups, scale, w.fpart, w.E, w.dpart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_recall_norm_kernel, dim3(1), dim3(RC_NT), 0, s, c.groups, scale, w.fpart, w.dpart, w.cpart,
                     w.norm, stats, count);
  SNAP_CHECK_LAUNCH();
  const size_t cells = (size_t)R * c.P;
  for (int l = 0; l < L; ++l) {
    const int rho = rc_isqrt(rho2[l]);
    const size_t lds = ((size_t)(2 * rho + 1) * RC_TW + 2 * (size_t)(RC_TW + 2 * rho)) * sizeof(double);
    hipLaunchKernelGGL(vote_recall_disc_kernel, dim3(plan.groups), dim3(RC_TW), lds, s, w.E, R, Ho, Wo, plan.ctiles,
                       plan.chunks, rho2[l], rho, half_r[l], w.norm, maps != nullptr ? maps + (size_t)l * cells : nullptr,
                       w.bpart + (size_t)l * plan.groups, w.ipart + (size_t)l * plan.groups);
    SNAP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(vote_recall_centres_kernel, dim3(K + 1, L), dim3(RC_NT), 0, s, w.E, R, Ho, Wo, lv, L, centres, K,
                     gt_index, w.norm, centre_log_mass, gt_log_mass, count);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_recall_finish_kernel, dim3(L), dim3(RC_NT), 0, s, Ho, Wo, plan.groups, w.bpart, w.ipart,
                     best_index, best_log_mass);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
