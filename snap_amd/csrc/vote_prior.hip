// A position / heading PRIOR fused into a vote volume or belief: snap_vote_prior_f32 (include/snap_hip.h).
//
// votes [R, Ho, Wo] f32 are log-scores (or NULL: every cell 0); the prior is a mixture of M <= 8 components, each a
// Gaussian in the plane whose centre depends on the rotation (the sensor does not sit at the grid's centre) times a von
// Mises factor per rotation, given as host-built tables (pose_exhaustive_voting.pose_prior).  With u the unnormalised
// log-prior of a cell and t = fl32(fl32(scale v) + u) over the FINITE cells F (vote_posterior's rule), the op returns
// out = t - log_z, the normalisers of the product, of the votes alone and of the prior alone (over the lattice and over
// F), E_post[u] and the components' responsibilities.
//
//   launch 1  vote_prior_max_kernel   <M>: tiles of 256 consecutive pixels, one pixel per thread, which walks its R
//             cells: u for EVERY cell (the prior's own normaliser runs over the whole lattice), t for the cells of F,
//             written to `out` (-inf elsewhere) so that launch 4 evaluates no mixture.  Per workgroup: max t, max u,
//             max fl32(scale v) and the two counts.
//   launch 2  vote_prior_sums_kernel  <M>: every workgroup folds the three maxima (maxima: exact); the same walk, u and
//             the M terms again by the SAME device function (the same bits).  Per pixel the <= R terms of a sum whose
//             terms have one sign are added in f32, then into the thread's float64 accumulators (registers; M is a
//             template parameter); e u, whose sign is not fixed under rounding, goes into float64 cell by cell.  ONE
//             partial row of 5 + M float64 and one count per workgroup.
//   launch 3  vote_prior_finish_kernel  one workgroup folds the rows column by column (vote_fold_sum) -> stats, resp,
//             count.
//   launch 4  vote_prior_norm_kernel  out = fl32(t - log_z) in place, four cells per thread where they are aligned.
// The tables (M R centre records, M R plane constants, M precisions) are staged in LDS once per workgroup and read at
// addresses that are the same in every lane.  A thread's pixel is fixed while it walks the rotations, and the centre
// changes with the rotation, so there is no column loop to hoist the row part of the quadratic out of; the seven
// multiply-adds of the quadratic are spent per (cell, component).
// No atomics, no hand-off between workgroups inside a launch: every sum's order is a function of (R, Ho, Wo, M) alone.
#include "vote_common.h"

namespace {

constexpr int PR_NT = 256;                  // threads of every launch; launches 1 and 2: pixels of a tile
constexpr int PR_WAVES = PR_NT / SNAP_WAVE;
constexpr int PR_MAX_R = 64;
constexpr int PR_MAX_M = 8;
constexpr int PR_MAX_GROUPS = 1024;         // workgroups of launches 1, 2 and 4
constexpr int PR_COLS = 16;                 // a partial row: S0, S1, Sprior, SpriorF, Svotes, pad x 3, resp[8]
constexpr int PR_RESP = 8;                  // first responsibility column

struct PrTables {
  const int32_t* centres;                   // [M, R, 2] (n_a, n_b)
  const float* planes;                      // [M, R, 3] (f_a, f_b, y)
  const float* comps;                       // [M, 4]    (Pxx, Pxy, Pyy, log w)
};

// The tables as the walk reads them: record i = m R + k.
template <int M>
struct PrLds {
  int n[M * PR_MAX_R][2];
  float f[M * PR_MAX_R][2];
  float c[M * PR_MAX_R];                    // fl32(log w_m + y_mk)
  float P[M][3];                            // Pxx, 2 Pxy (exact), Pyy
};

template <int M>
__device__ __forceinline__ void pr_stage(const PrTables& tb, int R, PrLds<M>* L) {
  for (int i = threadIdx.x; i < M * R; i += PR_NT) {
    L->n[i][0] = tb.centres[2 * i];
    L->n[i][1] = tb.centres[2 * i + 1];
    L->f[i][0] = tb.planes[3 * i];
    L->f[i][1] = tb.planes[3 * i + 1];
    L->c[i] = tb.comps[4 * (i / R) + 3] + tb.planes[3 * i + 2];
  }
  if (threadIdx.x < M) {
    L->P[threadIdx.x][0] = tb.comps[4 * threadIdx.x];
    L->P[threadIdx.x][1] = 2.f * tb.comps[4 * threadIdx.x + 1];
    L->P[threadIdx.x][2] = tb.comps[4 * threadIdx.x + 2];
  }
  __syncthreads();
}

// The M terms and u of the cell (k, a, b): the header's rounding points, one IEEE f32 operation each.
template <int M>
__device__ __forceinline__ float pr_prior(const PrLds<M>& L, int R, int k, int a, int b, float (&term)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int i = m * R + k;
    const float da = (float)(a - L.n[i][0]) - L.f[i][0];
    const float db = (float)(b - L.n[i][1]) - L.f[i][1];
    const float q = ((L.P[m][0] * da) * da + (L.P[m][1] * da) * db) + (L.P[m][2] * db) * db;
    term[m] = L.c[i] - 0.5f * q;
  }
  if constexpr (M == 1) {
    return term[0];
  } else {
    float mx = term[0];
#pragma unroll
    for (int m = 1; m < M; ++m) mx = fmaxf(mx, term[m]);
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) s += expf(term[m] - mx);
    return mx + logf(s);
  }
}

// ---- launch 1: t into `out`; the three maxima and the counts, per workgroup
template <int M>
__global__ __launch_bounds__(PR_NT) void vote_prior_max_kernel(const float* __restrict__ votes, int R, int P, int Wo,
                                                               float scale, int tiles, PrTables tb,
                                                               float* __restrict__ out, float* __restrict__ fpart,
                                                               int32_t* __restrict__ cpart) {
  __shared__ PrLds<M> L;
  __shared__ float shm[PR_WAVES];
  __shared__ int shc[PR_WAVES][2];
  pr_stage<M>(tb, R, &L);
  float tmax = -INFINITY, umax = -INFINITY, xmax = -INFINITY;
  int n_ok = 0, n_bad = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int p;
    if (!vote_tile_pixel<PR_NT>(tile, P, &p)) continue;
    int a, b;
    vote_row_col(p, Wo, &a, &b);
    for (int r = 0; r < R; ++r) {
      const size_t cell = (size_t)r * P + p;
      const float v = votes != nullptr ? votes[cell] : 0.f;
      float term[M];
      const float u = pr_prior<M>(L, R, r, a, b, term);
      umax = fmaxf(umax, u);
      float t = -INFINITY;
      if (vote_finite(v)) {
        const float x = votes != nullptr ? scale * v : 0.f;
        t = x + u;
        xmax = fmaxf(xmax, x);
        tmax = fmaxf(tmax, t);
        ++n_ok;
      } else if (!(v == -INFINITY)) {
        ++n_bad;                            // NaN or +inf
      }
      out[cell] = t;
    }
  }
  tmax = vote_block_max<PR_WAVES>(tmax, shm);
  umax = vote_block_max<PR_WAVES>(umax, shm);
  xmax = vote_block_max<PR_WAVES>(xmax, shm);
  const int c = vote_block_count_pair<PR_WAVES>(n_ok, n_bad, shc);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * 3] = tmax;
    fpart[(size_t)blockIdx.x * 3 + 1] = umax;
    fpart[(size_t)blockIdx.x * 3 + 2] = xmax;
  }
  if (threadIdx.x < 2) cpart[(size_t)blockIdx.x * 2 + threadIdx.x] = c;
}

// ---- launch 2: the 5 + M sums of this workgroup's pixels, and its count of cells of F without mass
template <int M>
__global__ __launch_bounds__(PR_NT) void vote_prior_sums_kernel(const float* __restrict__ votes, int R, int P, int Wo,
                                                                float scale, int tiles, int groups1, PrTables tb,
                                                                const float* __restrict__ fpart,
                                                                double* __restrict__ part,
                                                                int32_t* __restrict__ zpart) {
  __shared__ PrLds<M> L;
  __shared__ float shm[PR_WAVES];
  __shared__ double wred[PR_WAVES][PR_COLS];
  __shared__ int32_t shz[PR_WAVES];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  pr_stage<M>(tb, R, &L);
  const float tmax = vote_fold_max<PR_WAVES, 3>(fpart, 0, groups1, shm);
  const float umax = vote_fold_max<PR_WAVES, 3>(fpart, 1, groups1, shm);
  const float xmax = vote_fold_max<PR_WAVES, 3>(fpart, 2, groups1, shm);
  double a0 = 0.0, a1 = 0.0, ap = 0.0, apf = 0.0, av = 0.0, ar[M];
#pragma unroll
  for (int m = 0; m < M; ++m) ar[m] = 0.0;
  int n_zero = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int p;
    if (!vote_tile_pixel<PR_NT>(tile, P, &p)) continue;
    int a, b;
    vote_row_col(p, Wo, &a, &b);
    float s0 = 0.f, sp = 0.f, spf = 0.f, sv = 0.f, sr[M];
#pragma unroll
    for (int m = 0; m < M; ++m) sr[m] = 0.f;
    for (int r = 0; r < R; ++r) {
      const float v = votes != nullptr ? votes[(size_t)r * P + p] : 0.f;
      float term[M];
      const float u = pr_prior<M>(L, R, r, a, b, term);
      const float eu = expf(u - umax);
      sp += eu;
      if (vote_finite(v)) {
        const float x = votes != nullptr ? scale * v : 0.f;
        const float e = expf((x + u) - tmax);
        s0 += e;
        a1 += (double)e * (double)u;
        spf += eu;
        sv += expf(x - xmax);
        n_zero += e == 0.f ? 1 : 0;
#pragma unroll
        for (int m = 0; m < M; ++m) sr[m] += e * expf(term[m] - u);
      }
    }
    a0 += (double)s0;
    ap += (double)sp;
    apf += (double)spf;
    av += (double)sv;
#pragma unroll
    for (int m = 0; m < M; ++m) ar[m] += (double)sr[m];
  }
  {
    const double w0 = vote_wave_sum(a0), w1 = vote_wave_sum(a1), w2 = vote_wave_sum(ap), w3 = vote_wave_sum(apf),
                 w4 = vote_wave_sum(av);
    if (lane == 0) {
      wred[wave][0] = w0;
      wred[wave][1] = w1;
      wred[wave][2] = w2;
      wred[wave][3] = w3;
      wred[wave][4] = w4;
      wred[wave][5] = wred[wave][6] = wred[wave][7] = 0.0;
    }
  }
#pragma unroll
  for (int m = 0; m < PR_MAX_M; ++m) {
    double w = 0.0;
    if (m < M) w = vote_wave_sum(ar[m < M ? m : 0]);
    if (lane == 0) wred[wave][PR_RESP + m] = w;
  }
  n_zero = vote_wave_sum(n_zero);
  if (lane == 0) shz[wave] = n_zero;
  __syncthreads();
  if (t < PR_COLS) part[(size_t)blockIdx.x * PR_COLS + t] = (wred[0][t] + wred[1][t]) + (wred[2][t] + wred[3][t]);
  if (t == 0) zpart[blockIdx.x] = (shz[0] + shz[1]) + (shz[2] + shz[3]);
}

// ---- launch 3: one workgroup: stats, resp, count
__global__ __launch_bounds__(PR_NT) void vote_prior_finish_kernel(int M, int groups, const float* __restrict__ fpart,
                                                                  const int32_t* __restrict__ cpart,
                                                                  const double* __restrict__ part,
                                                                  const int32_t* __restrict__ zpart,
                                                                  double* __restrict__ resp,
                                                                  double* __restrict__ stats,
                                                                  int32_t* __restrict__ count) {
  __shared__ float shm[PR_WAVES];
  __shared__ double shd[PR_WAVES];
  __shared__ int32_t shc[PR_WAVES];
  const float tmax = vote_fold_max<PR_WAVES, 3>(fpart, 0, groups, shm);
  const float umax = vote_fold_max<PR_WAVES, 3>(fpart, 1, groups, shm);
  const float xmax = vote_fold_max<PR_WAVES, 3>(fpart, 2, groups, shm);
  const double S0 = vote_fold_sum<PR_WAVES, PR_COLS>(part, 0, groups, shd);
  const double S1 = vote_fold_sum<PR_WAVES, PR_COLS>(part, 1, groups, shd);
  const double Sp = vote_fold_sum<PR_WAVES, PR_COLS>(part, 2, groups, shd);
  const double Spf = vote_fold_sum<PR_WAVES, PR_COLS>(part, 3, groups, shd);
  const double Sv = vote_fold_sum<PR_WAVES, PR_COLS>(part, 4, groups, shd);
  double rs[PR_MAX_M];
  for (int m = 0; m < PR_MAX_M; ++m)        // (uniform trip count: the barriers inside are met by every thread)
    rs[m] = m < M ? vote_fold_sum<PR_WAVES, PR_COLS>(part, PR_RESP + m, groups, shd) : 0.0;
  const int32_t c0 = vote_fold_sum<PR_WAVES, 2>(cpart, 0, groups, shc);
  const int32_t c1 = vote_fold_sum<PR_WAVES, 2>(cpart, 1, groups, shc);
  const int32_t c2 = vote_fold_sum<PR_WAVES, 1>(zpart, 0, groups, shc);
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), ninf = -(double)INFINITY;
  const bool empty = !(tmax > -INFINITY);
  stats[0] = empty ? ninf : (double)tmax + log(S0);
  stats[1] = empty ? ninf : (double)xmax + log(Sv);
  stats[2] = (double)umax + log(Sp);
  stats[3] = empty ? ninf : (double)umax + log(Spf);   // (-inf where the prior has no f32 mass on F)
  stats[4] = empty ? nan : S1 / S0;
  stats[5] = stats[6] = stats[7] = 0.0;
  for (int m = 0; m < PR_MAX_M; ++m)
    if (m < M) resp[m] = empty ? nan : rs[m] / S0;
  count[0] = c0;
  count[1] = c1;
  count[2] = c2;
  count[3] = 0;
}

// ---- launch 4: out = t - log_z in place
__device__ __forceinline__ float pr_norm(float t, double log_z) {
  return t > -INFINITY ? (float)((double)t - log_z) : -INFINITY;
}
__global__ __launch_bounds__(PR_NT) void vote_prior_norm_kernel(float* __restrict__ out, int64_t n,
                                                                const double* __restrict__ stats) {
  const double log_z = stats[0];
  // the cells before the first 16-byte boundary and after the last whole group of four: one thread each
  int64_t head = (int64_t)((16 - reinterpret_cast<uintptr_t>(out) % 16) % 16 / 4);
  head = head < n ? head : n;
  const int64_t n4 = (n - head) / 4, stride = (int64_t)gridDim.x * PR_NT;
  const int64_t tail = head + n4 * 4;
  if (blockIdx.x == 0) {
    if (threadIdx.x < head) out[threadIdx.x] = pr_norm(out[threadIdx.x], log_z);
    const int64_t i = tail + ((int64_t)threadIdx.x - 64);
    if (threadIdx.x >= 64 && i < n) out[i] = pr_norm(out[i], log_z);
  }
  float4* out4 = reinterpret_cast<float4*>(out + head);
  for (int64_t i = (int64_t)blockIdx.x * PR_NT + threadIdx.x; i < n4; i += stride) {
    float4 q = out4[i];
    q.x = pr_norm(q.x, log_z);
    q.y = pr_norm(q.y, log_z);
    q.z = pr_norm(q.z, log_z);
    q.w = pr_norm(q.w, log_z);
    out4[i] = q;
  }
}

struct PrPlan {
  VotePlan pixel;                           // launches 1 and 2: one tile = 256 consecutive pixels, every rotation
  int norm_groups;
  int64_t cells;
};

bool pr_plan(int R, int Ho, int Wo, int M, PrPlan* plan) {
  if (R < 1 || R > PR_MAX_R || Ho < 1 || Wo < 1 || M < 1 || M > PR_MAX_M) return false;
  plan->cells = (int64_t)R * Ho * Wo;
  if (!vote_plan(plan->cells, 1, Ho, Wo, PR_NT, PR_MAX_GROUPS, &plan->pixel)) return false;
  const int64_t ng = snap_cdiv(plan->cells / 4 > 0 ? plan->cells / 4 : 1, PR_NT);
  plan->norm_groups = (int)(ng < PR_MAX_GROUPS ? ng : PR_MAX_GROUPS);
  return true;
}

// [groups][16] float64 partial rows | [groups][3] maxima | [groups][2] counts | [groups] counts of launch 2
struct PrWorkspace {
  double* part;
  float* fpart;
  int32_t* cpart;
  int32_t* zpart;
  size_t bytes;
};

PrWorkspace pr_workspace(const PrPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  const size_t g = plan.pixel.groups;
  return {l.take<double>(g * PR_COLS), l.take<float>(g * 3), l.take<int32_t>(g * 2), l.take<int32_t>(g), l.bytes};
}

template <int M>
void pr_launch_walks(const PrPlan& plan, const float* votes, int R, int Wo, float scale, const PrTables& tb, float* out,
                     const PrWorkspace& w, hipStream_t s) {
  const VotePlan& p = plan.pixel;
  hipLaunchKernelGGL(vote_prior_max_kernel<M>, dim3(p.groups), dim3(PR_NT), 0, s, votes, R, p.P, Wo, scale, p.tiles, tb,
                     out, w.fpart, w.cpart);
  hipLaunchKernelGGL(vote_prior_sums_kernel<M>, dim3(p.groups), dim3(PR_NT), 0, s, votes, R, p.P, Wo, scale, p.tiles,
                     p.groups, tb, w.fpart, w.part, w.zpart);
}

}  // namespace

extern "C" size_t snap_vote_prior_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t M) {
  PrPlan plan;
  if (!pr_plan(R, Ho, Wo, M, &plan)) return 0;
  return pr_workspace(plan, nullptr).bytes;
}

extern "C" int snap_vote_prior_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale, int32_t M,
                                   const int32_t* centres, const float* planes, const float* comps, float* out,
                                   double* resp, double* stats, int32_t* count, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!centres || !planes || !comps || !out || !resp || !stats || !count || !workspace) return SNAP_ERR_NULL;
  PrPlan plan;
  if (!pr_plan(R, Ho, Wo, M, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (votes != nullptr && (!(scale > 0.f) || !(scale < INFINITY))) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, pr_workspace(plan, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const PrWorkspace w = pr_workspace(plan, workspace);
  const PrTables tb = {centres, planes, comps};
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (M) {
#define PR_CASE(N) \
  case N: pr_launch_walks<N>(plan, votes, R, Wo, scale, tb, out, w, s); break;
    PR_CASE(1) PR_CASE(2) PR_CASE(3) PR_CASE(4) PR_CASE(5) PR_CASE(6) PR_CASE(7) PR_CASE(8)
#undef PR_CASE
  }
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_prior_finish_kernel, dim3(1), dim3(PR_NT), 0, s, M, plan.pixel.groups, w.fpart, w.cpart,
                     w.part, w.zpart, resp, stats, count);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_prior_norm_kernel, dim3(plan.norm_groups), dim3(PR_NT), 0, s, out, plan.cells, stats);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
