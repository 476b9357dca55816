// Draws from exhaustive vote volumes: snap_vote_sample_f32 (B independent cells of softmax(scale * votes)) and
// snap_vote_sample_back_f32 (one backward step of forward-filter / backward-sample for B chains), include/snap_hip.h.
//
// The mass of a cell is the filter's: p = vp_mass(fl32(scale * v), M), M the largest finite fl32(scale * v).  A draw is
// the inverse CDF in lattice order, by a hierarchical descent: the plane sums, the row sums of the chosen plane, the
// cells of the chosen row with their masses recomputed.  Every level is the same routine (vs_pick): chunks of 64
// entries, a Kogge-Stone scan over the wave's lanes on top of the carry of the chunks before, and the entry taken is
// the FIRST ONE WITH MASS whose inclusive prefix exceeds the target; the target of the next level is what is left above
// the entry's exclusive prefix, clamped at 0.  A level whose prefixes end below the target (the levels' sums differ in
// their rounding) takes its last entry with mass.  So a cell without mass is never returned, the result is a function
// of the inputs alone, and it lies within rounding of the dense float64 CDF.
//
// snap_vote_sample_f32, four launches:
// Launch 1 (vote_sample_peak_kernel):  per workgroup the largest finite scaled vote and the count of NaN / +inf cells
//   (vp_peak_kernel with the product fused), min(tiles, 2048) workgroups of 256 threads.
// Launch 2 (vote_sample_rows_kernel):  every workgroup folds the partial maxima into M; one wave per (r, a) row: a chain
//   per lane over b = lane, lane + 64, .., then the xor butterfly -> the row's sum of p (float64) and cells with mass.
// Launch 3 (vote_sample_fold_kernel, one workgroup): one wave per plane, the same chain and butterfly over its rows ->
//   plane sums; Z = the carry after vs_pick's own scan over the planes; stats and count.
// Launch 4 (vote_sample_draw_kernel):  one wave per draw: the uniforms (Philox or given), the descent, log_prob.
// One read of the volume for M, one for the row sums; a draw reads R plane sums, Ho row sums and Wo cells.
//
// snap_vote_sample_back_f32, eight launches: the filter's predict step (vp_launch_predict: the four kernels of
// vote_predict.h on the filter's grid, so M, sum p and S are the filter's bits; t0 and t2 live in one volume of
// the workspace, t1 in another); launches 2 and 3 above on the belief (scale 1: the product is exact); then
// (vote_sample_chain_kernel) one 256-thread workgroup per chain: the window's (tk, ta) row sums, a chain over tb each,
// into LDS (<= 512 float64), then wave 0 alone: W by vs_pick's scan, the branch, and either the descent above on the
// belief or vs_pick over the row sums and over the chosen row's <= 32 entries recomputed; last
// (vote_sample_count_kernel, one workgroup) the counts over the chains.
// No atomics and no inter-workgroup hand-off inside a launch; every sum's order is fixed by the shape.
// Measured on an MI355X at [36, 511, 511], whole calls: vote_sample 0.081 ms at B = 1024 and 0.192 ms at B = 65536
// (torch.softmax + torch.multinomial alongside: 10.4 ms), vote_sample_back 0.320 ms at B = 1024 with taps [8, 8, 8];
// at [36, 31, 33] and B = 65536 the draws themselves are the time, 0.067 ms against torch's 0.050 ms
// (profiles/vote_sample_bench.json).
#include "philox.h"
#include "vote_predict.h"

namespace {

constexpr int VS_NT = VP_NT;
constexpr int VS_WAVES = VP_WAVES;
constexpr int VS_MAX_B = 1 << 20;
constexpr int VS_MAX_WINDOW_ROWS = VP_MAX_TK * VP_MAX_TXY;

// per-workgroup partials: float [groups][1]; int32 [groups][1] (a) or [groups][2] (b); double [groups][2] (b)
constexpr int VS_FS = 1, VS_IS_DRAW = 1, VS_IS_BACK = 2, VS_DS = 2;
// the totals a single workgroup leaves for the draws: double [4]
enum { VS_T_Z = 0, VS_T_PEAK = 1, VS_T_SUMT2 = 2, VS_T_SUMP = 3, VS_TOTALS = 4 };

// ------------------------------- the scan and the pick ----------------------------------------
// Inclusive prefix over the 64 lanes (Kogge-Stone: lane i ends with a fixed tree over lanes 0 .. i).
__device__ __forceinline__ double vs_wave_scan(double v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// The sum of x(0 .. count - 1) as vs_pick sees it: the carry after the last chunk.  One whole wave, uniform arguments.
template <typename F>
__device__ __forceinline__ double vs_total(int count, F&& x) {
  const int lane = threadIdx.x & 63;
  double carry = 0.0;
  for (int64_t base = 0; base < count; base += 64) {
    const int64_t i = base + lane;
    const double v = i < count ? x((int)i) : 0.0;
    carry = __shfl(carry + vs_wave_scan(v, lane), 63);
  }
  return carry;
}

// The first entry with x > 0 whose inclusive prefix exceeds t, and its exclusive prefix; the last entry with x > 0 when
// no prefix does; at = -1 when no entry has x > 0.  One whole wave, uniform arguments; the result is uniform.
struct VsPick {
  int at;
  double below;
};
template <typename F>
__device__ __forceinline__ VsPick vs_pick(int count, double t, F&& x) {
  const int lane = threadIdx.x & 63;
  double carry = 0.0;
  VsPick last = {-1, 0.0};
  for (int64_t base = 0; base < count; base += 64) {
    const int64_t i = base + lane;
    const double v = i < count ? x((int)i) : 0.0;
    const double incl = carry + vs_wave_scan(v, lane);
    double excl = __shfl_up(incl, 1);
    if (lane == 0) excl = carry;
    const unsigned long long has = __ballot(v > 0.0);
    const unsigned long long hit = __ballot(v > 0.0 && incl > t);
    if (hit != 0) {
      const int l = __ffsll((long long)hit) - 1;
      return {(int)base + l, __shfl(excl, l)};
    }
    if (has != 0) {
      const int l = 63 - __clzll((long long)has);
      last.at = (int)base + l;
      last.below = __shfl(excl, l);
    }
    carry = __shfl(incl, 63);
  }
  return last;
}
__device__ __forceinline__ double vs_left(double t, double below) { return fmax(t - below, 0.0); }

// One draw from the masses of `votes` by the uniform u: the linear index, -1 when no cell has mass.  One whole wave.
struct VsVolume {
  const float* votes;
  float scale, M;
  int R, Ho, Wo;
  const double* planesum;   // [R]
  const double* rowsum;     // [R Ho]
  double Z;
};
__device__ __forceinline__ int vs_draw(const VsVolume& v, double u) {
  if (!(v.Z > 0.0)) return -1;
  double t = u * v.Z;
  const VsPick plane = vs_pick(v.R, t, [&](int i) { return v.planesum[i]; });
  if (plane.at < 0) return -1;
  t = vs_left(t, plane.below);
  const double* rows = v.rowsum + (size_t)plane.at * v.Ho;
  const VsPick row = vs_pick(v.Ho, t, [&](int i) { return rows[i]; });
  if (row.at < 0) return -1;
  t = vs_left(t, row.below);
  const float* cells = v.votes + ((int64_t)plane.at * v.Ho + row.at) * v.Wo;
  const VsPick cell = vs_pick(v.Wo, t, [&](int i) { return (double)vp_mass(v.scale * cells[i], v.M); });
  if (cell.at < 0) return -1;
  return (int)(((int64_t)plane.at * v.Ho + row.at) * v.Wo + cell.at);   // (< 2^31: vote_plan)
}

// (u0, u1) of draw b: read from `uniforms` [B, 2] or built from Philox(counter (b, stream, purpose, 0); key = seed).
__device__ __forceinline__ void vs_uniforms(const double* __restrict__ uniforms, int b, uint64_t seed, int32_t stream,
                                            uint32_t purpose, double* u0, double* u1) {
  if (uniforms) {
    *u0 = uniforms[(size_t)b * 2];
    *u1 = uniforms[(size_t)b * 2 + 1];
  } else {
    uint32_t x[4];
    philox4x32_10((uint32_t)b, (uint32_t)stream, purpose, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    *u0 = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * (1.0 / 9007199254740992.0);
    *u1 = ((double)(x[2] >> 5) * 67108864.0 + (double)(x[3] >> 6)) * (1.0 / 9007199254740992.0);
  }
}

// ---- launch 1 of snap_vote_sample_f32: vp_peak_kernel on fl32(scale * votes)
__global__ __launch_bounds__(VS_NT) void vote_sample_peak_kernel(const float* __restrict__ votes, float scale, int n,
                                                                 float* __restrict__ fpart, int32_t* __restrict__ ipart) {
  __shared__ float shf[VS_WAVES];
  __shared__ int shi[VS_WAVES];
  float m = -INFINITY;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * VS_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * VS_NT) {
    const float v = scale * votes[i];
    if (vote_finite(v))
      m = fmaxf(m, v);
    else if (!(v == -INFINITY))
      ++bad;                                // NaN or +inf
  }
  m = vote_block_max<VS_WAVES>(m, shf);
  bad = vote_block_sum<VS_WAVES>(bad, shi);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * VS_FS + VP_F_PEAK] = m;
    ipart[(size_t)blockIdx.x * VS_IS_DRAW + VP_I_BAD] = bad;
  }
}

// ---- the row sums of p, one wave per (r, a) row; rowcnt (the cells with mass) may be NULL
__global__ __launch_bounds__(VS_NT) void vote_sample_rows_kernel(const float* __restrict__ votes, float scale,
                                                                 int64_t rows, int Wo, const float* __restrict__ fpart,
                                                                 int groups, double* __restrict__ rowsum,
                                                                 int32_t* __restrict__ rowcnt) {
  __shared__ float shf[VS_WAVES];
  const float M = vote_fold_max<VS_WAVES, VS_FS>(fpart, VP_F_PEAK, groups, shf);
  const int64_t row = (int64_t)blockIdx.x * VS_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;                  // (after the fold's barriers)
  const float* src = votes + row * Wo;
  double s = 0.0;
  int c = 0;
  for (int64_t b = threadIdx.x & 63; b < Wo; b += 64) {
    const float m = vp_mass(scale * src[b], M);
    s += (double)m;
    c += m > 0.f ? 1 : 0;
  }
  s = vote_wave_sum(s);
  c = vote_wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    rowsum[row] = s;
    if (rowcnt) rowcnt[row] = c;
  }
}

// ---- one workgroup: plane sums, Z, and what the draws need of the per-workgroup partials.  BACK: entry point (b)
template <bool BACK>
__global__ __launch_bounds__(VS_NT) void vote_sample_fold_kernel(const double* __restrict__ rowsum,
                                                                 const int32_t* __restrict__ rowcnt, int R, int Ho,
                                                                 const float* __restrict__ fpart,
                                                                 const int32_t* __restrict__ ipart,
                                                                 const double* __restrict__ dpart, int groups,
                                                                 double* __restrict__ planesum, double* __restrict__ totals,
                                                                 float* __restrict__ stats, int32_t* __restrict__ count) {
  __shared__ float shf[VS_WAVES];
  __shared__ int shi[VS_WAVES];
  __shared__ double shd[VS_WAVES];
  __shared__ double shp[VP_MAX_R];          // the plane sums, for wave 0's scan
  constexpr int IS = BACK ? VS_IS_BACK : VS_IS_DRAW;
  const float M = vote_fold_max<VS_WAVES, VS_FS>(fpart, VP_F_PEAK, groups, shf);
  const int bad = vote_fold_sum<VS_WAVES, IS>(ipart, VP_I_BAD, groups, shi);
  double S = 0.0, sum_p = 0.0;
  if (BACK) {
    S = vote_fold_sum<VS_WAVES, VS_DS>(dpart, VP_D_SUMT2, groups, shd);
    sum_p = vote_fold_sum<VS_WAVES, VS_DS>(dpart, VP_D_SUMP, groups, shd);
  }
  const int lane = threadIdx.x & 63;
  int n_mass = 0;
  for (int r = threadIdx.x >> 6; r < R; r += VS_WAVES) {
    const double* rows = rowsum + (size_t)r * Ho;
    double s = 0.0;
    for (int64_t a = lane; a < Ho; a += 64) {
      s += rows[a];
      if (!BACK) n_mass += rowcnt[(size_t)r * Ho + a];
    }
    s = vote_wave_sum(s);
    if (lane == 0) {
      planesum[r] = s;
      shp[r] = s;
    }
  }
  n_mass = vote_block_sum<VS_WAVES>(n_mass, shi);   // (its barriers also publish shp to wave 0)
  if (threadIdx.x >= 64) return;
  const double Z = vs_total(R, [&](int i) { return shp[i]; });
  if (lane != 0) return;
  totals[VS_T_Z] = Z;
  totals[VS_T_PEAK] = (double)M;
  totals[VS_T_SUMT2] = S;
  totals[VS_T_SUMP] = sum_p;
  if (BACK) {
    stats[0] = sum_p > 0.0 ? (float)(S / sum_p) : 0.f;
    stats[1] = M;
    count[2] = bad;
  } else {
    stats[0] = (float)((double)M + log(Z));
    stats[1] = M;
    count[0] = n_mass;
    count[1] = bad;
  }
}

// ---- launch 4 of snap_vote_sample_f32: one wave per draw
__global__ __launch_bounds__(VS_NT) void vote_sample_draw_kernel(const float* __restrict__ votes, float scale, int R,
                                                                 int Ho, int Wo, const double* __restrict__ planesum,
                                                                 const double* __restrict__ rowsum,
                                                                 const double* __restrict__ totals, int B, uint64_t seed,
                                                                 int32_t stream, const double* __restrict__ uniforms,
                                                                 int32_t* __restrict__ index,
                                                                 float* __restrict__ log_prob) {
  const int64_t draw = (int64_t)blockIdx.x * VS_WAVES + (threadIdx.x >> 6);
  if (draw >= B) return;
  const VsVolume vol = {votes, scale, (float)totals[VS_T_PEAK], R, Ho, Wo, planesum, rowsum, totals[VS_T_Z]};
  double u0, u1;
  vs_uniforms(uniforms, (int)draw, seed, stream, 0u, &u0, &u1);
  const int at = vs_draw(vol, u0);
  if ((threadIdx.x & 63) != 0) return;
  index[draw] = at;
  log_prob[draw] = at < 0 ? -INFINITY : (float)(((double)(scale * votes[at]) - (double)vol.M) - log(vol.Z));
}

// ---- the chains of snap_vote_sample_back_f32: one workgroup per chain
struct VsWindow {
  const float* belief;
  const float* taps_k;
  const float* taps_a;      // row r
  const float* taps_b;      // row r
  int kfirst, la, lb, R, Ho, Wo, P, r, a, b;
  float M;
};
// The weight of window entry (tk, ta, tb) and its cell; 0 outside the volume.
__device__ __forceinline__ double vs_entry(const VsWindow& w, int tk, int ta, int tb, int* cell) {
  const int64_t sa = (int64_t)w.a + w.la + ta, sb = (int64_t)w.b + w.lb + tb;
  if (sa < 0 || sa >= w.Ho || sb < 0 || sb >= w.Wo) return 0.0;
  const int k = (w.r + w.kfirst + tk) % w.R;          // (r, kfirst < R <= 64, tk < 16)
  const int64_t at = (int64_t)k * w.P + sa * w.Wo + sb;
  *cell = (int)at;
  return (((double)w.taps_k[tk] * (double)w.taps_a[ta]) * (double)w.taps_b[tb]) * (double)vp_mass(w.belief[at], w.M);
}

__global__ __launch_bounds__(VS_NT) void vote_sample_chain_kernel(
    const float* __restrict__ belief, const float* __restrict__ taps_k, int lk, const float* __restrict__ taps_a,
    const float* __restrict__ taps_b, const int32_t* __restrict__ offsets, int R, int Ho, int Wo, int Tk, int Ta, int Tb,
    float eps, const double* __restrict__ planesum, const double* __restrict__ rowsum, const double* __restrict__ totals,
    const int32_t* __restrict__ next, uint64_t seed, int32_t stream, const double* __restrict__ uniforms,
    int32_t* __restrict__ prev, int32_t* __restrict__ jumped) {
  __shared__ double rows[VS_MAX_WINDOW_ROWS];
  const int chain = blockIdx.x;
  const int P = Ho * Wo, n = R * P;
  const int x = next[chain];
  if (x < 0 || x >= n) {                    // an ended chain stays ended (uniform over the workgroup)
    if (threadIdx.x == 0) {
      prev[chain] = -1;
      jumped[chain] = -1;
    }
    return;
  }
  VsWindow w;
  w.r = x / P;
  const int p = x - w.r * P;
  vote_row_col(p, Wo, &w.a, &w.b);
  w.belief = belief;
  w.taps_k = taps_k;
  w.taps_a = taps_a + (size_t)w.r * Ta;
  w.taps_b = taps_b + (size_t)w.r * Tb;
  w.kfirst = vote_mod(lk, R);
  w.la = offsets[(size_t)w.r * 2];
  w.lb = offsets[(size_t)w.r * 2 + 1];
  w.R = R, w.Ho = Ho, w.Wo = Wo, w.P = P;
  w.M = (float)totals[VS_T_PEAK];
  const int nrows = Tk * Ta;                // <= VS_MAX_WINDOW_ROWS: vp_plan
  for (int j = threadIdx.x; j < nrows; j += VS_NT) {
    const int tk = j / Ta, ta = j - tk * Ta;
    double s = 0.0;
    int cell;
    for (int tb = 0; tb < Tb; ++tb) s += vs_entry(w, tk, ta, tb, &cell);
    rows[j] = s;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const double W = vs_total(nrows, [&](int i) { return rows[i]; });
  const double S = totals[VS_T_SUMT2], sum_p = totals[VS_T_SUMP];
  const double A = S > 0.0 ? ((1.0 - (double)eps) * W) / S : 0.0;
  const double J = sum_p > 0.0 ? (double)eps / (double)n : 0.0;
  double u0, u1;
  vs_uniforms(uniforms, chain, seed, stream, 1u, &u0, &u1);
  int at = -1, jump = -1;
  if (A + J > 0.0) {
    if (u0 * (A + J) < J) {
      const VsVolume vol = {belief, 1.f, w.M, R, Ho, Wo, planesum, rowsum, totals[VS_T_Z]};
      at = vs_draw(vol, u1);
      jump = 1;
    } else {
      const double t = u1 * W;
      const VsPick row = vs_pick(nrows, t, [&](int i) { return rows[i]; });
      if (row.at >= 0) {
        const int tk = row.at / Ta, ta = row.at - tk * Ta;
        const VsPick entry = vs_pick(Tb, vs_left(t, row.below), [&](int i) {
          int cell;
          return vs_entry(w, tk, ta, i, &cell);
        });
        if (entry.at >= 0) {
          vs_entry(w, tk, ta, entry.at, &at);
          jump = 0;
        }
      }
    }
    if (at < 0) jump = -1;
  }
  if (threadIdx.x == 0) {
    prev[chain] = at;
    jumped[chain] = jump;
  }
}

// ---- the last launch of snap_vote_sample_back_f32: the counts over the chains (integers: any order)
__global__ __launch_bounds__(VS_NT) void vote_sample_count_kernel(const int32_t* __restrict__ prev,
                                                                  const int32_t* __restrict__ jumped, int B,
                                                                  int32_t* __restrict__ count) {
  __shared__ int shi[VS_WAVES];
  int with_prev = 0, jumps = 0;
  for (int i = threadIdx.x; i < B; i += VS_NT) {
    with_prev += prev[i] >= 0 ? 1 : 0;
    jumps += jumped[i] == 1 ? 1 : 0;
  }
  with_prev = vote_block_sum<VS_WAVES>(with_prev, shi);
  jumps = vote_block_sum<VS_WAVES>(jumps, shi);
  if (threadIdx.x == 0) {
    count[0] = with_prev;
    count[1] = jumps;
  }
}

// (a): [groups] f32 | [groups] int32 | [R Ho] float64 row sums | [R Ho] int32 row counts | [64] float64 plane sums |
//      [4] float64 totals
// (b): [R Ho Wo] f32 t0 / t2 | [R Ho Wo] f32 t1 | [groups] f32 | [groups][2] int32 | [groups][2] float64 |
//      [R Ho] float64 row sums | [64] float64 plane sums | [4] float64 totals
struct VsWorkspace {
  float* t02;
  float* t1;
  float* fpart;
  int32_t* ipart;
  double* dpart;
  double* rowsum;
  int32_t* rowcnt;
  double* planesum;
  double* totals;
  size_t bytes;
};

VsWorkspace vs_workspace(const VotePlan& plan, int R, int Ho, bool back, void* workspace) {
  VoteLayout l{workspace};
  const size_t n = (size_t)R * plan.P, rows = (size_t)R * Ho, g = (size_t)plan.groups;
  return {l.take<float>(back ? n : 0),
          l.take<float>(back ? n : 0),
          l.take<float>(g * VS_FS),
          l.take<int32_t>(g * (back ? VS_IS_BACK : VS_IS_DRAW)),
          l.take<double>(back ? g * VS_DS : 0),
          l.take<double>(rows),
          l.take<int32_t>(back ? 0 : rows),
          l.take<double>(VP_MAX_R),
          l.take<double>(VS_TOTALS),
          l.bytes};
}

bool vs_plan(int R, int Ho, int Wo, VotePlan* plan) {
  if (R < 1 || R > VP_MAX_R || Ho < 1 || Wo < 1) return false;
  return vote_plan((int64_t)R * Ho * Wo, R, Ho, Wo, VS_NT, VP_MAX_GROUPS, plan);
}

bool vs_draws_ok(int B) { return B >= 1 && B <= VS_MAX_B; }

}  // namespace

extern "C" size_t snap_vote_sample_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo) {
  VotePlan plan;
  if (!vs_plan(R, Ho, Wo, &plan)) return 0;
  return vs_workspace(plan, R, Ho, false, nullptr).bytes;
}

extern "C" int snap_vote_sample_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale, int32_t B,
                                    uint64_t seed, int32_t stream_id, const double* uniforms, int32_t* index,
                                    float* log_prob, float* stats, int32_t* count, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (!votes || !index || !log_prob || !stats || !count || !workspace) return SNAP_ERR_NULL;
  VotePlan plan;
  if (!vs_plan(R, Ho, Wo, &plan) || !vs_draws_ok(B)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale > 0.f) || !(scale < INFINITY)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, vs_workspace(plan, R, Ho, false, nullptr).bytes))
    return SNAP_ERR_WORKSPACE;
  const VsWorkspace w = vs_workspace(plan, R, Ho, false, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(VS_NT);
  const int64_t rows = (int64_t)R * Ho;
  hipLaunchKernelGGL(vote_sample_peak_kernel, dim3(plan.groups), block, 0, s, votes, scale, R * plan.P, w.fpart, w.ipart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_sample_rows_kernel, dim3((unsigned)snap_cdiv(rows, VS_WAVES)), block, 0, s, votes, scale, rows,
                     Wo, w.fpart, plan.groups, w.rowsum, w.rowcnt);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_sample_fold_kernel<false>, dim3(1), block, 0, s, w.rowsum, w.rowcnt, R, Ho, w.fpart, w.ipart,
                     (const double*)nullptr, plan.groups, w.planesum, w.totals, stats, count);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_sample_draw_kernel, dim3((unsigned)snap_cdiv(B, VS_WAVES)), block, 0, s, votes, scale, R, Ho,
                     Wo, w.planesum, w.rowsum, w.totals, B, seed, stream_id, uniforms, index, log_prob);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

extern "C" size_t snap_vote_sample_back_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta,
                                                        int32_t Tb) {
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return 0;
  return vs_workspace(plan, R, Ho, true, nullptr).bytes;
}

extern "C" int snap_vote_sample_back_f32(const float* belief, const float* taps_k, int32_t lk, const float* taps_a,
                                         const float* taps_b, const int32_t* offsets, int32_t R, int32_t Ho, int32_t Wo,
                                         int32_t Tk, int32_t Ta, int32_t Tb, float uniform_mix, const int32_t* next,
                                         int32_t B, uint64_t seed, int32_t stream_id, const double* uniforms,
                                         int32_t* prev, int32_t* jumped, float* stats, int32_t* count, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  if (!belief || !taps_k || !taps_a || !taps_b || !offsets || !next || !prev || !jumped || !stats || !count ||
      !workspace)
    return SNAP_ERR_NULL;
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, &plan) || !vs_draws_ok(B)) return SNAP_ERR_BAD_SHAPE;
  if (!(uniform_mix >= 0.f && uniform_mix <= 1.f)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, vs_workspace(plan, R, Ho, true, nullptr).bytes))
    return SNAP_ERR_WORKSPACE;
  const VsWorkspace w = vs_workspace(plan, R, Ho, true, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(VS_NT);
  const int64_t rows = (int64_t)R * Ho;
  const VpTaps taps = {taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb};
  const VpParts<VS_FS, VS_DS, VS_IS_BACK> part = {w.fpart, w.dpart, w.ipart};
  VP_CHECK(vp_launch_predict(plan, taps, belief, w.t02, w.t1, w.t02, part, s));   // t0, t1, t2
  hipLaunchKernelGGL(vote_sample_rows_kernel, dim3((unsigned)snap_cdiv(rows, VS_WAVES)), block, 0, s, belief, 1.f, rows,
                     Wo, w.fpart, plan.groups, w.rowsum, (int32_t*)nullptr);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_sample_fold_kernel<true>, dim3(1), block, 0, s, w.rowsum, (const int32_t*)nullptr, R, Ho,
                     w.fpart, w.ipart, w.dpart, plan.groups, w.planesum, w.totals, stats, count);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_sample_chain_kernel, dim3(B), block, 0, s, belief, taps_k, lk, taps_a, taps_b, offsets, R, Ho,
                     Wo, Tk, Ta, Tb, uniform_mix, w.planesum, w.rowsum, w.totals, next, seed, stream_id, uniforms, prev,
                     jumped);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_sample_count_kernel, dim3(1), block, 0, s, prev, jumped, B, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
