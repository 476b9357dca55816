// A road / lane RASTER prior fused into a vote volume or belief: snap_vote_raster_f32 (include/snap_hip.h).
//
// votes [R, Ho, Wo] f32 are log-scores (or NULL: every cell 0); the prior is a raster on the map grid, [X, Y, 4] f32 =
// (A, C, S, valid): a log-prior of position and a heading field kappa (cos, sin)(h phi).  In raster index units the
// cell (k, a, b) sits at (a, b) + n_k + f_k, one offset per rotation (models/votes/raster.raster_prior builds the table
// in float64), so the four bilinear weights are constants of the rotation plane.  g is the interpolated log-prior
// (`outside` where a tap of non-zero weight is off the raster or invalid), and for each of the S strengths of a ladder
// t_s = fl32(fl32(scale v) + fl32(lambda_s g)) over F = {v finite, g > -inf}.  The op returns out = t_w - log_z_w for
// one ladder index w and, per strength, log_z, the prior's own normaliser, E[g] and Var[g].
//
//   launch 1  vote_raster_max_kernel  <S>: tiles of 256 consecutive pixels, one pixel per thread, which walks its R
//             cells: g for EVERY cell, written to `out`, so that no later launch interpolates.  Per workgroup: the S
//             maxima of t_s, the largest g, the largest fl32(scale v), and three counts.
//   launch 2  vote_raster_sums_kernel <S>: every workgroup folds the maxima (maxima: exact); the same walk, g read back
//             from `out`.  Per pixel the <= R terms of a sum whose terms have one sign are added in f32, then into the
//             thread's float64 accumulators (registers; S is a template parameter, the ladder a by-value argument);
//             e g and (e g) g, whose signs are not fixed, go into float64 cell by cell.  ONE partial row of 4 S + 1
//             float64 and one count per workgroup.
//   launch 3  vote_raster_finish_kernel  one workgroup folds the rows column by column (vote_fold_sum) -> table, stats,
//             count, and reads the ground-truth cell's pair (g is still in `out`).
//   launch 4  vote_raster_norm_kernel  out = fl32(t_w - log_z_w) in place from (votes, g).
// The per-rotation table (n_k, the four weights, cos and sin of h theta_k) is staged in LDS once per workgroup and read
// at addresses that are the same in every lane; a tap is one 16-byte load, and neighbouring lanes read neighbouring taps.
// No atomics, no hand-off between workgroups inside a launch: every sum's order is a function of (R, Ho, Wo, S) alone.
#include "vote_common.h"

namespace {

constexpr int RS_NT = 256;                  // threads of every launch; launches 1 and 2: pixels of a tile
constexpr int RS_WAVES = RS_NT / SNAP_WAVE;
constexpr int RS_MAX_R = 64;
constexpr int RS_MAX_S = 8;
constexpr int RS_MAX_GROUPS = 1024;         // workgroups of launches 1, 2 and 4
constexpr int RS_FCOLS = RS_MAX_S + 2;      // a row of maxima: tmax_s x 8, gmax, xmax
constexpr int RS_GMAX = RS_MAX_S, RS_XMAX = RS_MAX_S + 1;
constexpr int RS_COLS = 4 * RS_MAX_S + 8;   // a partial row: level s owns columns 4 s .. 4 s + 3 = (S0, S1, S2, Sprior)
constexpr int RS_SV = 4 * RS_MAX_S;         // the votes' own sum
constexpr int64_t RS_MAX_RASTER = (int64_t)1 << 29;   // X Y below this: a tap's float index stays an int

struct RsLadder {
  float s[RS_MAX_S];
};
// Entry l of the by-value ladder (a select chain: no dynamically indexed copy of the kernel argument).
__device__ __forceinline__ float rs_pick(const RsLadder& ld, int l) {
  float x = ld.s[0];
#pragma unroll
  for (int i = 1; i < RS_MAX_S; ++i) x = i == l ? ld.s[i] : x;
  return x;
}

// The table as the walk reads it.
struct RsLds {
  int n[RS_MAX_R][2];
  float w[RS_MAX_R][4];                     // taps (0,0), (0,1), (1,0), (1,1)
  float cs[RS_MAX_R][2];                    // cos, sin of h theta_k
};

__device__ __forceinline__ void rs_stage(const int32_t* __restrict__ offsets, const float* __restrict__ planes, int R,
                                         RsLds* L) {
  for (int k = threadIdx.x; k < R; k += RS_NT) {
    const float fa = planes[4 * k], fb = planes[4 * k + 1];
    const float ga = 1.f - fa, gb = 1.f - fb;
    L->n[k][0] = offsets[2 * k];
    L->n[k][1] = offsets[2 * k + 1];
    L->w[k][0] = ga * gb;
    L->w[k][1] = ga * fb;
    L->w[k][2] = fa * gb;
    L->w[k][3] = fa * fb;
    L->cs[k][0] = planes[4 * k + 2];
    L->cs[k][1] = planes[4 * k + 3];
  }
  __syncthreads();
}

// g of the cell (k, a, b): the header's rounding points, one IEEE f32 operation each.  A tap of weight 0 is not read
// (the weights are the same in every lane: the branch is uniform); a tap off the raster is not read either.
__device__ __forceinline__ float rs_prior(const RsLds& L, const float4* __restrict__ raster, int X, int Y, float outside,
                                          int k, int a, int b) {
  const int64_t xa = (int64_t)a + L.n[k][0], yb = (int64_t)b + L.n[k][1];
  float bA = 0.f, bC = 0.f, bS = 0.f;
  bool ok = true;
#pragma unroll
  for (int tap = 0; tap < 4; ++tap) {
    const float w = L.w[k][tap];
    if (w != 0.f) {
      const int64_t x = xa + (tap >> 1), y = yb + (tap & 1);
      const bool in = x >= 0 && x < X && y >= 0 && y < Y;
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) q = raster[x * Y + y];
      ok = ok && in && q.w != 0.f;
      bA += w * q.x;
      bC += w * q.y;
      bS += w * q.z;
    }
  }
  const float g = (bA + L.cs[k][0] * bC) + L.cs[k][1] * bS;
  return ok ? g : outside;
}

// ---- launch 1: g into `out`; the maxima and the counts, per workgroup
template <int S>
__global__ __launch_bounds__(RS_NT) void vote_raster_max_kernel(const float* __restrict__ votes, int R, int P, int Wo,
                                                                float scale, int tiles,
                                                                const float4* __restrict__ raster, int X, int Y,
                                                                const int32_t* __restrict__ offsets,
                                                                const float* __restrict__ planes, float outside,
                                                                RsLadder ld, float* __restrict__ out,
                                                                float* __restrict__ fpart,
                                                                int32_t* __restrict__ cpart) {
  __shared__ RsLds L;
  __shared__ float shm[RS_WAVES];
  __shared__ int shc[RS_WAVES];
  rs_stage(offsets, planes, R, &L);
  float tmax[S], gmax = -INFINITY, xmax = -INFINITY;
#pragma unroll
  for (int l = 0; l < S; ++l) tmax[l] = -INFINITY;
  int n_ok = 0, n_bad = 0, n_cut = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int p;
    if (!vote_tile_pixel<RS_NT>(tile, P, &p)) continue;
    int a, b;
    vote_row_col(p, Wo, &a, &b);
    for (int r = 0; r < R; ++r) {
      const size_t cell = (size_t)r * P + p;
      const float v = votes != nullptr ? votes[cell] : 0.f;
      const float g = rs_prior(L, raster, X, Y, outside, r, a, b);
      gmax = fmaxf(gmax, g);
      if (vote_finite(v)) {
        const float x = votes != nullptr ? scale * v : 0.f;
        xmax = fmaxf(xmax, x);
        ++n_ok;
        if (g > -INFINITY) {
#pragma unroll
          for (int l = 0; l < S; ++l) tmax[l] = fmaxf(tmax[l], x + ld.s[l] * g);
        } else {
          ++n_cut;
        }
      } else if (!(v == -INFINITY)) {
        ++n_bad;                            // NaN or +inf
      }
      out[cell] = g;
    }
  }
  float* row = fpart + (size_t)blockIdx.x * RS_FCOLS;
#pragma unroll
  for (int l = 0; l < S; ++l) {
    const float m = vote_block_max<RS_WAVES>(tmax[l], shm);
    if (threadIdx.x == 0) row[l] = m;
  }
  gmax = vote_block_max<RS_WAVES>(gmax, shm);
  xmax = vote_block_max<RS_WAVES>(xmax, shm);
  n_ok = vote_block_sum<RS_WAVES>(n_ok, shc);
  n_bad = vote_block_sum<RS_WAVES>(n_bad, shc);
  n_cut = vote_block_sum<RS_WAVES>(n_cut, shc);
  if (threadIdx.x == 0) {
    row[RS_GMAX] = gmax;
    row[RS_XMAX] = xmax;
    cpart[(size_t)blockIdx.x * 3] = n_ok;
    cpart[(size_t)blockIdx.x * 3 + 1] = n_bad;
    cpart[(size_t)blockIdx.x * 3 + 2] = n_cut;
  }
}

// ---- launch 2: the 4 S + 1 sums of this workgroup's pixels, and its count of cells of F without mass at level w
template <int S>
__global__ __launch_bounds__(RS_NT) void vote_raster_sums_kernel(const float* __restrict__ votes, int R, int P,
                                                                 float scale, int tiles, int groups1, RsLadder ld,
                                                                 int write, const float* __restrict__ g_of,
                                                                 const float* __restrict__ fpart,
                                                                 double* __restrict__ part,
                                                                 int32_t* __restrict__ zpart) {
  __shared__ float shm[RS_WAVES];
  __shared__ double wred[RS_WAVES][4 * S + 1];
  __shared__ int32_t shz[RS_WAVES];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  float tmax[S], pmax[S];
#pragma unroll
  for (int l = 0; l < S; ++l) tmax[l] = vote_fold_max<RS_WAVES, RS_FCOLS>(fpart, l, groups1, shm);
  const float gmax = vote_fold_max<RS_WAVES, RS_FCOLS>(fpart, RS_GMAX, groups1, shm);
  const float xmax = vote_fold_max<RS_WAVES, RS_FCOLS>(fpart, RS_XMAX, groups1, shm);
#pragma unroll
  for (int l = 0; l < S; ++l) pmax[l] = ld.s[l] * gmax;   // (lambda > 0: the largest fl32(lambda g) is at the largest g)
  double a0[S], a1[S], a2[S], ap[S], av = 0.0;
#pragma unroll
  for (int l = 0; l < S; ++l) a0[l] = a1[l] = a2[l] = ap[l] = 0.0;
  int n_zero = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int p;
    if (!vote_tile_pixel<RS_NT>(tile, P, &p)) continue;
    float s0[S], sp[S], sv = 0.f;
#pragma unroll
    for (int l = 0; l < S; ++l) s0[l] = sp[l] = 0.f;
    for (int r = 0; r < R; ++r) {
      const size_t cell = (size_t)r * P + p;
      const float v = votes != nullptr ? votes[cell] : 0.f;
      const float g = g_of[cell];
      const bool on = g > -INFINITY;
      if (on) {
#pragma unroll
        for (int l = 0; l < S; ++l) sp[l] += expf(ld.s[l] * g - pmax[l]);
      }
      if (vote_finite(v)) {
        const float x = votes != nullptr ? scale * v : 0.f;
        sv += expf(x - xmax);
        if (on) {
          const double gd = (double)g;
#pragma unroll
          for (int l = 0; l < S; ++l) {
            const float e = expf((x + ld.s[l] * g) - tmax[l]);
            const double eg = (double)e * gd;
            s0[l] += e;
            a1[l] += eg;
            a2[l] += eg * gd;
            n_zero += (l == write && e == 0.f) ? 1 : 0;
          }
        }
      }
    }
#pragma unroll
    for (int l = 0; l < S; ++l) {
      a0[l] += (double)s0[l];
      ap[l] += (double)sp[l];
    }
    av += (double)sv;
  }
#pragma unroll
  for (int l = 0; l < S; ++l) {
    const double w0 = vote_wave_sum(a0[l]), w1 = vote_wave_sum(a1[l]), w2 = vote_wave_sum(a2[l]),
                 w3 = vote_wave_sum(ap[l]);
    if (lane == 0) {
      wred[wave][4 * l] = w0;
      wred[wave][4 * l + 1] = w1;
      wred[wave][4 * l + 2] = w2;
      wred[wave][4 * l + 3] = w3;
    }
  }
  av = vote_wave_sum(av);
  if (lane == 0) wred[wave][4 * S] = av;
  n_zero = vote_wave_sum(n_zero);
  if (lane == 0) shz[wave] = n_zero;
  __syncthreads();
  double* row = part + (size_t)blockIdx.x * RS_COLS;
  if (t < 4 * S) row[t] = (wred[0][t] + wred[1][t]) + (wred[2][t] + wred[3][t]);
  if (t == 4 * S) row[RS_SV] = (wred[0][t] + wred[1][t]) + (wred[2][t] + wred[3][t]);
  if (t == 0) zpart[blockIdx.x] = (shz[0] + shz[1]) + (shz[2] + shz[3]);
}

// ---- launch 3: one workgroup: table, stats, count
__global__ __launch_bounds__(RS_NT) void vote_raster_finish_kernel(const float* __restrict__ votes, float scale, int S,
                                                                   RsLadder ld, int64_t gt, int groups,
                                                                   const float* __restrict__ g_of,
                                                                   const float* __restrict__ fpart,
                                                                   const int32_t* __restrict__ cpart,
                                                                   const double* __restrict__ part,
                                                                   const int32_t* __restrict__ zpart,
                                                                   double* __restrict__ table,
                                                                   double* __restrict__ stats,
                                                                   int32_t* __restrict__ count) {
  __shared__ float shm[RS_WAVES];
  __shared__ double shd[RS_WAVES];
  __shared__ int32_t shc[RS_WAVES];
  const double nan = __longlong_as_double(0x7ff8000000000000ll), ninf = -(double)INFINITY;
  const float gmax = vote_fold_max<RS_WAVES, RS_FCOLS>(fpart, RS_GMAX, groups, shm);
  const float xmax = vote_fold_max<RS_WAVES, RS_FCOLS>(fpart, RS_XMAX, groups, shm);
  for (int l = 0; l < S; ++l) {             // (S is uniform: the barriers inside are met by every thread)
    const float tmax = vote_fold_max<RS_WAVES, RS_FCOLS>(fpart, l, groups, shm);
    const double S0 = vote_fold_sum<RS_WAVES, RS_COLS>(part, 4 * l, groups, shd);
    const double S1 = vote_fold_sum<RS_WAVES, RS_COLS>(part, 4 * l + 1, groups, shd);
    const double S2 = vote_fold_sum<RS_WAVES, RS_COLS>(part, 4 * l + 2, groups, shd);
    const double Sp = vote_fold_sum<RS_WAVES, RS_COLS>(part, 4 * l + 3, groups, shd);
    if (threadIdx.x == 0) {
      const bool empty = !(tmax > -INFINITY);
      const double mean = S1 / S0, var = S2 / S0 - mean * mean;
      double* row = table + (size_t)l * 4;
      row[0] = empty ? ninf : (double)tmax + log(S0);
      row[1] = gmax > -INFINITY ? (double)(rs_pick(ld, l) * gmax) + log(Sp) : ninf;
      row[2] = empty ? nan : mean;
      row[3] = empty ? nan : (var > 0.0 ? var : 0.0);
    }
  }
  const double Sv = vote_fold_sum<RS_WAVES, RS_COLS>(part, RS_SV, groups, shd);
  const int32_t c0 = vote_fold_sum<RS_WAVES, 3>(cpart, 0, groups, shc);
  const int32_t c1 = vote_fold_sum<RS_WAVES, 3>(cpart, 1, groups, shc);
  const int32_t c2 = vote_fold_sum<RS_WAVES, 3>(cpart, 2, groups, shc);
  const int32_t c3 = vote_fold_sum<RS_WAVES, 1>(zpart, 0, groups, shc);
  if (threadIdx.x != 0) return;
  double x_gt = nan, g_gt = nan;
  if (gt >= 0) {
    const float v = votes != nullptr ? votes[gt] : 0.f;
    if (vote_finite(v))
      x_gt = votes != nullptr ? (double)(scale * v) : 0.0;
    else if (v == -INFINITY)
      x_gt = ninf;
    g_gt = (double)g_of[gt];
  }
  stats[0] = xmax > -INFINITY ? (double)xmax + log(Sv) : ninf;
  stats[1] = x_gt;
  stats[2] = g_gt;
  stats[3] = 0.0;
  count[0] = c0;
  count[1] = c1;
  count[2] = c2;
  count[3] = c3;
}

// ---- launch 4: out = t_w - log_z_w in place, from (votes, g)
__global__ __launch_bounds__(RS_NT) void vote_raster_norm_kernel(const float* __restrict__ votes, float scale,
                                                                 float lambda, int write, int64_t n,
                                                                 const double* __restrict__ table, float* out) {
  const double log_z = table[(size_t)write * 4];
  const int64_t stride = (int64_t)gridDim.x * RS_NT;
  for (int64_t i = (int64_t)blockIdx.x * RS_NT + threadIdx.x; i < n; i += stride) {
    const float v = votes != nullptr ? votes[i] : 0.f;
    const float g = out[i];
    float o = -INFINITY;
    if (vote_finite(v) && g > -INFINITY) {
      const float x = votes != nullptr ? scale * v : 0.f;
      o = (float)((double)(x + lambda * g) - log_z);
    }
    out[i] = o;
  }
}

struct RsPlan {
  VotePlan pixel;                           // launches 1 and 2: one tile = 256 consecutive pixels, every rotation
  int norm_groups;
  int64_t cells;
};

bool rs_plan(int R, int Ho, int Wo, int X, int Y, int S, RsPlan* plan) {
  if (R < 1 || R > RS_MAX_R || Ho < 1 || Wo < 1 || X < 1 || Y < 1 || S < 1 || S > RS_MAX_S) return false;
  if ((int64_t)X * Y >= RS_MAX_RASTER) return false;
  plan->cells = (int64_t)R * Ho * Wo;
  if (!vote_plan(plan->cells, 1, Ho, Wo, RS_NT, RS_MAX_GROUPS, &plan->pixel)) return false;
  const int64_t ng = snap_cdiv(plan->cells, RS_NT);
  plan->norm_groups = (int)(ng < RS_MAX_GROUPS ? ng : RS_MAX_GROUPS);
  return true;
}

// [groups][40] float64 partial rows | [groups][10] maxima | [groups][3] counts | [groups] counts of launch 2
struct RsWorkspace {
  double* part;
  float* fpart;
  int32_t* cpart;
  int32_t* zpart;
  size_t bytes;
};

RsWorkspace rs_workspace(const RsPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  const size_t g = plan.pixel.groups;
  return {l.take<double>(g * RS_COLS), l.take<float>(g * RS_FCOLS), l.take<int32_t>(g * 3), l.take<int32_t>(g),
          l.bytes};
}

template <int S>
void rs_launch_walks(const RsPlan& plan, const float* votes, int R, int Wo, float scale, const float* raster, int X,
                     int Y, const int32_t* offsets, const float* planes, float outside, const RsLadder& ld, int write,
                     float* out, const RsWorkspace& w, hipStream_t s) {
  const VotePlan& p = plan.pixel;
  hipLaunchKernelGGL(vote_raster_max_kernel<S>, dim3(p.groups), dim3(RS_NT), 0, s, votes, R, p.P, Wo, scale, p.tiles,
                     reinterpret_cast<const float4*>(raster), X, Y, offsets, planes, outside, ld, out, w.fpart,
                     w.cpart);
  hipLaunchKernelGGL(vote_raster_sums_kernel<S>, dim3(p.groups), dim3(RS_NT), 0, s, votes, R, p.P, scale, p.tiles,
                     p.groups, ld, write, out, w.fpart, w.part, w.zpart);
}

}  // namespace

extern "C" size_t snap_vote_raster_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t X, int32_t Y,
                                                   int32_t S) {
  RsPlan plan;
  if (!rs_plan(R, Ho, Wo, X, Y, S, &plan)) return 0;
  return rs_workspace(plan, nullptr).bytes;
}

extern "C" int snap_vote_raster_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale,
                                    const float* raster, int32_t X, int32_t Y, const int32_t* offsets,
                                    const float* planes, float outside, const float* strengths, int32_t S,
                                    int32_t write, int64_t gt_index, float* out, double* table, double* stats,
                                    int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  if (!raster || !offsets || !planes || !strengths || !out || !table || !stats || !count || !workspace)
    return SNAP_ERR_NULL;
  RsPlan plan;
  if (!rs_plan(R, Ho, Wo, X, Y, S, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (write < 0 || write >= S || gt_index < -1 || gt_index >= plan.cells) return SNAP_ERR_BAD_SHAPE;
  if (reinterpret_cast<uintptr_t>(raster) % 16 != 0) return SNAP_ERR_UNSUPPORTED;
  if (votes != nullptr && (!(scale > 0.f) || !(scale < INFINITY))) return SNAP_ERR_UNSUPPORTED;
  if (!(outside < INFINITY)) return SNAP_ERR_UNSUPPORTED;   // (NaN and +inf)
  RsLadder ld = {};
  for (int l = 0; l < S; ++l) {
    const float x = strengths[l];
    if (!(x > 0.f) || !(x < INFINITY)) return SNAP_ERR_UNSUPPORTED;
    ld.s[l] = x;
  }
  if (!vote_workspace_ok(workspace, workspace_bytes, rs_workspace(plan, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const RsWorkspace w = rs_workspace(plan, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (S) {
#define RS_CASE(N)                                                                                                \
  case N:                                                                                                         \
    rs_launch_walks<N>(plan, votes, R, Wo, scale, raster, X, Y, offsets, planes, outside, ld, write, out, w, s); \
    break;
    RS_CASE(1) RS_CASE(2) RS_CASE(3) RS_CASE(4) RS_CASE(5) RS_CASE(6) RS_CASE(7) RS_CASE(8)
#undef RS_CASE
  }
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_raster_finish_kernel, dim3(1), dim3(RS_NT), 0, s, votes, scale, S, ld, (int64_t)gt_index,
                     plan.pixel.groups, out, w.fpart, w.cpart, w.part, w.zpart, table, stats, count);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_raster_norm_kernel, dim3(plan.norm_groups), dim3(RS_NT), 0, s, votes, scale, ld.s[write],
                     write, plan.cells, table, out);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
