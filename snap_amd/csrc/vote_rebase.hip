// A vote volume or belief carried into another MAP frame: snap_vote_rebase_f32 (include/snap_hip.h).
//
// src [R, Ho, Wo] f32 is a log-space vote volume or belief (-inf = impossible pose).  Composing a change of map frame on
// the LEFT of every pose, n_t_q = n_t_m @ m_t_q, is in index space a constant circular shift in the rotation and one
// affine map of every plane, the same for all rotations.  The operator GATHERS: the destination cell (r, a, b) reads
// the source at k = r - dk (circular) and (sa, sb) = A (a, b) + o with the trilinear split of (k, sa, sb), on the
// MASSES p = fl32(exp(scale (v - M))), M the largest finite source value; dst = log(cell mass) - log(sum of the cell
// masses): normalised log-probabilities.  Everything above the f32 mass is float64.
//
// The 1-D launches tile each rotation's pixels p = a * Wo + b into runs of 256, one cell per thread, the gather tiles a
// plane into RB_T x RB_T blocks, one cell per thread; min(tiles, 2048) workgroups of 256 threads stride over the tiles.
// Launch 1 (vote_rebase_peak_kernel):      per workgroup the largest finite source value and the NaN / +inf count.
// Launch 2 (vote_rebase_gather_kernel):    every workgroup folds the maxima into M (a maximum: exact).  Per tile the
//   affine map is monotone in a and in b also as it is rounded, so the floors of (sa, sb) at the tile's four corners
//   bound those of every cell: the FOOTPRINT, at most (15 (|A00| + |A01|) + 2 rounded up) <= 24 cells a side for a
//   rotation.  Both source planes' footprints are staged in LDS as masses -- exp runs once per staged cell, 4.5 times
//   per destination cell at worst instead of 8 -- 0 outside the plane and for -inf, NaN for NaN / +inf; the 8-tap blend
//   reads LDS, a tap of weight 0 or outside the plane skipped before its read.  A footprint beyond the staging area (a
//   table that is no rotation) is read from the source directly, same expressions.  The f32 cell mass goes to dst; per
//   workgroup the float64 sums of the cell masses and of each thread's own SOURCE cell's mass, and the count of cells
//   with no tap.
// Launch 3 (vote_rebase_normalise_kernel): every workgroup folds the partial sums into S; dst = fl32(log(mass) -
//   log(S)) in place; per workgroup the counts of finite / NaN cells written and their maximum.
// Launch 4 (vote_rebase_finish_kernel, one workgroup): stats and count.
// LDS of a gather workgroup: 2 x 24 x 25 x 4 B = 4800 B (row stride 25: odd, so a rotated walk spreads over the
// banks), far below the 160 KiB / 2 that two workgroups per CU would allow: residency is set by the gather's 82
// VGPRs, five workgroups per CU, not by LDS.
// No atomics and no inter-workgroup hand-off inside a launch: every sum is a per-thread chain over its tiles, a wave
// tree, the four waves, then the workgroups in a strided chain per thread and the same tree -- an order fixed by
// (R, Ho, Wo) alone, so two calls give the same bytes.
// HBM traffic (n = R Ho Wo cells of 4 bytes): reads src once in launch 1, in launch 2 each thread's own cell and the
// footprints (2 planes x (24 / 16)^2 = 4.5 n cell reads at worst, all but ~2 n of them L2 hits among neighbouring
// tiles), the masses in launch 3; writes the masses and dst: about 5 n cells plus the L2 re-reads (an estimate).
#include "vote_common.h"

namespace {

constexpr int RB_NT = 256;                  // threads of every launch
constexpr int RB_WAVES = RB_NT / SNAP_WAVE;
constexpr int RB_T = 16;                    // the gather's tile: RB_T x RB_T destination cells of one plane
constexpr int RB_FP = 24;                   // staged footprint: cells a side (floor span <= ceil(15 sqrt 2) = 22, + 2)
constexpr int RB_FS = RB_FP + 1;            // its row stride in LDS
constexpr int RB_MAX_R = 64;
constexpr int RB_MAX_GROUPS = 2048;
static_assert(RB_T * RB_T == RB_NT, "one destination cell per thread");

// per-workgroup partials: double [groups][2], float [groups][2], int32 [groups][4]
constexpr int RB_DS = 2, RB_FSTR = 2, RB_IS = 4;
enum { RB_D_DST = 0, RB_D_SRC = 1 };
enum { RB_F_PEAK = 0, RB_F_TOP = 1 };
enum { RB_I_BAD = 0, RB_I_NOTAP = 1, RB_I_FIN = 2, RB_I_NAN = 3 };

struct RbMap {
  double dk, A00, A01, A10, A11, oa, ob;
};

// The mass of a source cell: 0 for -inf, NaN for NaN / +inf, else exp in float64 rounded once.
__device__ __forceinline__ float rb_mass(float v, double scale, double M) {
  if (v == -INFINITY) return 0.f;
  if (!(v < INFINITY)) return __int_as_float(0x7fc00000);
  return (float)exp(scale * ((double)v - M));
}

__device__ __forceinline__ double rb_sa(const RbMap& m, int a, int b) { return (m.A00 * (double)a + m.A01 * (double)b) + m.oa; }
__device__ __forceinline__ double rb_sb(const RbMap& m, int a, int b) { return (m.A10 * (double)a + m.A11 * (double)b) + m.ob; }

// floor(s) as an int where a tap at it or its successor can lie in [0, extent): s in [-1, extent); else false.
__device__ __forceinline__ bool rb_floor(double s, int extent, int* i, double* f) {
  if (!(s >= -1.0 && s < (double)extent)) return false;
  const double fl = floor(s);
  *i = (int)fl;
  *f = s - fl;
  return true;
}
// The same floor clamped to [-1, extent]: monotone in s, equal to rb_floor's where that holds.
__device__ __forceinline__ int rb_floor_clamped(double s, int extent) {
  const double fl = floor(s);
  return fl < -1.0 ? -1 : (fl > (double)extent ? extent : (int)fl);   // (a NaN cannot occur: the table is finite)
}

// ---- launch 1
__global__ __launch_bounds__(RB_NT) void vote_rebase_peak_kernel(const float* __restrict__ src, int P, int tpp,
                                                                 int tiles, float* __restrict__ fpart,
                                                                 int32_t* __restrict__ ipart) {
  __shared__ float shf[RB_WAVES];
  __shared__ int shi[RB_WAVES];
  float m;
  int n_ok, n_bad;
  vote_scan_max<RB_NT>(src, P, tpp, tiles, &m, &n_ok, &n_bad);
  m = vote_block_max<RB_WAVES>(m, shf);
  n_bad = vote_block_sum<RB_WAVES>(n_bad, shi);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * RB_FSTR + RB_F_PEAK] = m;
    ipart[(size_t)blockIdx.x * RB_IS + RB_I_BAD] = n_bad;
  }
}

// ---- launch 2
__global__ __launch_bounds__(RB_NT) void vote_rebase_gather_kernel(const float* __restrict__ src, int R, int Ho, int Wo,
                                                                   int ta, int tb, int tiles, int groups1, float scale_f,
                                                                   RbMap map, const float* __restrict__ fpart,
                                                                   float* __restrict__ dst, double* __restrict__ dpart,
                                                                   int32_t* __restrict__ ipart) {
  __shared__ float stage[2][RB_FP * RB_FS];
  __shared__ float shf[RB_WAVES];
  __shared__ double shd[RB_WAVES];
  __shared__ int shi[RB_WAVES];
  const double M = (double)vote_fold_max<RB_WAVES, RB_FSTR>(fpart, RB_F_PEAK, groups1, shf);
  const double scale = (double)scale_f;
  const size_t P = (size_t)Ho * Wo;
  const int ty = threadIdx.x / RB_T, tx = threadIdx.x - ty * RB_T;
  double sum_dst = 0.0, sum_src = 0.0;
  int n_notap = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r = tile / (ta * tb);
    const int t2 = tile - r * (ta * tb);
    const int a0 = (t2 / tb) * RB_T, b0 = (t2 - (t2 / tb) * tb) * RB_T;
    const int a1 = min(a0 + RB_T, Ho) - 1, b1 = min(b0 + RB_T, Wo) - 1;   // the tile's last row and column
    // the rotation split (uniform over the workgroup)
    const double k = (double)r - map.dk;
    const double k0 = floor(k);
    const double fk = k - k0;
    const double wk[2] = {1.0 - fk, fk};
    int plane[2];
    plane[0] = vote_mod((int)k0, R);        // (|k0| <= R + 1: dk lies in [0, R))
    plane[1] = vote_next(plane[0], R);
    // the footprint: the clamped floors at the four corners bound every cell's (the map is monotone in a and in b)
    int lo_a = Ho, hi_a = -1, lo_b = Wo, hi_b = -1;
    for (int c = 0; c < 4; ++c) {
      const int ca = (c & 1) ? a1 : a0, cb = (c & 2) ? b1 : b0;
      const int fa = rb_floor_clamped(rb_sa(map, ca, cb), Ho), fb = rb_floor_clamped(rb_sb(map, ca, cb), Wo);
      lo_a = min(lo_a, fa), hi_a = max(hi_a, fa);
      lo_b = min(lo_b, fb), hi_b = max(hi_b, fb);
    }
    const int na = hi_a - lo_a + 2, nb = hi_b - lo_b + 2;   // rows lo_a .. hi_a + 1
    const bool staged = na <= RB_FP && nb <= RB_FP;
    __syncthreads();                        // (the previous tile's readers are done with the staging area)
    if (staged) {
      for (int kk = 0; kk < 2; ++kk) {
        if (wk[kk] == 0.0) continue;
        const float* sp = src + (size_t)plane[kk] * P;
        for (int i = threadIdx.x; i < na * nb; i += RB_NT) {
          const int ia = i / nb, ib = i - ia * nb;
          const int row = lo_a + ia, col = lo_b + ib;
          float p = 0.f;
          if (row >= 0 && row < Ho && col >= 0 && col < Wo) p = rb_mass(sp[(size_t)row * Wo + col], scale, M);
          stage[kk][ia * RB_FS + ib] = p;
        }
      }
    }
    __syncthreads();
    const int a = a0 + ty, b = b0 + tx;
    if (a < Ho && b < Wo) {
      const size_t at = (size_t)r * P + (size_t)a * Wo + b;
      const float own = rb_mass(src[at], scale, M);
      if (own == own) sum_src += (double)own;
      int ia = 0, ib = 0;
      double fa = 0.0, fb = 0.0;
      const bool in_a = rb_floor(rb_sa(map, a, b), Ho, &ia, &fa);
      const bool in_b = rb_floor(rb_sb(map, a, b), Wo, &ib, &fb);
      const bool in = in_a && in_b;
      const double wa[2] = {1.0 - fa, fa}, wb[2] = {1.0 - fb, fb};
      double mass = 0.0;
      bool any = false, poisoned = false;
      if (in) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
          for (int da = 0; da < 2; ++da) {
#pragma unroll
            for (int db = 0; db < 2; ++db) {
              const double w = (wk[kk] * wa[da]) * wb[db];
              const int row = ia + da, col = ib + db;
              if (w == 0.0 || row < 0 || row >= Ho || col < 0 || col >= Wo) continue;
              const float p = staged ? stage[kk][(row - lo_a) * RB_FS + (col - lo_b)]
                                     : rb_mass(src[(size_t)plane[kk] * P + (size_t)row * Wo + col], scale, M);
              any = true;
              if (p != p)
                poisoned = true;
              else
                mass += w * (double)p;
            }
          }
        }
      }
      const float cell = poisoned ? __int_as_float(0x7fc00000) : (float)mass;
      dst[at] = cell;
      if (!poisoned) sum_dst += (double)cell;
      n_notap += any ? 0 : 1;
    }
  }
  sum_dst = vote_block_sum<RB_WAVES>(sum_dst, shd);
  sum_src = vote_block_sum<RB_WAVES>(sum_src, shd);
  n_notap = vote_block_sum<RB_WAVES>(n_notap, shi);
  if (threadIdx.x == 0) {
    dpart[(size_t)blockIdx.x * RB_DS + RB_D_DST] = sum_dst;
    dpart[(size_t)blockIdx.x * RB_DS + RB_D_SRC] = sum_src;
    ipart[(size_t)blockIdx.x * RB_IS + RB_I_NOTAP] = n_notap;
  }
}

// ---- launch 3
__global__ __launch_bounds__(RB_NT) void vote_rebase_normalise_kernel(int n, int groups2,
                                                                      const double* __restrict__ dpart,
                                                                      float* __restrict__ dst, float* __restrict__ fpart,
                                                                      int32_t* __restrict__ ipart) {
  __shared__ double shd[RB_WAVES];
  __shared__ float shf[RB_WAVES];
  __shared__ int shi[RB_WAVES];
  const double S = vote_fold_sum<RB_WAVES, RB_DS>(dpart, RB_D_DST, groups2, shd);
  const double log_s = S > 0.0 ? log(S) : 0.0;   // (S == 0: no cell has mass, log_s is not used)
  float top = -INFINITY;
  int n_fin = 0, n_nan = 0;
  for (int64_t i = (int64_t)blockIdx.x * RB_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RB_NT) {
    const float m = dst[i];
    const double w = m != m ? (double)m : (m > 0.f ? log((double)m) : -(double)INFINITY);
    const float out = vote_normalised(w, log_s);
    dst[i] = out;
    n_fin += vote_finite(out) ? 1 : 0;
    n_nan += out != out ? 1 : 0;
    top = fmaxf(top, out);                  // (fmaxf drops a NaN)
  }
  top = vote_block_max<RB_WAVES>(top, shf);
  n_fin = vote_block_sum<RB_WAVES>(n_fin, shi);
  n_nan = vote_block_sum<RB_WAVES>(n_nan, shi);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * RB_FSTR + RB_F_TOP] = top;
    ipart[(size_t)blockIdx.x * RB_IS + RB_I_FIN] = n_fin;
    ipart[(size_t)blockIdx.x * RB_IS + RB_I_NAN] = n_nan;
  }
}

// ---- launch 4
__global__ __launch_bounds__(RB_NT) void vote_rebase_finish_kernel(int groups1, int groups2, float scale,
                                                                   const double* __restrict__ dpart,
                                                                   const float* __restrict__ fpart,
                                                                   const int32_t* __restrict__ ipart,
                                                                   double* __restrict__ stats,
                                                                   int32_t* __restrict__ count) {
  __shared__ double shd[RB_WAVES];
  __shared__ float shf[RB_WAVES];
  __shared__ int shi[RB_WAVES];
  const float M = vote_fold_max<RB_WAVES, RB_FSTR>(fpart, RB_F_PEAK, groups1, shf);
  const float top = vote_fold_max<RB_WAVES, RB_FSTR>(fpart, RB_F_TOP, groups1, shf);
  const int n_bad = vote_fold_sum<RB_WAVES, RB_IS>(ipart, RB_I_BAD, groups1, shi);
  const int n_fin = vote_fold_sum<RB_WAVES, RB_IS>(ipart, RB_I_FIN, groups1, shi);
  const int n_nan = vote_fold_sum<RB_WAVES, RB_IS>(ipart, RB_I_NAN, groups1, shi);
  const int n_notap = vote_fold_sum<RB_WAVES, RB_IS>(ipart, RB_I_NOTAP, groups2, shi);
  const double s_dst = vote_fold_sum<RB_WAVES, RB_DS>(dpart, RB_D_DST, groups2, shd);
  const double s_src = vote_fold_sum<RB_WAVES, RB_DS>(dpart, RB_D_SRC, groups2, shd);
  if (threadIdx.x == 0) {
    stats[0] = s_src > 0.0 ? (double)scale * (double)M + log(s_src) : -(double)INFINITY;
    stats[1] = s_src > 0.0 ? s_dst / s_src : 0.0;
    stats[2] = (double)M;
    stats[3] = (double)top;
    count[0] = n_fin;
    count[1] = n_nan;
    count[2] = n_bad;
    count[3] = n_notap;
  }
}

struct RbPlan {
  VotePlan cell;                            // launches 1, 3: one tile = 256 consecutive pixels of one rotation
  int ta, tb, tiles, groups, n;             // launch 2: RB_T x RB_T tiles per plane, tiles = R ta tb
};

bool rb_plan(int R, int Ho, int Wo, RbPlan* plan) {
  if (R < 1 || R > RB_MAX_R || Ho < 1 || Wo < 1) return false;
  if (!vote_plan((int64_t)R * Ho * Wo, R, Ho, Wo, RB_NT, RB_MAX_GROUPS, &plan->cell)) return false;
  plan->ta = (int)snap_cdiv(Ho, RB_T);
  plan->tb = (int)snap_cdiv(Wo, RB_T);
  const int64_t tiles = (int64_t)R * plan->ta * plan->tb;
  if (!vote_cells_fit(tiles)) return false;   // (ta tb <= Ho Wo: it always does)
  plan->tiles = (int)tiles;
  plan->groups = plan->tiles < RB_MAX_GROUPS ? plan->tiles : RB_MAX_GROUPS;
  plan->n = R * Ho * Wo;
  return true;
}

// [groups2][2] float64 | [groups1][2] f32 | [max(groups1, groups2)][4] int32
struct RbWorkspace {
  double* dpart;
  float* fpart;
  int32_t* ipart;
  size_t bytes;
};

RbWorkspace rb_workspace(const RbPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  const int most = plan.cell.groups > plan.groups ? plan.cell.groups : plan.groups;
  return {l.take<double>((size_t)plan.groups * RB_DS), l.take<float>((size_t)plan.cell.groups * RB_FSTR),
          l.take<int32_t>((size_t)most * RB_IS), l.bytes};
}

bool rb_finite(double v) { return v - v == 0.0; }

}  // namespace

extern "C" size_t snap_vote_rebase_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo) {
  RbPlan plan;
  if (!rb_plan(R, Ho, Wo, &plan)) return 0;
  return rb_workspace(plan, nullptr).bytes;
}

extern "C" int snap_vote_rebase_f32(const float* src, int32_t R, int32_t Ho, int32_t Wo, float scale, double dk,
                                    double A00, double A01, double A10, double A11, double oa, double ob, float* dst,
                                    double* stats, int32_t* count, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!src || !dst || !stats || !count || !workspace) return SNAP_ERR_NULL;
  RbPlan plan;
  if (!rb_plan(R, Ho, Wo, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale > 0.f) || !(scale < INFINITY)) return SNAP_ERR_UNSUPPORTED;
  if (!(dk >= 0.0 && dk < (double)R)) return SNAP_ERR_UNSUPPORTED;
  if (!(rb_finite(A00) && rb_finite(A01) && rb_finite(A10) && rb_finite(A11) && rb_finite(oa) && rb_finite(ob)))
    return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, rb_workspace(plan, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const RbWorkspace w = rb_workspace(plan, workspace);
  const VotePlan& c = plan.cell;
  const RbMap map = {dk, A00, A01, A10, A11, oa, ob};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(RB_NT);
  hipLaunchKernelGGL(vote_rebase_peak_kernel, dim3(c.groups), block, 0, s, src, c.P, c.tiles_per_plane, c.tiles,
                     w.fpart, w.ipart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_rebase_gather_kernel, dim3(plan.groups), block, 0, s, src, R, Ho, Wo, plan.ta, plan.tb,
                     plan.tiles, c.groups, scale, map, w.fpart, dst, w.dpart, w.ipart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_rebase_normalise_kernel, dim3(c.groups), block, 0, s, plan.n, plan.groups, w.dpart, dst,
                     w.fpart, w.ipart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_rebase_finish_kernel, dim3(1), block, 0, s, c.groups, plan.groups, scale, w.dpart, w.fpart,
                     w.ipart, stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
