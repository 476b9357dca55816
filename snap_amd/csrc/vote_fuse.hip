// Multi-frame fusion of aligned vote volumes: snap_vote_fuse_f32 (include/snap_hip.h).
//
// volumes [N, R, Ho, Wo] f32 are the vote volumes of N query frames with known relative motion; for an anchor-frame
// pose index (r, a, b) frame n's index is (r + dk, a + da, b + db) with (dk, da, db) = shifts[n, r] (a function of
// (n, r) alone: pose_exhaustive_voting.sequence_shift_table).  fused[r, a, b] = sum_n w_n * (trilinear blend of
// volume n at that index, circular in k), -inf where any frame does not see the pose, NaN where a tap is NaN / +inf.
//
// Launch 1 (vote_fuse_table_kernel, one thread per (n, r)): the shift row -> one 64-byte table entry: the range of
//   output rows / columns at which the frame's sample is inside, the flat offsets of the two source planes' first tap
//   relative to the output cell, which of the three axes have an upper tap (fraction > 0) and the 8 tap weights.
// Launch 2 (vote_fuse_kernel, <= 2048 workgroups striding over tiles): one tile = one output rotation and 256
//   consecutive pixels p = a * Wo + b, one per thread.  The rotation is uniform over the tile, so every table entry is
//   read through uniform (scalar) loads and the body is chosen by a uniform switch over the 8 combinations of
//   "upper tap present" per axis: inside a body the <= 8 loads are straight-line (all in flight together), each a
//   wave-contiguous, unaligned run of a source row (the lanes' pixels are consecutive; a run that crosses a row end is
//   still contiguous in the flat index).  Absent taps are never read.  Overlapping reads of neighbouring lanes / taps
//   are served by L1 / L2.  One (finite, NaN) pair of counts per workgroup.
// Launch 3 (vote_fuse_count_kernel, one workgroup): folds the <= 2048 pairs in a fixed tree.
// No atomics; the order of every sum is fixed (frames ascending, taps k-major then a then b), so two calls give the
// same bits.
#include "vote_common.h"

namespace {

constexpr int VF_NT = 256;                  // launch 2: threads = pixels of a tile
constexpr int VF_WAVES = VF_NT / SNAP_WAVE;
constexpr int VF_MAX_N = 16;
constexpr int VF_MAX_R = 64;
constexpr int VF_MAX_GROUPS = 2048;         // launch 2 workgroups
constexpr int VF_NC = 1024;                 // launch 3 threads

struct VfEntry {
  int32_t amin, amax, bmin, bmax;           // the sample is inside iff amin <= a <= amax and bmin <= b <= bmax
  int32_t o0, o1;                           // flat offset of tap (k0 | k1, a + ia, b + ib) relative to the plane-0 cell p
  int32_t kind;                             // bit 2 / 1 / 0: the k / a / b axis has an upper tap (its fraction > 0)
  int32_t pad;
  float w[8];                               // tap weights, tap = 4 kk + 2 aa + bb: ((k factor) * (a factor)) * (b factor)
};
static_assert(sizeof(VfEntry) == 64, "one table entry is 16 dwords");

// d -> (floor, fraction in [0, 1)): the fraction is the ONE f32 subtraction d - floorf(d); where that rounds to 1
// (a tiny negative d) the position is taken as the next integer.
__device__ __forceinline__ void vf_split(float d, float* l, float* f) {
  float fl = floorf(d);
  float fr = d - fl;
  if (fr >= 1.f) {
    fl += 1.f;
    fr = 0.f;
  }
  *l = fl;
  *f = fr;
}

__global__ __launch_bounds__(VF_NT) void vote_fuse_table_kernel(const float* __restrict__ shifts, int N, int R, int Ho,
                                                                int Wo, VfEntry* __restrict__ table) {
  const int i = blockIdx.x * VF_NT + threadIdx.x;
  if (i >= N * R) return;
  const int r = i % R;
  const float dk = shifts[(size_t)i * 3], da = shifts[(size_t)i * 3 + 1], db = shifts[(size_t)i * 3 + 2];
  VfEntry e;
  e.amin = e.bmin = 1;                      // an empty range: the frame sees no pose of this rotation
  e.amax = e.bmax = 0;
  e.o0 = e.o1 = e.kind = e.pad = 0;
  for (int t = 0; t < 8; ++t) e.w[t] = 0.f;
  if (vote_finite(dk) && vote_finite(da) && vote_finite(db)) {
    float lk, fk, la, fa, lb, fb;
    vf_split(dk, &lk, &fk);
    vf_split(da, &la, &fa);
    vf_split(db, &lb, &fb);
    if (la >= -(float)(Ho - 1) && la <= (float)(Ho - 1) && lb >= -(float)(Wo - 1) && lb <= (float)(Wo - 1)) {
      const int ia = (int)la, ib = (int)lb;
      // 0 <= a + ia and a + ia + fa <= Ho - 1
      e.amin = max(0, -ia);
      e.amax = Ho - 1 - ia - (fa > 0.f ? 1 : 0);
      e.bmin = max(0, -ib);
      e.bmax = Wo - 1 - ib - (fb > 0.f ? 1 : 0);
      float km = fmodf(lk, (float)R);       // exact
      if (km < 0.f) km += (float)R;
      int k0 = r + (int)km;
      if (k0 >= R) k0 -= R;
      if (k0 >= R) k0 = 0;                  // (km + R rounded to R: unreachable for |lk| < 2^24, harmless beyond)
      const int k1 = vote_next(k0, R);
      const int P = Ho * Wo;
      e.o0 = k0 * P + ia * Wo + ib;
      e.o1 = k1 * P + ia * Wo + ib;
      e.kind = (fk > 0.f ? 4 : 0) | (fa > 0.f ? 2 : 0) | (fb > 0.f ? 1 : 0);
      const float wk[2] = {1.f - fk, fk}, wa[2] = {1.f - fa, fa}, wb[2] = {1.f - fb, fb};
      for (int t = 0; t < 8; ++t) e.w[t] = (wk[t >> 2] * wa[(t >> 1) & 1]) * wb[t & 1];
    }
  }
  table[i] = e;
}

// One frame's blend at one pixel: the taps present, k-major then a then b, f32 fma from -0 (so the first product is
// kept as it is, sign of zero included).  `src` points at the plane-0 cell of this pixel in the frame's volume.
template <bool K, bool A, bool B>
__device__ __forceinline__ float vf_blend(const float* __restrict__ src, int o0, int o1, int Wo, const float (&w)[8],
                                          bool* bad, bool* masked) {
  float v[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const bool kk = t >> 2, aa = (t >> 1) & 1, bb = t & 1;
    if ((kk && !K) || (aa && !A) || (bb && !B)) continue;
    v[t] = src[(int64_t)(kk ? o1 : o0) + (aa ? Wo : 0) + (bb ? 1 : 0)];
  }
  float acc = -0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const bool kk = t >> 2, aa = (t >> 1) & 1, bb = t & 1;
    if ((kk && !K) || (aa && !A) || (bb && !B)) continue;
    *bad |= !(v[t] < INFINITY);             // NaN or +inf
    *masked |= v[t] == -INFINITY;
    acc = fmaf(w[t], v[t], acc);
  }
  return acc;
}

__global__ __launch_bounds__(VF_NT) void vote_fuse_kernel(const float* __restrict__ volumes,
                                                          const VfEntry* __restrict__ table,
                                                          const float* __restrict__ weights, int N, int R, int P, int Wo,
                                                          int tiles_per_plane, int tiles, float* __restrict__ fused,
                                                          int32_t* __restrict__ cnt) {
  __shared__ int wcnt[VF_WAVES][2];
  const int t = threadIdx.x;
  int n_fin = 0, n_nan = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p, a, b;
    if (!vote_tile_cell<VF_NT>(tile, tiles_per_plane, P, &r, &p)) continue;
    vote_row_col(p, Wo, &a, &b);
    bool bad = false, masked = false;
    float acc = -0.f;
    for (int n = 0; n < N; ++n) {
      const VfEntry* e = table + (n * R + r);                     // uniform over the workgroup
      const float wn = weights != nullptr ? weights[n] : 1.f;
      const bool inside = a >= e->amin && a <= e->amax && b >= e->bmin && b <= e->bmax;
      if (!inside) {
        masked = true;                      // no tap of this frame is read
        continue;
      }
      const float* src = volumes + ((int64_t)n * R * P + p);
      const int o0 = e->o0, o1 = e->o1;
      float w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = e->w[i];
      float bl;
      switch (e->kind) {
        case 0: bl = vf_blend<false, false, false>(src, o0, o1, Wo, w, &bad, &masked); break;
        case 1: bl = vf_blend<false, false, true>(src, o0, o1, Wo, w, &bad, &masked); break;
        case 2: bl = vf_blend<false, true, false>(src, o0, o1, Wo, w, &bad, &masked); break;
        case 3: bl = vf_blend<false, true, true>(src, o0, o1, Wo, w, &bad, &masked); break;
        case 4: bl = vf_blend<true, false, false>(src, o0, o1, Wo, w, &bad, &masked); break;
        case 5: bl = vf_blend<true, false, true>(src, o0, o1, Wo, w, &bad, &masked); break;
        case 6: bl = vf_blend<true, true, false>(src, o0, o1, Wo, w, &bad, &masked); break;
        default: bl = vf_blend<true, true, true>(src, o0, o1, Wo, w, &bad, &masked); break;
      }
      acc = fmaf(wn, bl, acc);
    }
    const float out = bad ? __int_as_float(0x7fc00000) : masked ? -INFINITY : acc;
    fused[(int64_t)r * P + p] = out;
    n_fin += vote_finite(out) ? 1 : 0;
    n_nan += out != out ? 1 : 0;
  }
  const int n = vote_block_count_pair<VF_WAVES>(n_fin, n_nan, wcnt);
  if (t < 2) cnt[(size_t)blockIdx.x * 2 + t] = n;
}

__global__ __launch_bounds__(VF_NC) void vote_fuse_count_kernel(const int32_t* __restrict__ cnt, int groups,
                                                                int32_t* __restrict__ count) {
  __shared__ int sh[VF_NC / SNAP_WAVE][2];
  const int t = threadIdx.x;
  int c0 = 0, c1 = 0;
  for (int g = t; g < groups; g += VF_NC) {
    c0 += cnt[(size_t)g * 2];
    c1 += cnt[(size_t)g * 2 + 1];
  }
  const int s = vote_block_count_pair<VF_NC / SNAP_WAVE>(c0, c1, sh);
  if (t < 2) count[t] = s;
}

bool vf_plan(int N, int R, int Ho, int Wo, VotePlan* plan) {
  if (N < 1 || N > VF_MAX_N || R < 1 || R > VF_MAX_R || Ho < 1 || Wo < 1) return false;
  return vote_plan((int64_t)N * R * Ho * Wo, R, Ho, Wo, VF_NT, VF_MAX_GROUPS, plan);
}

// [N][R] 64-byte table entries | [groups][2] int32 counts
// (the table entries are 64-byte records read as dwords: the workspace's 8-byte alignment is all the kernels need)
struct VfWorkspace {
  VfEntry* table;
  int32_t* cnt;
  size_t bytes;
};

VfWorkspace vf_workspace(const VotePlan& plan, int N, int R, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<VfEntry>((size_t)N * R), l.take<int32_t>((size_t)plan.groups * 2), l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_fuse_workspace_bytes(int32_t N, int32_t R, int32_t Ho, int32_t Wo) {
  VotePlan plan;
  if (!vf_plan(N, R, Ho, Wo, &plan)) return 0;
  return vf_workspace(plan, N, R, nullptr).bytes;
}

extern "C" int snap_vote_fuse_f32(const float* volumes, const float* shifts, const float* weights, int32_t N, int32_t R,
                                  int32_t Ho, int32_t Wo, float* fused, int32_t* count, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (!volumes || !shifts || !fused || !count || !workspace) return SNAP_ERR_NULL;
  VotePlan plan;
  if (!vf_plan(N, R, Ho, Wo, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!vote_workspace_ok(workspace, workspace_bytes, vf_workspace(plan, N, R, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const VfWorkspace w = vf_workspace(plan, N, R, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vote_fuse_table_kernel, dim3((unsigned)snap_cdiv(N * R, VF_NT)), dim3(VF_NT), 0, s, shifts, N, R,
                     Ho, Wo, w.table);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_fuse_kernel, dim3(plan.groups), dim3(VF_NT), 0, s, volumes, w.table, weights, N, R, plan.P,
                     Wo, plan.tiles_per_plane, plan.tiles, fused, w.cnt);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_fuse_count_kernel, dim3(1), dim3(VF_NC), 0, s, w.cnt, plan.groups, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
