// Most likely pose TRACK over exhaustive vote volumes (max-product / Viterbi recursion on the (r, a, b) lattice):
// snap_vote_viterbi_f32 and snap_vote_backstep_i32 (include/snap_hip.h).
//
// score_prev [R, Ho, Wo] f32 is the log score of the best path into every pose of the previous frame (-inf = no path),
// votes [R, Ho, Wo] the new frame's vote volume.  d = score_prev - M (M = the largest finite score) is carried through
// three separable MAX-PLUS tap passes over LOG-taps (rotation, circular; rows and columns with the OUTPUT rotation's
// tables, the filter's order and indexing) into m2; best = max(log_stay + m2, log_jump) (the jump's predecessor is the
// previous frame's best cell J); score_out = fl32(scale * votes) + best, and back[x] = the linear index of the
// predecessor that attains it.  Every operation is one f32 addition, subtraction, product or comparison: no exp, no
// log, no sum, no float64.  Each pass keeps the LOWEST tap index among equals (taps ascending, update on strict >).
//
// This is the max-product recursion under K_max(x | x') = max((1 - eps) T(x | x'), eps / n), which lies within a factor
// 2 (log 2 per step) of the filter's (1 - eps) T + eps / n.  The filter's renormalisation of the transported mass
// (sum p / S) is constant over the lattice: it cannot change an argmax and is left out.
//
// A tile is one rotation and 256 consecutive pixels p = a * Wo + b, one cell per thread; every launch but the last has
// min(tiles, 2048) workgroups of 256 threads striding over the tiles (the tap rows of a tile are uniform).
// Launch 1 (vote_viterbi_peak_kernel):   per workgroup (the largest finite score_prev, the lowest index that has it)
//   and the count of NaN / +inf cells.
// Launch 2 (vote_viterbi_rotate_kernel): every workgroup folds the partials into (M, J); m0 = the k-tap maximum over
//   d, the subtraction fused (the <= Tk re-reads of score_prev are L2 hits), into score_out; the chosen tap as a byte.
// Launch 3 (vote_viterbi_rows_kernel):   m1 = the a-tap maximum over m0 (each tap a wave-contiguous run of a source
//   row), into the workspace; the chosen tap as a byte.
// Launch 4 (vote_viterbi_emit_kernel):   m2 = the b-tap maximum over m1; stay against jump; the predecessor composed
//   from the three chosen taps (the column tap of this cell gives b', the row tap byte at (r, a, b') gives a', the
//   rotation tap byte at (r, a', b') gives k': two byte gathers within a few rows of the cell); score_out and back;
//   per workgroup the counts and (the largest score_out, the lowest index that has it).
// Launch 5 (vote_viterbi_finish_kernel, one workgroup): stats and count.
// With score_prev == NULL launches 1-3 are skipped and launch 4 runs without its column pass.  No atomics and no
// inter-workgroup hand-off inside a launch; maxima are exact and every argmax fold is "larger value, then lower
// index", a total order, so the result does not depend on a fold order.
// HBM traffic (n = R Ho Wo cells): reads score_prev 2 (+ L2 re-reads), m0, m1, votes; writes m0, m1, score_out, back:
// 9 passes of 4-byte cells, and the two byte volumes written once and gathered once: 10 n cells of 4 bytes in all with
// a score_prev (the filter: 12), 3 n without.  Measured on an MI355X at [36, 511, 511], taps [8, 8, 8] (the filter tests'
// default noise), whole calls alternated with the filter's in one process: 0.255 ms against the filter's 0.396 ms
// (profiles/vote_viterbi_bench.json).
#include "vote_predict.h"

namespace {

constexpr int VT_NT = VP_NT;                // threads = cells of a tile
constexpr int VT_WAVES = VP_WAVES;

// per-workgroup partials: float [groups][2], int32 [groups][6]
enum { VT_F_PEAK = 0, VT_F_TOP = 1, VT_FS = 2 };
enum { VT_I_BAD = 0, VT_I_PEAK_AT = 1, VT_I_FIN = 2, VT_I_BAD_VOTE = 3, VT_I_JUMP = 4, VT_I_TOP_AT = 5, VT_IS = 6 };

// ---- launch 1
__global__ __launch_bounds__(VT_NT) void vote_viterbi_peak_kernel(const float* __restrict__ prev, int n,
                                                                  float* __restrict__ fpart,
                                                                  int32_t* __restrict__ ipart) {
  __shared__ float shf[VT_WAVES];
  __shared__ int shi[VT_WAVES];
  float m = -INFINITY;
  int at = VOTE_NO_INDEX, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * VT_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * VT_NT) {
    const float v = prev[i];
    if (vote_finite(v)) {
      if (v > m) {                          // (i ascends: the lowest index of this thread's cells)
        m = v;
        at = (int)i;
      }
    } else if (!(v == -INFINITY)) {
      ++bad;                                // NaN or +inf
    }
  }
  vote_block_argmax<VT_WAVES>(&m, &at, shf, shi);
  bad = vote_block_sum<VT_WAVES>(bad, shi);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * VT_FS + VT_F_PEAK] = m;
    ipart[(size_t)blockIdx.x * VT_IS + VT_I_PEAK_AT] = at;
    ipart[(size_t)blockIdx.x * VT_IS + VT_I_BAD] = bad;
  }
}

// ---- launch 2: m0[r, a, b] = max_tk ( ltaps_k[tk] + d[(r + lk + tk) mod R, a, b] )
__global__ __launch_bounds__(VT_NT) void vote_viterbi_rotate_kernel(const float* __restrict__ prev,
                                                                    const float* __restrict__ ltaps_k, int lk, int R,
                                                                    int P, int Tk, int tiles_per_plane, int tiles,
                                                                    const float* __restrict__ fpart,
                                                                    const int32_t* __restrict__ ipart,
                                                                    float* __restrict__ m0, uint8_t* __restrict__ ck) {
  __shared__ float shf[VT_WAVES];
  __shared__ int shi[VT_WAVES];
  float M;
  int J;
  vote_fold_argmax<VT_WAVES, VT_FS, VT_IS>(fpart, VT_F_PEAK, ipart, VT_I_PEAK_AT, gridDim.x, &M, &J, shf, shi);
  const int kfirst = vote_mod(lk, R);
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p;
    if (!vote_tile_cell<VT_NT>(tile, tiles_per_plane, P, &r, &p)) continue;
    int k = r + kfirst;                     // (>= 0: one side of vote_wrap)
    if (k >= R) k -= R;
    float best = -INFINITY;
    int arg = 0;
    for (int i = 0; i < Tk; ++i) {
      const float v = prev[(int64_t)k * P + p];
      const float d = vote_finite(v) ? v - M : -INFINITY;
      const float c = ltaps_k[i] + d;
      if (c > best) {
        best = c;
        arg = i;
      }
      k = vote_next(k, R);
    }
    m0[(int64_t)r * P + p] = best;
    ck[(int64_t)r * P + p] = (uint8_t)arg;
  }
}

// ---- launch 3: m1[r, a, b] = max_ta ( ltaps_a[r, ta] + m0[r, a + la[r] + ta, b] )
__global__ __launch_bounds__(VT_NT) void vote_viterbi_rows_kernel(const float* __restrict__ m0,
                                                                  const float* __restrict__ ltaps_a,
                                                                  const int32_t* __restrict__ offsets, int Ho, int Wo,
                                                                  int P, int Ta, int tiles_per_plane, int tiles,
                                                                  float* __restrict__ m1, uint8_t* __restrict__ ca) {
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p, a, b;
    if (!vote_tile_cell<VT_NT>(tile, tiles_per_plane, P, &r, &p)) continue;
    vote_row_col(p, Wo, &a, &b);
    const float* w = ltaps_a + (size_t)r * Ta;                    // uniform over the workgroup
    const int64_t first = (int64_t)a + offsets[(size_t)r * 2];
    const float* src = m0 + (int64_t)r * P + b;
    float best = -INFINITY;
    int arg = 0;
    for (int i = 0; i < Ta; ++i) {
      const int64_t sa = first + i;
      if (sa >= 0 && sa < Ho) {             // (outside: -inf, never chosen)
        const float c = w[i] + src[sa * Wo];
        if (c > best) {
          best = c;
          arg = i;
        }
      }
    }
    m1[(int64_t)r * P + p] = best;
    ca[(int64_t)r * P + p] = (uint8_t)arg;
  }
}

// ---- launch 4: m2[r, a, b] = max_tb ( ltaps_b[r, tb] + m1[r, a, b + lb[r] + tb] ), stay against jump, the update
// A value above -inf was chosen at a tap whose source is inside the volume and itself above -inf, so the composed
// predecessor of a cell with m2 > -inf is inside the volume at every link.
template <bool WITH_PREV>
__global__ __launch_bounds__(VT_NT) void vote_viterbi_emit_kernel(
    const float* __restrict__ m1, const uint8_t* __restrict__ ca, const uint8_t* __restrict__ ck,
    const float* __restrict__ ltaps_b, const int32_t* __restrict__ offsets, int lk, int R, int Wo, int P, int Tb,
    int tiles_per_plane, int tiles, const float* __restrict__ votes, float scale, float log_stay, float log_jump,
    float* __restrict__ fpart, int32_t* __restrict__ ipart, float* __restrict__ score_out, int32_t* __restrict__ back) {
  __shared__ float shf[VT_WAVES];
  __shared__ int shi[VT_WAVES];
  float M = -INFINITY;
  int J = VOTE_NO_INDEX;
  if (WITH_PREV)
    vote_fold_argmax<VT_WAVES, VT_FS, VT_IS>(fpart, VT_F_PEAK, ipart, VT_I_PEAK_AT, gridDim.x, &M, &J, shf, shi);
  const float jump = J != VOTE_NO_INDEX ? log_jump : -INFINITY;
  const int kfirst = vote_mod(lk, R);
  float top = -INFINITY;
  int top_at = VOTE_NO_INDEX, n_fin = 0, n_bad_vote = 0, n_jump = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int r, p;
    if (!vote_tile_cell<VT_NT>(tile, tiles_per_plane, P, &r, &p)) continue;
    const int idx = r * P + p;              // (< 2^31: vote_plan)
    float best = 0.f;
    int pred = -1;
    bool jumped = false;
    if (WITH_PREV) {
      int a, b;
      vote_row_col(p, Wo, &a, &b);
      const float* w = ltaps_b + (size_t)r * Tb;
      const int64_t first = (int64_t)b + offsets[(size_t)r * 2 + 1];
      const float* src = m1 + (int64_t)r * P + (int64_t)a * Wo;
      float m2 = -INFINITY;
      int tb = 0;
      for (int i = 0; i < Tb; ++i) {
        const int64_t sb = first + i;
        if (sb >= 0 && sb < Wo) {
          const float c = w[i] + src[sb];
          if (c > m2) {
            m2 = c;
            tb = i;
          }
        }
      }
      const float stay = log_stay + m2;
      if (stay >= jump) {                   // (the transported predecessor wins a tie)
        best = stay;
        if (m2 > -INFINITY) {
          const int bs = (int)(first + tb);
          const int as = a + offsets[(size_t)r * 2] + ca[(int64_t)r * P + (int64_t)a * Wo + bs];
          int ks = r + kfirst + ck[(int64_t)r * P + (int64_t)as * Wo + bs];
          ks %= R;
          pred = ks * P + as * Wo + bs;
        }
      } else {
        best = jump;
        pred = J;
        jumped = true;
      }
    }
    const float vote = votes[idx];
    float out;
    if (!(vote < INFINITY)) {               // NaN or +inf
      out = -INFINITY;
      ++n_bad_vote;
    } else if (vote == -INFINITY || best == -INFINITY) {
      out = -INFINITY;
    } else {
      out = scale * vote + best;
    }
    if (out == -INFINITY) {
      pred = -1;
      jumped = false;
    }
    score_out[idx] = out;
    back[idx] = pred;
    n_fin += vote_finite(out) ? 1 : 0;
    n_jump += jumped ? 1 : 0;
    if (out > top) {                        // (idx ascends with the tile: the lowest index of this thread's cells)
      top = out;
      top_at = idx;
    }
  }
  vote_block_argmax<VT_WAVES>(&top, &top_at, shf, shi);
  n_fin = vote_block_sum<VT_WAVES>(n_fin, shi);
  n_bad_vote = vote_block_sum<VT_WAVES>(n_bad_vote, shi);
  n_jump = vote_block_sum<VT_WAVES>(n_jump, shi);
  if (threadIdx.x == 0) {
    fpart[(size_t)blockIdx.x * VT_FS + VT_F_TOP] = top;
    ipart[(size_t)blockIdx.x * VT_IS + VT_I_TOP_AT] = top_at;
    ipart[(size_t)blockIdx.x * VT_IS + VT_I_FIN] = n_fin;
    ipart[(size_t)blockIdx.x * VT_IS + VT_I_BAD_VOTE] = n_bad_vote;
    ipart[(size_t)blockIdx.x * VT_IS + VT_I_JUMP] = n_jump;
  }
}

// ---- launch 5
__global__ __launch_bounds__(VT_NT) void vote_viterbi_finish_kernel(int groups, int with_prev,
                                                                    const float* __restrict__ fpart,
                                                                    const int32_t* __restrict__ ipart,
                                                                    float* __restrict__ stats,
                                                                    int32_t* __restrict__ count) {
  __shared__ float shf[VT_WAVES];
  __shared__ int shi[VT_WAVES];
  const int n_fin = vote_fold_sum<VT_WAVES, VT_IS>(ipart, VT_I_FIN, groups, shi);
  const int n_bad_vote = vote_fold_sum<VT_WAVES, VT_IS>(ipart, VT_I_BAD_VOTE, groups, shi);
  const int n_jump = vote_fold_sum<VT_WAVES, VT_IS>(ipart, VT_I_JUMP, groups, shi);
  float top, M = -INFINITY;
  int top_at, J = VOTE_NO_INDEX, n_bad = 0;
  vote_fold_argmax<VT_WAVES, VT_FS, VT_IS>(fpart, VT_F_TOP, ipart, VT_I_TOP_AT, groups, &top, &top_at, shf, shi);
  if (with_prev) {
    n_bad = vote_fold_sum<VT_WAVES, VT_IS>(ipart, VT_I_BAD, groups, shi);
    vote_fold_argmax<VT_WAVES, VT_FS, VT_IS>(fpart, VT_F_PEAK, ipart, VT_I_PEAK_AT, groups, &M, &J, shf, shi);
  }
  if (threadIdx.x == 0) {
    stats[0] = M;
    stats[1] = top;
    count[0] = n_fin;
    count[1] = n_bad;
    count[2] = n_bad_vote;
    count[3] = n_jump;
    count[4] = J == VOTE_NO_INDEX ? -1 : J;
    count[5] = top_at == VOTE_NO_INDEX ? -1 : top_at;
  }
}

__global__ __launch_bounds__(VT_NT) void vote_backstep_kernel(const int32_t* __restrict__ back, int n,
                                                              const int32_t* __restrict__ cur,
                                                              int32_t* __restrict__ prev, int B) {
  const int i = blockIdx.x * VT_NT + threadIdx.x;
  if (i >= B) return;
  const int c = cur[i];
  prev[i] = (c >= 0 && c < n) ? back[c] : -1;
}

// [R Ho Wo] f32 m1 | [R Ho Wo] u8 rotation taps | [R Ho Wo] u8 row taps | [groups][2] f32 | [groups][6] int32
struct VtWorkspace {
  float* m1;
  uint8_t* ck;
  uint8_t* ca;
  float* fpart;
  int32_t* ipart;
  size_t bytes;
};

VtWorkspace vt_workspace(const VpPlan& plan, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<float>(plan.n), l.take<uint8_t>(plan.n), l.take<uint8_t>(plan.n),
          l.take<float>((size_t)plan.groups * VT_FS), l.take<int32_t>((size_t)plan.groups * VT_IS), l.bytes};
}

bool vt_log_weight_ok(float v) { return v <= 0.f; }   // (-inf included; false for NaN)

}  // namespace

extern "C" size_t snap_vote_viterbi_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta,
                                                    int32_t Tb) {
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return 0;
  return vt_workspace(plan, nullptr).bytes;
}

extern "C" int snap_vote_viterbi_f32(const float* score_prev, const float* votes, const float* ltaps_k, int32_t lk,
                                     const float* ltaps_a, const float* ltaps_b, const int32_t* offsets, int32_t R,
                                     int32_t Ho, int32_t Wo, int32_t Tk, int32_t Ta, int32_t Tb, float scale,
                                     float log_stay, float log_jump, float* score_out, int32_t* back, float* stats,
                                     int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  if (!votes || !ltaps_k || !ltaps_a || !ltaps_b || !offsets || !score_out || !back || !stats || !count || !workspace)
    return SNAP_ERR_NULL;
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, Tk, Ta, Tb, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale > 0.f) || !(scale < INFINITY)) return SNAP_ERR_UNSUPPORTED;
  if (!vt_log_weight_ok(log_stay) || !vt_log_weight_ok(log_jump)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, vt_workspace(plan, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const VtWorkspace w = vt_workspace(plan, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(plan.groups), block(VT_NT);
  if (score_prev != nullptr) {
    hipLaunchKernelGGL(vote_viterbi_peak_kernel, grid, block, 0, s, score_prev, plan.n, w.fpart, w.ipart);
    SNAP_CHECK_LAUNCH();
    hipLaunchKernelGGL(vote_viterbi_rotate_kernel, grid, block, 0, s, score_prev, ltaps_k, lk, R, plan.P, Tk,
                       plan.tiles_per_plane, plan.tiles, w.fpart, w.ipart, score_out, w.ck);
    SNAP_CHECK_LAUNCH();
    hipLaunchKernelGGL(vote_viterbi_rows_kernel, grid, block, 0, s, score_out, ltaps_a, offsets, Ho, Wo, plan.P, Ta,
                       plan.tiles_per_plane, plan.tiles, w.m1, w.ca);
    SNAP_CHECK_LAUNCH();
    hipLaunchKernelGGL(vote_viterbi_emit_kernel<true>, grid, block, 0, s, w.m1, w.ca, w.ck, ltaps_b, offsets, lk, R,
                       Wo, plan.P, Tb, plan.tiles_per_plane, plan.tiles, votes, scale, log_stay, log_jump, w.fpart,
                       w.ipart, score_out, back);
    SNAP_CHECK_LAUNCH();
  } else {
    hipLaunchKernelGGL(vote_viterbi_emit_kernel<false>, grid, block, 0, s, w.m1, w.ca, w.ck, ltaps_b, offsets, lk, R,
                       Wo, plan.P, Tb, plan.tiles_per_plane, plan.tiles, votes, scale, log_stay, log_jump, w.fpart,
                       w.ipart, score_out, back);
    SNAP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(vote_viterbi_finish_kernel, dim3(1), block, 0, s, plan.groups, score_prev != nullptr ? 1 : 0,
                     w.fpart, w.ipart, stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

extern "C" int snap_vote_backstep_i32(const int32_t* back, int32_t n, const int32_t* cur, int32_t* prev, int32_t B,
                                      void* stream) {
  if (!back || !cur || !prev) return SNAP_ERR_NULL;
  if (n < 1 || B < 1) return SNAP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(vote_backstep_kernel, dim3((unsigned)snap_cdiv(B, VT_NT)), dim3(VT_NT), 0,
                     static_cast<hipStream_t>(stream), back, n, cur, prev, B);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
