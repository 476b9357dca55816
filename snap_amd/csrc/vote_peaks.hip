// Top-K peaks of a vote volume with non-maximum suppression: snap_vote_peaks_f32 (include/snap_hip.h).
//
// votes [R, Ho, Wo] f32 (the scores of exhaustive_pose_voting; any shape) -> the K greatest PEAKS.  A cell is a peak
// iff it beats every other cell of its window (|dr| <= radius_r circular, |da|, |db| <= radius_xy clipped) in the
// strict total order "greater value, then smaller flat index"; NaN and -inf cells are never peaks and a NaN
// neighbour compares like -inf.  Selection: value descending, then flat ascending.
//
// Everything compares through ONE 32-bit key per cell, vp_key(): the order-preserving map of the f32 bits
// (NaN -> the key of -inf, -0 -> the key of +0, so equal floats have equal keys).  With keys u the peak test is
//   u(c) > max over neighbours n of ( u(n) - [flat(n) > flat(c)] )   and   u(c) > key(-inf),
// (u > v - 1 <=> u >= v; cells outside the spatial border carry key 1, below every real key, so the
// subtraction never wraps), i.e. a plain integer max over the window.  A candidate is the 64-bit key
// (u << 32 | ~flat): unique per cell, greater = better, 0 = empty slot.
//
// Pass 1 (vote_peaks_tiles_kernel, <= 1024 workgroups striding over the (rotation, 16-row band, 64-column block)
// tiles): stage the tile's keys with their halo for the 2 radius_r + 1 rotations in LDS, test the 16 x 64 cells,
// compact the peaks in the fixed (wave, row, lane) order with ballots, and fold them into the workgroup's running
// best K by RANK (a candidate's rank = the number of greater keys: a function of the key set alone).  Each
// workgroup writes its K keys, sorted, and its NaN count to its workspace slot.
// Pass 2 (vote_peaks_merge_kernel, one workgroup, one sorted slot list per thread): K rounds of "greatest list
// head"; then one thread per output row, the score re-read from votes[flat] (its own bits, -0 included).
// No atomics anywhere: no result depends on the order in which workgroups or waves arrive.
#include "vote_common.h"

namespace {

constexpr int VP_TA = 16;                 // tile rows
constexpr int VP_TB = 64;                 // tile columns = one wave per staged row
constexpr int VP_NT = 256;
constexpr int VP_WAVES = VP_NT / SNAP_WAVE;
constexpr int VP_ROWS = VP_TA / VP_WAVES;   // rows of a tile column one thread tests
constexpr int VP_MAX_K = 64;
constexpr int VP_MAX_RR = 2;
constexpr int VP_MAX_RX = 4;
// radius_xy >= 1: two cells of one 2 x 2 block see each other, and the order is strict -> one peak per block
constexpr int VP_MAX_PEAKS = (VP_TA / 2) * (VP_TB / 2);
constexpr int VP_LIST = VP_MAX_K + VP_MAX_PEAKS;
constexpr int VP_MAX_GROUPS = 1024;       // pass-1 workgroups = pass-2 threads
constexpr uint32_t VP_KEY_NINF = 0x007fffffu;   // vp_key(-inf)
constexpr uint32_t VP_KEY_OUTSIDE = 1u;

__device__ __forceinline__ uint32_t vp_key(float v) {
  uint32_t b = __float_as_uint(v);
  if (v != v) b = 0xff800000u;
  if (b == 0x80000000u) b = 0u;
  return b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ uint32_t vp_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t vp_umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// bytes of LDS in front of the staged keys: list | nbuf | per-wave counts
constexpr size_t VP_LDS_HEAD = (size_t)(VP_LIST + VP_MAX_K) * sizeof(uint64_t) + 2 * VP_WAVES * sizeof(int);

inline size_t vp_lds_bytes(int rr, int rx) {
  return VP_LDS_HEAD + (size_t)(2 * rr + 1) * (VP_TA + 2 * rx) * (VP_TB + 2 * rx) * sizeof(uint32_t);
}

// RR_T / RX_T >= 0: the radii as compile-time constants (the window loops unroll); -1: the launch arguments.
// Only the default radius (1, 1) is instantiated with constants; every other setting runs the <-1, -1> body.
template <int RR_T, int RX_T>
__global__ __launch_bounds__(VP_NT) void vote_peaks_tiles_kernel(
    const float* __restrict__ votes, int R, int Ho, int Wo, int K, int rr_arg, int rx_arg, int bands, int cblocks,
    int tiles, uint64_t* __restrict__ slots, int32_t* __restrict__ nan_counts) {
  const int rr = RR_T >= 0 ? RR_T : rr_arg;
  const int rx = RX_T >= 0 ? RX_T : rx_arg;
  const int NP = 2 * rr + 1, SH = VP_TA + 2 * rx, SW = VP_TB + 2 * rx;
  extern __shared__ __align__(16) unsigned char vp_lds[];
  uint64_t* list = reinterpret_cast<uint64_t*>(vp_lds);   // [0, nb): the running best, sorted; behind it: new peaks
  uint64_t* nbuf = list + VP_LIST;                        // the next best, by rank
  int* wcount = reinterpret_cast<int*>(nbuf + VP_MAX_K);  // peaks per wave
  int* wnan = wcount + VP_WAVES;
  uint32_t* stage = reinterpret_cast<uint32_t*>(wnan + VP_WAVES);   // [NP][SH][SW] keys

  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  int nb = 0;          // entries of the running best (uniform)
  int nan_seen = 0;    // NaN votes among the cells this thread staged as OWNED cells

  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int cb = tile % cblocks, band = (tile / cblocks) % bands, r = tile / (cblocks * bands);
    const int a0 = band * VP_TA, b0 = cb * VP_TB;

    // ---- stage: one wave per (rotation, row) of the haloed tile; 64 body columns, then the 2 rx halo columns
    for (int row = wave; row < NP * SH; row += VP_WAVES) {
      const int p = row / SH, y = row - p * SH;
      const int rn = vote_wrap(r + p - rr, R);
      const int a = a0 + y - rx;
      const bool row_ok = a >= 0 && a < Ho;
      const float* src = votes + ((int64_t)rn * Ho + (row_ok ? a : 0)) * Wo;
      uint32_t* dst = stage + row * SW;
      const bool owned = p == rr && y >= rx && y < rx + VP_TA;
      {
        const int b = b0 + lane;
        uint32_t u = VP_KEY_OUTSIDE;
        if (row_ok && b < Wo) {
          const float v = src[b];
          u = vp_key(v);
          if (owned && v != v) ++nan_seen;
        }
        dst[rx + lane] = u;
      }
      if (lane < 2 * rx) {
        const int x = lane < rx ? lane : VP_TB + lane;
        const int b = b0 + x - rx;
        uint32_t u = VP_KEY_OUTSIDE;
        if (row_ok && b >= 0 && b < Wo) u = vp_key(src[b]);
        dst[x] = u;
      }
    }
    __syncthreads();

    // ---- test: column `lane`, rows wave * VP_ROWS + i.  A candidate below the K-th running best cannot be selected.
    const uint64_t kth = nb == K ? list[K - 1] : 0;
    uint64_t mine[VP_ROWS];
    int total = 0;                 // peaks of this wave in the rows so far
    int offs[VP_ROWS];             // this thread's place among them
#pragma unroll
    for (int i = 0; i < VP_ROWS; ++i) {
      const int ty = wave * VP_ROWS + i;
      const uint32_t uc = stage[(rr * SH + ty + rx) * SW + lane + rx];
      uint32_t m = 0;
      for (int p = 0; p < NP; ++p) {
        if (p == rr) continue;
        const uint32_t later = vote_wrap(r + p - rr, R) > r ? 1u : 0u;
        const uint32_t* pl = stage + (p * SH + ty) * SW + lane;
        for (int dy = 0; dy <= 2 * rx; ++dy)
          for (int dx = 0; dx <= 2 * rx; ++dx) m = vp_umax(m, pl[dy * SW + dx] - later);
      }
      const uint32_t* pl = stage + (rr * SH + ty) * SW + lane;
      for (int dy = 0; dy <= 2 * rx; ++dy)
        for (int dx = 0; dx <= 2 * rx; ++dx) {
          if (dy == rx && dx == rx) continue;
          const uint32_t later = (dy > rx || (dy == rx && dx > rx)) ? 1u : 0u;
          m = vp_umax(m, pl[dy * SW + dx] - later);
        }
      // (a centre outside the volume holds VP_KEY_OUTSIDE < VP_KEY_NINF: never a peak)
      const uint32_t flat = ((uint32_t)(r * Ho + a0 + ty)) * (uint32_t)Wo + (uint32_t)(b0 + lane);
      const uint64_t key = ((uint64_t)uc << 32) | (uint32_t)~flat;
      const bool peak = uc > m && uc > VP_KEY_NINF && key > kth;
      mine[i] = peak ? key : 0;
      const uint64_t mask = __ballot(peak);
      offs[i] = total + __popcll(mask & ((1ull << lane) - 1));
      total += __popcll(mask);
    }
    if (lane == 0) wcount[wave] = total;
    __syncthreads();

    // ---- compact behind the running best, in (wave, row, lane) order
    int base = nb, n = nb;
#pragma unroll
    for (int w = 0; w < VP_WAVES; ++w) {
      const int c = wcount[w];
      if (w < wave) base += c;
      n += c;
    }
#pragma unroll
    for (int i = 0; i < VP_ROWS; ++i)
      if (mine[i] != 0 && base + offs[i] < VP_LIST) list[base + offs[i]] = mine[i];
    if (n > VP_LIST) n = VP_LIST;        // (unreachable: see VP_MAX_PEAKS)

    // ---- fold by rank: keys are unique, so the ranks 0 .. n-1 are a permutation
    if (n > nb) {
      __syncthreads();
      for (int e = t; e < n; e += VP_NT) {
        const uint64_t k = list[e];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += list[j] > k ? 1 : 0;
        if (rank < K) nbuf[rank] = k;
      }
      __syncthreads();
      nb = n < K ? n : K;
      if (t < nb) list[t] = nbuf[t];
    }
    __syncthreads();
  }

  if (t < K) slots[(int64_t)blockIdx.x * K + t] = t < nb ? list[t] : 0;
  nan_seen = vote_wave_sum(nan_seen);
  if (lane == 0) wnan[wave] = nan_seen;
  __syncthreads();
  if (t == 0) nan_counts[blockIdx.x] = vote_waves_sum<VP_WAVES>(wnan);
}

__global__ __launch_bounds__(VP_MAX_GROUPS) void vote_peaks_merge_kernel(
    const float* __restrict__ votes, const uint64_t* __restrict__ slots, const int32_t* __restrict__ nan_counts,
    int groups, int K, int R, int Ho, int Wo, int32_t* __restrict__ index, float* __restrict__ score,
    int32_t* __restrict__ count) {
  constexpr int NW = VP_MAX_GROUPS / SNAP_WAVE;
  __shared__ uint64_t wmax[2][NW];
  __shared__ uint64_t winner[VP_MAX_K];
  __shared__ int wnan[NW];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const uint64_t* mylist = slots + (int64_t)t * K;
  int head = 0;
  uint64_t cur = t < groups ? mylist[0] : 0;
  for (int j = 0; j < K; ++j) {
    uint64_t m = cur;
    for (int o = 32; o > 0; o >>= 1) m = vp_umax64(m, __shfl_xor(m, o));
    if (lane == 0) wmax[j & 1][wave] = m;
    __syncthreads();    // (the other half of wmax is rewritten only behind the NEXT round's barrier)
    uint64_t best = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) best = vp_umax64(best, wmax[j & 1][w]);
    if (t == 0) winner[j] = best;
    if (best != 0 && cur == best) {     // keys are unique: exactly one list advances
      ++head;
      cur = head < K ? mylist[head] : 0;
    }
  }
  const int nan_seen = vote_wave_sum(t < groups ? nan_counts[t] : 0);
  if (lane == 0) wnan[wave] = nan_seen;
  __syncthreads();
  // ---- one thread per output row (the winners are sorted: the empty rows are the tail)
  if (t < K) {
    const uint64_t best = winner[t];
    if (best != 0) {
      const int flat = (int)~(uint32_t)best;
      const int r = flat / (Ho * Wo), rem = flat - r * (Ho * Wo), a = rem / Wo;
      index[t * 3 + 0] = r;
      index[t * 3 + 1] = a;
      index[t * 3 + 2] = rem - a * Wo;
      // (a key always names a cell of the volume; the bound keeps a corrupted workspace from becoming a wild read)
      score[t] = r < R ? votes[flat] : __int_as_float(0x7fc00000);
    } else {
      index[t * 3 + 0] = index[t * 3 + 1] = index[t * 3 + 2] = -1;
      score[t] = -INFINITY;
    }
  }
  if (t == 0) {
    int found = 0;
    for (int j = 0; j < K; ++j) found += winner[j] != 0 ? 1 : 0;
    count[0] = found;
    count[1] = vote_waves_sum<NW>(wnan);
  }
}

struct VpPlan {
  int bands, cblocks, tiles, groups;
};

bool vp_plan(int R, int Ho, int Wo, int K, int rr, int rx, VpPlan* plan) {
  if (R <= 0 || Ho <= 0 || Wo <= 0 || K < 1 || K > VP_MAX_K) return false;
  if (rr < 0 || rr > VP_MAX_RR || 2 * rr + 1 > R || rx < 1 || rx > VP_MAX_RX) return false;
  if (!vote_cells_fit((int64_t)R * Ho * Wo)) return false;
  plan->bands = (int)snap_cdiv(Ho, VP_TA);
  plan->cblocks = (int)snap_cdiv(Wo, VP_TB);
  plan->tiles = R * plan->bands * plan->cblocks;
  plan->groups = plan->tiles < VP_MAX_GROUPS ? plan->tiles : VP_MAX_GROUPS;
  return true;
}

// [groups][K] candidate keys | [groups] NaN counts
struct VpWorkspace {
  uint64_t* slots;
  int32_t* nan_counts;
  size_t bytes;
};

VpWorkspace vp_workspace(const VpPlan& plan, int K, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<uint64_t>((size_t)plan.groups * K), l.take<int32_t>(plan.groups), l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_peaks_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t K, int32_t radius_r,
                                                  int32_t radius_xy) {
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, K, radius_r, radius_xy, &plan)) return 0;
  return vp_workspace(plan, K, nullptr).bytes;
}

extern "C" int snap_vote_peaks_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, int32_t K,
                                   int32_t radius_r, int32_t radius_xy, int32_t* index, float* score,
                                   int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  if (!votes || !index || !score || !count || !workspace) return SNAP_ERR_NULL;
  VpPlan plan;
  if (!vp_plan(R, Ho, Wo, K, radius_r, radius_xy, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!vote_workspace_ok(workspace, workspace_bytes, vp_workspace(plan, K, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const VpWorkspace w = vp_workspace(plan, K, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t lds = vp_lds_bytes(radius_r, radius_xy);
  if (radius_r == 1 && radius_xy == 1)
    hipLaunchKernelGGL((vote_peaks_tiles_kernel<1, 1>), dim3(plan.groups), dim3(VP_NT), lds, s, votes, R, Ho, Wo, K,
                       radius_r, radius_xy, plan.bands, plan.cblocks, plan.tiles, w.slots, w.nan_counts);
  else
    hipLaunchKernelGGL((vote_peaks_tiles_kernel<-1, -1>), dim3(plan.groups), dim3(VP_NT), lds, s, votes, R, Ho, Wo, K,
                       radius_r, radius_xy, plan.bands, plan.cblocks, plan.tiles, w.slots, w.nan_counts);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_peaks_merge_kernel, dim3(1), dim3(VP_MAX_GROUPS), 0, s, votes, w.slots, w.nan_counts,
                     plan.groups, K, R, Ho, Wo, index, score, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
