// Dense plane alignment score at continuous poses: snap_plane_align_score_f32 (include/snap_hip.h).
//
// fq [Hq, Wq, D] / vq [Hq, Wq] is the query plane, fm [Hm, Wm, D] / vm [Hm, Wm] the map plane, poses [P, 4] =
// (cos, sin, tx, ty) in cell units.  For pose p every valid query cell (i, j) is carried into the map
// (rotate_sample.h with cell = 1: half-pixel centres, clamped taps, the zero-weight-invalid-tap rule) and
// raw(p) = sum over the counted cells of fq[i, j, :] . mix(fm taps)[:]; score = raw / sum(vq) where more than
// `threshold` cells count, -inf elsewhere.
//
// Launch 1 (pas_tcount_kernel, one workgroup): tcount = sum vq.
// Launch 2 (pas_partial_kernel, P x chunks workgroups): the query plane is cut into 16 x 16 cell tiles, row-major,
//   and a chunk is PAS_CHUNK consecutive tiles: the tiling is a function of (Hq, Wq) alone, so the order of every sum
//   is too.  A workgroup is 32 cell slots of 8 lanes; a cell's 8 lanes each take the channels 4 l .. 4 l + 3 of every
//   32-channel block, so one tap of one cell is one contiguous 128-byte read per block (the four taps of neighbouring
//   cells overlap and are served by L1 / L2), and the four weights are formed once per cell.  A lane's products run
//   through one f32 chain (channels ascending), the 8 lanes fold in a 3-step xor tree, and everything above the cell
//   is float64: per slot over its cells in tile order, then slots, then waves.  One (raw, count) pair per workgroup.
// Launch 3 (pas_final_kernel, one thread per pose): the chunks ascending, the division, the threshold.
// No atomics; results do not depend on P or on the order of the poses.
#include "vote_common.h"
#include "rotate_sample.h"

namespace {

constexpr int PAS_NT = 256;                 // launch 2 threads
constexpr int PAS_LPC = 8;                  // lanes per cell
constexpr int PAS_SLOTS = PAS_NT / PAS_LPC; // cells in flight per workgroup
constexpr int PAS_TILE = 16;                // tile edge in cells
constexpr int PAS_CHUNK = 16;               // tiles per workgroup
constexpr int PAS_WAVES = PAS_NT / SNAP_WAVE;
constexpr int PAS_MAX_EXTENT = 1024;
constexpr int PAS_MAX_D = 128;
constexpr int PAS_MAX_P = 1 << 20;          // exclusive
constexpr int PAS_NC = 1024;                // launch 1 threads

struct PasPartial {
  double raw;
  int32_t cnt;
  int32_t pad;
};
static_assert(sizeof(PasPartial) == 16, "one partial is 4 dwords");

__device__ __forceinline__ double pas_shfl_xor(double v, int mask) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, mask);
  hi = __shfl_xor(hi, mask);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(PAS_NC) void pas_tcount_kernel(const uint8_t* __restrict__ vq, int cells,
                                                            int32_t* __restrict__ tcount) {
  __shared__ int sh[PAS_NC / SNAP_WAVE];
  const int t = threadIdx.x;
  int c = 0;
  for (int g = t; g < cells; g += PAS_NC) c += vq[g] != 0 ? 1 : 0;
  // (written out, not vote_block_sum: every thread folding the 16 waves takes 18 VGPRs for this kernel's 17)
  c = vote_wave_sum(c);
  if ((t & 63) == 0) sh[t >> 6] = c;
  __syncthreads();
  if (t == 0) tcount[0] = vote_waves_sum<PAS_NC / SNAP_WAVE>(sh);
}

__global__ __launch_bounds__(PAS_NT) void pas_partial_kernel(const float* __restrict__ fq,
                                                             const uint8_t* __restrict__ vq,
                                                             const float* __restrict__ fm,
                                                             const uint8_t* __restrict__ vm,
                                                             const float* __restrict__ poses, int Hq, int Wq, int Hm,
                                                             int Wm, int D, int tiles_j, int tiles, int chunks,
                                                             PasPartial* __restrict__ partial) {
  __shared__ double wraw[PAS_WAVES];
  __shared__ int wcnt[PAS_WAVES];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int slot = t / PAS_LPC, l = t % PAS_LPC;
  const int p = blockIdx.x / chunks, chunk = blockIdx.x - p * chunks;
  float tfm[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) tfm[k] = poses[(size_t)p * 4 + k];
  const bool pose_ok = vote_finite(tfm[0]) && vote_finite(tfm[1]) && vote_finite(tfm[2]) && vote_finite(tfm[3]);
  double acc = 0.0;
  int cnt = 0;
  const int tile_end = min(tiles, (chunk + 1) * PAS_CHUNK);
  for (int tile = chunk * PAS_CHUNK; pose_ok && tile < tile_end; ++tile) {
    const int ti = tile / tiles_j, tj = tile - ti * tiles_j;
    for (int it = 0; it < PAS_TILE * PAS_TILE / PAS_SLOTS; ++it) {
      const int lc = it * PAS_SLOTS + slot;
      const int i = ti * PAS_TILE + lc / PAS_TILE, j = tj * PAS_TILE + lc % PAS_TILE;
      if (i >= Hq || j >= Wq) continue;
      if (vq[i * Wq + j] == 0) continue;
      // inside the map; the taps are clamped into the plane, so every index below is in range
      const SnapRotSample s = snap_rot_sample(tfm, i, j, Hm, Wm, 1.f, vm);
      if (!s.ok) continue;
      const float* q = fq + (size_t)(i * Wq + j) * D;
      const float* m00 = fm + (size_t)(s.i0 * Wm + s.j0) * D;
      const float* m01 = fm + (size_t)(s.i0 * Wm + s.j1) * D;
      const float* m10 = fm + (size_t)(s.i1 * Wm + s.j0) * D;
      const float* m11 = fm + (size_t)(s.i1 * Wm + s.j1) * D;
      float dot = 0.f;
      for (int c = l * 4; c < D; c += PAS_LPC * 4) {
        const float4 a = *reinterpret_cast<const float4*>(q + c);
        const float4 b00 = *reinterpret_cast<const float4*>(m00 + c);
        const float4 b01 = *reinterpret_cast<const float4*>(m01 + c);
        const float4 b10 = *reinterpret_cast<const float4*>(m10 + c);
        const float4 b11 = *reinterpret_cast<const float4*>(m11 + c);
        dot += a.x * snap_rot_mix(s, b00.x, b01.x, b10.x, b11.x);
        dot += a.y * snap_rot_mix(s, b00.y, b01.y, b10.y, b11.y);
        dot += a.z * snap_rot_mix(s, b00.z, b01.z, b10.z, b11.z);
        dot += a.w * snap_rot_mix(s, b00.w, b01.w, b10.w, b11.w);
      }
      // the cell's 8 lanes hold 8 partial dots: a symmetric tree, the same bits in each of them
      dot += __shfl_xor(dot, 1);
      dot += __shfl_xor(dot, 2);
      dot += __shfl_xor(dot, 4);
      if (l == 0) {
        acc += (double)dot;
        cnt += 1;
      }
    }
  }
  // slots of a wave (lanes 0, 8, .., 56 carry them; the others add zeros), then the waves
  for (int o = PAS_LPC; o < SNAP_WAVE; o <<= 1) {
    acc += pas_shfl_xor(acc, o);
    cnt += __shfl_xor(cnt, o);
  }
  if (lane == 0) {
    wraw[wave] = acc;
    wcnt[wave] = cnt;
  }
  __syncthreads();
  if (t == 0) {
    PasPartial out;
    out.raw = vote_waves_sum<PAS_WAVES>(wraw);
    out.cnt = vote_waves_sum<PAS_WAVES>(wcnt);
    out.pad = 0;
    partial[blockIdx.x] = out;
  }
}

__global__ __launch_bounds__(PAS_NT) void pas_final_kernel(const PasPartial* __restrict__ partial,
                                                           const float* __restrict__ poses,
                                                           const int32_t* __restrict__ tcount, int P, int chunks,
                                                           float threshold, float* __restrict__ score,
                                                           int32_t* __restrict__ overlap) {
  const int p = blockIdx.x * PAS_NT + threadIdx.x;
  if (p >= P) return;
  bool pose_ok = true;
  for (int k = 0; k < 4; ++k) pose_ok = pose_ok && vote_finite(poses[(size_t)p * 4 + k]);
  double raw = 0.0;
  int cnt = 0;
  for (int c = 0; c < chunks; ++c) {
    const PasPartial v = partial[(size_t)p * chunks + c];
    raw += v.raw;
    cnt += v.cnt;
  }
  const bool keep = pose_ok && (float)cnt > threshold;
  score[p] = keep ? (float)(raw / (double)tcount[0]) : -INFINITY;
  overlap[p] = pose_ok ? cnt : 0;
}

struct PasPlan {
  int tiles_j, tiles, chunks;
};

bool pas_plan(int Hq, int Wq, int Hm, int Wm, int D, int P, PasPlan* plan) {
  if (Hq < 1 || Wq < 1 || Hm < 1 || Wm < 1 || Hq > PAS_MAX_EXTENT || Wq > PAS_MAX_EXTENT || Hm > PAS_MAX_EXTENT ||
      Wm > PAS_MAX_EXTENT)
    return false;
  if (D < 4 || D > PAS_MAX_D || D % 4 != 0 || P < 1 || P >= PAS_MAX_P) return false;
  plan->tiles_j = (int)snap_cdiv(Wq, PAS_TILE);
  plan->tiles = (int)snap_cdiv(Hq, PAS_TILE) * plan->tiles_j;       // <= 4096
  plan->chunks = (int)snap_cdiv(plan->tiles, PAS_CHUNK);            // <= 256: P * chunks < 2^28
  return true;
}

// [P][chunks] 16-byte partials | tcount (one 8-byte word)
struct PasWorkspace {
  PasPartial* partial;
  int32_t* tcount;
  size_t bytes;
};

PasWorkspace pas_workspace(const PasPlan& plan, int P, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<PasPartial>((size_t)P * plan.chunks), l.take<int32_t>(1), l.bytes};
}

}  // namespace

extern "C" size_t snap_plane_align_score_workspace_bytes(int32_t Hq, int32_t Wq, int32_t Hm, int32_t Wm, int32_t D,
                                                         int32_t P) {
  PasPlan plan;
  if (!pas_plan(Hq, Wq, Hm, Wm, D, P, &plan)) return 0;
  return pas_workspace(plan, P, nullptr).bytes;
}

extern "C" int snap_plane_align_score_f32(const float* fq, const uint8_t* vq, const float* fm, const uint8_t* vm,
                                          const float* poses, int32_t Hq, int32_t Wq, int32_t Hm, int32_t Wm,
                                          int32_t D, int32_t P, float threshold, float* score, int32_t* overlap,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!fq || !vq || !fm || !vm || !poses || !score || !overlap || !workspace) return SNAP_ERR_NULL;
  PasPlan plan;
  if (!pas_plan(Hq, Wq, Hm, Wm, D, P, &plan)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, pas_workspace(plan, P, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  // (the feature rows are read as float4: D % 4 == 0 keeps every row 16-byte aligned when the planes are)
  if (reinterpret_cast<uintptr_t>(fq) % 16 != 0 || reinterpret_cast<uintptr_t>(fm) % 16 != 0)
    return SNAP_ERR_UNSUPPORTED;
  const PasWorkspace w = pas_workspace(plan, P, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pas_tcount_kernel, dim3(1), dim3(PAS_NC), 0, s, vq, Hq * Wq, w.tcount);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(pas_partial_kernel, dim3((unsigned)(P * plan.chunks)), dim3(PAS_NT), 0, s, fq, vq, fm, vm, poses,
                     Hq, Wq, Hm, Wm, D, plan.tiles_j, plan.tiles, plan.chunks, w.partial);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(pas_final_kernel, dim3((unsigned)snap_cdiv(P, PAS_NT)), dim3(PAS_NT), 0, s, w.partial, poses,
                     w.tcount, P, plan.chunks, threshold, score, overlap);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
