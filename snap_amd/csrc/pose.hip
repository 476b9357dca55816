// Pose-likelihood kernels: point-vs-map similarity + softmax statistics (k10),
// correspondence sampling + 2-point Kabsch (k11), pose scoring with LDS-staged
// score planes (k12) and the refinement lattice (k13).
//
// Replaces snap/models/bev_localizer.py:157-173 and
// snap/models/pose_estimation.py:49-82,100-165,168-205.
//
// Data layout in HBM (per scene b):
//   fq   [Nq, Dm]      query matching features (L2-normalised, masked)
//   fm   [X*Y, Dm]     map matching features
//   sim  [Nq, X*Y]     sim_points, one contiguous X*Y plane per query point
//   chunk_stats [Nq, ceil(XY/64), 2]  per-64-cell (max, sum exp) of the softmax
// The prob_points tensor of the reference is never materialised on the product
// path: its row-softmax is represented by chunk_stats (1/32 of the bytes) and
// re-evaluated on the fly by the sampler.
#include <stdlib.h>

#include "common.h"
#include "philox.h"

namespace {

constexpr int SIM_CH = 64;  // cells per softmax chunk == one wave
constexpr int SIM_TQ = 64;  // query rows per workgroup tile

// ---------------------------------------------------------------------------
// k10: similarity.  MODE 0: write sim + chunk stats.  MODE 1: write prob.
// grid = (ceil(XY/256), ceil(Nq/TQ), B), block = 256 (thread <-> map cell).
// Each thread keeps its map cell's Dm-vector in registers and streams the TQ
// query rows (LDS broadcast reads); sim rows are written 1 KiB-coalesced.
// ---------------------------------------------------------------------------
template <int DM, int MODE>
__global__ __launch_bounds__(256) void sim_kernel(
    const float* __restrict__ fq, const float* __restrict__ fm, int Nq, int XY, float scale,
    int clip, const float* __restrict__ num_valid, float* __restrict__ sim,
    float* __restrict__ stats, const float* __restrict__ rowstats, float* __restrict__ prob,
    const float* __restrict__ row_weight) {
  __shared__ float q_s[SIM_TQ * DM];
  const int b = blockIdx.z;
  const int n0 = blockIdx.y * SIM_TQ;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int NC = (XY + SIM_CH - 1) / SIM_CH;
  const bool cvalid = cell < XY;
  // query rows staged K-MAJOR ([k][row]) so that two consecutive rows of one k are an
  // aligned 8-byte pair: the dot products of TWO rows advance with one v_pk_fma_f32.
  for (int i = threadIdx.x; i < SIM_TQ * DM; i += 256) {
    const int r = i / DM, k = i - r * DM;
    q_s[k * SIM_TQ + r] = (n0 + r < Nq) ? fq[((int64_t)b * Nq + n0) * DM + i] : 0.f;
  }
  f32x2 mv[DM];
  if (cvalid) {
    const f32x4* src = reinterpret_cast<const f32x4*>(fm + ((int64_t)b * XY + cell) * DM);
#pragma unroll
    for (int k = 0; k < DM / 4; ++k) {
      const f32x4 t = src[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) mv[4 * k + e] = f32x2{t[e], t[e]};
    }
  } else {
#pragma unroll
    for (int k = 0; k < DM; ++k) mv[k] = f32x2{0.f, 0.f};
  }
  __syncthreads();
  const float nv = num_valid[b];
  const float rnv = 1.0f / nv;      // sim = x * (1 / num_valid): one rounding away from x / num_valid
  const int rows = min(SIM_TQ, Nq - n0);
  for (int r0 = 0; r0 < rows; r0 += 2) {
    f32x2 dot2 = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < DM; ++k)   // per component the same k-ordered fmaf chain as before
      dot2 = __builtin_elementwise_fma(*reinterpret_cast<const f32x2*>(q_s + k * SIM_TQ + r0), mv[k], dot2);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = r0 + h;
      if (r >= rows) break;
      const int64_t row = (int64_t)b * Nq + n0 + r;
      const float dot = h ? dot2.y : dot2.x;
      float x = clip ? fmaxf(dot, 0.f) : dot;
      x *= scale;
      // bev_localizer.py:165-172: confidence weights (masked softmax over the query points)
      // replace the 1 / num_valid normalisation when add_confidence_query is set
      const float wrow = row_weight ? row_weight[row] : rnv;
      if (MODE == 0) {
        if (cvalid) sim[row * XY + cell] = x * wrow;
        const float m = wave_max(cvalid ? x : -INFINITY);
        const float s = wave_sum(cvalid ? expf(x - m) : 0.f);
        if (lane == 0 && chunk < NC) {
          stats[(row * NC + chunk) * 2 + 0] = m;
          stats[(row * NC + chunk) * 2 + 1] = s;
        }
      } else {
        const float M = rowstats[row * 2 + 0], T = rowstats[row * 2 + 1];
        if (cvalid) prob[row * XY + cell] = row_weight ? (expf(x - M) / T) * wrow : (expf(x - M) / T) / nv;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// k10 on the f32 matrix cores (MODE 0 of the kernel above: sim + chunk statistics).
// D[n, cell] = sum_k fq[n, k] fm[cell, k] as 32x32x2 f32 MFMAs (each the exact k-ordered fmaf
// chain the VALU kernel runs, so sim and the sampler's re-evaluation keep their bits).
// grid as above; a wave owns the 64 cells of one softmax chunk (B operand, held in registers for
// the whole tile) and the tile's 64 query rows (A operand): 2 x 2 tiles of 32 x 32, DM / 2 MFMAs
// each.  Neither operand touches LDS: lane (l31, lhi) of an MFMA holds element k = 2 j + lhi of
// row / column l31, picked out of the lane's own contiguous DM-vector.  The epilogue is the staged
// one below (sim_stage_tile, sim_row_stats, sim_row_store), shared with the split-bf16 kernels.
// The VALU kernel was bound by its packed-FMA issue (97 % VALU busy, 1.65 ms at C2 for a
// 2.44 GB write that the HBM can take in 0.4 ms).
// ---------------------------------------------------------------------------
template <int DM>
__device__ __forceinline__ void sim_load_operand(const float* __restrict__ row, bool valid, int lhi,
                                                 float (&out)[DM / 2]) {
  if (!valid) {
#pragma unroll
    for (int j = 0; j < DM / 2; ++j) out[j] = 0.f;
    return;
  }
  const f32x4* src = reinterpret_cast<const f32x4*>(row);
#pragma unroll
  for (int q = 0; q < DM / 4; ++q) {
    const f32x4 t = src[q];
    out[2 * q] = lhi ? t[1] : t[0];
    out[2 * q + 1] = lhi ? t[3] : t[2];
  }
}

// max / sum over the 16 lanes of a DPP row (row_ror 8/4/2/1: symmetric steps, so every lane of
// the row ends with the same bits)
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, snap_dpp<0x128>(v));
  v = fmaxf(v, snap_dpp<0x124>(v));
  v = fmaxf(v, snap_dpp<0x122>(v));
  return fmaxf(v, snap_dpp<0x121>(v));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += snap_dpp<0x128>(v);
  v += snap_dpp<0x124>(v);
  v += snap_dpp<0x122>(v);
  return v + snap_dpp<0x121>(v);
}

// ---- the staged epilogue of the matrix-core similarity kernels ---------------------------------
// The MFMA C layout gives a lane ONE cell of 16 rows -- 64 dword stores per 32-row tile, and narrow
// stores are issue-bound.  So the tile (32 rows x 64 cells) goes through a per-wave LDS buffer:
// staged, 16 lanes own one query row's 64 cells as float4, a wave store covers four 256-byte row
// segments with dwordx4 (8 stores per tile instead of 32), and the chunk's (max, sum exp) is a
// reduction inside one 16-lane DPP row.  The buffer is private to the wave: LDS ops of one wave
// complete in order, no barrier.
constexpr int SIM_LD = 64 + 4;   // +4: rows 4 apart hit distinct banks

// rows as the A operand, cells as B: acc[tj][r] = sim[row (r & 3) + 8 (r >> 2) + 4 lhi][cell 32 tj + l31]
__device__ __forceinline__ void sim_stage_tile(float (*st)[SIM_LD], const f32x16 (&acc)[2], int l31,
                                               int lhi) {
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int r = 0; r < 16; ++r) st[(r & 3) + 8 * (r >> 2) + 4 * lhi][32 * tj + l31] = acc[tj][r];
}

// One staged query row of a 4-row pass: which row, whether it exists, the factor sim carries
// (bev_localizer.py:165-172: the confidence weight replaces 1 / num_valid).
struct SimRow {
  int rr;        // row of the 32-row tile
  bool live;
  int64_t row;   // b * Nq + n (row 0 of the scene for a dead row: never stored)
  float wrow;
};
__device__ __forceinline__ SimRow sim_staged_row(int p, int sub, int b, int Nq, int n_tile,
                                                 const float* __restrict__ row_weight, float rnv) {
  SimRow r;
  r.rr = 4 * p + sub;
  const int n = n_tile + r.rr;
  r.live = n < Nq;
  r.row = (int64_t)b * Nq + (r.live ? n : 0);
  r.wrow = row_weight ? row_weight[r.row] : rnv;
  return r;
}

// The staged row epilogue, in two steps around the caller's `if (live)`.
//   TAIL: the chunk may end after `ncell` < 64 cells and sim rows may be unaligned (XY % 4 != 0).
//   Without TAIL every chunk is full and every row segment 16-byte aligned: no masks (4 compare /
//   select per element), and sim leaves with non-temporal stores (streamed once, read back later
//   by the scoring kernel: nothing of it is worth an L2 line now).
//   CLIP: 0 / 1 at compile time, -1 = the run-time flag `clip`.
// Step 1 (every lane: the DPP rows must be whole): the lane's four cells [c4, c4 + 4) of the row
// -> x = clip, scale, and the chunk's (max, sum exp) over the row's 16 lanes.
struct SimRowStats {
  f32x4 x;
  float m, sum;
};
template <bool TAIL, int CLIP>
__device__ __forceinline__ SimRowStats sim_row_stats(const float* staged, int clip, float scale,
                                                     int c4, int ncell) {
  f32x4 x = *reinterpret_cast<const f32x4*>(staged);
  float m = -INFINITY;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (CLIP < 0 ? clip != 0 : CLIP != 0) x[e] = fmaxf(x[e], 0.f);
    x[e] *= scale;
    if (!TAIL || c4 + e < ncell) m = fmaxf(m, x[e]);
  }
  m = row16_max(m);
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (!TAIL || c4 + e < ncell) sum += __expf(x[e] - m);   // v_exp_f32: ~1e-6 relative on the chunk mass
  sum = row16_sum(sum);
  return SimRowStats{x, m, sum};
}
// Step 2 (live rows): sim = x * wrow at o = &sim[row][cell0 + c4].
template <bool TAIL>
__device__ __forceinline__ void sim_row_store(const f32x4& x, float wrow, float* o, int c4, int ncell,
                                              int XY) {
  if constexpr (!TAIL) {
    __builtin_nontemporal_store(f32x4{x[0] * wrow, x[1] * wrow, x[2] * wrow, x[3] * wrow},
                                reinterpret_cast<f32x4*>(o));
  } else if (c4 + 3 < ncell && ((XY & 3) == 0)) {
    *reinterpret_cast<f32x4*>(o) = f32x4{x[0] * wrow, x[1] * wrow, x[2] * wrow, x[3] * wrow};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c4 + e < ncell) o[e] = x[e] * wrow;
  }
}

template <int DM>
__global__ __launch_bounds__(256, DM <= 32 ? 4 : 2) void sim_mfma_kernel(
    const float* __restrict__ fq, const float* __restrict__ fm, int Nq, int XY, float scale,
    int clip, const float* __restrict__ num_valid, float* __restrict__ sim,
    float* __restrict__ stats, const float* __restrict__ row_weight) {
  const int b = blockIdx.z;
  const int n0 = blockIdx.y * SIM_TQ;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int chunk = blockIdx.x * 4 + wave;
  const int cell0 = chunk * SIM_CH;
  const int NC = (XY + SIM_CH - 1) / SIM_CH;
  if (cell0 >= XY) return;                      // (whole wave; no barrier in this kernel)
  float bq[2][DM / 2], aq[2][DM / 2];
  bool cv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int cell = cell0 + 32 * t + l31;
    cv[t] = cell < XY;
    sim_load_operand<DM>(fm + ((int64_t)b * XY + (cv[t] ? cell : 0)) * DM, cv[t], lhi, bq[t]);
    const int row = n0 + 32 * t + l31;
    sim_load_operand<DM>(fq + ((int64_t)b * Nq + (row < Nq ? row : 0)) * DM, row < Nq, lhi, aq[t]);
  }
  // staged epilogue, one 32-row tile (ti) at a time
  __shared__ __attribute__((aligned(16))) float stage[4][32][SIM_LD];
  float (*st)[SIM_LD] = stage[wave];
  const float rnv = 1.0f / num_valid[b];   // as the VALU kernel: the two stay bit-identical
  const int sub = lane >> 4;            // row within a 4-row pass
  const int c4 = (lane & 15) * 4;       // first of the lane's 4 cells
  const int ncell = XY - cell0;         // live cells of this chunk (>= 1)
  // One 32-row half at a time: the stores of half 0 drain while the matrix pipe works on half 1
  // (measured: the contraction costs 0.46 ms and the stores 0.38 ms of the kernel's 1.17 ms when
  // all MFMAs run first -- they did not overlap), and the kernel holds 32 accumulator registers
  // instead of 64 (one more wave per SIMD).
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
    for (int j = 0; j < DM / 2; ++j)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
        acc[tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[ti][j], bq[tj][j], acc[tj], 0, 0, 0);
    sim_stage_tile(st, acc, l31, lhi);
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const SimRow r = sim_staged_row(p, sub, b, Nq, n0 + 32 * ti, row_weight, rnv);
      const SimRowStats e = sim_row_stats<true, -1>(&st[r.rr][c4], clip, scale, c4, ncell);
      if (r.live) {
        sim_row_store<true>(e.x, r.wrow, sim + r.row * XY + cell0 + c4, c4, ncell, XY);
        if ((lane & 15) == 0) {
          stats[(r.row * NC + chunk) * 2 + 0] = e.m;
          stats[(r.row * NC + chunk) * 2 + 1] = e.sum;
        }
      }
    }
  }
}

// ---- the same similarity with the contraction on the BF16 matrix cores, f32-grade -------------
// f32 MFMAs cost 0.46 ms of the kernel above at C2 (39 GFLOP at half the f32 matrix peak).  Here
// fq / fm are split once into NS bf16 parts per element (hi = bf16(v), mid = bf16(v - hi), lo =
// bf16(v - hi - mid): conv_split.hip's arithmetic; NS = 3 keeps 24 significand bits per operand,
// six part products per MAC, error ~2^-24 per product -- inside the f32 chain's own rounding) by
// sim_presplit_kernel, and the tile is NS (NS + 1) / 2 x DM / 16 v_mfma_f32_32x32x16_bf16 per
// 32 x 32 block instead of DM / 2 f32 MFMAs: 2.7 x fewer matrix cycles at NS = 3.  The epilogue is
// sim_stage_tile, sim_row_stats and sim_row_store, as in sim_mfma_kernel.

// x [R, DM] f32 -> [R][NS][DM] bf16
template <int NS>
__global__ __launch_bounds__(256) void sim_presplit_kernel(const float* __restrict__ x, int64_t n,
                                                           int DM, __bf16* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = i / DM;
  const int k = (int)(i - r * DM);
  float v = x[i];
#pragma unroll
  for (int p = 0; p < NS; ++p) {
    const __bf16 b = (__bf16)v;
    out[(r * NS + p) * DM + k] = b;
    v -= (float)b;
  }
}

// One operand row's split parts for an MFMA lane: out[s][p] = elements [16 s + 8 lhi, + 8) of part p.
// `src` = the row's [NS][DM] block + 8 lhi (any readable row when !valid: the registers are zeroed).
template <int DM, int NS>
__device__ __forceinline__ void sim_split_load(const __bf16* __restrict__ src, bool valid,
                                               bf16x8 (&out)[DM / 16][NS]) {
#pragma unroll
  for (int s = 0; s < DM / 16; ++s)
#pragma unroll
    for (int p = 0; p < NS; ++p) {
      out[s][p] = *reinterpret_cast<const bf16x8*>(src + p * DM + 16 * s);
      if (!valid) out[s][p] = bf16x8{};
    }
}

// acc[tj] = sum over k-steps and part pairs (pa + pb < NS) of aq[.][pa] x bq[tj][.][pb], smallest
// terms first: the order of split_product (NS = 2 runs the last three pairs of the NS = 3 list).
// SWAP = false: query rows are the MFMA's A operand (the C layout of sim_stage_tile); SWAP = true:
// map cells are A -- the same products in the same k positions, the transposed accumulator tile.
template <int NS, bool SWAP, int KS>
__device__ __forceinline__ void sim_split_products(const bf16x8 (&aq)[KS][NS],
                                                   const bf16x8 (&bq)[2][KS][NS], f32x16 (&acc)[2]) {
  constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int i = (NS == 3 ? 0 : 3); i < 6; ++i)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
        acc[tj] = SWAP ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq[tj][s][PB[i]], aq[s][PA[i]], acc[tj], 0, 0, 0)
                       : __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[s][PA[i]], bq[tj][s][PB[i]], acc[tj], 0, 0, 0);
}

template <int DM, int NS>
__global__ __launch_bounds__(256, 3) void sim_split_kernel(
    const __bf16* __restrict__ fqs, const __bf16* __restrict__ fms, int Nq, int XY, float scale,
    int clip, const float* __restrict__ num_valid, float* __restrict__ sim,
    float* __restrict__ stats, const float* __restrict__ row_weight) {
  constexpr int KS = DM / 16;
  const int b = blockIdx.z;
  const int n0 = blockIdx.y * SIM_TQ;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int chunk = blockIdx.x * 4 + wave;
  const int cell0 = chunk * SIM_CH;
  const int NC = (XY + SIM_CH - 1) / SIM_CH;
  if (cell0 >= XY) return;
  // B operand (map cells), both 32-cell tiles, kept for both row halves
  bf16x8 bq[2][KS][NS];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int cell = cell0 + 32 * t + l31;
    const bool cv = cell < XY;
    sim_split_load<DM, NS>(fms + ((int64_t)b * XY + (cv ? cell : 0)) * (NS * DM) + 8 * lhi, cv, bq[t]);
  }
  __shared__ __attribute__((aligned(16))) float stage[4][32][SIM_LD];
  float (*st)[SIM_LD] = stage[wave];
  const float rnv = 1.0f / num_valid[b];
  const int sub = lane >> 4;
  const int c4 = (lane & 15) * 4;
  const int ncell = XY - cell0;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    bf16x8 aq[KS][NS];
    const int arow = n0 + 32 * ti + l31;
    sim_split_load<DM, NS>(fqs + ((int64_t)b * Nq + (arow < Nq ? arow : 0)) * (NS * DM) + 8 * lhi,
                           arow < Nq, aq);
    f32x16 acc[2];
    sim_split_products<NS, false>(aq, bq, acc);
    sim_stage_tile(st, acc, l31, lhi);
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const SimRow r = sim_staged_row(p, sub, b, Nq, n0 + 32 * ti, row_weight, rnv);
      const SimRowStats e = sim_row_stats<true, -1>(&st[r.rr][c4], clip, scale, c4, ncell);
      if (r.live) {
        sim_row_store<true>(e.x, r.wrow, sim + r.row * XY + cell0 + c4, c4, ncell, XY);
        if ((lane & 15) == 0) {
          stats[(r.row * NC + chunk) * 2 + 0] = e.m;
          stats[(r.row * NC + chunk) * 2 + 1] = e.sum;
        }
      }
    }
  }
}

// The same kernel for XY % 256 == 0 (every chunk of every workgroup full: C2 128 x 128, C4 256 x 256,
// the reference's 120 x 160 map), leaner around the same pieces -- identical bits in sim and in
// the chunk statistics (tests/test_gpu_kernels.py compares the two kernels bit for bit):
//   * operand roles swapped in the MFMA (sim_split_products<NS, true>): a lane then holds FOUR
//     CONSECUTIVE cells of one row per accumulator quad, so the tile goes to the staging buffer in
//     8 ds_write_b128 instead of 32 ds_write_b32 (stride 68 floats: the 16 rows of a lane group land
//     on distinct banks; the b32 pattern of sim_stage_tile has a 25 % conflict rate);
//   * the row epilogue without TAIL and with the clip flag at compile time;
//   * the (max, sum) pairs of the workgroup's four chunks leave as ONE 32-byte store per row (they
//     are adjacent in [row][chunk][2]) instead of four 8-byte partial-line writes: the statistics
//     were a third of the kernel's write requests.
template <int DM, int NS, bool CLIP>
__global__ __launch_bounds__(256, 3) void sim_split_fast_kernel(
    const __bf16* __restrict__ fqs, const __bf16* __restrict__ fms, int Nq, int XY, float scale,
    const float* __restrict__ num_valid, float* __restrict__ sim, float* __restrict__ stats,
    const float* __restrict__ row_weight) {
  constexpr int KS = DM / 16;
  const int b = blockIdx.z;
  const int n0 = blockIdx.y * SIM_TQ;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int chunk = blockIdx.x * 4 + wave;
  const int cell0 = chunk * SIM_CH;
  const int NC = XY / SIM_CH;
  bf16x8 bq[2][KS][NS];
#pragma unroll
  for (int t = 0; t < 2; ++t)
    sim_split_load<DM, NS>(fms + ((int64_t)b * XY + cell0 + 32 * t + l31) * (NS * DM) + 8 * lhi, true, bq[t]);
  __shared__ __attribute__((aligned(16))) float stage[4][32][SIM_LD];
  __shared__ __attribute__((aligned(16))) float sstat[SIM_TQ][8];
  float (*st)[SIM_LD] = stage[wave];
  const float rnv = 1.0f / num_valid[b];
  const int sub = lane >> 4;
  const int c4 = (lane & 15) * 4;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    bf16x8 aq[KS][NS];
    const int arow = n0 + 32 * ti + l31;
    sim_split_load<DM, NS>(fqs + ((int64_t)b * Nq + (arow < Nq ? arow : 0)) * (NS * DM) + 8 * lhi,
                           arow < Nq, aq);
    f32x16 acc[2];
    // (cells as the A operand, rows as B: acc[tj][r] = sim[row l31][cell 32 tj + (r & 3) + 8 (r >> 2) + 4 lhi])
    sim_split_products<NS, true>(aq, bq, acc);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(&st[l31][32 * tj + 8 * g + 4 * lhi]) =
            f32x4{acc[tj][4 * g], acc[tj][4 * g + 1], acc[tj][4 * g + 2], acc[tj][4 * g + 3]};
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const SimRow r = sim_staged_row(p, sub, b, Nq, n0 + 32 * ti, row_weight, rnv);
      const SimRowStats e = sim_row_stats<false, CLIP ? 1 : 0>(&st[r.rr][c4], 0, scale, c4, SIM_CH);
      if (r.live) sim_row_store<false>(e.x, r.wrow, sim + r.row * XY + cell0 + c4, c4, SIM_CH, XY);
      if ((lane & 15) == 0) {
        sstat[32 * ti + r.rr][2 * wave] = e.m;
        sstat[32 * ti + r.rr][2 * wave + 1] = e.sum;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * SIM_TQ) {
    const int r = threadIdx.x >> 1, h = threadIdx.x & 1;
    const int n = n0 + r;
    if (n < Nq)
      *reinterpret_cast<f32x4*>(stats + (((int64_t)b * Nq + n) * NC + blockIdx.x * 4) * 2 + 4 * h) =
          *reinterpret_cast<const f32x4*>(&sstat[r][4 * h]);
  }
}

// layers.masked_softmax over the query points (snap/models/layers.py:38-43) + its inclusive CDF
// (the sampler's row distribution).  One workgroup per scene; fixed-order sums.
// The CDF is NON-DECREASING, a row of weight 0 repeats its predecessor's value bit for bit (the sampler's
// search for the first cdf[n] > target can then never return it) and cdf[N - 1] == 1: the segment boundaries
// are a SERIAL sum of the segment masses (two prefixes of a tree-ordered scan may differ by an ulp the wrong
// way, also across a segment of mass 0), the running sum inside a segment is capped by the segment's upper
// boundary, and everything from the segment's last non-zero entry on IS that boundary.
__global__ __launch_bounds__(256) void masked_softmax_rows_kernel(
    const float* __restrict__ x, const uint8_t* __restrict__ mask, int N, float* __restrict__ w,
    float* __restrict__ cdf) {
  __shared__ float red[256];
  __shared__ float seg_s[256];
  __shared__ float edge[257];
  __shared__ int any_s;
  const int b = blockIdx.x, t = threadIdx.x;
  const float* xr = x + (int64_t)b * N;
  const uint8_t* mr = mask + (int64_t)b * N;
  const int seg = (N + 255) / 256;
  const int i0 = min(t * seg, N), i1 = min(i0 + seg, N);
  int any = 0;
  for (int i = i0; i < i1; ++i) any |= mr[i];
  if (t == 0) any_s = 0;
  __syncthreads();
  if (any) atomicOr(&any_s, 1);
  __syncthreads();
  const bool all = any_s == 0;                 // nothing valid: the mask becomes all-true
  float m = -INFINITY;
  for (int i = i0; i < i1; ++i)
    if (all || mr[i]) m = fmaxf(m, xr[i]);
  red[t] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] = fmaxf(red[t], red[t + o]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  float loc = 0.f;
  int lastnz = -1;                             // last entry of the segment with a non-zero weight
  for (int i = i0; i < i1; ++i) {
    const float e = (all || mr[i]) ? expf(xr[i] - m) : 0.f;
    if (e > 0.f) lastnz = i;
    loc += e;
  }
  red[t] = loc;
  seg_s[t] = loc;
  __syncthreads();
  // inclusive scan of the 256 segment sums (Hillis-Steele, fixed order)
  for (int o = 1; o < 256; o <<= 1) {
    const float add = t >= o ? red[t - o] : 0.f;
    __syncthreads();
    red[t] += add;
    __syncthreads();
  }
  const float total = red[255];
  if (t == 0) {
    float acc = 0.f;
    edge[0] = 0.f;
    for (int k = 0; k < 256; ++k) {
      acc += seg_s[k];
      edge[k + 1] = acc;
    }
  }
  __syncthreads();
  const float lo = edge[t], hi = edge[t + 1], ctotal = edge[256];
  float run = lo;
  for (int i = i0; i < i1; ++i) {
    const float e = (all || mr[i]) ? expf(xr[i] - m) : 0.f;
    run += e;
    w[(int64_t)b * N + i] = e / total;
    cdf[(int64_t)b * N + i] = (i >= lastnz ? hi : fminf(run, hi)) / ctotal;
  }
}

// one wave per (b, n): row max M and total T = sum_c s_c * exp(m_c - M).
__global__ __launch_bounds__(256) void row_stats_kernel(const float* __restrict__ stats,
                                                        int64_t rows, int NC,
                                                        float* __restrict__ rowstats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* st = stats + row * NC * 2;
  float m = -INFINITY;
  for (int c = lane; c < NC; c += 64) m = fmaxf(m, st[2 * c]);
  m = wave_max(m);
  float t = 0.f;
  for (int c = lane; c < NC; c += 64) t += st[2 * c + 1] * expf(st[2 * c] - m);
  t = wave_sum(t);
  if (lane == 0) {
    rowstats[row * 2 + 0] = m;
    rowstats[row * 2 + 1] = t;
  }
}

// ---------------------------------------------------------------------------
// k11a: iid categorical sampling of correspondences ~ prob_points.
// prob mass is uniform over query points (every row softmax sums to 1), so:
// n = floor(u1 * Nq); cell ~ softmax row n by two-level inverse CDF:
// chunk from chunk_stats, then the 64 cells of that chunk re-evaluated.
// One wave per sample.
// (philox4x32_10: philox.h)
// ---------------------------------------------------------------------------

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ float wave_scan_incl(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// ---- the steps of one draw, shared by both sampler kernels (and the prefix table's builder) ----
// All wave-uniform except lane_prefix / pick_lane / pick_cell_store, which run across the 64 lanes.

// (u1, u2) of sample s of scene b: read from `uniforms` or drawn from Philox(seed; s, b).  A dead
// slot (!live: the NQ-per-wave kernel's tail) reads nothing.
__device__ __forceinline__ void draw_uniforms(const float* __restrict__ uniforms, int b, int S, int s,
                                              uint64_t seed, bool live, float& u1, float& u2) {
  if (uniforms) {
    u1 = live ? uniforms[((int64_t)b * S + s) * 2 + 0] : 0.f;
    u2 = live ? uniforms[((int64_t)b * S + s) * 2 + 1] : 0.f;
  } else {
    uint32_t rnd[4];
    philox4x32_10((uint32_t)s, (uint32_t)b, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), rnd);
    u1 = (float)(rnd[0] >> 8) * (1.0f / 16777216.0f);
    u2 = (float)(rnd[1] >> 8) * (1.0f / 16777216.0f);
  }
}

// the query row of a draw: uniform over the rows, or -- rows carrying the confidence weights as
// mass (bev_localizer.py:165-168) -- the first n whose inclusive CDF exceeds u1 * total
// (wave-uniform binary search)
__device__ __forceinline__ int pick_row(const float* __restrict__ row_cdf, int b, int Nq, float u1) {
  int n;
  if (row_cdf) {
    const float* cdf = row_cdf + (int64_t)b * Nq;
    const float tgt = u1 * cdf[Nq - 1];
    int lo = 0, hi = Nq - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] > tgt) hi = mid; else lo = mid + 1;
    }
    n = lo;
  } else {
    n = min((int)(u1 * (float)Nq), Nq - 1);
  }
  return __builtin_amdgcn_readfirstlane(n);
}

// level 1 of a row with chunk statistics st[NC][2]: lane l owns the contiguous chunk range
// [cb, ce).  M = the row maximum, local = the mass of the lane's range (w_c = s_c * exp(m_c - M));
// returns the inclusive prefix of `local` over the lanes.
__device__ __forceinline__ float lane_prefix(const float* __restrict__ st, int cb, int ce, int lane,
                                             float& M, float& local) {
  M = -INFINITY;
  for (int c = cb; c < ce; ++c) M = fmaxf(M, st[2 * c]);
  M = wave_max(M);
  local = 0.f;
  for (int c = cb; c < ce; ++c) local += st[2 * c + 1] * __expf(st[2 * c] - M);
  return wave_scan_incl(local, lane);
}

// the first lane whose inclusive prefix exceeds the target (rounding: else the last non-empty lane)
__device__ __forceinline__ int pick_lane(float incl, float target, bool nonempty) {
  const unsigned long long bal = __ballot(incl > target && nonempty);
  int L;
  if (bal) {
    L = __ffsll((long long)bal) - 1;
  } else {
    const unsigned long long ne = __ballot(nonempty);
    L = 63 - __clzll((long long)ne);
  }
  return __builtin_amdgcn_readfirstlane(L);
}

// level 2: e = the lane's cell mass relative to the chunk maximum (0 for !cvalid); the first valid
// cell of chunk `cstar` whose inclusive prefix exceeds resid (else the last valid one) is the draw.
// Lane 0 writes corr[b, s] = (n, i, j) if `write`.
__device__ __forceinline__ void pick_cell_store(float e, bool cvalid, float resid, int lane, int cstar,
                                                int n, int Y, bool write, int32_t* __restrict__ o) {
  const float ci = wave_scan_incl(e, lane);
  const unsigned long long b2 = __ballot(cvalid && ci > resid);
  int pick;
  if (b2) {
    pick = __ffsll((long long)b2) - 1;
  } else {
    const unsigned long long nv = __ballot(cvalid);
    pick = 63 - __clzll((long long)nv);
  }
  if (lane == 0 && write) {
    const int c = cstar * SIM_CH + pick;
    o[0] = n;
    o[1] = c / Y;
    o[2] = c - (c / Y) * Y;
  }
}

// one wave per (b, n): lane_prefix of the row, stored -- exactly the quantities the table-free
// sampler rebuilds per SAMPLE (2 passes over the row's statistics, 2 x cpl expf, a wave max and a
// wave scan).  ~34 samples share a row at C2; with this table a sample reads 64 floats and only the
// selected lane re-evaluates its own chunks.  Bit-identical samples.
__global__ __launch_bounds__(256) void chunk_prefix_kernel(const float* __restrict__ stats,
                                                           int64_t rows, int NC,
                                                           float* __restrict__ lane_incl,
                                                           float* __restrict__ rowmax) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int cpl = (NC + 63) / 64;
  const int cb = lane * cpl, ce = min(cb + cpl, NC);
  float M, local;
  lane_incl[row * 64 + lane] = lane_prefix(stats + row * NC * 2, cb, ce, lane, M, local);
  if (lane == 0) rowmax[row] = M;
}

template <int DM>
__global__ __launch_bounds__(256) void ransac_sample_kernel(
    const float* __restrict__ fq, const float* __restrict__ fm, const float* __restrict__ stats,
    int Nq, int X, int Y, float scale, int clip, int S, uint64_t seed,
    const float* __restrict__ uniforms, int32_t* __restrict__ corr,
    const float* __restrict__ lane_incl, const float* __restrict__ rowmax,
    const float* __restrict__ row_cdf, const float* __restrict__ sim,
    const float* __restrict__ row_unscale) {
  const int lane = threadIdx.x & 63;
  // one wave = one correspondence: everything that depends only on (scene, sample) is wave-uniform.
  // readfirstlane tells the compiler so: the Philox rounds, the row / chunk bookkeeping and the
  // address arithmetic then run on the scalar unit instead of 64-wide on the (saturated) VALU
  const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int b = blockIdx.y;
  if (s >= S) return;
  const int XY = X * Y;
  const int NC = (XY + SIM_CH - 1) / SIM_CH;
  float u1, u2;
  draw_uniforms(uniforms, b, S, s, seed, true, u1, u2);
  const int n = pick_row(row_cdf, b, Nq, u1);
  const int64_t row = (int64_t)b * Nq + n;
  const float* st = stats + row * NC * 2;

  // level 1: pick the chunk.  lane l owns the contiguous chunk range [l*cpl, (l+1)*cpl).
  const int cpl = (NC + 63) / 64;
  const int cb = lane * cpl, ce = min(cb + cpl, NC);
  float M, local = 0.f, incl;
  const bool table = lane_incl != nullptr;
  if (table) {                   // per-row prefix table (chunk_prefix_kernel)
    M = rowmax[row];
    incl = lane_incl[row * 64 + lane];
  } else {
    incl = lane_prefix(st, cb, ce, lane, M, local);
  }
  const float total = __shfl(incl, 63, 64);
  const float target = u2 * total;
  const int L = pick_lane(incl, target, ce > cb);
  // the chunks of lane L: lane i evaluates the mass of chunk cbL + i (one exp per lane, side by
  // side), then the walk runs over those values in the same order and with the same additions as
  // a serial walk by lane L would
  const int cbL = L * cpl, ceL = min(cbL + cpl, NC);
  const int nL = ceL - cbL;                                 // 1 .. cpl chunks (uniform)
  const float inclL = __shfl(incl, L, 64);
  float localL = __shfl(local, L, 64);
  float run = 0.f;
  int cstar = ceL - 1;
  float resid = INFINITY;
  bool found = false;
  // (pass 0 re-sums lane L's chunk masses when only the table's prefix is known; pass 1 walks)
  for (int pass = table ? 0 : 1; pass < 2; ++pass) {
    if (pass == 1) run = inclL - localL;
    float acc = 0.f;
    for (int base = 0; base < nL; base += 64) {             // (nL <= 64 up to 512 x 512 maps)
      float ex = 0.f, wgt = 0.f;
      if (base + lane < nL) {
        ex = __expf(st[2 * (cbL + base + lane)] - M);
        wgt = st[2 * (cbL + base + lane) + 1] * ex;
      }
      const int m = min(64, nL - base);
      for (int i = 0; i < m; ++i) {
        const float wi = __shfl(wgt, i, 64);
        if (pass == 0) {
          acc += wi;
        } else {
          if (!found && run + wi > target) {
            cstar = cbL + base + i;
            resid = (target - run) / __shfl(ex, i, 64);     // relative to the chunk's own max
            found = true;
          }
          run += wi;
        }
      }
    }
    if (pass == 0) localL = acc;
  }
  const float mc = st[2 * cstar];

  // level 2: the 64 cells of the chunk.
  const int cell = cstar * SIM_CH + lane;
  const bool cvalid = cell < XY;
  float e = 0.f;
  if (cvalid && sim) {
    // the chunk's scores were written by the similarity kernel: 256 contiguous bytes of sim
    // (x = sim * num_valid, or sim / weight, to within one rounding) instead of re-evaluating 64
    // dot products from 8 KB of map features -- the sampler was bound by that L2 traffic
    // (10.8 GB per C2 step, 1.75 ms)
    e = __expf(sim[row * (int64_t)XY + cell] * row_unscale[row] - mc);
  } else if (cvalid) {
    const f32x4* mp = reinterpret_cast<const f32x4*>(fm + ((int64_t)b * XY + cell) * DM);
    const f32x4* qp = reinterpret_cast<const f32x4*>(fq + row * DM);
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < DM / 4; ++k) {
      const f32x4 a = qp[k], c = mp[k];
      dot = fmaf(a[0], c[0], dot); dot = fmaf(a[1], c[1], dot); dot = fmaf(a[2], c[2], dot); dot = fmaf(a[3], c[3], dot);
    }
    float x = clip ? fmaxf(dot, 0.f) : dot;
    x *= scale;
    e = __expf(x - mc);
  }
  pick_cell_store(e, cvalid, resid, lane, cstar, n, Y, true, corr + ((int64_t)b * S + s) * 3);
}

// The same draw for the common configuration (per-row prefix table + chunk scores read from sim),
// NQ correspondences per wave in lock step.  One correspondence is three DEPENDENT memory round
// trips (row table -> chunk statistics -> the chunk's 64 scores) and ~450 instructions: with one
// per wave the kernel ran at the pace of those round trips (32 waves per CU / ~5 us each = the
// measured 0.8 ms for 1.28 M correspondences at C2).  Here the NQ chains of a wave are issued
// phase by phase, so each round trip serves NQ correspondences.  Every step is the piece
// ransac_sample_kernel calls, and the walk adds in the same order: identical samples.
template <int NQ>
__global__ __launch_bounds__(256) void ransac_sample_fast_kernel(
    const float* __restrict__ stats, int Nq, int X, int Y, int S, uint64_t seed,
    const float* __restrict__ uniforms, int32_t* __restrict__ corr,
    const float* __restrict__ lane_incl, const float* __restrict__ rowmax,
    const float* __restrict__ row_cdf, const float* __restrict__ sim,
    const float* __restrict__ row_unscale) {
  const int lane = threadIdx.x & 63;
  const int s0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + (threadIdx.x >> 6)) * NQ);
  const int b = blockIdx.y;
  if (s0 >= S) return;
  const int XY = X * Y;
  const int NC = (XY + SIM_CH - 1) / SIM_CH;
  const int cpl = (NC + 63) / 64;                           // <= 64 (checked by the launcher)
  const int cb = lane * cpl, ce = min(cb + cpl, NC);
  bool live[NQ];
  int n[NQ];
  float u2[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    live[q] = s0 + q < S;
    float u1;
    draw_uniforms(uniforms, b, S, s0 + q, seed, live[q], u1, u2[q]);
    n[q] = pick_row(row_cdf, b, Nq, u1);
  }
  // round trip 1: the row's maximum, its per-lane inclusive prefix, its un-scale factor
  float M[NQ], incl[NQ], ru[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int64_t row = (int64_t)b * Nq + n[q];
    M[q] = rowmax[row];
    incl[q] = lane_incl[row * 64 + lane];
    ru[q] = row_unscale[row];
  }
  // level 1: the lane whose chunk range holds the target; round trip 2: that range's statistics
  int cbL[NQ], nL[NQ];
  float target[NQ], inclL[NQ], sm[NQ], ss[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const float total = __shfl(incl[q], 63, 64);
    target[q] = u2[q] * total;
    const int L = pick_lane(incl[q], target[q], ce > cb);
    cbL[q] = L * cpl;
    nL[q] = min(cbL[q] + cpl, NC) - cbL[q];
    inclL[q] = __shfl(incl[q], L, 64);
    const float* st = stats + ((int64_t)b * Nq + n[q]) * NC * 2;
    sm[q] = ss[q] = 0.f;
    if (lane < nL[q]) {
      sm[q] = st[2 * (cbL[q] + lane)];
      ss[q] = st[2 * (cbL[q] + lane) + 1];
    }
  }
  // the walk over lane L's chunks (masses side by side, additions in the serial order);
  // round trip 3: the selected chunk's 64 scores
  int cstar[NQ];
  float resid[NQ], mc[NQ], x[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const float ex = lane < nL[q] ? __expf(sm[q] - M[q]) : 0.f;
    const float wgt = ss[q] * ex;
    float localL = 0.f;
    for (int i = 0; i < nL[q]; ++i) localL += __shfl(wgt, i, 64);
    float run = inclL[q] - localL;
    int cs = cbL[q] + nL[q] - 1;
    float rs = INFINITY;
    bool found = false;
    for (int i = 0; i < nL[q]; ++i) {
      const float wi = __shfl(wgt, i, 64);
      if (!found && run + wi > target[q]) {
        cs = cbL[q] + i;
        rs = (target[q] - run) / __shfl(ex, i, 64);
        found = true;
      }
      run += wi;
    }
    cstar[q] = cs;
    resid[q] = rs;
    mc[q] = __shfl(sm[q], cs - cbL[q], 64);
    const int cell = cs * SIM_CH + lane;
    x[q] = (cell < XY && live[q]) ? sim[((int64_t)b * Nq + n[q]) * XY + cell] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const bool cvalid = cstar[q] * SIM_CH + lane < XY;
    const float e = cvalid ? __expf(x[q] * ru[q] - mc[q]) : 0.f;
    pick_cell_store(e, cvalid, resid[q], lane, cstar[q], n[q], Y, live[q],
                    corr + ((int64_t)b * S + s0 + q) * 3);
  }
}

// ---------------------------------------------------------------------------
// k11b: best-of-retries + 2-point Kabsch (closed form of the 2x2 SVD).
// ---------------------------------------------------------------------------
__global__ void poses_from_corr_kernel(const int32_t* __restrict__ corr,
                                       const float* __restrict__ q_xy, int B, int Nq, int P,
                                       int retries, float cell, float* __restrict__ poses) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * P) return;
  const int b = (int)(i / P), p = (int)(i - (int64_t)b * P);
  const int32_t* cb = corr + ((int64_t)b * P * retries * 2) * 3;
  float best = INFINITY;
  float bi0x = 0, bi0y = 0, bi1x = 0, bi1y = 0, bj0x = 0, bj0y = 0, bj1x = 0, bj1y = 0;
  for (int r = 0; r < retries; ++r) {
    const int32_t* c0 = cb + ((int64_t)(p * retries + r) * 2 + 0) * 3;
    const int32_t* c1 = c0 + 3;
    const float i0x = q_xy[((int64_t)b * Nq + c0[0]) * 2 + 0], i0y = q_xy[((int64_t)b * Nq + c0[0]) * 2 + 1];
    const float i1x = q_xy[((int64_t)b * Nq + c1[0]) * 2 + 0], i1y = q_xy[((int64_t)b * Nq + c1[0]) * 2 + 1];
    const float j0x = ((float)c0[1] + 0.5f) * cell, j0y = ((float)c0[2] + 0.5f) * cell;
    const float j1x = ((float)c1[1] + 0.5f) * cell, j1y = ((float)c1[2] + 0.5f) * cell;
    float ratio = 0.f;
    if (retries > 1) {
      const float dix = i1x - i0x, diy = i1y - i0y, djx = j1x - j0x, djy = j1y - j0y;
      const float d_i = sqrtf(dix * dix + diy * diy), d_j = sqrtf(djx * djx + djy * djy);
      ratio = fmaxf(d_i / fmaxf(d_j, 1e-5f), d_j / fmaxf(d_i, 1e-5f));
    }
    if (r == 0 || ratio < best) {
      best = ratio;
      bi0x = i0x; bi0y = i0y; bi1x = i1x; bi1y = i1y;
      bj0x = j0x; bj0y = j0y; bj1x = j1x; bj1y = j1y;
    }
  }
  // kabsch_algorithm_2d(j_xy (map), i_xy (query)) -> map_t_query.
  const float mux = (bj0x + bj1x) * 0.5f, muy = (bj0y + bj1y) * 0.5f;   // map mean
  const float nux = (bi0x + bi1x) * 0.5f, nuy = (bi0y + bi1y) * 0.5f;   // query mean
  const float ax = bj1x - bj0x, ay = bj1y - bj0y;                       // map diff
  const float qx = bi1x - bi0x, qy = bi1y - bi0y;                       // query diff
  const float dot = ax * qx + ay * qy;
  const float crs = qx * ay - qy * ax;
  const float nrm = sqrtf(dot * dot + crs * crs);
  float c = 1.f, s = 0.f;
  if (nrm > 0.f) { c = dot / nrm; s = crs / nrm; }
  const float tx = mux - (c * nux - s * nuy);
  const float ty = muy - (s * nux + c * nuy);
  float* o = poses + i * 3;
  o[0] = atan2f(s, c);
  o[1] = tx;
  o[2] = ty;
}

// ---------------------------------------------------------------------------
// k12: pose scoring.  grid = (point chunks, pose chunks, B), block = 1024.
// The score plane sim[b, n] (X*Y fp32, or a row band of it) is staged in LDS once
// and gathered from there by every pose; each thread keeps PPT poses (cos, sin,
// t) and their accumulators in registers.  Compulsory HBM traffic: sim read once
// per pose chunk.  Partial sums per point chunk are reduced in fixed order
// (deterministic).
// ---------------------------------------------------------------------------
constexpr int PS_THREADS = 1024;
constexpr int PS_LDS_FLOATS = 24 * 1024;  // 96 KiB plane / band buffer

struct ScoreArgs {
  const float* sim;
  const float* q_xy;
  const uint8_t* valid_q;
  const uint8_t* map_valid;
  int Nq, X, Y, P;
  float cell;      // (pose_score_kernel only: its table is in metres)
  int points_per_chunk;
  int RB, NB;      // rows per band, number of bands
  float* partial;  // [B, NCH, P]
  const float* table;  // [B, P, 4] = (cos, sin, tx, ty)
};

__global__ void pose_table_kernel(const float* __restrict__ poses, int64_t total,
                                  float* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float th = poses[i * 3 + 0];
  f32x4 t;
  t[0] = cosf(th); t[1] = sinf(th); t[2] = poses[i * 3 + 1]; t[3] = poses[i * 3 + 2];
  reinterpret_cast<f32x4*>(table)[i] = t;
}

// Same poses as affine maps in CELL units, half-cell shift folded in:
//   cu = A*qx - B*qy + Cx,  cv = B*qx + A*qy + Cy   with A = cos/cell, B = sin/cell,
//   Cx = tx/cell - 0.5, Cy = ty/cell - 0.5.
// (Transform2D.transform followed by "/ cell_size" and the "- 0.5" of interpolate_nd,
// pose_estimation.py:74 + grids.py:129, re-associated: <= 1 ulp on the coordinate.)
__global__ void pose_table_cells_kernel(const float* __restrict__ poses, int64_t total,
                                        float cell, float* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float th = poses[i * 3 + 0];
  f32x4 t;
  t[0] = cosf(th) / cell; t[1] = sinf(th) / cell;
  t[2] = poses[i * 3 + 1] / cell - 0.5f; t[3] = poses[i * 3 + 2] / cell - 0.5f;
  reinterpret_cast<f32x4*>(table)[i] = t;
}

// ---- pieces shared by the scoring kernels -------------------------------------------------------
// the thread's PPT poses (slot k = pose p_base + k * PS_THREADS + tid) from the pose table, sums at 0.
// Out-of-range slots score pose P-1 again; only the final store is guarded.
template <int PPT>
__device__ __forceinline__ void score_load_poses(const ScoreArgs& a, int b, int p_base, int tid,
                                                 f32x2 (&pcs)[PPT], f32x2 (&pt)[PPT],
                                                 float (&acc)[PPT]) {
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = p_base + k * PS_THREADS + tid;
    acc[k] = 0.f;
    const f32x4 t = reinterpret_cast<const f32x4*>(a.table)[(int64_t)b * a.P + min(p, a.P - 1)];
    pcs[k] = f32x2{t[0], t[1]};
    pt[k] = f32x2{t[2], t[3]};
  }
}
// ... and their sums over the point chunk into partial[b, chunk, p]
template <int PPT>
__device__ __forceinline__ void score_store_partial(const ScoreArgs& a, int b, int NCH, int chunk,
                                                    int p_base, int tid, const float (&acc)[PPT]) {
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = p_base + k * PS_THREADS + tid;
    if (p < a.P) a.partial[((int64_t)b * NCH + chunk) * a.P + p] = acc[k];
  }
}

template <int PPT, bool MASK, bool BANDS>
__global__ __launch_bounds__(PS_THREADS) void pose_score_kernel(const ScoreArgs a) {
  extern __shared__ float plane[];
  const int b = blockIdx.z;
  // pose chunk fastest: workgroups sharing the same score planes are dispatched
  // back to back and hit L2 / Infinity Cache on the re-read.
  const int chunk = blockIdx.y;
  const int NCH = gridDim.y;
  const int p_base = blockIdx.x * (PS_THREADS * PPT);
  const int tid = threadIdx.x;
  f32x2 pcs[PPT], pt[PPT];   // (cos, sin), (tx, ty): metres (pose_table_kernel)
  float acc[PPT];
  score_load_poses<PPT>(a, b, p_base, tid, pcs, pt, acc);
  const int n_begin = chunk * a.points_per_chunk;
  const int n_end = min(n_begin + a.points_per_chunk, a.Nq);
  const float Xf = (float)a.X, Yf = (float)a.Y;
  const uint8_t* mvalid = a.map_valid ? a.map_valid + (int64_t)b * a.X * a.Y : nullptr;
  for (int n = n_begin; n < n_end; ++n) {
    if (!a.valid_q[(int64_t)b * a.Nq + n]) continue;  // block-uniform
    const float qx = a.q_xy[((int64_t)b * a.Nq + n) * 2 + 0];
    const float qy = a.q_xy[((int64_t)b * a.Nq + n) * 2 + 1];
    const float* src = a.sim + ((int64_t)b * a.Nq + n) * a.X * a.Y;
    const int nbands = BANDS ? a.NB : 1;
    for (int band = 0; band < nbands; ++band) {
      const int r0 = band * (a.RB - 1);
      const int nrows = min(a.RB, a.X - r0);
      const int nfl = nrows * a.Y;
      __syncthreads();  // previous consumers done
      {
        const float* s0 = src + (int64_t)r0 * a.Y;
        if (((a.Y & 3) == 0)) {
          const f32x4* s4 = reinterpret_cast<const f32x4*>(s0);
          f32x4* d4 = reinterpret_cast<f32x4*>(plane);
          for (int i = tid; i < (nfl >> 2); i += PS_THREADS) d4[i] = s4[i];
        } else {
          for (int i = tid; i < nfl; i += PS_THREADS) plane[i] = s0[i];
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        // (j_t_i @ xy) / cell_size  -- Transform2D.transform, geometry.py:137-139.  This kernel keeps
        // the reference's own sequence (divide by the cell size, four taps, four products); the
        // LDS-DMA kernels below use score_sample / score_lerp on the cell-unit table instead.
        const float xm = (pcs[k].x * qx - pcs[k].y * qy) + pt[k].x;
        const float ym = (pcs[k].y * qx + pcs[k].x * qy) + pt[k].y;
        const float u = xm / a.cell, v = ym / a.cell;
        const float cu = u - 0.5f, cv = v - 0.5f;
        const float fu = floorf(cu), fv = floorf(cv);
        const int i0 = (int)fminf(fmaxf(fu, 0.f), Xf - 1.f);
        bool mine = true;
        if (BANDS) mine = min(i0 / (a.RB - 1), a.NB - 1) == band;
        const int i1 = (int)fminf(fmaxf(fu + 1.f, 0.f), Xf - 1.f);
        const int j0 = (int)fminf(fmaxf(fv, 0.f), Yf - 1.f);
        const int j1 = (int)fminf(fmaxf(fv + 1.f, 0.f), Yf - 1.f);
        const float wu1 = cu - fu, wu0 = 1.f - wu1;
        const float wv1 = cv - fv, wv0 = 1.f - wv1;
        const int l0 = mine ? (i0 - r0) * a.Y : 0, l1 = mine ? (i1 - r0) * a.Y : 0;
        const float s00 = plane[l0 + j0], s01 = plane[l0 + j1];
        const float s10 = plane[l1 + j0], s11 = plane[l1 + j1];
        const float val =
            (((wu0 * wv0) * s00 + (wu0 * wv1) * s01) + (wu1 * wv0) * s10) + (wu1 * wv1) * s11;
        bool ok = mine;
        if (MASK) {
          ok = ok && (u >= 0.f) && (u < Xf) && (v >= 0.f) && (v < Yf);
          ok = ok && mvalid[i0 * a.Y + j0] && mvalid[i0 * a.Y + j1] && mvalid[i1 * a.Y + j0] &&
               mvalid[i1 * a.Y + j1];
        }
        acc[k] += ok ? val : 0.f;
        // keep the PPT bodies sequential: interleaving them spills (16 live
        // bilinear contexts); 4 waves/SIMD already hide the LDS latency.
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  score_store_partial<PPT>(a, b, NCH, chunk, p_base, tid, acc);
}

// ---- the LDS-DMA scoring kernels ----------------------------------------------------------------
// Three kernels stream a point's scores HBM -> LDS by the LDS-DMA path (global_load_lds_dwordx4: no
// VGPR round trip, wave-uniform LDS base + lane*16, i.e. a linear copy) into one of two buffers
// while every thread gathers from the other; one barrier per buffer.  They differ in WHAT is staged
// -- the whole plane (pose_score_db_kernel: X*(Y+4)*4 <= 68 KiB, the 128x128 map), row bands of it
// (pose_score_band_db_kernel) or a window around a centre pose (pose_score_window_kernel) -- and in
// how the per-pose work is scheduled around the barrier.  The sample itself -- coordinates from the
// cell-unit pose table, clamp, floor, weights, the 2x2 gather and the two lerps -- and the order
// of the sums (the chunk's valid points ascending; chunks ascending in the reduce pass) are the
// pieces below in all three: that is why their scores are the same bits.

__device__ __forceinline__ float uniform_f(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
constexpr int PS_DB_MAX_POINTS = 1024;  // valid points of one chunk staged in LDS
constexpr int PS_DB_ROUNDS = 5;           // 16-byte DMA chunks per thread per plane (max)
constexpr int PS_DB_PLANE_BYTES = PS_DB_ROUNDS * PS_THREADS * 16 - 12 * 1024;  // 68 KiB padded plane

// The chunk's valid points [n_begin, n_end), compacted (ascending) into LDS up front by wave 0: the
// staging loop then touches global memory ONLY through the LDS-DMA stream, so the vmcnt(0) at the
// top of an iteration waits for exactly the buffer it is about to read and the next one's DMA
// flies under the arithmetic (any other global load inside the loop would sit behind the in-order
// vmcnt and serialise load and compute).  The caller's barrier publishes the list.
__device__ __forceinline__ void score_point_list(const ScoreArgs& a, int b, int n_begin, int n_end,
                                                 int tid, int* pt_n, float* pt_x, float* pt_y,
                                                 int* pt_count) {
  if (tid >= 64) return;
  const uint8_t* vq = a.valid_q + (int64_t)b * a.Nq;
  int count = 0;
  for (int n0 = n_begin; n0 < n_end; n0 += 64) {
    const int n = n0 + tid;
    const bool v = n < n_end && vq[n] != 0;
    const unsigned long long m = __ballot(v);
    if (v) {
      const int slot = count + __popcll(m & ((1ull << tid) - 1ull));
      pt_n[slot] = n;
      pt_x[slot] = a.q_xy[((int64_t)b * a.Nq + n) * 2 + 0];
      pt_y[slot] = a.q_xy[((int64_t)b * a.Nq + n) * 2 + 1];
    }
    count += __popcll(m);
  }
  if (tid == 0) *pt_count = count;
}

// LDS rows are padded by one 16-byte chunk (pitch S = row + 4 floats): bank(i, j) = (4 i + j) mod
// 32, so samples clamped to the first / last COLUMN (out-of-map poses: a large share of RANSAC
// hypotheses) spread over 8 banks instead of all hitting one.  The DMA writes LDS contiguously but
// each lane may fetch any global chunk, so the pad costs one duplicate chunk per row and no extra
// instructions.  goff[k] = float offset, from the staged region's first cell, of the 16-byte chunk
// this thread fetches in DMA round k (region-invariant).  CRP = chunks per padded row, Y = the
// global row pitch; chunks past `clamp_to` fetch chunk clamp_to (never issued: see score_dma_issue).
template <int ROUNDS>
__device__ __forceinline__ void score_dma_offsets(int tid, int CRP, int Y, int clamp_to,
                                                  int (&goff)[ROUNDS]) {
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    const int c = min(k * PS_THREADS + tid, clamp_to);
    const int row = c / CRP;
    goff[k] = row * Y + 4 * min(c - row * CRP, CRP - 2);
  }
}
// the first `nchunks` chunks of a region: src = its first cell, dst = the LDS buffer
template <int ROUNDS>
__device__ __forceinline__ void score_dma_issue(const float* src, float* dst,
                                                const int (&goff)[ROUNDS], int nchunks, int tid) {
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    const int c = k * PS_THREADS + tid;
    if (c < nchunks)
      lds_dma16(src + goff[k], dst + 4 * c);
  }
}

// One sample of point (qx, qy) under pose (pcs, pt), qx2 = (qx, qx), qyn = (-qy, qy).
// 'nearest' extension == sampling at the clamped coordinate; the cell is capped at (X-2, Y-2) = lim2
// (weight 1 there) so the 2x2 footprint always lies inside the plane.
struct ScoreSample {
  f32x2 w;   // lerp weights along rows (x) and columns (y)
  int off;   // the cell's offset in full-plane rows of pitch Sf
  f32x2 r;   // the unclamped coordinate (mask test)
};
__device__ __forceinline__ ScoreSample score_sample(f32x2 pcs, f32x2 pt, f32x2 qx2, f32x2 qyn,
                                                    f32x2 lim1, f32x2 lim2, float Sf) {
  ScoreSample o;
  o.r = __builtin_elementwise_fma(pcs, qx2, __builtin_elementwise_fma(pcs.yx, qyn, pt));
  const f32x2 c = __builtin_elementwise_min(__builtin_elementwise_max(o.r, f32x2{0.f, 0.f}), lim1);
  const f32x2 f = __builtin_elementwise_min(f32x2{floorf(c.x), floorf(c.y)}, lim2);
  o.w = c - f;
  o.off = (int)fmaf(f.x, Sf, f.y);
  return o;
}
// The 2x2 footprint at q, rows of pitch S: two ds_read2_b32 off ONE address (offsets {0,1} and
// {S,S+1}); each lands as a (col j, col j+1) register pair, so the row lerp is packed f32.
struct ScoreTaps { f32x2 s0, s1; };
__device__ __forceinline__ ScoreTaps score_fetch(const float* q, int S) {
  ScoreTaps t;
  t.s0 = f32x2{q[0], q[1]};
  t.s1 = f32x2{q[S], q[S + 1]};
  return t;
}
__device__ __forceinline__ float score_lerp(const ScoreTaps& tp, f32x2 w) {
  const f32x2 t = __builtin_elementwise_fma(f32x2{w.x, w.x}, tp.s1 - tp.s0, tp.s0);
  return fmaf(w.y, t.y - t.x, t.x);
}
__device__ __forceinline__ float score_gather(const float* q, int S, f32x2 w) {
  return score_lerp(score_fetch(q, S), w);
}

// Whole plane, double-buffered: the plane of the NEXT valid query point streams in while every
// thread gathers from the current one.  This keeps the HBM stream busy during the gather phase --
// the kernel's roofline is the single read of sim.  YC: compile-time row length (0 = run time).
template <int PPT, bool MASK, int YC>
__global__ __launch_bounds__(PS_THREADS) void pose_score_db_kernel(const ScoreArgs a) {
  extern __shared__ float plane[];
  const int b = blockIdx.z;
  const int chunk = blockIdx.y;
  const int NCH = gridDim.y;
  const int p_base = blockIdx.x * (PS_THREADS * PPT);
  const int tid = threadIdx.x;
  const int Y = YC ? YC : a.Y;
  const int XY = a.X * Y;
  const int S = Y + 4;                     // padded LDS row pitch
  const int CRP = (Y >> 2) + 1;            // chunks per padded row
  const int nchunks = a.X * CRP;
  const int PLANE = a.X * S;               // floats per LDS plane
  f32x2 pcs[PPT], pt[PPT];
  float acc[PPT];
  score_load_poses<PPT>(a, b, p_base, tid, pcs, pt, acc);
  const int n_begin = chunk * a.points_per_chunk;
  const int n_end = min(n_begin + a.points_per_chunk, a.Nq);
  const float Xf = (float)a.X, Yf = (float)Y;
  const float Sf = (float)S;
  const f32x2 lim1 = {Xf - 1.f, Yf - 1.f}, lim2 = {Xf - 2.f, Yf - 2.f};
  const uint8_t* mvalid = a.map_valid ? a.map_valid + (int64_t)b * XY : nullptr;

  int goff[PS_DB_ROUNDS];
  score_dma_offsets<PS_DB_ROUNDS>(tid, CRP, Y, nchunks - 1, goff);
  auto issue = [&](int n, int buf) {
    score_dma_issue<PS_DB_ROUNDS>(a.sim + ((int64_t)b * a.Nq + n) * XY, plane + buf * PLANE, goff,
                                  nchunks, tid);
  };
  __shared__ int pt_n[PS_DB_MAX_POINTS];
  __shared__ float pt_x[PS_DB_MAX_POINTS], pt_y[PS_DB_MAX_POINTS];
  __shared__ int pt_count;
  score_point_list(a, b, n_begin, n_end, tid, pt_n, pt_x, pt_y, &pt_count);
  __syncthreads();
  const int count = pt_count;
  int buf = 0;
  if (count > 0) issue(pt_n[0], 0);

  // One sample = coords() (score_sample: pure VALU, needs only the pose and the point) + fetch +
  // blend.  The loop is software-pipelined across the barrier: the coordinates of the first G
  // poses for plane i+1 are computed at the end of iteration i, so every wave fires LDS reads
  // right after the barrier instead of all 16 waves doing address arithmetic while the LDS sits idle.
  auto coords = [&](int k, float qx, float qy) {
    return score_sample(pcs[k], pt[k], f32x2{qx, qx}, f32x2{-qy, qy}, lim1, lim2, Sf);
  };
  auto blend = [&](int k, const ScoreSample& o, const ScoreTaps& tp) {
    const float val = score_lerp(tp, o.w);
    bool ok = true;
    if (MASK) {
      const float u = o.r.x + 0.5f, v = o.r.y + 0.5f;
      ok = (u >= 0.f) && (u < Xf) && (v >= 0.f) && (v < Yf);
      const float gu = floorf(o.r.x), gv = floorf(o.r.y);
      const int i0 = (int)fminf(fmaxf(gu, 0.f), Xf - 1.f);
      const int i1 = (int)fminf(fmaxf(gu + 1.f, 0.f), Xf - 1.f);
      const int j0 = (int)fminf(fmaxf(gv, 0.f), Yf - 1.f);
      const int j1 = (int)fminf(fmaxf(gv + 1.f, 0.f), Yf - 1.f);
      ok = ok && mvalid[i0 * Y + j0] && mvalid[i0 * Y + j1] && mvalid[i1 * Y + j0] &&
           mvalid[i1 * Y + j1];
    }
    acc[k] += ok ? val : 0.f;
  };
  constexpr int G = PPT / 2;
  ScoreSample pre[G];
  {
    const float qx = count > 0 ? pt_x[0] : 0.f, qy = count > 0 ? pt_y[0] : 0.f;
#pragma unroll
    for (int k = 0; k < G; ++k) pre[k] = coords(k, qx, qy);
  }
  for (int i = 0; i < count; ++i) {
    const int inext = min(i + 1, count - 1);
    const float qx = uniform_f(pt_x[i]), qy = uniform_f(pt_y[i]);  // wave-uniform: keep in SGPRs
    const float nqx = uniform_f(pt_x[inext]), nqy = uniform_f(pt_y[inext]);
    wait_vm<0>();
    __syncthreads();  // plane i landed for every wave; the other buffer is free
    if (i + 1 < count) issue(pt_n[i + 1], buf ^ 1);
    const float* pl = plane + buf * PLANE;
    // group 0 reads go out back to back (addresses were ready before the barrier); group
    // 1's coordinates are computed under their latency.  Same again for group 1 with the
    // next plane's group-0 coordinates as the cover.
    ScoreTaps tp[G];
    ScoreSample c1[PPT - G];
#pragma unroll
    for (int k = 0; k < G; ++k) tp[k] = score_fetch(pl + pre[k].off, S);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = G; k < PPT; ++k) c1[k - G] = coords(k, qx, qy);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < G; ++k) blend(k, pre[k], tp[k]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = G; k < PPT; ++k) tp[k - G] = score_fetch(pl + c1[k - G].off, S);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < G; ++k) pre[k] = coords(k, nqx, nqy);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = G; k < PPT; ++k) blend(k, c1[k - G], tp[k - G]);
    buf ^= 1;
  }
  score_store_partial<PPT>(a, b, NCH, chunk, p_base, tid, acc);
}

// Banded variant for planes that do not fit LDS (256x256 maps of the eval path, BASELINE
// configs[3]): the plane of a point streams through LDS in NB bands of RB rows (+1 halo row);
// the samples of the thread's 10 poses (score_sample) are computed once per point and kept in
// registers across its bands, every band then costs a membership test and score_gather.  No
// validity mask (MASK launches take the older band kernel).
template <int PPT>
__global__ __launch_bounds__(PS_THREADS) void pose_score_band_db_kernel(const ScoreArgs a) {
  extern __shared__ float plane[];
  const int b = blockIdx.z;
  const int chunk = blockIdx.y;
  const int NCH = gridDim.y;
  const int p_base = blockIdx.x * (PS_THREADS * PPT);
  const int tid = threadIdx.x;
  const int Y = a.Y;
  const int XY = a.X * Y;
  const int S = Y + 4;
  const int CRP = (Y >> 2) + 1;
  const int RB = a.RB, NB = a.NB;          // band rows (without the halo row), band count
  const int PLANE = (RB + 1) * S;          // floats per LDS band buffer
  f32x2 pcs[PPT], pt[PPT];
  float acc[PPT];
  score_load_poses<PPT>(a, b, p_base, tid, pcs, pt, acc);
  const int n_begin = chunk * a.points_per_chunk;
  const int n_end = min(n_begin + a.points_per_chunk, a.Nq);
  const float Xf = (float)a.X, Yf = (float)Y, Sf = (float)S;
  const f32x2 lim1 = {Xf - 1.f, Yf - 1.f}, lim2 = {Xf - 2.f, Yf - 2.f};

  // (band-invariant; rows past the band end are masked by the chunk count of the band)
  int goff[PS_DB_ROUNDS];
  score_dma_offsets<PS_DB_ROUNDS>(tid, CRP, Y, INT_MAX, goff);
  auto issue = [&](int n, int band, int buf) {
    const int r0 = band * RB;
    const int rows = min(RB + 1, a.X - r0);
    score_dma_issue<PS_DB_ROUNDS>(a.sim + ((int64_t)b * a.Nq + n) * XY + (int64_t)r0 * Y,
                                  plane + buf * PLANE, goff, rows * CRP, tid);
  };
  __shared__ int pt_n[PS_DB_MAX_POINTS];
  __shared__ float pt_x[PS_DB_MAX_POINTS], pt_y[PS_DB_MAX_POINTS];
  __shared__ int pt_count;
  score_point_list(a, b, n_begin, n_end, tid, pt_n, pt_x, pt_y, &pt_count);
  __syncthreads();
  const int count = pt_count;
  const int steps = count * NB;            // (point, band) pairs, band fastest
  int buf = 0;
  if (steps > 0) issue(pt_n[0], 0, 0);
  f32x2 w[PPT];
  int off[PPT];   // cell offset in full-plane padded rows; its row = off / S (fv < Y < S)
  int i = 0, band = 0;
  for (int t = 0; t < steps; ++t) {
    if (band == 0) {
      // per-point state of the 10 poses
      const float qx = uniform_f(pt_x[i]), qy = uniform_f(pt_y[i]);
      const f32x2 qx2 = {qx, qx}, qyn = {-qy, qy};
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const ScoreSample o = score_sample(pcs[k], pt[k], qx2, qyn, lim1, lim2, Sf);
        w[k] = o.w;
        off[k] = o.off;
      }
    }
    wait_vm<0>();
    __syncthreads();  // band t landed for every wave; the other buffer is free
    {
      int ni = i, nb = band + 1;
      if (nb == NB) { nb = 0; ++ni; }
      if (t + 1 < steps) issue(pt_n[ni], nb, buf ^ 1);
    }
    const float* pl = plane + buf * PLANE;
    const int shift = band * RB * S;         // band rows [band*RB, band*RB + RB)
    const int span = RB * S;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const bool in = (unsigned)(off[k] - shift) < (unsigned)span;
      const float val = score_gather(pl + (in ? off[k] - shift : 0), S, w[k]);
      acc[k] += in ? val : 0.f;
    }
    buf ^= 1;
    if (++band == NB) { band = 0; ++i; }
  }
  score_store_partial<PPT>(a, b, NCH, chunk, p_base, tid, acc);
}

// Windowed variant for pose sets whose samples of a point all fall within `rad` cells of ONE centre
// pose per scene -- the 41 x 41 x 41 refinement lattice of grid_refinement (pose_estimation.py:168-205:
// +-4 m, +-5 degrees around the RANSAC pose).  The general kernels above stream the WHOLE score plane of
// every point through LDS once per pose chunk (256 x 256 maps: 262 KB per point and chunk, nine chunks
// for 68 921 poses = 11 GB per scene); here a point's plane is read as ONE window of <= (2 rad + 3) rows x
// (2 rad + 6) columns around the centre pose's image of the point (~80 x 84 cells = 27 KB): 0.14 GB per
// pose chunk.  No validity mask (MASK launches take the general kernels).
struct ScoreWinArgs {
  ScoreArgs s;
  const float* ctable;   // [B, 4] the centre poses as cell-unit affine maps (pose_table_cells_kernel)
  int rad;               // every sample of a point lies within `rad` cells of the centre's
  int WR, WC;            // window rows / columns (WC % 4 == 0)
};
constexpr int PS_WIN_ROUNDS = 3;          // 16-byte DMA chunks per thread and window (max): 48 KB per buffer
constexpr int PS_WIN_PPT = 12;

template <int PPT>
__global__ __launch_bounds__(PS_THREADS) void pose_score_window_kernel(const ScoreWinArgs w) {
  extern __shared__ float plane[];
  const ScoreArgs& a = w.s;
  const int b = blockIdx.z;
  const int chunk = blockIdx.y;
  const int NCH = gridDim.y;
  const int p_base = blockIdx.x * (PS_THREADS * PPT);
  const int tid = threadIdx.x;
  const int X = a.X, Y = a.Y;
  const int XY = X * Y;
  const int WR = w.WR, WC = w.WC, rad = w.rad;
  const int S = WC + 4;                    // LDS row pitch (floats): the window row + one pad chunk
  const int CRP = (WC >> 2) + 1;           // 16-byte chunks per LDS row
  const int PLANE = WR * S;
  f32x2 pcs[PPT], pt[PPT];
  float acc[PPT];
  score_load_poses<PPT>(a, b, p_base, tid, pcs, pt, acc);
  const f32x4 ct = reinterpret_cast<const f32x4*>(w.ctable)[b];
  const int n_begin = chunk * a.points_per_chunk;
  const int n_end = min(n_begin + a.points_per_chunk, a.Nq);
  const float Xf = (float)X, Yf = (float)Y, Sf = (float)S;
  const f32x2 lim1 = {Xf - 1.f, Yf - 1.f}, lim2 = {Xf - 2.f, Yf - 2.f};

  // (offsets relative to the window's first cell: window-invariant)
  int goff[PS_WIN_ROUNDS];
  score_dma_offsets<PS_WIN_ROUNDS>(tid, CRP, Y, INT_MAX, goff);
  const int nchunks = WR * CRP;
  // first cell (row0, col0) of the window of point (qx, qy): the centre pose's cell minus the radius,
  // one more for the floor, kept inside the plane; col0 % 4 == 0 (16-byte DMA chunks)
  auto origin = [&](float qx, float qy) {
    const float cu = fmaf(ct[0], qx, fmaf(ct[1], -qy, ct[2]));
    const float cv = fmaf(ct[1], qx, fmaf(ct[0], qy, ct[3]));
    const float ru = fminf(fmaxf(floorf(cu) - (float)(rad + 1), 0.f), (float)(X - WR));
    const float rv = fminf(fmaxf(floorf(cv) - (float)(rad + 1), 0.f), (float)(Y - WC));
    return make_int2((int)ru, ((int)rv) & ~3);
  };
  auto issue = [&](int n, int2 o, int buf) {
    score_dma_issue<PS_WIN_ROUNDS>(a.sim + ((int64_t)b * a.Nq + n) * XY + (int64_t)o.x * Y + o.y,
                                   plane + buf * PLANE, goff, nchunks, tid);
  };
  __shared__ int pt_n[PS_DB_MAX_POINTS];
  __shared__ float pt_x[PS_DB_MAX_POINTS], pt_y[PS_DB_MAX_POINTS];
  __shared__ int pt_count;
  score_point_list(a, b, n_begin, n_end, tid, pt_n, pt_x, pt_y, &pt_count);
  __syncthreads();
  const int count = pt_count;
  int buf = 0;
  int2 o_cur = make_int2(0, 0);
  if (count > 0) {
    o_cur = origin(uniform_f(pt_x[0]), uniform_f(pt_y[0]));
    issue(pt_n[0], o_cur, 0);
  }
  const int off_max = PLANE - S - 2;
  for (int i = 0; i < count; ++i) {
    const float qx = uniform_f(pt_x[i]), qy = uniform_f(pt_y[i]);
    const f32x2 qx2 = {qx, qx}, qyn = {-qy, qy};
    const int obase = o_cur.x * S + o_cur.y;
    wait_vm<0>();
    __syncthreads();  // window i landed for every wave; the other buffer is free
    if (i + 1 < count) {
      o_cur = origin(uniform_f(pt_x[i + 1]), uniform_f(pt_y[i + 1]));
      issue(pt_n[i + 1], o_cur, buf ^ 1);
    }
    const float* pl = plane + buf * PLANE;
    // four poses at a time: coordinates, the eight LDS reads, the lerps (per-pose state stays in 5 registers)
#pragma unroll
    for (int g = 0; g < PPT; g += 4) {
      f32x2 wt[4];
      const float* q[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const ScoreSample o = score_sample(pcs[g + j], pt[g + j], qx2, qyn, lim1, lim2, Sf);
        wt[j] = o.w;
        // (a pose outside the promised radius reads a clamped cell of the window: wrong, never out of bounds)
        q[j] = pl + min(max(o.off - obase, 0), off_max);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[g + j] += score_gather(q[j], S, wt[j]);
    }
    buf ^= 1;
  }
  score_store_partial<PPT>(a, b, NCH, chunk, p_base, tid, acc);
}

__global__ void pose_score_reduce_kernel(const float* __restrict__ partial, int NCH, int P,
                                         int64_t total, float* __restrict__ scores) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over B*P
  if (i >= total) return;
  const int64_t b = i / P, p = i - b * P;
  float t = 0.f;
#pragma unroll 8
  for (int c = 0; c < NCH; ++c) t += partial[(b * NCH + c) * P + p];
  scores[i] = t;
}

inline int score_chunks(int B, int Nq, int pose_chunks) {
  // aim for >= 512 workgroups overall, at least 8 points per chunk.
  int nch = (512 + B * pose_chunks - 1) / (B * pose_chunks);
  nch = nch < 1 ? 1 : nch;
  const int maxch = (Nq + 7) / 8;
  if (nch > maxch) nch = maxch;
  const int minch = (Nq + PS_DB_MAX_POINTS - 1) / PS_DB_MAX_POINTS;  // LDS point list of the db kernel
  if (nch < minch) nch = minch;
  if (nch < 1) nch = 1;
  return nch;
}
constexpr int PS_PPT = 10;
constexpr int PS_BAND_PPT = 10;  // the banded kernel keeps per-pose sampling state in registers (128 VGPRs at 10: 20 001 hypotheses = two pose chunks, not three)
inline int score_pose_chunks(int P) { return (P + PS_THREADS * PS_PPT - 1) / (PS_THREADS * PS_PPT); }

// What both scoring entry points share on the host: the kernel arguments (whole plane as one band),
// the point chunking -- and so the order of every sum -- and the workspace carved into the pose
// table (16-byte aligned, first) and the per-chunk partial sums.  Returns the point chunk count.
inline int score_setup(ScoreArgs& a, const float* sim, const float* q_xy, const uint8_t* valid_q,
                       const uint8_t* map_valid, int B, int Nq, int X, int Y, int P, float cell_size,
                       void* workspace) {
  a.sim = sim; a.q_xy = q_xy; a.valid_q = valid_q; a.map_valid = map_valid;
  a.Nq = Nq; a.X = X; a.Y = Y; a.P = P;
  a.cell = cell_size;
  const int nch = score_chunks(B, Nq, score_pose_chunks(P));
  a.points_per_chunk = (Nq + nch - 1) / nch;
  a.RB = X; a.NB = 1;
  float* table = static_cast<float*>(workspace);
  a.table = table;
  a.partial = table + (size_t)B * P * 4;
  return nch;
}

// the scoring kernel `fn` on grid (gx, nch, B) with `args` as its one parameter, then the fixed-order
// sum of partial[B, nch, P] into scores[B, P].  Above 64 KiB of LDS the kernel's limit is raised
// to attr_bytes first.
inline int score_launch_and_reduce(const void* fn, int gx, int nch, int B, void* args,
                                   size_t lds_bytes, size_t attr_bytes, const float* partial, int P,
                                   float* scores, hipStream_t s) {
  if (lds_bytes > 64 * 1024 &&
      hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attr_bytes) != hipSuccess)
    return SNAP_ERR_LAUNCH;
  void* kargs[] = {args};
  if (hipLaunchKernel(fn, dim3(gx, nch, B), dim3(PS_THREADS), kargs, lds_bytes, s) != hipSuccess)
    return SNAP_ERR_LAUNCH;
  SNAP_CHECK_LAUNCH();
  const int64_t total = (int64_t)B * P;
  hipLaunchKernelGGL(pose_score_reduce_kernel, dim3((unsigned)snap_cdiv(total, 256)), dim3(256), 0,
                     s, partial, nch, P, total, scores);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

__global__ void refine_lattice_kernel(const float* __restrict__ init,
                                      const float* __restrict__ offs_r,
                                      const float* __restrict__ offs_p, int B, int nr, int np_,
                                      float* __restrict__ out) {
  const int64_t per = (int64_t)nr * np_ * np_;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per * B) return;
  const int b = (int)(i / per);
  int64_t r = i - (int64_t)b * per;
  const int iy = (int)(r % np_); r /= np_;
  const int ix = (int)(r % np_);
  const int ir = (int)(r / np_);
  const float th0 = init[b * 3 + 0], tx0 = init[b * 3 + 1], ty0 = init[b * 3 + 2];
  const float c = cosf(th0), s = sinf(th0);
  const float ox = offs_p[ix], oy = offs_p[iy];
  // compose: angle = a0 + a1; t = t0 + R(a0) t1   (geometry.py:141-144)
  out[i * 3 + 0] = th0 + offs_r[ir];
  out[i * 3 + 1] = tx0 + (c * ox - s * oy);
  out[i * 3 + 2] = ty0 + (s * ox + c * oy);
}

// The order np.argmax / jnp.argmax put on (value, index) pairs: NaN is the maximum and the FIRST NaN wins;
// among numbers the larger value wins and the first of equal values.  An empty slot is (-inf, 0x7fffffff):
// it loses to every real element, including a real -inf.  `>` alone would drop a NaN behind any number.
__device__ __forceinline__ bool argmax_takes(float ov, int oi, float mv, int mi) {
  const bool on = ov != ov, mn = mv != mv;
  if (on != mn) return on;
  return (on || ov == mv) ? oi < mi : ov > mv;
}

// NT threads per row: long rows (the 68 921-pose refinement lattice with one scene per GPU) take 1024 -- one
// workgroup is all the parallelism a row has here, and the scan is bound by its loads in flight
template <int NT>
__global__ __launch_bounds__(NT) void argmax_rows_kernel(const float* __restrict__ scores, int P,
                                                         int start, int32_t* __restrict__ idx) {
  __shared__ float bv[NT];
  __shared__ int bi[NT];
  const int b = blockIdx.x;
  const float* row = scores + (int64_t)b * P;
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int p = start + threadIdx.x; p < P; p += NT) {
    const float v = row[p];
    if (argmax_takes(v, p, best, besti)) { best = v; besti = p; }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = besti;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const float ov = bv[threadIdx.x + o];
      const int oi = bi[threadIdx.x + o];
      const float mv = bv[threadIdx.x];
      const int mi = bi[threadIdx.x];
      if (argmax_takes(ov, oi, mv, mi)) {
        bv[threadIdx.x] = ov;
        bi[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) idx[b] = bi[0] - start;
}

template <int MODE>
int launch_sim(int Dm, dim3 grid, hipStream_t s, const float* fq, const float* fm, int Nq, int XY,
               float scale, int clip, const float* nv, float* sim, float* stats,
               const float* rowstats, float* prob, const float* row_weight) {
  switch (Dm) {
    case 8: hipLaunchKernelGGL((sim_kernel<8, MODE>), grid, dim3(256), 0, s, fq, fm, Nq, XY, scale, clip, nv, sim, stats, rowstats, prob, row_weight); break;
    case 16: hipLaunchKernelGGL((sim_kernel<16, MODE>), grid, dim3(256), 0, s, fq, fm, Nq, XY, scale, clip, nv, sim, stats, rowstats, prob, row_weight); break;
    case 32: hipLaunchKernelGGL((sim_kernel<32, MODE>), grid, dim3(256), 0, s, fq, fm, Nq, XY, scale, clip, nv, sim, stats, rowstats, prob, row_weight); break;
    case 64: hipLaunchKernelGGL((sim_kernel<64, MODE>), grid, dim3(256), 0, s, fq, fm, Nq, XY, scale, clip, nv, sim, stats, rowstats, prob, row_weight); break;
    default: return SNAP_ERR_UNSUPPORTED;
  }
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

}  // namespace

extern "C" size_t snap_sim_rowstats_bytes(int32_t B, int32_t Nq) {
  return (size_t)B * Nq * 2 * sizeof(float);
}

extern "C" int snap_sim_softmax_f32(const float* fq, const float* fm, int32_t B, int32_t Nq,
                                    int32_t XY, int32_t Dm, float scale, int32_t clip_negative,
                                    const float* num_valid, float* sim, float* chunk_stats,
                                    float* prob, float* rowstats, void* stream) {
  return snap_sim_softmax_weighted_f32(fq, fm, B, Nq, XY, Dm, scale, clip_negative, num_valid,
                                       nullptr, sim, chunk_stats, prob, rowstats, stream);
}

extern "C" int snap_sim_softmax_weighted_f32(const float* fq, const float* fm, int32_t B,
                                             int32_t Nq, int32_t XY, int32_t Dm, float scale,
                                             int32_t clip_negative, const float* num_valid,
                                             const float* row_weight, float* sim,
                                             float* chunk_stats, float* prob, float* rowstats,
                                             void* stream) {
  if (!fq || !fm || !num_valid || !sim || !chunk_stats) return SNAP_ERR_NULL;
  if (prob && !rowstats) return SNAP_ERR_NULL;
  if (B <= 0 || Nq <= 0 || XY <= 0) return SNAP_ERR_BAD_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)snap_cdiv(XY, 256), (unsigned)snap_cdiv(Nq, SIM_TQ), (unsigned)B);
  // (the VALU kernel takes unaligned inputs and other Dm; tests reach it through a 4-byte
  //  offset view and compare the two bit for bit)
  const bool aligned = ((reinterpret_cast<uintptr_t>(fq) | reinterpret_cast<uintptr_t>(fm)) & 15) == 0;
  int rc = SNAP_OK;
  if (aligned && (Dm == 8 || Dm == 16 || Dm == 32 || Dm == 64)) {
#define SNAP_SIM_MFMA_CASE(D)                                                                     \
  case D:                                                                                         \
    hipLaunchKernelGGL(sim_mfma_kernel<D>, grid, dim3(256), 0, s, fq, fm, Nq, XY, scale,          \
                       clip_negative, num_valid, sim, chunk_stats, row_weight);                   \
    break;
    switch (Dm) {
      SNAP_SIM_MFMA_CASE(8)
      SNAP_SIM_MFMA_CASE(16)
      SNAP_SIM_MFMA_CASE(32)
      SNAP_SIM_MFMA_CASE(64)
    }
#undef SNAP_SIM_MFMA_CASE
    SNAP_CHECK_LAUNCH();
  } else {
    rc = launch_sim<0>(Dm, grid, s, fq, fm, Nq, XY, scale, clip_negative, num_valid, sim,
                       chunk_stats, nullptr, nullptr, row_weight);
  }
  if (rc != SNAP_OK) return rc;
  if (rowstats) {
    const int64_t rows = (int64_t)B * Nq;
    const int NC = (XY + SIM_CH - 1) / SIM_CH;
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)snap_cdiv(rows, 4)), dim3(256), 0, s,
                       (const float*)chunk_stats, rows, NC, rowstats);
    SNAP_CHECK_LAUNCH();
  }
  if (prob) {
    rc = launch_sim<1>(Dm, grid, s, fq, fm, Nq, XY, scale, clip_negative, num_valid, nullptr,
                       nullptr, rowstats, prob, row_weight);
  }
  return rc;
}

extern "C" size_t snap_sim_split_workspace_bytes(int32_t B, int32_t Nq, int32_t XY, int32_t Dm,
                                                 int32_t parts) {
  if (B <= 0 || Nq <= 0 || XY <= 0 || Dm <= 0 || parts < 2 || parts > 3) return 0;
  return ((size_t)B * Nq + (size_t)B * XY) * parts * Dm * sizeof(__bf16);
}

extern "C" int snap_sim_softmax_split_f32(const float* fq, const float* fm, int32_t B, int32_t Nq,
                                          int32_t XY, int32_t Dm, float scale, int32_t clip_negative,
                                          const float* num_valid, const float* row_weight,
                                          int32_t parts, float* sim, float* chunk_stats,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!fq || !fm || !num_valid || !sim || !chunk_stats || !workspace) return SNAP_ERR_NULL;
  if (B <= 0 || Nq <= 0 || XY <= 0) return SNAP_ERR_BAD_SHAPE;
  if ((Dm != 16 && Dm != 32 && Dm != 64) || (parts != 2 && parts != 3)) return SNAP_ERR_UNSUPPORTED;
  if (workspace_bytes < snap_sim_split_workspace_bytes(B, Nq, XY, Dm, parts)) return SNAP_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return SNAP_ERR_BAD_SHAPE;
  const bool force_general = (clip_negative & 2) != 0;   // bit 1: tests / tools pin the general kernel
  clip_negative &= 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  __bf16* fqs = static_cast<__bf16*>(workspace);
  __bf16* fms = fqs + (size_t)B * Nq * parts * Dm;
  const int64_t nq = (int64_t)B * Nq * Dm, nm = (int64_t)B * XY * Dm;
  if (parts == 3) {
    hipLaunchKernelGGL(sim_presplit_kernel<3>, dim3((unsigned)snap_cdiv(nq, 256)), dim3(256), 0, s, fq, nq, Dm, fqs);
    hipLaunchKernelGGL(sim_presplit_kernel<3>, dim3((unsigned)snap_cdiv(nm, 256)), dim3(256), 0, s, fm, nm, Dm, fms);
  } else {
    hipLaunchKernelGGL(sim_presplit_kernel<2>, dim3((unsigned)snap_cdiv(nq, 256)), dim3(256), 0, s, fq, nq, Dm, fqs);
    hipLaunchKernelGGL(sim_presplit_kernel<2>, dim3((unsigned)snap_cdiv(nm, 256)), dim3(256), 0, s, fm, nm, Dm, fms);
  }
  SNAP_CHECK_LAUNCH();
  const dim3 grid((unsigned)snap_cdiv(XY, 256), (unsigned)snap_cdiv(Nq, SIM_TQ), (unsigned)B);
  // full-chunk shapes (XY % 256 == 0, 16-byte aligned rows) take the lean kernel: same bits
  const bool fast = (XY % 256 == 0) && !(reinterpret_cast<uintptr_t>(sim) & 15) &&
                    !(reinterpret_cast<uintptr_t>(chunk_stats) & 15) && !force_general;
#define SNAP_SIM_SPLIT_CASE(D, P)                                                                  \
  do {                                                                                             \
    if (fast && clip_negative)                                                                     \
      hipLaunchKernelGGL((sim_split_fast_kernel<D, P, true>), grid, dim3(256), 0, s, (const __bf16*)fqs, \
                         (const __bf16*)fms, Nq, XY, scale, num_valid, sim, chunk_stats, row_weight); \
    else if (fast)                                                                                 \
      hipLaunchKernelGGL((sim_split_fast_kernel<D, P, false>), grid, dim3(256), 0, s, (const __bf16*)fqs, \
                         (const __bf16*)fms, Nq, XY, scale, num_valid, sim, chunk_stats, row_weight); \
    else                                                                                           \
      hipLaunchKernelGGL((sim_split_kernel<D, P>), grid, dim3(256), 0, s, (const __bf16*)fqs,      \
                         (const __bf16*)fms, Nq, XY, scale, clip_negative, num_valid, sim, chunk_stats, \
                         row_weight);                                                              \
  } while (0)
  if (parts == 3) {
    if (Dm == 16) SNAP_SIM_SPLIT_CASE(16, 3); else if (Dm == 32) SNAP_SIM_SPLIT_CASE(32, 3); else SNAP_SIM_SPLIT_CASE(64, 3);
  } else {
    if (Dm == 16) SNAP_SIM_SPLIT_CASE(16, 2); else if (Dm == 32) SNAP_SIM_SPLIT_CASE(32, 2); else SNAP_SIM_SPLIT_CASE(64, 2);
  }
#undef SNAP_SIM_SPLIT_CASE
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

extern "C" int snap_ransac_sample_f32(const float* fq, const float* fm, const float* chunk_stats,
                                      int32_t B, int32_t Nq, int32_t X, int32_t Y, int32_t Dm,
                                      float scale, int32_t clip_negative, int32_t S, uint64_t seed,
                                      const float* uniforms, int32_t* corr, void* stream) {
  return snap_ransac_sample_ws_f32(fq, fm, chunk_stats, B, Nq, X, Y, Dm, scale, clip_negative, S,
                                   seed, uniforms, corr, nullptr, 0, stream);
}

extern "C" size_t snap_ransac_sample_workspace_bytes(int32_t B, int32_t Nq) {
  return (size_t)B * Nq * 65 * sizeof(float);   // 64 lane prefixes + the row maximum
}

extern "C" int snap_ransac_sample_ws_f32(const float* fq, const float* fm, const float* chunk_stats,
                                         int32_t B, int32_t Nq, int32_t X, int32_t Y, int32_t Dm,
                                         float scale, int32_t clip_negative, int32_t S,
                                         uint64_t seed, const float* uniforms, int32_t* corr,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return snap_ransac_sample_rows_f32(fq, fm, chunk_stats, nullptr, B, Nq, X, Y, Dm, scale,
                                     clip_negative, S, seed, uniforms, corr, workspace,
                                     workspace_bytes, stream);
}

extern "C" int snap_ransac_sample_rows_f32(const float* fq, const float* fm,
                                           const float* chunk_stats, const float* row_cdf,
                                           int32_t B, int32_t Nq, int32_t X, int32_t Y,
                                           int32_t Dm, float scale, int32_t clip_negative,
                                           int32_t S, uint64_t seed, const float* uniforms,
                                           int32_t* corr, void* workspace, size_t workspace_bytes,
                                           void* stream) {
  return snap_ransac_sample_sim_f32(fq, fm, chunk_stats, row_cdf, nullptr, nullptr, B, Nq, X, Y, Dm,
                                    scale, clip_negative, S, seed, uniforms, corr, workspace,
                                    workspace_bytes, stream);
}

extern "C" int snap_ransac_sample_sim_f32(const float* fq, const float* fm,
                                          const float* chunk_stats, const float* row_cdf,
                                          const float* sim, const float* row_unscale, int32_t B,
                                          int32_t Nq, int32_t X, int32_t Y, int32_t Dm, float scale,
                                          int32_t clip_negative, int32_t S, uint64_t seed,
                                          const float* uniforms, int32_t* corr, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  if (!fq || !fm || !chunk_stats || !corr) return SNAP_ERR_NULL;
  if ((sim == nullptr) != (row_unscale == nullptr)) return SNAP_ERR_NULL;
  if (B <= 0 || Nq <= 0 || X <= 0 || Y <= 0 || S <= 0) return SNAP_ERR_BAD_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* lane_incl = nullptr;
  float* rowmax = nullptr;
  if (workspace) {
    if (workspace_bytes < snap_ransac_sample_workspace_bytes(B, Nq)) return SNAP_ERR_WORKSPACE;
    const int64_t rows = (int64_t)B * Nq;
    lane_incl = static_cast<float*>(workspace);
    rowmax = lane_incl + rows * 64;
    const int NC = (X * Y + SIM_CH - 1) / SIM_CH;
    hipLaunchKernelGGL(chunk_prefix_kernel, dim3((unsigned)snap_cdiv(rows, 4)), dim3(256), 0, s,
                       chunk_stats, rows, NC, lane_incl, rowmax);
    SNAP_CHECK_LAUNCH();
  }
  {
    const int NC = (X * Y + SIM_CH - 1) / SIM_CH;
    // (without a workspace: the table-free kernel, one correspondence per wave, same samples)
    if (lane_incl && sim && row_unscale && (NC + 63) / 64 <= 64) {
      constexpr int NQ = 4;
      const dim3 fgrid((unsigned)snap_cdiv(S, 4 * NQ), (unsigned)B);
      hipLaunchKernelGGL(ransac_sample_fast_kernel<NQ>, fgrid, dim3(256), 0, s, chunk_stats, Nq, X, Y, S,
                         seed, uniforms, corr, (const float*)lane_incl, (const float*)rowmax, row_cdf,
                         sim, row_unscale);
      SNAP_CHECK_LAUNCH();
      return SNAP_OK;
    }
  }
  const dim3 grid((unsigned)snap_cdiv(S, 4), (unsigned)B);
  switch (Dm) {
    case 8: hipLaunchKernelGGL(ransac_sample_kernel<8>, grid, dim3(256), 0, s, fq, fm, chunk_stats, Nq, X, Y, scale, clip_negative, S, seed, uniforms, corr, (const float*)lane_incl, (const float*)rowmax, row_cdf, sim, row_unscale); break;
    case 16: hipLaunchKernelGGL(ransac_sample_kernel<16>, grid, dim3(256), 0, s, fq, fm, chunk_stats, Nq, X, Y, scale, clip_negative, S, seed, uniforms, corr, (const float*)lane_incl, (const float*)rowmax, row_cdf, sim, row_unscale); break;
    case 32: hipLaunchKernelGGL(ransac_sample_kernel<32>, grid, dim3(256), 0, s, fq, fm, chunk_stats, Nq, X, Y, scale, clip_negative, S, seed, uniforms, corr, (const float*)lane_incl, (const float*)rowmax, row_cdf, sim, row_unscale); break;
    case 64: hipLaunchKernelGGL(ransac_sample_kernel<64>, grid, dim3(256), 0, s, fq, fm, chunk_stats, Nq, X, Y, scale, clip_negative, S, seed, uniforms, corr, (const float*)lane_incl, (const float*)rowmax, row_cdf, sim, row_unscale); break;
    default: return SNAP_ERR_UNSUPPORTED;
  }
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

extern "C" int snap_masked_softmax_rows_f32(const float* x, const uint8_t* mask, int32_t B,
                                            int32_t N, float* weights, float* cdf, void* stream) {
  if (!x || !mask || !weights || !cdf) return SNAP_ERR_NULL;
  if (B <= 0 || N <= 0) return SNAP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(masked_softmax_rows_kernel, dim3((unsigned)B), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, mask, N, weights, cdf);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

extern "C" int snap_poses_from_corr_f32(const int32_t* corr, const float* q_xy, int32_t B,
                                        int32_t Nq, int32_t P, int32_t retries, float cell_size,
                                        float* poses, void* stream) {
  if (!corr || !q_xy || !poses) return SNAP_ERR_NULL;
  if (B <= 0 || Nq <= 0 || P <= 0 || retries <= 0) return SNAP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(poses_from_corr_kernel, dim3((unsigned)snap_cdiv((int64_t)B * P, 256)),
                     dim3(256), 0, static_cast<hipStream_t>(stream), corr, q_xy, B, Nq, P, retries,
                     cell_size, poses);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

extern "C" size_t snap_pose_score_workspace_bytes(int32_t B, int32_t Nq, int32_t P, int32_t X,
                                                  int32_t Y) {
  (void)X; (void)Y;
  const int pch = score_pose_chunks(P);
  const int nch = score_chunks(B, Nq, pch);
  // pose table (16-byte aligned, first) + per-chunk partial sums.
  return (size_t)B * P * 4 * sizeof(float) + (size_t)B * nch * P * sizeof(float);
}

extern "C" int snap_pose_score_f32(const float* sim, const float* poses, const float* q_xy,
                                   const uint8_t* valid_q, const uint8_t* map_valid, int32_t B,
                                   int32_t Nq, int32_t X, int32_t Y, int32_t P, float cell_size,
                                   int32_t mask_oob, float* scores, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!sim || !poses || !q_xy || !valid_q || !scores || !workspace) return SNAP_ERR_NULL;
  if (mask_oob && !map_valid) return SNAP_ERR_NULL;
  if (B <= 0 || Nq <= 0 || X <= 0 || Y <= 0 || P <= 0) return SNAP_ERR_BAD_SHAPE;
  if (Y > PS_LDS_FLOATS / 2) return SNAP_ERR_UNSUPPORTED;
  if (workspace_bytes < snap_pose_score_workspace_bytes(B, Nq, P, X, Y)) return SNAP_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return SNAP_ERR_BAD_SHAPE;
  ScoreArgs a;
  const int nch = score_setup(a, sim, q_xy, valid_q, map_valid, B, Nq, X, Y, P, cell_size, workspace);
  if ((int64_t)X * Y > PS_LDS_FLOATS) {
    a.RB = PS_LDS_FLOATS / Y;
    a.NB = (X - 1 + (a.RB - 1) - 1) / (a.RB - 1);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool bands = a.NB > 1;
  // double-buffered LDS-DMA variant: two whole planes must fit (2 * XY * 4 <= 128 KiB).
  const bool use_db = !bands && (Y % 4 == 0) && X >= 2 && Y >= 2 &&
                      ((int64_t)X * (Y + 4) * 4 <= PS_DB_PLANE_BYTES);
  // banded double-buffered variant: a plane that does not fit streams through in row bands
  const int band_rows = (int)(PS_DB_PLANE_BYTES / ((size_t)(Y + 4) * sizeof(float))) - 1;
  const bool use_band_db = !use_db && !mask_oob && (Y % 4 == 0) && X >= 2 && Y >= 2 &&
                           band_rows >= 1 && X > band_rows;
  const void* fn = nullptr;
  size_t lds_bytes = (size_t)min((int64_t)a.RB * Y, (int64_t)PS_LDS_FLOATS) * sizeof(float);
  size_t attr_bytes = PS_LDS_FLOATS * sizeof(float);
  int gx = score_pose_chunks(P);
  if (use_band_db) {
    a.RB = band_rows;
    a.NB = (X - 1 + band_rows - 1) / band_rows;     // cell rows 0 .. X-2
    fn = (const void*)&pose_score_band_db_kernel<PS_BAND_PPT>;
    lds_bytes = (size_t)2 * (band_rows + 1) * (Y + 4) * sizeof(float);
    // (the banded kernel carries PS_BAND_PPT poses per thread; the point chunking and the partial
    // buffer layout [B, nch, P] are the same)
    gx = (P + PS_THREADS * PS_BAND_PPT - 1) / (PS_THREADS * PS_BAND_PPT);
  } else if (use_db) {
    if (Y == 128)
      fn = mask_oob ? (const void*)&pose_score_db_kernel<PS_PPT, true, 128>
                    : (const void*)&pose_score_db_kernel<PS_PPT, false, 128>;
    else
      fn = mask_oob ? (const void*)&pose_score_db_kernel<PS_PPT, true, 0>
                    : (const void*)&pose_score_db_kernel<PS_PPT, false, 0>;
    lds_bytes = (size_t)2 * X * (Y + 4) * sizeof(float);
  } else if (mask_oob) fn = bands ? (const void*)&pose_score_kernel<PS_PPT, true, true>
                           : (const void*)&pose_score_kernel<PS_PPT, true, false>;
  else fn = bands ? (const void*)&pose_score_kernel<PS_PPT, false, true>
                  : (const void*)&pose_score_kernel<PS_PPT, false, false>;
  if (use_db || use_band_db) {
    attr_bytes = 2 * PS_DB_PLANE_BYTES;
    hipLaunchKernelGGL(pose_table_cells_kernel, dim3((unsigned)snap_cdiv((int64_t)B * P, 256)),
                       dim3(256), 0, s, poses, (int64_t)B * P, cell_size, static_cast<float*>(workspace));
  } else {
    hipLaunchKernelGGL(pose_table_kernel, dim3((unsigned)snap_cdiv((int64_t)B * P, 256)),
                       dim3(256), 0, s, poses, (int64_t)B * P, static_cast<float*>(workspace));
  }
  SNAP_CHECK_LAUNCH();
  return score_launch_and_reduce(fn, gx, nch, B, &a, lds_bytes, attr_bytes, a.partial, P, scores, s);
}

extern "C" size_t snap_pose_score_window_workspace_bytes(int32_t B, int32_t Nq, int32_t P, int32_t X,
                                                         int32_t Y) {
  return snap_pose_score_workspace_bytes(B, Nq, P, X, Y) + (size_t)B * 4 * sizeof(float) + 16;
}

extern "C" int32_t snap_pose_score_window_supported(int32_t X, int32_t Y, int32_t radius_cells) {
  if (X < 2 || Y < 4 || Y % 4 != 0 || radius_cells < 0) return 0;
  const int WR = min(2 * radius_cells + 3, X);
  const int WC = min((2 * radius_cells + 6 + 3) & ~3, Y);
  return (int64_t)WR * ((WC >> 2) + 1) <= (int64_t)PS_WIN_ROUNDS * PS_THREADS ? 1 : 0;
}

extern "C" int snap_pose_score_window_f32(const float* sim, const float* poses, const float* centers,
                                          int32_t radius_cells, const float* q_xy,
                                          const uint8_t* valid_q, int32_t B, int32_t Nq, int32_t X,
                                          int32_t Y, int32_t P, float cell_size, float* scores,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!sim || !poses || !centers || !q_xy || !valid_q || !scores || !workspace) return SNAP_ERR_NULL;
  if (B <= 0 || Nq <= 0 || X <= 0 || Y <= 0 || P <= 0) return SNAP_ERR_BAD_SHAPE;
  if (!snap_pose_score_window_supported(X, Y, radius_cells)) return SNAP_ERR_UNSUPPORTED;
  if (workspace_bytes < snap_pose_score_window_workspace_bytes(B, Nq, P, X, Y)) return SNAP_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return SNAP_ERR_BAD_SHAPE;
  ScoreWinArgs w;
  ScoreArgs& a = w.s;
  const int nch = score_setup(a, sim, q_xy, valid_q, nullptr, B, Nq, X, Y, P, cell_size, workspace);
  float* ctable = a.partial + (size_t)B * nch * P;
  ctable = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ctable) + 15) & ~(uintptr_t)15);
  w.ctable = ctable;
  w.rad = radius_cells;
  w.WR = min(2 * radius_cells + 3, X);
  w.WC = min((2 * radius_cells + 6 + 3) & ~3, Y);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pose_table_cells_kernel, dim3((unsigned)snap_cdiv((int64_t)B * P, 256)), dim3(256), 0,
                     s, poses, (int64_t)B * P, cell_size, static_cast<float*>(workspace));
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(pose_table_cells_kernel, dim3((unsigned)snap_cdiv((int64_t)B, 256)), dim3(256), 0, s,
                     centers, (int64_t)B, cell_size, ctable);
  SNAP_CHECK_LAUNCH();
  const size_t lds_bytes = (size_t)2 * w.WR * (w.WC + 4) * sizeof(float);
  const int gx = (P + PS_THREADS * PS_WIN_PPT - 1) / (PS_THREADS * PS_WIN_PPT);
  return score_launch_and_reduce((const void*)&pose_score_window_kernel<PS_WIN_PPT>, gx, nch, B, &w,
                                 lds_bytes, lds_bytes, a.partial, P, scores, s);
}

extern "C" int snap_refine_lattice_f32(const float* init, const float* offs_r, const float* offs_p,
                                       int32_t B, int32_t nr, int32_t np_, float* out,
                                       void* stream) {
  if (!init || !offs_r || !offs_p || !out) return SNAP_ERR_NULL;
  if (B <= 0 || nr <= 0 || np_ <= 0) return SNAP_ERR_BAD_SHAPE;
  const int64_t total = (int64_t)B * nr * np_ * np_;
  hipLaunchKernelGGL(refine_lattice_kernel, dim3((unsigned)snap_cdiv(total, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), init, offs_r, offs_p, B, nr, np_, out);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

extern "C" int snap_argmax_rows_f32(const float* scores, int32_t B, int32_t P, int32_t start,
                                    int32_t* idx, void* stream) {
  if (!scores || !idx) return SNAP_ERR_NULL;
  if (B <= 0 || P <= 0 || start < 0 || start >= P) return SNAP_ERR_BAD_SHAPE;
  if (P - start > 4096)
    hipLaunchKernelGGL(argmax_rows_kernel<1024>, dim3(B), dim3(1024), 0, static_cast<hipStream_t>(stream),
                       scores, P, start, idx);
  else
    hipLaunchKernelGGL(argmax_rows_kernel<256>, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       scores, P, start, idx);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
