// The pose distribution of a vote volume: snap_vote_posterior_f32 (include/snap_hip.h).
//
// votes [R, Ho, Wo] f32 are unnormalised log-scores; with x = scale * v over the FINITE cells (the contributing set
// F; -inf = masked, NaN / +inf = excluded and counted) the op returns log_z = log sum_F exp(x), the two marginals
// log_prob_xy [Ho, Wo] and log_prob_r [R], the moments of p = exp(x - log_z) (means, central second moments,
// circular mean / resultant of the rotation, entropy) and the interpolated log-probability of a ground-truth index.
//
// Launch A (vote_posterior_tiles_kernel, <= 1024 workgroups striding over tiles of 256 consecutive pixels
// p = a * Wo + b; one pixel per thread, so a wave's loads of one rotation are 256 contiguous bytes):
//   walk 1 over r: the pixel's maximum m_p = max fl(scale * v) and its cell counts; the tile maximum m_t;
//   walk 2 over r (the tile's 256 R cells again: L2): e = expf(fma(scale, v, -m_p)), s_p = sum_r e and
//     t_p = sum_r e (x - m_p) in f32 (<= R terms of one sign); per rotation the wave's tree sum of e * f_p,
//     f_p = expf(m_p - m_t), the pixel's weight relative to the tile maximum.
//   Above the pixel everything is float64: W = sum_p f_p s_p, W a, W b, W a^2, W a b, W b^2, the entropy term
//   T = sum_p f_p (t_p + (m_p - m_t) s_p) = sum w (x - m_t), and the R per-rotation sums across the four waves.
//   A workgroup with several tiles folds (m_t, sums) into its running (m, sums) by the same rescaling launch B uses.
//   It writes s_p (into log_prob_xy) and m_p (workspace) per pixel and ONE partial row (m, 7 sums, R sums) and two
//   counts per workgroup.  A tile (workgroup) without a contributing cell has m = -inf and all sums exactly 0: it is
//   never rescaled (no exp(-inf - (-inf))).
// Launch B (vote_posterior_finish_kernel, 1 + n workgroups of 1024 threads): every workgroup folds the
//   <= 1024 (m_g, W_g) pairs into the global maximum M and Z' = sum_g exp(m_g - M) W_g in one fixed tree (the same
//   bits in every workgroup); workgroups 1 .. n write log_prob_xy[p] = (m_p - M) + log s_p - log Z' in float64,
//   rounded once; workgroup 0 folds the partial rows column by column (8 chunks of workgroups in order, then the
//   chunks in order) and writes log_prob_r, the statistics, the counts and the ground-truth sample.
// No atomics and no inter-workgroup hand-off inside a launch: every sum's order is a function of (R, Ho, Wo) alone.
#include "vote_common.h"

namespace {

constexpr int PO_NT = 256;                  // launch A: threads = pixels of a tile
constexpr int PO_WAVES = PO_NT / SNAP_WAVE;
constexpr int PO_MAX_R = 64;
constexpr int PO_MAX_GROUPS = 1024;         // launch A workgroups = launch B threads
constexpr int PO_HEAD = 8;                  // partial row: m | W, Wa, Wb, Waa, Wab, Wbb, T | s[R]
constexpr int PO_COLS = PO_HEAD + PO_MAX_R;
constexpr int PO_NB = 1024;                 // launch B threads
constexpr int PO_NB_WAVES = PO_NB / SNAP_WAVE;
constexpr int PO_CHUNKS = 8;                // launch B, workgroup 0: column sums in 8 chunks of workgroups
constexpr int PO_CHUNK_COLS = PO_NB / PO_CHUNKS;
constexpr int PO_MAX_NORM_GROUPS = 256;
static_assert(PO_COLS <= PO_CHUNK_COLS && PO_COLS <= PO_NT, "one thread per partial column");

__global__ __launch_bounds__(PO_NT) void vote_posterior_tiles_kernel(
    const float* __restrict__ votes, int R, int P, int Wo, float scale, int tiles, float* __restrict__ sum_xy,
    float* __restrict__ pix_m, double* __restrict__ part, int32_t* __restrict__ cnt) {
  __shared__ float wmax[PO_WAVES];
  __shared__ float wsum[PO_WAVES][PO_MAX_R];
  __shared__ double wred[PO_WAVES][PO_HEAD - 1];
  __shared__ double acc[PO_COLS];           // the running sums, relative to m_run (column 0 unused)
  __shared__ float m_run_s;
  __shared__ int wcnt[PO_WAVES][2];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int cols = PO_HEAD + R;
  if (t < cols) acc[t] = 0.0;
  if (t == 0) m_run_s = -INFINITY;
  int n_ok = 0, n_bad = 0;

  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();                        // acc / m_run_s of the previous tile; wmax, wsum, wred free again
    int p;
    const bool in = vote_tile_pixel<PO_NT>(tile, P, &p);
    const float* src = votes + p;
    // ---- walk 1: the pixel's maximum and counts
    float m_p = -INFINITY;
    if (in) {
#pragma unroll 4
      for (int r = 0; r < R; ++r) {
        const float v = src[(size_t)r * P];
        if (vote_finite(v)) {
          m_p = fmaxf(m_p, scale * v);
          ++n_ok;
        } else if (!(v == -INFINITY)) {
          ++n_bad;                          // NaN or +inf
        }
      }
      pix_m[p] = m_p;
    }
    const float wm = wave_max(m_p);          // (vote_block_max written out: wmax needs no second barrier here)
    if (lane == 0) wmax[wave] = wm;
    __syncthreads();
    const float m_t = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (m_t == -INFINITY) {                 // (uniform) no contributing cell: contributes exactly nothing
      if (in) sum_xy[p] = 0.f;
      continue;
    }
    // ---- walk 2: weights relative to the pixel's own maximum, scaled to the tile's by f_p
    const bool live = in && m_p > -INFINITY;
    const float f_p = live ? expf(m_p - m_t) : 0.f;
    float s_p = 0.f, t_p = 0.f;
    for (int r = 0; r < R; ++r) {
      float e = 0.f;
      if (live) {
        const float v = src[(size_t)r * P];
        if (vote_finite(v)) {
          const float d = fmaf(scale, v, -m_p);
          e = expf(d);
          s_p += e;
          t_p += e * d;
        }
      }
      const float ws = wave_sum(e * f_p);
      if (lane == 0) wsum[wave][r] = ws;
    }
    if (in) sum_xy[p] = s_p;
    // ---- float64 above the pixel
    double val[PO_HEAD - 1];
    {
      int a, b;
      vote_row_col(p, Wo, &a, &b);
      const double fd = (double)f_p, sd = (double)s_p, da = (double)a, db = (double)b;
      const double W = live ? sd * fd : 0.0;
      val[0] = W;
      val[1] = W * da;
      val[2] = W * db;
      val[3] = W * (da * da);
      val[4] = W * (da * db);
      val[5] = W * (db * db);
      val[6] = live ? fd * ((double)t_p + ((double)m_p - (double)m_t) * sd) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < PO_HEAD - 1; ++i) {
      const double s = vote_wave_sum(val[i]);
      if (lane == 0) wred[wave][i] = s;
    }
    __syncthreads();
    // ---- fold the tile into the running sums: thread c owns column c
    double nv = 0.0;
    const float m_run = m_run_s;
    const float m_new = fmaxf(m_run, m_t);
    if (t >= 1 && t < cols) {
      const double fa = m_run > -INFINITY ? exp((double)m_run - (double)m_new) : 0.0;
      const double fb = exp((double)m_t - (double)m_new);
      double pv;
      if (t < PO_HEAD) {
        pv = (wred[0][t - 1] + wred[1][t - 1]) + (wred[2][t - 1] + wred[3][t - 1]);
      } else {
        const int r = t - PO_HEAD;
        pv = ((double)wsum[0][r] + (double)wsum[1][r]) + ((double)wsum[2][r] + (double)wsum[3][r]);
      }
      if (t == PO_HEAD - 1) {               // T is relative to the maximum: shift both sides to the new one
        const double Wp = (wred[0][0] + wred[1][0]) + (wred[2][0] + wred[3][0]);
        const double ta = m_run > -INFINITY ? fa * (acc[t] + ((double)m_run - (double)m_new) * acc[1]) : 0.0;
        nv = ta + fb * (pv + ((double)m_t - (double)m_new) * Wp);
      } else {
        nv = acc[t] * fa + pv * fb;
      }
    }
    __syncthreads();
    if (t >= 1 && t < cols) acc[t] = nv;
    if (t == 0) m_run_s = m_new;
  }
  __syncthreads();
  if (t < cols) part[(size_t)blockIdx.x * cols + t] = t == 0 ? (double)m_run_s : acc[t];
  n_ok = vote_wave_sum(n_ok);
  n_bad = vote_wave_sum(n_bad);
  if (lane == 0) {
    wcnt[wave][0] = n_ok;
    wcnt[wave][1] = n_bad;
  }
  __syncthreads();
  if (t < 2) cnt[(size_t)blockIdx.x * 2 + t] = (wcnt[0][t] + wcnt[1][t]) + (wcnt[2][t] + wcnt[3][t]);
}

__global__ __launch_bounds__(PO_NB) void vote_posterior_finish_kernel(
    const float* __restrict__ votes, int R, int Ho, int Wo, int P, float scale, const float* __restrict__ gt,
    int groups, int norm_groups, const double* __restrict__ part, const float* __restrict__ pix_m,
    const int32_t* __restrict__ cnt, float* __restrict__ lxy, float* __restrict__ lr, float* __restrict__ stats,
    int32_t* __restrict__ count) {
  __shared__ float shm[PO_NB_WAVES];
  __shared__ double shz[PO_NB_WAVES];
  __shared__ int shc[PO_NB_WAVES][2];
  __shared__ double fg[PO_MAX_GROUPS];
  __shared__ double red[PO_CHUNKS][PO_CHUNK_COLS];
  __shared__ double tot[PO_COLS];
  __shared__ double csw[2][PO_MAX_R];       // cos / sin of a rotation times its sum
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int cols = PO_HEAD + R;
  const float nan = __int_as_float(0x7fc00000);

  // ---- the global maximum and Z' = sum_g exp(m_g - M) W_g: one fixed tree, the same in every workgroup
  const float m_g = t < groups ? (float)part[(size_t)t * cols] : -INFINITY;
  const double W_g = t < groups ? part[(size_t)t * cols + 1] : 0.0;
  // (vote_block_max / vote_block_sum written out: shm and shz are used once, so neither needs a second barrier)
  const float wm = wave_max(m_g);
  if (lane == 0) shm[wave] = wm;
  __syncthreads();
  float M = -INFINITY;
  for (int w = 0; w < PO_NB_WAVES; ++w) M = fmaxf(M, shm[w]);
  const double f = m_g > -INFINITY ? exp((double)m_g - (double)M) : 0.0;
  const double zs = vote_wave_sum(f * W_g);
  if (lane == 0) shz[wave] = zs;
  __syncthreads();
  const double Zp = vote_waves_sum<PO_NB_WAVES>(shz);   // (the 16 waves in sequence)
  const bool empty = !(M > -INFINITY);
  const double logZp = empty ? 0.0 : log(Zp);

  if (blockIdx.x > 0) {
    // ---- normalise the per-pixel sums in place
    for (int64_t p = (int64_t)(blockIdx.x - 1) * PO_NB + t; p < P; p += (int64_t)norm_groups * PO_NB) {
      const float s = lxy[p], m = pix_m[p];
      lxy[p] = (m > -INFINITY && s > 0.f) ? (float)((((double)m - (double)M) + log((double)s)) - logZp) : -INFINITY;
    }
    return;
  }

  // ---- workgroup 0: counts, the column sums, log_prob_r, the statistics, the ground-truth sample
  {
    // (written out, not vote_block_count_pair: thread 64 stores both counts with its stats, one dwordx2)
    const int c0 = vote_wave_sum(t < groups ? cnt[(size_t)t * 2] : 0);
    const int c1 = vote_wave_sum(t < groups ? cnt[(size_t)t * 2 + 1] : 0);
    if (lane == 0) {
      shc[wave][0] = c0;
      shc[wave][1] = c1;
    }
  }
  fg[t] = f;
  __syncthreads();
  {
    const int col = t % PO_CHUNK_COLS, chunk = t / PO_CHUNK_COLS;
    const int per = (groups + PO_CHUNKS - 1) / PO_CHUNKS;
    const int g0 = chunk * per, g1 = min(groups, g0 + per);
    double s = 0.0;
    if (col >= 1 && col < cols) {
      // (no branch in the loop: the loads of successive workgroups' rows stay independent and in flight together;
      //  a workgroup without contributing cells has fg = 0 and a row of zeros, its m = -inf kept out by the select)
      const bool is_t = col == PO_HEAD - 1;
#pragma unroll 8
      for (int g = g0; g < g1; ++g) {
        const double fgg = fg[g];
        const double v = part[(size_t)g * cols + col];
        const double mg = is_t ? part[(size_t)g * cols] : 0.0;
        const double wg = is_t ? part[(size_t)g * cols + 1] : 0.0;
        const double shift = fgg > 0.0 ? (mg - (double)M) * wg : 0.0;
        s += fgg > 0.0 ? fgg * (v + shift) : 0.0;
      }
    }
    red[chunk][col] = s;
  }
  __syncthreads();
  if (t < cols) {
    double s = 0.0;
    for (int c = 0; c < PO_CHUNKS; ++c) s += red[c][t];
    tot[t] = s;
  }
  __syncthreads();

  if (t < R) {                              // (one rotation per thread: the float64 cos / sin are the long part)
    const double w = tot[PO_HEAD + t];
    const double ang = 6.283185307179586476925 * (double)t / (double)R;
    csw[0][t] = cos(ang) * w;
    csw[1][t] = sin(ang) * w;
    lr[t] = (!empty && w > 0.0) ? (float)(log(w) - logZp) : -INFINITY;
  }
  __syncthreads();

  const double log_z = empty ? -(double)INFINITY : (double)M + logZp;
  if (t == 64) {
    int c0 = 0, c1 = 0;
    for (int w = 0; w < PO_NB_WAVES; ++w) {
      c0 += shc[w][0];
      c1 += shc[w][1];
    }
    count[0] = c0;
    count[1] = c1;
    stats[0] = (float)log_z;
    stats[1] = M;
    if (empty) {
      for (int i = 2; i < 12; ++i) stats[i] = nan;
    } else {
      const double W = tot[1];
      const double ea = tot[2] / W, eb = tot[3] / W;
      stats[2] = (float)ea;
      stats[3] = (float)eb;
      stats[4] = (float)(tot[4] / W - ea * ea);
      stats[5] = (float)(tot[5] / W - ea * eb);
      stats[6] = (float)(tot[6] / W - eb * eb);
      double zr = 0.0, c = 0.0, s = 0.0;
      for (int r = 0; r < R; ++r) {
        zr += tot[PO_HEAD + r];
        c += csw[0][r];
        s += csw[1][r];
      }
      c /= zr;
      s /= zr;
      stats[7] = (float)c;
      stats[8] = (float)s;
      double k = atan2(s, c) * (double)R / 6.283185307179586476925;
      if (k < 0.0) k += (double)R;
      float kf = (float)k;
      if (kf >= (float)R) kf = 0.f;         // (a tiny negative angle rounds up to R: the same direction as 0)
      stats[9] = kf;
      stats[10] = (float)hypot(c, s);
      stats[11] = (float)(logZp - tot[PO_HEAD - 1] / W);
    }
    stats[13] = stats[14] = stats[15] = 0.f;
  }
  if (t == 128) {
    float res = nan;
    int valid = 0;
    if (gt != nullptr && !empty) {
      const float k = gt[0], i = gt[1], j = gt[2];
      if (vote_finite(k) && vote_finite(i) && vote_finite(j) && i >= 0.f && i <= (float)(Ho - 1) && j >= 0.f &&
          j <= (float)(Wo - 1)) {
        const double kfl = floor((double)k), ifl = floor((double)i), jfl = floor((double)j);
        const double wk = (double)k - kfl, wi = (double)i - ifl, wj = (double)j - jfl;
        double km = fmod(kfl, (double)R);
        if (km < 0.0) km += (double)R;
        int k0 = (int)km;
        if (k0 >= R) k0 = 0;
        const int k1 = vote_next(k0, R);
        const int i0 = (int)ifl, j0 = (int)jfl;
        double sum = 0.0;
        bool ok = true;
        for (int tap = 0; tap < 8; ++tap) {
          const int dk = tap >> 2, di = (tap >> 1) & 1, dj = tap & 1;
          const double w = (dk ? wk : 1.0 - wk) * (di ? wi : 1.0 - wi) * (dj ? wj : 1.0 - wj);
          if (w == 0.0) continue;           // a tap of weight 0 is not read
          const int rr = dk ? k1 : k0, aa = i0 + di, bb = j0 + dj;
          if (aa >= Ho || bb >= Wo) {       // (unreachable: the upper tap's weight is 0 on the last row / column)
            ok = false;
            continue;
          }
          const float v = votes[((size_t)rr * Ho + aa) * Wo + bb];
          if (vote_finite(v))
            sum += w * (double)(scale * v);
          else
            ok = false;
        }
        if (ok) {
          res = (float)(sum - log_z);
          valid = 1;
        }
      }
    }
    stats[12] = res;
    count[2] = valid;
  }
}

struct PoPlan : VotePlan {   // (the tiles are cut from ONE plane: every rotation of a pixel belongs to its thread)
  int norm_groups;
};

bool po_plan(int R, int Ho, int Wo, PoPlan* plan) {
  if (R < 1 || R > PO_MAX_R || Ho < 1 || Wo < 1) return false;
  if (!vote_plan((int64_t)R * Ho * Wo, 1, Ho, Wo, PO_NT, PO_MAX_GROUPS, plan)) return false;
  const int64_t ng = snap_cdiv(plan->P, 4 * PO_NB);
  plan->norm_groups = (int)(ng < PO_MAX_NORM_GROUPS ? ng : PO_MAX_NORM_GROUPS);
  return true;
}

// [groups][8 + R] float64 partial rows | [Ho Wo] f32 pixel maxima | [groups][2] counts
struct PoWorkspace {
  double* part;
  float* pix_m;
  int32_t* cnt;
  size_t bytes;
};

PoWorkspace po_workspace(const PoPlan& plan, int R, void* workspace) {
  VoteLayout l{workspace};
  return {l.take<double>((size_t)plan.groups * (PO_HEAD + R)), l.take<float>(plan.P),
          l.take<int32_t>((size_t)plan.groups * 2), l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_posterior_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo) {
  PoPlan plan;
  if (!po_plan(R, Ho, Wo, &plan)) return 0;
  return po_workspace(plan, R, nullptr).bytes;
}

extern "C" int snap_vote_posterior_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale,
                                       const float* gt_index, float* log_prob_xy, float* log_prob_r, float* stats,
                                       int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  if (!votes || !log_prob_xy || !log_prob_r || !stats || !count || !workspace) return SNAP_ERR_NULL;
  PoPlan plan;
  if (!po_plan(R, Ho, Wo, &plan)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale > 0.f) || !(scale < INFINITY)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, po_workspace(plan, R, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const PoWorkspace w = po_workspace(plan, R, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vote_posterior_tiles_kernel, dim3(plan.groups), dim3(PO_NT), 0, s, votes, R, plan.P, Wo, scale,
                     plan.tiles, log_prob_xy, w.pix_m, w.part, w.cnt);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_posterior_finish_kernel, dim3(1 + plan.norm_groups), dim3(PO_NB), 0, s, votes, R, Ho, Wo,
                     plan.P, scale, gt_index, plan.groups, plan.norm_groups, w.part, w.pix_m, w.cnt, log_prob_xy,
                     log_prob_r, stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
