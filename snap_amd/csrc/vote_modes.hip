// Per-peak mass, mean and covariance of a vote volume: snap_vote_modes_f32 (include/snap_hip.h).
//
// votes [R, Ho, Wo] f32 are unnormalised log-scores; x = (double)scale * (double)v over the FINITE cells
// (vote_posterior's rule).  peaks [K, 3] int32 = (r, a, b) rows on the device (vote_peaks' table; a row with a component
// out of range is EMPTY).  A peak's window is |dr| <= win_r (circular), |da|, |db| <= win_xy (clipped); a cell inside
// several windows belongs to the peak with the smallest D = wr^2 (da^2 + db^2) + win_xy^2 dr^2 (int32, exact), ties to
// the lowest k: a partition.  Per mode: the log mass of its owned contributing cells, their mean offset from the peak
// and the six central second moments, and the NEES of a ground-truth index under (covariance + I / 12).
//
// Launch 1 (vote_modes_planes_kernel, K (2 win_r + 1) workgroups of 256): workgroup (k, j) walks the
//   (2 win_xy + 1)^2 cells of peak k's window in rotation r_k + j - win_r, cell i = t, t + 256, ... per thread (<= 17),
//   with the peak table in LDS for the ownership test.  Walk 1: the largest owned finite vote, the counts, and one bit
//   per owned contributing cell; walk 2 (the same cells again: L2) e = exp(x - m) and the sums e, e da, e db, e da^2,
//   e da db, e db^2 in float64.  One partial row (m, 6 sums) and two counts per workgroup.
// Launch 2 (vote_modes_finish_kernel, one workgroup, thread k = mode k): the mode's maximum over its planes, the
//   planes' sums rescaled to it and added in the order dr = -win_r .. win_r (the rotation moments follow from dr, which
//   is constant in a plane), then the outputs.
// No atomics; a thread's cells, the workgroup reductions (vote_common.h) and the order of the planes are functions of
// (K, win_r, win_xy) alone, so two calls give the same bytes.
#include "vote_common.h"

namespace {

constexpr int MD_NT = 256;
constexpr int MD_WAVES = MD_NT / SNAP_WAVE;
constexpr int MD_MAX_K = 64;
constexpr int MD_MAX_WIN_R = 4;
constexpr int MD_MAX_WIN_XY = 32;
constexpr int MD_MAX_SIDE = 2 * MD_MAX_WIN_XY + 1;
constexpr int MD_MAX_ITERS = (MD_MAX_SIDE * MD_MAX_SIDE + MD_NT - 1) / MD_NT;   // cells of a window per thread
constexpr int MD_COLS = 8;                  // partial row: m | S0, Sa, Sb, Saa, Sab, Sbb | 0
static_assert(MD_MAX_ITERS <= 32, "one bit per cell of a thread");
static_assert(MD_MAX_K <= SNAP_WAVE, "the finish kernel holds one mode per thread of one wave");

// Row k of the peak table -> LDS; an empty row (a component out of range) as r = -1.
__device__ __forceinline__ void md_load_peak(const int32_t* __restrict__ peaks, int k, int R, int Ho, int Wo,
                                             int (*s_pk)[3]) {
  const int r = peaks[k * 3], a = peaks[k * 3 + 1], b = peaks[k * 3 + 2];
  const bool ok = r >= 0 && r < R && a >= 0 && a < Ho && b >= 0 && b < Wo;
  s_pk[k][0] = ok ? r : -1;
  s_pk[k][1] = ok ? a : 0;
  s_pk[k][2] = ok ? b : 0;
}

// r - r_k as its nearest representative (0 <= r, r_k < R).  |result| = R / 2 either way for an even R: outside every
// supported window (2 win_r + 1 <= R).
__device__ __forceinline__ int md_wrap_offset(int d, int R) {
  if (2 * d > R) d -= R;
  if (2 * d < -R) d += R;
  return d;
}

// Does peak k own cell (r, a, b), which lies in its window at D = dist?  Not if another non-empty peak has the cell in
// its window at a smaller D, or at the same D with a lower row number.
__device__ __forceinline__ bool md_owned(const int (*s_pk)[3], int K, int k, int dist, int r, int a, int b, int R,
                                         int win_r, int win_xy, int wr2, int wxy2) {
  bool owned = true;
  for (int q = 0; q < K; ++q) {
    const int rq = s_pk[q][0];
    if (rq < 0 || q == k) continue;
    const int dr = md_wrap_offset(r - rq, R), da = a - s_pk[q][1], db = b - s_pk[q][2];
    if (abs(dr) > win_r || abs(da) > win_xy || abs(db) > win_xy) continue;
    const int dq = wr2 * (da * da + db * db) + wxy2 * (dr * dr);   // <= 16 * 2048 + 1024 * 16
    if (dq < dist || (dq == dist && q < k)) owned = false;
  }
  return owned;
}

__global__ __launch_bounds__(MD_NT) void vote_modes_planes_kernel(
    const float* __restrict__ votes, int R, int Ho, int Wo, float scale, const int32_t* __restrict__ peaks, int K,
    int win_r, int win_xy, double* __restrict__ part, int32_t* __restrict__ cpart) {
  __shared__ int s_pk[MD_MAX_K][3];
  __shared__ float shm[MD_WAVES];
  __shared__ double shd[MD_WAVES];
  __shared__ int shc[MD_WAVES][2];
  const int t = threadIdx.x;
  const int planes = 2 * win_r + 1;
  const int k = blockIdx.x / planes, dr = blockIdx.x - k * planes - win_r;
  if (t < K) md_load_peak(peaks, t, R, Ho, Wo, s_pk);
  __syncthreads();
  double* row = part + (size_t)blockIdx.x * MD_COLS;
  int32_t* crow = cpart + (size_t)blockIdx.x * 2;
  const int rk = s_pk[k][0], ak = s_pk[k][1], bk = s_pk[k][2];
  if (rk < 0) {                             // (uniform) an empty row owns nothing; no address is formed from it
    if (t < MD_COLS) row[t] = t == 0 ? -(double)INFINITY : 0.0;
    if (t < 2) crow[t] = 0;
    return;
  }
  const int r = vote_wrap(rk + dr, R);
  const int side = 2 * win_xy + 1, cells = side * side;
  const int wr = win_r > 1 ? win_r : 1, wr2 = wr * wr, wxy2 = win_xy * win_xy;
  const float* plane = votes + (size_t)r * Ho * Wo;

  // ---- walk 1: ownership, the largest owned finite vote, the counts
  uint32_t live = 0;                        // bit n: this thread's n-th cell is owned and contributes
  float vm = -INFINITY;
  int n_ok = 0, n_bad = 0;
  for (int n = 0, i = t; i < cells; ++n, i += MD_NT) {
    const int ia = i / side;
    const int da = ia - win_xy, db = i - ia * side - win_xy;
    const int a = ak + da, b = bk + db;
    if (a < 0 || a >= Ho || b < 0 || b >= Wo) continue;
    const int dist = wr2 * (da * da + db * db) + wxy2 * (dr * dr);
    if (!md_owned(s_pk, K, k, dist, r, a, b, R, win_r, win_xy, wr2, wxy2)) continue;
    const float v = plane[(size_t)a * Wo + b];
    if (vote_finite(v)) {
      vm = fmaxf(vm, v);
      ++n_ok;
      live |= 1u << n;
    } else if (!(v == -INFINITY)) {
      ++n_bad;                              // NaN or +inf
    }
  }
  vm = vote_block_max<MD_WAVES>(vm, shm);
  const int c = vote_block_count_pair<MD_WAVES>(n_ok, n_bad, shc);
  if (t < 2) crow[t] = c;
  // (scale > 0 and a float64 product rounds monotonically: the largest x is the x of the largest v)
  const double ds = (double)scale;
  const double m = vm > -INFINITY ? ds * (double)vm : -(double)INFINITY;

  // ---- walk 2: the weights relative to the plane's maximum and their offset moments
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int n = 0, i = t; i < cells; ++n, i += MD_NT) {
    if (!((live >> n) & 1u)) continue;
    const int ia = i / side;
    const int da = ia - win_xy, db = i - ia * side - win_xy;
    const float v = plane[(size_t)(ak + da) * Wo + (bk + db)];
    const double e = exp(ds * (double)v - m);
    const double fa = (double)da, fb = (double)db;
    s[0] += e;
    s[1] += e * fa;
    s[2] += e * fb;
    s[3] += e * (fa * fa);
    s[4] += e * (fa * fb);
    s[5] += e * (fb * fb);
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double tot = vote_block_sum<MD_WAVES>(s[q], shd);
    if (t == 0) row[1 + q] = tot;
  }
  if (t == 0) {
    row[0] = m;
    row[7] = 0.0;
  }
}

// x^T A^-1 x of a symmetric positive definite 3 x 3 A = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]: the
// cofactors over the determinant.
__device__ __forceinline__ double md_quadratic_form(double a00, double a01, double a02, double a11, double a12,
                                                    double a22, double x0, double x1, double x2) {
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double q = x0 * (c00 * x0 + c01 * x1 + c02 * x2) + x1 * (c01 * x0 + c11 * x1 + c12 * x2) +
                   x2 * (c02 * x0 + c12 * x1 + c22 * x2);
  return q / det;
}

__global__ __launch_bounds__(SNAP_WAVE) void vote_modes_finish_kernel(
    int R, const int32_t* __restrict__ peaks, int K, int win_r, const float* __restrict__ gt,
    const double* __restrict__ part, const int32_t* __restrict__ cpart, float* __restrict__ stats,
    int32_t* __restrict__ count) {
  const int k = threadIdx.x;
  if (k >= K) return;
  const float nan = __int_as_float(0x7fc00000);
  const int planes = 2 * win_r + 1;
  const double* rows = part + (size_t)k * planes * MD_COLS;
  const int32_t* crows = cpart + (size_t)k * planes * 2;
  float* out = stats + (size_t)k * 16;
  double M = -(double)INFINITY;
  int c0 = 0, c1 = 0;
  for (int j = 0; j < planes; ++j) {
    M = fmax(M, rows[j * MD_COLS]);
    c0 += crows[j * 2];
    c1 += crows[j * 2 + 1];
  }
  count[k * 2] = c0;
  count[k * 2 + 1] = c1;
  for (int i = 12; i < 16; ++i) out[i] = 0.f;
  if (!(M > -(double)INFINITY)) {           // an empty row, or no owned contributing cell
    out[0] = out[1] = -INFINITY;
    for (int i = 2; i < 12; ++i) out[i] = nan;
    return;
  }
  // (M is finite, so the row is not empty: its components are in range)
  const int rk = peaks[k * 3], ak = peaks[k * 3 + 1], bk = peaks[k * 3 + 2];
  double S0 = 0.0, Sr = 0.0, Sa = 0.0, Sb = 0.0, Srr = 0.0, Sra = 0.0, Srb = 0.0, Saa = 0.0, Sab = 0.0, Sbb = 0.0;
  for (int j = 0; j < planes; ++j) {        // dr = -win_r .. win_r, in this order
    const double* p = rows + j * MD_COLS;
    if (!(p[0] > -(double)INFINITY)) continue;
    const double f = exp(p[0] - M), d = (double)(j - win_r);
    const double s0 = f * p[1], sa = f * p[2], sb = f * p[3];
    S0 += s0;
    Sr += d * s0;
    Sa += sa;
    Sb += sb;
    Srr += (d * d) * s0;
    Sra += d * sa;
    Srb += d * sb;
    Saa += f * p[4];
    Sab += f * p[5];
    Sbb += f * p[6];
  }
  const double er = Sr / S0, ea = Sa / S0, eb = Sb / S0;
  const double vrr = Srr / S0 - er * er, vra = Sra / S0 - er * ea, vrb = Srb / S0 - er * eb;
  const double vaa = Saa / S0 - ea * ea, vab = Sab / S0 - ea * eb, vbb = Sbb / S0 - eb * eb;
  double mr = (double)rk + er;
  if (mr < 0.0) mr += (double)R;
  if (mr >= (double)R) mr -= (double)R;
  const double ma = (double)ak + ea, mb = (double)bk + eb;
  float mrf = (float)mr;
  if (mrf >= (float)R) mrf = 0.f;           // (just below R rounds up to R: the same rotation as 0)
  out[0] = (float)(M + log(S0));
  out[1] = (float)M;
  out[2] = mrf;
  out[3] = (float)ma;
  out[4] = (float)mb;
  out[5] = (float)vrr;
  out[6] = (float)vra;
  out[7] = (float)vrb;
  out[8] = (float)vaa;
  out[9] = (float)vab;
  out[10] = (float)vbb;
  float nees = nan;
  if (gt != nullptr) {
    const float gk = gt[0], gi = gt[1], gj = gt[2];
    if (vote_finite(gk) && vote_finite(gi) && vote_finite(gj)) {
      const double e0 = remainder((double)gk - mr, (double)R);   // the nearest representative (IEEE: exact)
      const double e1 = (double)gi - ma, e2 = (double)gj - mb;
      const double cell = 1.0 / 12.0;       // the variance of a uniform distribution over one lattice cell
      nees = (float)md_quadratic_form(vrr + cell, vra, vrb, vaa + cell, vab, vbb + cell, e0, e1, e2);
    }
  }
  out[11] = nees;
}

bool md_supported(int R, int Ho, int Wo, int K, int win_r, int win_xy) {
  if (R < 1 || Ho < 1 || Wo < 1 || !vote_cells_fit((int64_t)R * Ho * Wo)) return false;
  if (K < 1 || K > MD_MAX_K || win_r < 0 || win_r > MD_MAX_WIN_R || 2 * win_r + 1 > R) return false;
  return win_xy >= 1 && win_xy <= MD_MAX_WIN_XY;
}

// [K (2 win_r + 1)][8] float64 partial rows | [K (2 win_r + 1)][2] counts
struct MdWorkspace {
  double* part;
  int32_t* cpart;
  size_t bytes;
};

MdWorkspace md_workspace(int K, int win_r, void* workspace) {
  VoteLayout l{workspace};
  const size_t groups = (size_t)K * (2 * win_r + 1);
  return {l.take<double>(groups * MD_COLS), l.take<int32_t>(groups * 2), l.bytes};
}

}  // namespace

extern "C" size_t snap_vote_modes_workspace_bytes(int32_t R, int32_t Ho, int32_t Wo, int32_t K, int32_t win_r,
                                                  int32_t win_xy) {
  if (!md_supported(R, Ho, Wo, K, win_r, win_xy)) return 0;
  return md_workspace(K, win_r, nullptr).bytes;
}

extern "C" int snap_vote_modes_f32(const float* votes, int32_t R, int32_t Ho, int32_t Wo, float scale,
                                   const int32_t* peaks, int32_t K, int32_t win_r, int32_t win_xy,
                                   const float* gt_index, float* stats, int32_t* count, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!votes || !peaks || !stats || !count || !workspace) return SNAP_ERR_NULL;
  if (!md_supported(R, Ho, Wo, K, win_r, win_xy)) return SNAP_ERR_BAD_SHAPE;
  if (!(scale > 0.f) || !(scale < INFINITY)) return SNAP_ERR_UNSUPPORTED;
  if (!vote_workspace_ok(workspace, workspace_bytes, md_workspace(K, win_r, nullptr).bytes)) return SNAP_ERR_WORKSPACE;
  const MdWorkspace w = md_workspace(K, win_r, workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vote_modes_planes_kernel, dim3(K * (2 * win_r + 1)), dim3(MD_NT), 0, s, votes, R, Ho, Wo, scale,
                     peaks, K, win_r, win_xy, w.part, w.cpart);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(vote_modes_finish_kernel, dim3(1), dim3(SNAP_WAVE), 0, s, R, peaks, K, win_r, gt_index,
                     w.part, w.cpart, stats, count);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}
