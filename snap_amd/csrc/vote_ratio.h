// The RATIO step of the vote-volume smoother (snap_vote_smooth_f32): its two kernels and the one function that launches
// them, shared by vote_smooth.hip and vote_pairs.hip: the pairwise posterior of a step is built on the very
// q = gamma_{t+1} / prior the smoother carries back, so lg, G and q have to be the smoother's bits.  They are, because
// both files run the two kernels below through vr_launch_ratio (and -ffp-contract=off is in force), on the predict
// step's launch shape and with its linkage (vote_predict.h): min(tiles, VP_MAX_GROUPS) workgroups of VP_NT threads
// striding over the n cells.
//
// Float64 per cell: a cell has ratio mass iff next is finite and prior > 0; then lg = next - log(prior); G = max lg;
// q = fl32(exp(lg - G)) iff fl32(lg - G) >= VP_CUT, else 0; Q = sum q.
//
// The ratio step owns the partial columns after the predict step's (VR_D_G, VR_D_Q; VR_I_BADNEXT, VR_I_RATIO), the
// including file the others.
#ifndef SNAP_CSRC_VOTE_RATIO_H_
#define SNAP_CSRC_VOTE_RATIO_H_

#include "vote_predict.h"

enum { VR_D_G = 2, VR_D_Q = 3 };
enum { VR_I_BADNEXT = 2, VR_I_RATIO = 3 };

// The largest of the workgroup's values (a maximum: exact in any order), the same bits in every thread.
__device__ __forceinline__ double vr_block_max(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double m = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  __syncthreads();
  return m;
}
template <int DS>
__device__ __forceinline__ double vr_fold_max(const double* __restrict__ dpart, int col, int groups, double* sh) {
  double v = -(double)INFINITY;
  for (int g = threadIdx.x; g < groups; g += VP_NT) v = fmax(v, dpart[(size_t)g * DS + col]);
  return vr_block_max(v, sh);
}

// The ratio of one cell, float64: lg = next - log(prior); false where the cell has no ratio mass (next not finite, or
// a prior of 0).
__device__ __forceinline__ bool vr_ratio(const VpPrior& c, float t2, float next, double* lg) {
  if (!vote_finite(next)) return false;
  const double prior = vp_prior(c, t2);
  if (!(prior > 0.0)) return false;
  *lg = (double)next - log(prior);
  return true;
}

// ---- every workgroup folds the partial sums into S; per cell lg; per workgroup the largest lg (float64), the count of
// NaN / +inf cells of `next` and of cells with ratio mass
template <int DS, int IS>
__device__ __forceinline__ void vr_max(const float* __restrict__ t2, const float* __restrict__ next, int n, float eps,
                                       double* __restrict__ dpart, int32_t* __restrict__ ipart) {
  __shared__ double shd[VP_WAVES];
  __shared__ int shi[VP_WAVES];
  const VpPrior c = vp_prior_setup(vote_fold_sum<VP_WAVES, DS>(dpart, VP_D_SUMT2, gridDim.x, shd), true, eps, n);
  double G = -(double)INFINITY;
  int bad = 0, mass = 0;
  for (int64_t i = (int64_t)blockIdx.x * VP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * VP_NT) {
    const float v = next[i];
    double lg;
    if (vr_ratio(c, t2[i], v, &lg)) {
      G = fmax(G, lg);
      ++mass;
    } else if (!vote_finite(v) && !(v == -INFINITY)) {
      ++bad;                                // NaN or +inf
    }
  }
  G = vr_block_max(G, shd);
  bad = vote_block_sum<VP_WAVES>(bad, shi);
  mass = vote_block_sum<VP_WAVES>(mass, shi);
  if (threadIdx.x == 0) {
    dpart[(size_t)blockIdx.x * DS + VR_D_G] = G;
    ipart[(size_t)blockIdx.x * IS + VR_I_BADNEXT] = bad;
    ipart[(size_t)blockIdx.x * IS + VR_I_RATIO] = mass;
  }
}

// ---- every workgroup folds the maxima into G (a maximum: exact), recomputes lg (the same expression: the same bits)
// and writes q, ONCE: the float64 log and exp sit on this pass, not on the taps; per workgroup sum q (float64)
template <int DS>
__device__ __forceinline__ void vr_mass(const float* __restrict__ t2, const float* __restrict__ next, int n, float eps,
                                        float* __restrict__ q, double* __restrict__ dpart) {
  __shared__ double shd[VP_WAVES];
  const VpPrior c = vp_prior_setup(vote_fold_sum<VP_WAVES, DS>(dpart, VP_D_SUMT2, gridDim.x, shd), true, eps, n);
  const double G = vr_fold_max<DS>(dpart, VR_D_G, gridDim.x, shd);
  double sum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * VP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * VP_NT) {
    double lg;
    float m = 0.f;
    if (vr_ratio(c, t2[i], next[i], &lg)) {   // (then G is finite and lg <= G)
      const double d = lg - G;
      if ((float)d >= VP_CUT) m = (float)exp(d);
    }
    q[i] = m;
    sum += (double)m;
  }
  sum = vote_block_sum<VP_WAVES>(sum, shd);
  if (threadIdx.x == 0) dpart[(size_t)blockIdx.x * DS + VR_D_Q] = sum;
}

namespace {   // (LINKAGE, vote_predict.h)

// The kernels: each is one body above.
template <int DS, int IS>
__global__ __launch_bounds__(VP_NT) void vr_max_kernel(const float* __restrict__ t2, const float* __restrict__ next,
                                                       int n, float eps, double* __restrict__ dpart,
                                                       int32_t* __restrict__ ipart) {
  vr_max<DS, IS>(t2, next, n, eps, dpart, ipart);
}
template <int DS>
__global__ __launch_bounds__(VP_NT) void vr_mass_kernel(const float* __restrict__ t2, const float* __restrict__ next,
                                                        int n, float eps, float* __restrict__ q,
                                                        double* __restrict__ dpart) {
  vr_mass<DS>(t2, next, n, eps, q, dpart);
}

// Launches 5-6 of the smoother and of the tap posteriors, in this order: max (t2, next -> G), mass (-> q, Q).  q is a
// volume of its own.  Returns SNAP_OK or SNAP_ERR_LAUNCH.
template <int FS, int DS, int IS>
int vr_launch_ratio(const VpPlan& plan, const float* t2, const float* next, float eps, float* q,
                    const VpParts<FS, DS, IS>& part, hipStream_t s) {
  const dim3 grid(plan.groups), block(VP_NT);
  hipLaunchKernelGGL((vr_max_kernel<DS, IS>), grid, block, 0, s, t2, next, plan.n, eps, part.d, part.i);
  SNAP_CHECK_LAUNCH();
  hipLaunchKernelGGL((vr_mass_kernel<DS>), grid, block, 0, s, t2, next, plan.n, eps, q, part.d);
  SNAP_CHECK_LAUNCH();
  return SNAP_OK;
}

}  // namespace

#endif  // SNAP_CSRC_VOTE_RATIO_H_
