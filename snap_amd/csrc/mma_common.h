// Device primitives shared by the GEMM-shaped kernels (included by common.h; no kernels, nothing
// host-side): the vector types, the f32 -> bf16 split and its packing into MFMA fragments, the
// operand element types, the vector-memory waits, the 16-byte LDS-DMA, the half-type stores, the
// swizzled fragment fetch with the ordered split product (and its k-step for an operand that is
// stationary in registers), the accumulator row map, and the fused input prologue.
#ifndef SNAP_CSRC_MMA_COMMON_H_
#define SNAP_CSRC_MMA_COMMON_H_

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// Four f32 -> NS x four bf16 (packed two per dword): hi = bf16(v), mid = bf16(v - hi), lo =
// bf16(v - hi - mid).  split_step takes one part off an element PAIR: one v_cvt_pk_bf16_f32 (RNE);
// the value it represents is recovered by a shift / mask of the packed dword and subtracted
// exactly in f32 (3 VALU per element and part instead of the 4 the generic vector conversion
// costs), which leaves the residual in `pr`.
__device__ __forceinline__ unsigned split_step(f32x2& pr) {
  const bf16x2 b = __builtin_convertvector(pr, bf16x2);
  unsigned u;
  __builtin_memcpy(&u, &b, 4);
  pr = f32x2{pr[0] - __uint_as_float(u << 16), pr[1] - __uint_as_float(u & 0xffff0000u)};   // exact
  return u;
}
template <int NS>
__device__ __forceinline__ void split_bf16(const f32x4& v, u32x2 (&out)[NS]) {
  f32x2 pr[2] = {{v[0], v[1]}, {v[2], v[3]}};
#pragma unroll
  for (int p = 0; p < NS; ++p)
#pragma unroll
    for (int h = 0; h < 2; ++h) out[p][h] = split_step(pr[h]);
}
// The two-part split pair by pair (U2: u32x2 or unsigned[2]).  Same values; only the order in
// which the four conversions are written differs from split_bf16<2>, and the schedulers follow
// it: each order keeps the instruction stream (and, for the 128 x 128 tail kernels of
// conv_split.hip, the scratch size) its callers had before the two were one file.
template <class U2>
__device__ __forceinline__ void split_bf16(const f32x4& v, U2& hi, U2& lo) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f32x2 pr = {v[2 * h], v[2 * h + 1]};
    hi[h] = split_step(pr);
    lo[h] = split_step(pr);
  }
}
// Two split 4-element halves (k = 0..3 | 4..7 of a lane's octet) -> the hi / lo MFMA fragments
__device__ __forceinline__ void pack_frag(const u32x2 (&h)[2], const u32x2 (&l)[2], bf16x8& hi, bf16x8& lo) {
  const u32x4 hh = {h[0][0], h[0][1], h[1][0], h[1][1]};
  const u32x4 ll = {l[0][0], l[0][1], l[1][0], l[1][1]};
  __builtin_memcpy(&hi, &hh, 16);
  __builtin_memcpy(&lo, &ll, 16);
}

// Element type of the rounded operands of the training-precision engines: bf16 (default) or IEEE
// half (F16: the reference's dtype=float16 train config, train_localization.py:93 -- 11 significand
// bits instead of 8, the exponent range of half: values beyond 65504 round to inf and reach the
// trainer's non-finite check, gradients below 6e-8 flush -- which is what DynamicScale is for,
// trainer.py:391-392).
template <bool F16> struct Elem;
template <> struct Elem<false> {
  typedef __bf16 T; typedef bf16x8 x8; typedef bf16x4 x4;
  static __device__ __forceinline__ f32x16 mfma(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Elem<true> {
  typedef _Float16 T; typedef f16x8 x8; typedef f16x4 x4;
  static __device__ __forceinline__ f32x16 mfma(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// s_waitcnt vmcnt(N): at most N of the wave's vector-memory instructions still in flight
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// ... for an n the optimiser knows (an unrolled stage loop): one case survives
__device__ __forceinline__ void wait_vm_n(int n) {
  switch (n) {
#define SNAP_W(N) case N: wait_vm<N>(); break;
#define SNAP_W8(B) SNAP_W(B) SNAP_W(B + 1) SNAP_W(B + 2) SNAP_W(B + 3) SNAP_W(B + 4) SNAP_W(B + 5) SNAP_W(B + 6) SNAP_W(B + 7)
    SNAP_W8(0) SNAP_W8(8) SNAP_W8(16) SNAP_W8(24) SNAP_W8(32) SNAP_W8(40) SNAP_W8(48) SNAP_W8(56)
#undef SNAP_W8
#undef SNAP_W
    default: wait_vm<0>(); break;
  }
}

// LDS-DMA: every lane moves 16 bytes global -> LDS without a register (the LDS address is the
// wave-uniform base of lane 0's `lds_dst` + 16 x lane)
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void cglobal_void_t;
__device__ __forceinline__ void lds_dma16(const void* src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((cglobal_void_t*)src, (lds_void_t*)lds_dst, 16, 0, 0);
}

// four f32 -> elements index .. index + 3 of a bf16 (HALF = 1) / IEEE half (HALF = 2) array, RNE
template <int HALF>
__device__ __forceinline__ void store_half4(void* base, int64_t index, f32x4 v) {
  static_assert(HALF == 1 || HALF == 2, "1 = bf16, 2 = IEEE half");
  if constexpr (HALF == 1)
    *reinterpret_cast<bf16x4*>(static_cast<__bf16*>(base) + index) = __builtin_convertvector(v, bf16x4);
  else
    *reinterpret_cast<f16x4*>(static_cast<_Float16*>(base) + index) = __builtin_convertvector(v, f16x4);
}

// Operand images of the split engines: [row][16 k] bf16 = 32 B per row, the two 16-byte k-octets
// XOR-swizzled by (row >> 3) & 1 so that the MFMA fragment fetch -- one ds_read_b128 per lane --
// is conflict-free.  Byte offset of the octet lane half `lhi` fetches of row R:
__device__ __forceinline__ int frag_offset(int R, int lhi) {
  return R * 32 + ((lhi ^ ((R >> 3) & 1)) * 16);
}
// ... and the NS parts of it, `part_stride` bytes apart
template <int NS>
__device__ __forceinline__ void load_frag(const char* p0, int part_stride, bf16x8 (&out)[NS]) {
#pragma unroll
  for (int p = 0; p < NS; ++p) out[p] = *reinterpret_cast<const bf16x8*>(p0 + p * part_stride);
}

// One k-step of the split product on TM x TN 32 x 32 tiles: the part products, smallest terms
// first; the (i, j) accumulators interleave so that two MFMAs on the same accumulator are TM * TN
// issues apart.  `after_first` runs behind the first product group of a multi-part product (a
// loop that issues its DMA under the MFMAs).
struct NoOp { __device__ __forceinline__ void operator()() const {} };
template <int PA, int PB, int NS, int TM, int TN>
__device__ __forceinline__ void part_product(f32x16 (&acc)[TM][TN], const bf16x8 (&av)[TM][NS],
                                             const bf16x8 (&bv)[TN][NS]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i][PA], bv[j][PB], acc[i][j], 0, 0, 0);
}
template <int NS, int TM, int TN, class F = NoOp>
__device__ __forceinline__ void split_product(f32x16 (&acc)[TM][TN], const bf16x8 (&av)[TM][NS],
                                              const bf16x8 (&bv)[TN][NS], F&& after_first = F()) {
  static_assert(NS >= 1 && NS <= 3, "one, two or three bf16 parts");
  if constexpr (NS == 3) {
    part_product<2, 0>(acc, av, bv);
    after_first();
    part_product<0, 2>(acc, av, bv);
    part_product<1, 1>(acc, av, bv);
    part_product<1, 0>(acc, av, bv);
    part_product<0, 1>(acc, av, bv);
  } else if constexpr (NS == 2) {
    part_product<1, 0>(acc, av, bv);
    after_first();
    part_product<0, 1>(acc, av, bv);
  }
  part_product<0, 0>(acc, av, bv);
}
// The two-part ("bf16x3") k-step of a kernel whose A operand is ONE row tile held in registers as
// separate hi / lo fragments: fetch the slab's TN column-tile fragments (parts `part_stride` bytes
// apart), then split_product's groups lo hi, hi lo, hi hi on a [1][2] view of the operands.
template <int TN>
__device__ __forceinline__ void bf16x3_step(f32x16 (&acc)[TN], const bf16x8& a_hi, const bf16x8& a_lo,
                                            const char* slab, int part_stride, int l31, int lhi) {
  bf16x8 bv[TN][2];
#pragma unroll
  for (int j = 0; j < TN; ++j) load_frag<2>(slab + frag_offset(j * 32 + l31, lhi), part_stride, bv[j]);
  const bf16x8 av[1][2] = {{a_hi, a_lo}};
  split_product<2>(reinterpret_cast<f32x16(&)[1][TN]>(acc), av, bv);
}

// Row of a 32 x 32 accumulator tile that element r of an f32x16 holds in lane half lhi (the MFMA
// C layout: lane & 31 is the column)
__device__ __forceinline__ int mfma_row(int r, int lhi) { return (r & 3) + 8 * (r >> 2) + 4 * lhi; }

// The fused input prologue.  PRO is a COMPILE-TIME parameter: a run-time switch here is lowered to
// a branch tree per staged element and wrecks the schedule of the whole main loop.
template <int PRO>
__device__ __forceinline__ float apply_pro(float v, float mu, float sc, float beta, float s,
                                           float t) {
  if constexpr (PRO == SNAP_PRO_AFFINE) return v * s + t;
  if constexpr (PRO == SNAP_PRO_GN_RELU) return snap_relu((v - mu) * sc + beta);
  if constexpr (PRO == SNAP_PRO_RELU_GN) return (snap_relu(v) - mu) * sc + beta;
  if constexpr (PRO == SNAP_PRO_RELU) return snap_relu(v);
  return v;
}

#endif  // SNAP_CSRC_MMA_COMMON_H_
