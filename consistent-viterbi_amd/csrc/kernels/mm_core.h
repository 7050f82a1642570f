// mm_core.h -- device helpers of the lock-step matrix-core kernels (fit.hip: bw_fwd_mm /
// bw_bwd_mm; posterior.hip: post_fwd_mm / post_bwd_mm): a workgroup of WV waves advances
// G = 16 MT sequences one step as the product X (G x NP) . M (NP x NP) on
// v_mfma_f64_16x16x4_f64.  The operand layouts are described at bw_fwd_mm (fit.hip).
#ifndef CV_KERNELS_MM_CORE_H
#define CV_KERNELS_MM_CORE_H

#include <hip/hip_runtime.h>

namespace cvf {

typedef double f64x4_t __attribute__((ext_vector_type(4)));

// a select of two computed values: without the empty asm the compiler turns a per-lane `?:`
// with arithmetic on one side into an exec-masked branch, and a branch here waits for every
// outstanding load (vmcnt(0))
__device__ __forceinline__ double sel(bool c, double a, double b) {
  asm("" : "+v"(a));
  asm("" : "+v"(b));
  return c ? a : b;
}

__device__ __forceinline__ double block_sum(double v, double* red) {
  // 256 threads = 4 waves: wave shuffle-reduce, then across the 4 waves through LDS
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // red[] may still be read by the previous call
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double block_max(double v, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)u, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double row16_sum(double v) {  // sum over the 16 lanes of a DPP row
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  return v;
}
__device__ __forceinline__ double row16_max(double v) {
  v = fmax(v, dpp_f64<0xB1>(v));
  v = fmax(v, dpp_f64<0x4E>(v));
  v = fmax(v, dpp_f64<0x141>(v));
  v = fmax(v, dpp_f64<0x140>(v));
  return v;
}

// X^T[k][g] with a row stride of G + 1 doubles: one ds_write_b64 (16 lanes: 16 consecutive k,
// one g) spreads over 16 bank pairs; an operand read (16 consecutive g at k and k + 1) is a
// 2-way conflict.  Additive, so every (tile, register) offset is a compile-time constant the
// LDS instructions carry (an XOR swizzle kept 16-32 per-lane addresses live and spilled).
template <int G>
__device__ __forceinline__ int xt_at(int k, int g) { return k * (G + 1) + g; }

// the WV waves' partials of sequence gi (red[w * G + gi]) added in one fixed (pairwise) order
template <int WV>
__device__ __forceinline__ double wsum(const double* red, int G, int gi) {
  if constexpr (WV == 4) return (red[gi] + red[G + gi]) + (red[2 * G + gi] + red[3 * G + gi]);
  else return wsum<WV / 2>(red, G, gi) + wsum<WV / 2>(red + (WV / 2) * G, G, gi);
}
template <int WV>
__device__ __forceinline__ double wmax(const double* red, int G, int gi) {
  double v = red[gi];
#pragma unroll
  for (int w = 1; w < WV; ++w) v = fmax(v, red[w * G + gi]);
  return v;
}

template <int NP, int MT, int WV, class Pre>
__device__ __forceinline__ void mm_step(const double* __restrict__ xt, const double* __restrict__ M, int N, int w,
                                        int l, f64x4_t (&acc)[MT][NP / (16 * WV)], Pre&& pre) {
#ifndef CVF_MM_PF
  constexpr int PF = 4;
#else
  constexpr int PF = CVF_MM_PF;
#endif
  constexpr int CT = NP / (16 * WV), NK = NP / 4, G = 16 * MT;
  const int cl = l & 15, kq = l >> 4;
  int col[CT];
#pragma unroll
  for (int n = 0; n < CT; ++n) col[n] = min(16 * (w * CT + n) + cl, N - 1);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < CT; ++n) acc[m][n] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  // A rows PF k-blocks ahead (L2), the LDS operand one k-block ahead
  // the products at a higher issue priority than the other workgroup's phase-E VALU work on
  // the SIMD (A/B: forward 77.8 vs 79.1 ms, backward 110.0 vs 110.8 ms at config-4 shape)
#ifndef CVF_MM_NOPRIO
  __builtin_amdgcn_s_setprio(2);
#endif
  double ring[PF][CT];
#define CVF_MM_LOAD(KK, DST)                                                  \
  {                                                                           \
    const int k_ = min(4 * (KK) + kq, N - 1);                                 \
    _Pragma("unroll") for (int n = 0; n < CT; ++n) DST[n] = M[(size_t)k_ * N + col[n]]; \
  }
#pragma unroll
  for (int p = 0; p < PF; ++p) CVF_MM_LOAD(p, ring[p])
  // loads the caller wants in flight during the products: issued after the ring's first
  // blocks, so the in-order wait for those does not wait for them
  pre();
  double av[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) av[m] = xt[xt_at<G>(kq, 16 * m + cl)];
#pragma unroll 1
  for (int kk0 = 0; kk0 < NK; kk0 += PF) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int kk = kk0 + p;
      double bv[CT], an[MT];
#pragma unroll
      for (int n = 0; n < CT; ++n) bv[n] = ring[p][n];
      CVF_MM_LOAD(min(kk + PF, NK - 1), ring[p])
      const int kn = 4 * min(kk + 1, NK - 1) + kq;
#pragma unroll
      for (int m = 0; m < MT; ++m) an[m] = xt[xt_at<G>(kn, 16 * m + cl)];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < CT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bv[n], acc[m][n], 0, 0, 0);
#pragma unroll
      for (int m = 0; m < MT; ++m) av[m] = an[m];
    }
  }
#ifndef CVF_MM_NOPRIO
  __builtin_amdgcn_s_setprio(0);
#endif
#undef CVF_MM_LOAD
}

}  // namespace cvf

#endif  // CV_KERNELS_MM_CORE_H
