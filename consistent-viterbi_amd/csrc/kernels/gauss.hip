// gauss.hip -- MI355X (gfx950) kernels of the diagonal-covariance Gaussian emissions (DESIGN.md
// "Gaussian emissions"): cv_gauss_emissions* and the moments of cv_expected_counts_gauss*.
//   gauss_emis   E[e][j] = c_j - kappa sum_d (x_ed - mean_jd)^2 w_jd: a state per lane, the lane's
//                mean and w of one block of dimensions in registers (the whole of them for D <= 32,
//                loaded once per workgroup; above that walked block by block), 16 rows of x at a
//                time broadcast through LDS, E stored coalesced along j.  Direct (x - mean)^2 on the
//                VALU: one rounding in the difference, one in the square, one explicit fma per
//                dimension in ascending d.  No reduction across lanes, so every entry has one order.
//   gm_rowok     the chunk's rows whose sequence is CV_SEQ_OK (bisection of the offsets)
//   gm_gemm      M_p = G^T Phi over the rows of part p, Phi = [1 | y | y^2] formed on the fly from x
//                and the center, on v_mfma_f64_16x16x4_f64 (the tiling of counts.hip's post_xi_gemm);
//                the rows of a sequence that is not OK enter G and Phi as zeros by a select
//   gm_fold      acc += the parts in ascending order
//   gm_final     g_cnt, m1, m2 from acc after the last chunk
// No atomic adds: every sum has one order fixed by (rows, NP, D, part_rows), so runs repeat bit
// for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss.h"
#include "mm_core.h"

namespace cvg {

using cvf::f64x4_t;

constexpr uint8_t kSeqOk = 0;  // CV_SEQ_OK of include/cviterbi.h
constexpr double kKappa = 0.21714724095162590;  // 0.5 / ln 10, correctly rounded
constexpr int kGaussRows = 16;  // rows of x per LDS stage of gauss_emis

// NaN or +-inf, on the bit pattern
__device__ __forceinline__ bool not_finite(double v) {
  return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

// Workgroup (x, y): the states blockDim.x * y + tid, the row tiles x, x + gridDim.x, ...  DB: the
// dimensions per register block; g.DP is a multiple of it and the tables are 0 in [D, DP), where
// the staged x is 0 too: fma(0, 0, q) = q exactly, so the padding never shows.
template <int DB>
__global__ __launch_bounds__(256) void gauss_emis(GaussArgs g) {
  constexpr int R = kGaussRows;
  __shared__ __attribute__((aligned(16))) double xs[R][DB];
  __shared__ int bad[R];
  const int tid = threadIdx.x, nt = blockDim.x, N = g.nstates;
  const int j = blockIdx.y * nt + tid;
  const bool on = j < N;
  const int jc = on ? j : N - 1;
  const double cj = g.c[jc];
  const int nblk = g.DP / DB;
  double mu[DB], w[DB];
  auto load_params = [&](int d0) {
#pragma unroll
    for (int k = 0; k < DB; ++k) {
      mu[k] = g.mu_t[(size_t)(d0 + k) * N + jc];
      w[k] = g.w_t[(size_t)(d0 + k) * N + jc];
    }
  };
  if (nblk == 1) load_params(0);
  const int64_t ntiles = (g.nrows + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * R;
    double q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) q[r] = 0.0;
    __syncthreads();  // the last tile's reads of bad are done
    if (tid < R) bad[tid] = 0;
    for (int b = 0; b < nblk; ++b) {
      __syncthreads();  // the last block's reads of xs are done; bad is reset
      for (int i = tid; i < R * DB; i += nt) {
        const int r = i / DB, k = i % DB, d = b * DB + k;
        double v = 0.0;
        if (r0 + r < g.nrows && d < g.D) {
          v = g.x[(size_t)(r0 + r) * (size_t)g.ldx + d];
          if (not_finite(v)) bad[r] = 1;
        }
        xs[r][k] = v;
      }
      if (nblk > 1) load_params(b * DB);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < DB; ++k) {
          const double d = xs[r][k] - mu[k];
          const double s = d * d;
          q[r] = __builtin_fma(s, w[k], q[r]);
        }
    }
    // bad is complete: every block's staging lies before the last barrier
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t e = r0 + r;
      if (on && e < g.nrows) {
        const double t = kKappa * q[r];
        g.out[(size_t)e * (size_t)g.ld + j] = bad[r] ? __builtin_nan("") : cj - t;
      }
    }
  }
}

hipError_t launch_gauss_emis(const GaussArgs& g, int cus, hipStream_t stream) {
  if (g.nrows == 0) return hipSuccess;
  if (!g.x || !g.c || !g.mu_t || !g.w_t || !g.out || g.nrows < 0 || g.D < 1 || g.D > kGaussMaxDims ||
      g.DP != gauss_padded_dims(g.D) || g.ldx < g.D || g.nstates < 1 || g.ld < g.nstates)
    return hipErrorInvalidValue;
  const int waves = g.nstates >= 256 ? 4 : (g.nstates + 63) / 64;
  const int nt = 64 * waves;
  const unsigned gy = (unsigned)((g.nstates + nt - 1) / nt);
  const int64_t tiles = (g.nrows + kGaussRows - 1) / kGaussRows;
  const int64_t want = (int64_t)(cus > 0 ? cus : 256) * 8;
  const unsigned gx = (unsigned)(tiles < want ? tiles : want);
  if (gy > 65535u) return hipErrorInvalidValue;
  const dim3 grid(gx, gy), block((unsigned)nt);
  if (g.DP == 8) hipLaunchKernelGGL(gauss_emis<8>, grid, block, 0, stream, g);
  else if (g.DP == 16) hipLaunchKernelGGL(gauss_emis<16>, grid, block, 0, stream, g);
  else hipLaunchKernelGGL(gauss_emis<32>, grid, block, 0, stream, g);
  return hipGetLastError();
}

// ---- moments ---------------------------------------------------------------------------------
// one thread per row: the row's sequence by bisection of the chunk's offsets, then its status
__global__ __launch_bounds__(256) void gm_rowok(GmArgs m) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= m.nrows) return;
  const int64_t e = m.elem_base + r;
  int64_t lo = m.seq_begin, hi = m.seq_end;  // the last s in [lo, hi) with offsets[s] <= e
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (m.offsets[mid] <= e) lo = mid;
    else hi = mid;
  }
  m.rowok[r] = m.status[lo] == kSeqOk ? 1 : 0;
}

// Workgroup b: part b / (tiles), output tile b % tiles of 128 states x 128 columns of Phi; four
// waves of 64 x 64, 16 rows of G and Phi at a time through double-buffered LDS.  Thread tid stages
// row (tid >> 4), 8 columns from 8 (tid & 15) of each operand.
constexpr int kGmKB = 16;
__global__ __launch_bounds__(256, 2) void gm_gemm(GmArgs m) {
  constexpr int TS = 128, KB = kGmKB, LS = TS + 2;
  __shared__ __attribute__((aligned(16))) double gs[2][KB * LS], ps[2][KB * LS];
  const int NP = m.np, WP = m.wp, N = m.nstates, D = m.D;
  const int ntm = (NP + TS - 1) / TS, ntn = (WP + TS - 1) / TS;
  const int64_t b = blockIdx.x;
  const int tile = (int)(b % (ntm * ntn));
  const int64_t part = b / (ntm * ntn);
  const int m0 = TS * (tile / ntn), n0 = TS * (tile % ntn);
  const int64_t r0 = part * m.part_rows;
  const int64_t r1 = r0 + m.part_rows < m.nrows ? r0 + m.part_rows : m.nrows;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, kk = l >> 4, cl = l & 15;
  const int wm = w >> 1, wn = w & 1;
  const int srow = tid >> 4, scol = 8 * (tid & 15);
  auto stage_load = [&](int64_t rb, double (&ga)[8], double (&pa)[8]) {
    const int64_t row = rb + srow;
    const bool ok = row < r1 && m.rowok[row < r1 ? row : r0] != 0;  // the select on the status
    const double* G = m.g + (size_t)(ok ? row : r0) * (size_t)m.ldg;
    const double* X = m.x + (size_t)(m.elem_base + (ok ? row : r0)) * (size_t)m.ldx;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int jj = m0 + scol + q, c = n0 + scol + q;
      ga[q] = (ok && jj < N) ? G[jj] : 0.0;
      double v = 0.0;
      if (ok && c <= 2 * D) {
        if (c == 0) {
          v = 1.0;
        } else {
          const int d = c <= D ? c - 1 : c - 1 - D;
          const double y = X[d] - m.center[d];
          v = c <= D ? y : y * y;
        }
      }
      pa[q] = v;
    }
  };
  auto stage_store = [&](int buf, const double (&ga)[8], const double (&pa)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      gs[buf][srow * LS + scol + q] = ga[q];
      ps[buf][srow * LS + scol + q] = pa[q];
    }
  };
  f64x4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  double ga[8], pa[8];
  stage_load(r0, ga, pa);
  stage_store(0, ga, pa);
  __syncthreads();
  int buf = 0;
  for (int64_t rb = r0; rb < r1; rb += KB) {
    const bool next = rb + KB < r1;  // workgroup-uniform
    if (next) stage_load(rb + KB, ga, pa);  // in flight during this stage's products
#pragma unroll
    for (int ks = 0; ks < KB / 4; ++ks) {
      const int row = 4 * ks + kk;
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = gs[buf][row * LS + 64 * wm + 16 * a + cl];
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = ps[buf][row * LS + 64 * wn + 16 * c + cl];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[c], acc[a][c], 0, 0, 0);
    }
    if (next) stage_store(buf ^ 1, ga, pa);
    __syncthreads();  // the next stage complete; this one free
    buf ^= 1;
  }
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  double* out = m.part + (size_t)part * NP * WP;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = m0 + 64 * wm + 16 * a + (l >> 4) + 4 * q, col = n0 + 64 * wn + 16 * c + (l & 15);
        if (row < NP && col < WP) out[(size_t)row * WP + col] = acc[a][c][q];
      }
}

// acc += the parts in ascending order, one thread per entry
__global__ __launch_bounds__(256) void gm_fold(GmArgs m) {
  const size_t nn = (size_t)m.np * m.wp, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nn) return;
  double s = m.acc[idx];
  for (int64_t p = 0; p < m.nparts; ++p) s += m.part[(size_t)p * nn + idx];
  m.acc[idx] = s;
}

__global__ __launch_bounds__(256) void gm_final(const double* __restrict__ acc, int nstates, int D, int wp,
                                                double* __restrict__ g_cnt, double* __restrict__ m1,
                                                double* __restrict__ m2) {
  const size_t W = 2 * (size_t)D + 1, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)nstates * W) return;
  const size_t j = idx / W, c = idx % W;
  const double v = acc[j * wp + c];
  if (c == 0) g_cnt[j] = v;
  else if (c <= (size_t)D) m1[j * D + (c - 1)] = v;
  else m2[j * D + (c - 1 - D)] = v;
}

hipError_t launch_gm_chunk(const GmArgs& m, hipStream_t stream) {
  if (m.nrows == 0) return hipSuccess;
  if (m.nrows < 0 || m.np < 64 || m.np % 64 || m.nstates < 1 || m.nstates > m.np || m.ldg < m.nstates || m.D < 1 ||
      m.D > kGaussMaxDims || m.wp != gm_padded_width(m.D) || m.ldx < m.D || m.part_rows < 1 || m.part_rows % 4 ||
      m.seq_end <= m.seq_begin)
    return hipErrorInvalidValue;
  if (!m.g || !m.x || !m.center || !m.offsets || !m.status || !m.rowok || !m.part || !m.acc ||
      m.nparts != (m.nrows + m.part_rows - 1) / m.part_rows)
    return hipErrorInvalidValue;
  const int64_t tiles = (int64_t)((m.np + 127) / 128) * ((m.wp + 127) / 128), blocks = m.nparts * tiles;
  if (blocks >= (int64_t)1 << 31) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gm_rowok, dim3((unsigned)((m.nrows + 255) / 256)), dim3(256), 0, stream, m);
  hipLaunchKernelGGL(gm_gemm, dim3((unsigned)blocks), dim3(256), 0, stream, m);
  hipLaunchKernelGGL(gm_fold, dim3((unsigned)(((size_t)m.np * m.wp + 255) / 256)), dim3(256), 0, stream, m);
  return hipGetLastError();
}

hipError_t launch_gm_final(const double* acc, int nstates, int D, int wp, double* g_cnt, double* m1, double* m2,
                           hipStream_t stream) {
  if (!acc || !g_cnt || !m1 || !m2 || nstates < 1 || D < 1 || wp != gm_padded_width(D)) return hipErrorInvalidValue;
  const size_t n = (size_t)nstates * (2 * (size_t)D + 1);
  hipLaunchKernelGGL(gm_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, acc, nstates, D, wp, g_cnt, m1, m2);
  return hipGetLastError();
}

}  // namespace cvg
