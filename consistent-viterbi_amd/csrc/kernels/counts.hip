// counts.hip -- MI355X (gfx950) kernels of cv_expected_counts* (DESIGN.md "Expected counts"): the
// expected initial counts sum_s gamma_0 and transition counts sum_s sum_t xi_t(i, j) of the model
// cv_posterior_batch evaluates.
//   post_cnt_bwd_mm / post_cnt_bwd_gen   the backward pass of posterior.hip with its counts arm
//                                        (post_bwd.h): also stores u_{t+1}, 1 / rsum_t and gamma_0
//   post_xi_gemm, post_xi_fold           S += R^T U over a chunk's rows, in fixed parts
//   post_cnt_a, post_cnt_pi              a_cnt = A o S and pi_cnt after the last chunk
// No atomic adds anywhere: every sum has one order, so runs repeat bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mm_core.h"
#include "post_bwd.h"
#include "posterior.h"

namespace cvp {

template <int NP, int MT, int WV, bool GAMMA>
__global__ __launch_bounds__(64 * WV, 2) void post_cnt_bwd_mm(PostArgs g) {
  bwd_mm_body<NP, MT, WV, GAMMA, true>(g);
}
__global__ __launch_bounds__(256) void post_cnt_bwd_gen(PostArgs g) { bwd_gen_body<true>(g); }

// ---- expected transition counts: S = sum_e (alpha^[e] inv[e])^T U[e] ---------------------------
// xi_t(i, j) = alpha^_t[i] A[i][j] u_{t+1}[j] / rsum_t, so sum_t xi_t = A o (R^T U) with R = alpha^
// o inv: one GEMM over the chunk's rows (the tiling of fit.hip's bw_xi_gemm_lds: 128 x 128 output
// tiles per workgroup, four waves of 64 x 64, 16 rows of R and U at a time through double-
// buffered LDS).  A row whose inv is 0 -- a last element, a sequence that is not OK -- enters as
// zeros whatever its memory holds (the U row of a last element is never written).  Every
// workgroup owns one tile of one part, a fixed row range, and stores it whole to part[p]: the
// order of every sum is fixed by (rows, NP, part_rows) alone, so runs repeat bit for bit.
// XCD-aware block map as in bw_xi_gemm: the tiles of one part are dispatched together to one XCD.
constexpr int kXiKB = 16;  // rows per LDS stage
__global__ __launch_bounds__(256, 2) void post_xi_gemm(XiArgs x) {
  constexpr int TS = 128, KB = kXiKB, LS = TS + 2;  // LS: row stride (doubles) of a stage
  __shared__ __attribute__((aligned(16))) double rs[2][KB * LS], us[2][KB * LS];
  const int NP = x.np;
  const int ntt = (NP + TS - 1) / TS;
  const int64_t b = blockIdx.x, j = b / 8;
  const int tile = (int)(j % (ntt * ntt));
  const int64_t part = (j / (ntt * ntt)) * 8 + b % 8;
  if (part >= x.nparts) return;  // workgroup-uniform (padding blocks of the map)
  const int m0 = TS * (tile / ntt), n0 = TS * (tile % ntt);
  const int64_t r0 = part * x.part_rows;
  const int64_t r1 = r0 + x.part_rows < x.nrows ? r0 + x.part_rows : x.nrows;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, kk = l >> 4, cl = l & 15;
  const int wm = w >> 1, wn = w & 1;
  // staging: thread tid copies row (tid >> 4) of R and U, 8 doubles from column 8 (tid & 15);
  // NP is a multiple of 64, so the 8 columns are inside the rows together or not at all
  const int srow = tid >> 4, scol = 8 * (tid & 15);
  const bool vm = m0 + scol < NP, vn = n0 + scol < NP;
  const int cm = vm ? m0 + scol : 0, cn = vn ? n0 + scol : 0;
  double iv = 0.0;  // the staged row's inv
  auto stage_load = [&](int64_t rb, double (&ra)[8], double (&ua)[8]) {
    const int64_t row = rb + srow < r1 ? rb + srow : r0;
    const double* R = x.rows + (size_t)row * NP + cm;
    const double* U = x.urows + (size_t)row * NP + cn;
    iv = rb + srow < r1 ? x.inv[row] : 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      ra[q] = R[q];
      ua[q] = U[q];
    }
  };
  auto stage_store = [&](int buf, const double (&ra)[8], const double (&ua)[8]) {
    const bool onr = iv != 0.0 && vm, onu = iv != 0.0 && vn;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      rs[buf][srow * LS + scol + q] = onr ? ra[q] * iv : 0.0;
      us[buf][srow * LS + scol + q] = onu ? ua[q] : 0.0;
    }
  };
  f64x4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  double ra[8], ua[8];
  stage_load(r0, ra, ua);
  stage_store(0, ra, ua);
  __syncthreads();
  int buf = 0;
  for (int64_t rb = r0; rb < r1; rb += KB) {
    const bool next = rb + KB < r1;  // workgroup-uniform
    if (next) stage_load(rb + KB, ra, ua);  // in flight during this stage's products
#pragma unroll
    for (int ks = 0; ks < KB / 4; ++ks) {
      const int row = 4 * ks + kk;
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = rs[buf][row * LS + 64 * wm + 16 * a + cl];
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = us[buf][row * LS + 64 * wn + 16 * c + cl];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[c], acc[a][c], 0, 0, 0);
    }
    if (next) stage_store(buf ^ 1, ra, ua);
    __syncthreads();  // the next stage complete; this one free
    buf ^= 1;
  }
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  double* out = x.part + (size_t)part * NP * NP;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = m0 + 64 * wm + 16 * a + (l >> 4) + 4 * q, col = n0 + 64 * wn + 16 * c + (l & 15);
        if (row < NP && col < NP) out[(size_t)row * NP + col] = acc[a][c][q];
      }
}

// s += the parts in ascending order, one thread per entry
__global__ __launch_bounds__(256) void post_xi_fold(XiArgs x) {
  const size_t nn = (size_t)x.np * x.np, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nn) return;
  double s = x.s[idx];
  for (int64_t p = 0; p < x.nparts; ++p) s += x.part[(size_t)p * nn + idx];
  x.s[idx] = s;
}

// a_cnt = A o S, compact: one product per entry, so exactly 0 wherever A is 0
__global__ __launch_bounds__(256) void post_cnt_a(CountsFinalArgs c) {
  const int N = c.nstates;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)N * N) return;
  const size_t at = idx / N * c.np + idx % N;
  c.a_cnt[idx] = c.a[at] * c.s[at];
}

// pi_cnt[j] = sum of gamma_0[j] over the OK sequences: 16 states per workgroup (one 128-byte
// segment of each slot), thread row q adds the sequences q, q + 16, ... in order, then the 16
// rows pairwise in one fixed tree
__global__ __launch_bounds__(256) void post_cnt_pi(CountsFinalArgs c) {
  __shared__ double red[16][17];
  const int q = threadIdx.x >> 4, l = threadIdx.x & 15, j = blockIdx.x * 16 + l;  // j < NP
  double v = 0.0;
  for (int64_t s = q; s < c.nseq; s += 16)
    if (c.status[s] == kSeqOk) v += c.g0[(size_t)s * c.np + j];
  red[q][l] = v;
  __syncthreads();
#pragma unroll
  for (int h = 8; h >= 1; h >>= 1) {
    if (q < h) red[q][l] += red[q + h][l];
    __syncthreads();
  }
  if (q == 0 && j < c.nstates) c.pi_cnt[j] = red[0][l];
}

// ---- launchers -----------------------------------------------------------------------------
template <int NP>
static void launch_cnt_bwd_mm(const PostArgs& g, unsigned grid, hipStream_t stream) {
  if (g.gamma) hipLaunchKernelGGL((post_cnt_bwd_mm<NP, 2, 4, true>), dim3(grid), dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((post_cnt_bwd_mm<NP, 2, 4, false>), dim3(grid), dim3(256), 0, stream, g);
}

hipError_t launch_post_cnt_bwd(const PostArgs& g, bool generic, hipStream_t stream) {
  if (!post_args_ok(g) || !g.rows || !g.urows || !g.inv || !g.g0) return hipErrorInvalidValue;
  const int64_t n = g.seq_end - g.seq_begin;
  if (n == 0) return hipSuccess;
  if (generic || g.nstates > kPostMmStates) {
    const size_t lds = gen_lds(reinterpret_cast<const void*>(&post_cnt_bwd_gen), g.np);
    hipLaunchKernelGGL(post_cnt_bwd_gen, dim3((unsigned)n), dim3(256), lds, stream, g);
    return hipGetLastError();
  }
  const unsigned grid = (unsigned)((n + kPostGroup - 1) / kPostGroup);
  switch (g.np) {
    case 64: launch_cnt_bwd_mm<64>(g, grid, stream); break;
    case 128: launch_cnt_bwd_mm<128>(g, grid, stream); break;
    case 192: launch_cnt_bwd_mm<192>(g, grid, stream); break;
    default: launch_cnt_bwd_mm<256>(g, grid, stream); break;
  }
  return hipGetLastError();
}

hipError_t launch_post_xi(const XiArgs& x, hipStream_t stream) {
  if (x.np < 64 || x.np % 64 || x.nrows < 0 || x.part_rows < 1 || !x.part || !x.s) return hipErrorInvalidValue;
  if (x.nrows == 0) return hipSuccess;
  if (x.nparts != (x.nrows + x.part_rows - 1) / x.part_rows) return hipErrorInvalidValue;
  const int64_t ntt = (x.np + 127) / 128, blocks = (x.nparts + 7) / 8 * 8 * ntt * ntt;
  if (blocks >= (int64_t)1 << 31) return hipErrorInvalidValue;
  hipLaunchKernelGGL(post_xi_gemm, dim3((unsigned)blocks), dim3(256), 0, stream, x);
  hipLaunchKernelGGL(post_xi_fold, dim3((unsigned)(((size_t)x.np * x.np + 255) / 256)), dim3(256), 0, stream, x);
  return hipGetLastError();
}

hipError_t launch_post_counts_final(const CountsFinalArgs& c, hipStream_t stream) {
  if (c.nstates < 1 || c.np != post_padded_states(c.nstates) || c.nseq < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(post_cnt_a, dim3((unsigned)(((size_t)c.nstates * c.nstates + 255) / 256)), dim3(256), 0, stream, c);
  hipLaunchKernelGGL(post_cnt_pi, dim3((unsigned)(c.np / 16)), dim3(256), 0, stream, c);
  return hipGetLastError();
}

}  // namespace cvp

