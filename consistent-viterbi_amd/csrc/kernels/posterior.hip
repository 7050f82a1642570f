// posterior.hip -- MI355X (gfx950) sum-product kernels: sequence log-likelihood and posterior
// state marginals of the standard HMM (cv_posterior_batch, DESIGN.md "Posterior").
//   post_fwd_mm / post_bwd_mm     N <= 256: 32 sequences per workgroup in lock step, one step =
//                                 X (32 x NP) . A (NP x NP) on v_mfma_f64_16x16x4_f64 (mm_step,
//                                 the tiling of fit.hip's bw_fwd_mm -- layouts described there)
//   post_fwd_gen / post_bwd_gen   N <= 4096: one workgroup per sequence, the step's vectors in
//                                 LDS, A streamed from L2 (coalesced over the output states)
// f64, probability space.  Tables are zero padded to NP states (A, A^T, pi, and the emission
// column of each observation), so rows / columns >= N need no test: they multiply by 0.
//
// Scaling: every row is rescaled by 2^-e, e = the exponent of the row maximum -- an exact
// operation (v_ldexp_f64), so the only roundings are the products' and sums'.  The forward
// pass carries sum e as an integer and takes one log10 at the sequence's last element:
//   loglik = log10(sum_j alpha^_{T-1}[j]) + (sum e) log10(2).
// gamma_t = alpha^_t o beta^_t / sum(alpha^_t o beta^_t) needs no exponent at all.
// cv_posterior_emissions*: the emission rows are staged per call, each scaled by its own 2^-k
// (emis.hip); the sequence's sum k (g.kshift) joins sum e as an integer before that one log10.
// Every reduction runs in one fixed order (registers over the lane's tiles, DPP over the 16
// lanes of a row, then the 4 waves through LDS), so runs repeat bit for bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mm_core.h"
#include "post_bwd.h"
#include "posterior.h"

namespace cvp {

constexpr double kLog10Of2 = 0.30102999566398119521;

__device__ __forceinline__ double final_loglik(double sum, int e, int64_t esum) {
  return log10(ldexp(sum, -e)) + (double)esum * kLog10Of2;
}

__device__ __forceinline__ void write_result(const PostArgs& g, int64_t s, int T, bool bad, double ll) {
  uint8_t st = kSeqOk;
  if (T == 0) {
    st = kSeqEmpty;
    ll = 0.0;
  } else if (bad) {
    st = kSeqBadObs;
    ll = __builtin_nan("");
  } else if (!(ll > -__builtin_inf())) {
    st = kSeqInfeasible;
    ll = -__builtin_inf();
  }
  g.loglik[s] = ll;
  g.status[s] = st;
}

// ---- N <= 256: forward -------------------------------------------------------------------
// Wave w owns the output columns 16 (w CT + n) + (l & 15), n < CT, of all G = 32 sequences;
// acc[m][n][r] is sequence 16 m + (l >> 4) + 4 r (the f64 C/D layout).  Step t: y = (alpha^_{t-1}
// . A) o b(o_t) o mask_t, its row maximum and row sum in one reduction round, alpha^_t = y 2^-e
// to the workspace (STORE) and, transposed, to LDS as the next operand.  A finished sequence's
// operand row is 0 and its stores go to the dump slot: masked, not branched around.
template <int NP, int MT, int WV, bool STORE>
__global__ __launch_bounds__(64 * WV, 2) void post_fwd_mm(PostArgs g) {
  constexpr int CT = NP / (16 * WV), G = 16 * MT;
  __shared__ __attribute__((aligned(16))) double xt[NP * (G + 1)];
  __shared__ double redm[WV][G], reds[WV][G], s_ll[G];
  __shared__ int64_t s_seq[G], s_e0[G], s_r0[G], s_es[G];  // s_es: the sequence's exponent sum
  __shared__ int s_T[G], s_ob[4][G], s_fc[4][G], s_bad[G];
  __shared__ int s_tmax;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, cl = l & 15;
  double* const dump = g.dump + (size_t)((blockIdx.x * WV + w) & (kPostDumpWaves - 1)) * 64 + l;
  if (tid < G) {
    s_bad[tid] = 0;
    s_ll[tid] = 0.0;
    s_es[tid] = 0;
  }
  post_setup<G>(g, s_seq, s_e0, s_r0, s_T, &s_tmax);
  const int tmax = s_tmax;
  auto fetch = [&](int t) {  // observation and forced state of step t into slot t & 3
    if (tid < G) {
      const bool v = t < s_T[tid];
      int o = 0, fc = -1;
      if (v) {
        const int64_t e = s_e0[tid] + t;
        o = g.obs[e];
        if (g.forced) fc = g.forced[e];
        if (o < 0 || o >= g.nobs) {
          s_bad[tid] = 1;
          o = 0;
        }
      }
      s_ob[t & 3][tid] = o;
      s_fc[t & 3][tid] = fc;
    }
  };
  if (tmax > 0) {  // workgroup-uniform
    fetch(0);
    fetch(1);
    fetch(2);
    __syncthreads();
    int col[CT];
#pragma unroll
    for (int n = 0; n < CT; ++n) col[n] = 16 * (w * CT + n) + cl;
    f64x4_t acc[MT][CT];
    for (int t = 0;; ++t) {
      double em[MT][4][CT];
      auto load_em = [&] {  // b(o_t): L2 hits, in flight during the products
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double* er = g.et + (size_t)s_ob[t & 3][16 * m + (l >> 4) + 4 * r] * NP;
#pragma unroll
            for (int n = 0; n < CT; ++n) em[m][r][n] = er[col[n]];
          }
      };
      if (t > 0) {
        fetch(t + 2);  // slot (t + 2) & 3 held step t - 2, last read before step t - 1's barriers
        cvf::mm_step<NP, MT, WV>(xt, g.a, NP, w, l, acc, load_em);
      } else {
        load_em();
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < CT; ++n) {
            const double p = g.pi[col[n]];
            acc[m][n] = f64x4_t{p, p, p, p};
          }
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = 16 * m + (l >> 4) + 4 * r;
          const int fc = s_fc[t & 3][gi];
          double vm = 0.0, vs = 0.0;
#pragma unroll
          for (int n = 0; n < CT; ++n) {
            double y = acc[m][n][r] * em[m][r][n];
            y = (fc < 0 || fc == col[n]) ? y : 0.0;
            acc[m][n][r] = y;
            vm = fmax(vm, y);
            vs += y;
          }
          vm = cvf::row16_max(vm);
          vs = cvf::row16_sum(vs);
          if (cl == 0) {
            redm[w][gi] = vm;
            reds[w][gi] = vs;
          }
        }
      __syncthreads();
      const bool more = t + 1 < tmax;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = 16 * m + (l >> 4) + 4 * r;
          const double rmax = cvf::wmax<WV>(&redm[0][0], G, gi);
          const int e = row_exp(rmax);
          const int T = s_T[gi];
          const bool on = t < T, on1 = t + 1 < T;
          if (w == 0 && cl == 0 && on) {  // one lane per sequence keeps its exponent sum (LDS)
            const int64_t es = s_es[gi] + e;
            s_es[gi] = es;
            if (!on1)  // the sequence's last element: once per sequence
              s_ll[gi] = final_loglik(cvf::wsum<WV>(&reds[0][0], G, gi), e, es + (g.kshift ? g.kshift[s_seq[gi]] : 0));
          }
          double* arow = g.rows + (size_t)(s_r0[gi] + t) * NP;
#pragma unroll
          for (int n = 0; n < CT; ++n) {
            const double a = ldexp(acc[m][n][r], -e);
            if (STORE) *(on ? arow + col[n] : dump) = a;
            if (more) xt[cvf::xt_at<G>(col[n], gi)] = on1 ? a : 0.0;
          }
        }
      __syncthreads();  // xt complete; redm / reds free
      if (!more) break;
    }
  }
  __syncthreads();
  if (tid < G && s_seq[tid] >= 0) write_result(g, s_seq[tid], s_T[tid], s_bad[tid] != 0, s_ll[tid]);
}

// ---- N <= 256: backward, gamma and its argmax: bwd_mm_body (post_bwd.h) ---------------------
template <int NP, int MT, int WV, bool GAMMA>
__global__ __launch_bounds__(64 * WV, 2) void post_bwd_mm(PostArgs g) {
  bwd_mm_body<NP, MT, WV, GAMMA, false>(g);
}

// ---- N <= 4096: one workgroup per sequence (the layout: post_bwd.h) ----------------------------
__global__ __launch_bounds__(256) void post_fwd_gen(PostArgs g) {
  extern __shared__ double sm[];
  __shared__ double red[4];
  const int N = g.nstates, NP = g.np, tid = threadIdx.x;
  double* x = sm;
  double* y = sm + NP;
  const int64_t k = g.seq_begin + blockIdx.x;
  const int64_t s = g.order ? g.order[k] : k;
  const int64_t e0 = g.offsets[s];
  const int T = (int)(g.offsets[s + 1] - e0);
  bool bad = false;
  int64_t esum = 0;
  double ll = 0.0;
  for (int t = 0; t < T; ++t) {
    int o = g.obs[e0 + t];
    const int fc = g.forced ? g.forced[e0 + t] : -1;
    if (o < 0 || o >= g.nobs) {
      bad = true;
      o = 0;
    }
    const double* er = g.et + (size_t)o * NP;
    double vm = 0.0, vs = 0.0;
    for (int j = tid; j < NP; j += 256) {
      double v = (t == 0 ? g.pi[j] : dot_col(x, g.a, N, NP, j)) * er[j];
      v = (fc < 0 || fc == j) ? v : 0.0;
      y[j] = v;
      vm = fmax(vm, v);
      vs += v;
    }
    const double rmax = cvf::block_max(vm, red);  // its barriers: every read of x is done
    const double rsum = cvf::block_sum(vs, red);
    const int e = row_exp(rmax);
    if (t == T - 1) ll = final_loglik(rsum, e, esum + e + (g.kshift ? g.kshift[s] : 0));
    esum += e;
    double* arow = g.rows ? g.rows + (size_t)(e0 - g.elem_base + t) * NP : nullptr;
    for (int j = tid; j < NP; j += 256) {
      const double a = ldexp(y[j], -e);
      x[j] = a;
      if (arow) arow[j] = a;
    }
    __syncthreads();
  }
  if (tid == 0) write_result(g, s, T, bad, ll);
}

__global__ __launch_bounds__(256) void post_bwd_gen(PostArgs g) { bwd_gen_body<false>(g); }

// ---- launchers -----------------------------------------------------------------------------
template <int NP>
static void launch_fwd_mm(const PostArgs& g, unsigned grid, hipStream_t stream) {
  if (g.rows) hipLaunchKernelGGL((post_fwd_mm<NP, 2, 4, true>), dim3(grid), dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((post_fwd_mm<NP, 2, 4, false>), dim3(grid), dim3(256), 0, stream, g);
}
template <int NP>
static void launch_bwd_mm(const PostArgs& g, unsigned grid, hipStream_t stream) {
  if (g.gamma) hipLaunchKernelGGL((post_bwd_mm<NP, 2, 4, true>), dim3(grid), dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((post_bwd_mm<NP, 2, 4, false>), dim3(grid), dim3(256), 0, stream, g);
}

hipError_t launch_post_fwd(const PostArgs& g, bool generic, hipStream_t stream) {
  if (!post_args_ok(g)) return hipErrorInvalidValue;
  const int64_t n = g.seq_end - g.seq_begin;
  if (n == 0) return hipSuccess;
  if (generic || g.nstates > kPostMmStates) {
    const size_t lds = gen_lds(reinterpret_cast<const void*>(&post_fwd_gen), g.np);
    hipLaunchKernelGGL(post_fwd_gen, dim3((unsigned)n), dim3(256), lds, stream, g);
    return hipGetLastError();
  }
  const unsigned grid = (unsigned)((n + kPostGroup - 1) / kPostGroup);
  switch (g.np) {
    case 64: launch_fwd_mm<64>(g, grid, stream); break;
    case 128: launch_fwd_mm<128>(g, grid, stream); break;
    case 192: launch_fwd_mm<192>(g, grid, stream); break;
    default: launch_fwd_mm<256>(g, grid, stream); break;
  }
  return hipGetLastError();
}

hipError_t launch_post_bwd(const PostArgs& g, bool generic, hipStream_t stream) {
  if (g.urows) return launch_post_cnt_bwd(g, generic, stream);  // the counts arm: counts.hip
  if (!post_args_ok(g) || !g.rows) return hipErrorInvalidValue;
  const int64_t n = g.seq_end - g.seq_begin;
  if (n == 0) return hipSuccess;
  if (generic || g.nstates > kPostMmStates) {
    const size_t lds = gen_lds(reinterpret_cast<const void*>(&post_bwd_gen), g.np);
    hipLaunchKernelGGL(post_bwd_gen, dim3((unsigned)n), dim3(256), lds, stream, g);
    return hipGetLastError();
  }
  const unsigned grid = (unsigned)((n + kPostGroup - 1) / kPostGroup);
  switch (g.np) {
    case 64: launch_bwd_mm<64>(g, grid, stream); break;
    case 128: launch_bwd_mm<128>(g, grid, stream); break;
    case 192: launch_bwd_mm<192>(g, grid, stream); break;
    default: launch_bwd_mm<256>(g, grid, stream); break;
  }
  return hipGetLastError();
}

}  // namespace cvp
