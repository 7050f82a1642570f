// post_bwd.h -- the backward pass of the sum-product kernels, shared by posterior.hip (post_bwd_mm,
// post_bwd_gen: path and gamma), counts.hip (post_cnt_bwd_mm, post_cnt_bwd_gen: the same pass
// with the counts arm of cv_expected_counts*) and grad.hip (post_grad_bwd_mm, post_grad_bwd_gen:
// the counts arm under per-sequence weights, cv_loglik_grad_emissions*).  One body each, inlined
// into its kernels; the layouts are described in posterior.hip.
#ifndef CV_KERNELS_POST_BWD_H
#define CV_KERNELS_POST_BWD_H

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "mm_core.h"
#include "posterior.h"

namespace cvp {

using cvf::f64x4_t;

// per-sequence status values of include/cviterbi.h
constexpr uint8_t kSeqOk = 0, kSeqInfeasible = 1, kSeqEmpty = 2, kSeqBadObs = 3;

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ int row16_min_i32(int v) {  // minimum over the 16 lanes of a DPP row
  v = min(v, dpp_i32<0xB1>(v));
  v = min(v, dpp_i32<0x4E>(v));
  v = min(v, dpp_i32<0x141>(v));
  v = min(v, dpp_i32<0x140>(v));
  return v;
}

// exponent of a row maximum (0 for an all-zero row: nothing to rescale)
__device__ __forceinline__ int row_exp(double m) { return m > 0.0 ? ilogb(m) : 0; }

// the group's sequences: id (-1: none), element offset, row base in g.rows, length; the longest
template <int G>
__device__ __forceinline__ void post_setup(const PostArgs& g, int64_t* s_seq, int64_t* s_e0, int64_t* s_r0, int* s_T,
                                           int* s_tmax) {
  const int tid = threadIdx.x;
  if (tid < G) {
    const int64_t k = g.seq_begin + (int64_t)blockIdx.x * G + tid;
    int64_t s = -1, e0 = g.elem_base;
    int T = 0;
    if (k < g.seq_end) {
      s = g.order ? g.order[k] : k;
      e0 = g.offsets[s];
      T = (int)(g.offsets[s + 1] - e0);
    }
    s_seq[tid] = s;
    s_e0[tid] = e0;
    s_r0[tid] = T > 0 ? e0 - g.elem_base : 0;
    s_T[tid] = T;
  }
  __syncthreads();
  if (tid == 0) {
    int tm = 0;
    for (int k = 0; k < G; ++k) tm = max(tm, s_T[k]);
    *s_tmax = tm;
  }
  __syncthreads();
}

// ---- N <= 256: backward, gamma and its argmax --------------------------------------------
// The group's sequences are aligned at their last elements: step r is t = T_g - 1 - r.  The
// operand in LDS is u_{t+1} = b(o_{t+1}) o mask_{t+1} o beta^_{t+1}; W_t = u_{t+1} . A^T, beta^_t =
// W_t 2^-e, p = alpha^_t o W_t (alpha^_t's loads in flight during the products).  One reduction
// round per step: max W (the rescaling), sum p (gamma's normaliser) and the first index of
// max p (the path; the waves own ascending column ranges, so the lowest wave wins a tie).
// COUNTS (cv_expected_counts*, the kernel post_cnt_bwd_mm): the operand u_{t+1} also goes to row
// t of g.urows as it is written to LDS, 1 / rsum_t to g.inv, and gamma_0 to the sequence's slot
// of g.g0.  One body, inlined into both kernels.
// GRAD (cv_loglik_grad_emissions*, the kernel post_grad_bwd_mm; with COUNTS): inv, gamma_0 and the
// gamma rows carry the sequence's weight w_s as one more product after the division, behind the
// same selects (a sequence that is not OK stores zeros whatever its weight holds), and the rows go
// to g.egrad at the caller's stride g.ld_grad in place of g.gamma.
template <int G>
__device__ __forceinline__ double* grad_weights() {  // LDS of the kernels with the GRAD arm only
  __shared__ double s_w[G];
  return s_w;
}
template <int NP, int MT, int WV, bool GAMMA, bool COUNTS, bool GRAD = false>
__device__ __forceinline__ void bwd_mm_body(const PostArgs g) {
  static_assert(COUNTS || !GRAD, "the gradient arm extends the counts arm");
  constexpr int CT = NP / (16 * WV), G = 16 * MT;
  __shared__ __attribute__((aligned(16))) double xt[NP * (G + 1)];
  __shared__ double redm[WV][G], reds[WV][G], redv[WV][G];
  __shared__ int redi[WV][G];
  __shared__ int64_t s_seq[G], s_e0[G], s_r0[G];
  __shared__ int s_T[G], s_ob[4][G], s_fc[4][G], s_ok[G];
  __shared__ int s_tmax;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, cl = l & 15;
  const int N = g.nstates;
  double* const dump = g.dump + (size_t)((blockIdx.x * WV + w) & (kPostDumpWaves - 1)) * 64 + l;
  post_setup<G>(g, s_seq, s_e0, s_r0, s_T, &s_tmax);
  if (tid < G) s_ok[tid] = s_seq[tid] >= 0 && g.status[s_seq[tid]] == kSeqOk;
  double* s_w = nullptr;
  if constexpr (GRAD) {
    s_w = grad_weights<G>();
    if (tid < G) s_w[tid] = (g.weight && s_seq[tid] >= 0) ? g.weight[s_seq[tid]] : 1.0;
  }
  const int tmax = s_tmax;
  if (tmax <= 0) return;  // workgroup-uniform
  auto fetch = [&](int r) {  // observation and forced state of step r (element T - 1 - r)
    if (tid < G) {
      const int t = s_T[tid] - 1 - r;
      int o = 0, fc = -1;
      if (t >= 0) {
        const int64_t e = s_e0[tid] + t;
        o = g.obs[e];
        if (g.forced) fc = g.forced[e];
        o = (o < 0 || o >= g.nobs) ? 0 : o;  // a BADOBS sequence: its status masks it below
      }
      s_ob[r & 3][tid] = o;
      s_fc[r & 3][tid] = fc;
    }
  };
  fetch(0);
  fetch(1);
  fetch(2);
  __syncthreads();
  int col[CT];
#pragma unroll
  for (int n = 0; n < CT; ++n) col[n] = 16 * (w * CT + n) + cl;
  f64x4_t acc[MT][CT];
  for (int r = 0;; ++r) {
    double al[MT][4][CT];
    auto load_alpha = [&] {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int gi = 16 * m + (l >> 4) + 4 * q;
          const double* arow = g.rows + (size_t)(s_r0[gi] + max(s_T[gi] - 1 - r, 0)) * NP;
#pragma unroll
          for (int n = 0; n < CT; ++n) al[m][q][n] = arow[col[n]];
        }
    };
    if (r > 0) {
      fetch(r + 2);
      cvf::mm_step<NP, MT, WV>(xt, g.at, NP, w, l, acc, load_alpha);
    } else {
      load_alpha();
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < CT; ++n) acc[m][n] = f64x4_t{1.0, 1.0, 1.0, 1.0};  // beta_{T-1} = 1
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int gi = 16 * m + (l >> 4) + 4 * q;
        const bool live = r < s_T[gi] && s_ok[gi] != 0;
        double vm = 0.0, vs = 0.0, bv = -1.0;
        int bi = INT_MAX;
#pragma unroll
        for (int n = 0; n < CT; ++n) {
          const double W = acc[m][n][q];
          const double p = live ? al[m][q][n] * W : 0.0;
          al[m][q][n] = p;
          vm = fmax(vm, W);
          vs += p;
          const bool up = p > bv;  // ascending columns: the first maximum stays
          bv = up ? p : bv;
          bi = up ? col[n] : bi;
        }
        vm = cvf::row16_max(vm);
        vs = cvf::row16_sum(vs);
        const double rv = cvf::row16_max(bv);
        const int ri = row16_min_i32(bv == rv ? bi : INT_MAX);
        if (cl == 0) {
          redm[w][gi] = vm;
          reds[w][gi] = vs;
          redv[w][gi] = rv;
          redi[w][gi] = ri;
        }
      }
    __syncthreads();
    const bool more = r + 1 < tmax;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int gi = 16 * m + (l >> 4) + 4 * q;
        const int t = s_T[gi] - 1 - r;
        const bool on = t >= 0, on1 = t >= 1;
        const int e = row_exp(cvf::wmax<WV>(&redm[0][0], G, gi));
        const double rsum = cvf::wsum<WV>(&reds[0][0], G, gi);
        const int64_t el = s_e0[gi] + max(t, 0);
        if (g.path && w == 0 && cl == 0 && on) {
          double best = redv[0][gi];
          int bi = redi[0][gi];
#pragma unroll
          for (int k = 1; k < WV; ++k) {
            const bool up = redv[k][gi] > best;
            best = up ? redv[k][gi] : best;
            bi = up ? redi[k][gi] : bi;
          }
          g.path[el] = rsum > 0.0 ? bi : -1;
        }
        if constexpr (GRAD) {
          const double ws = s_w[gi];
          if (GAMMA) {  // the gradient row of E, straight into the caller's array
            double* grow = g.egrad + (size_t)el * (size_t)g.ld_grad;
#pragma unroll
            for (int n = 0; n < CT; ++n) {
              const double gm = rsum > 0.0 ? (al[m][q][n] / rsum) * ws : 0.0;
              *((on && col[n] < N) ? grow + col[n] : dump) = gm;
            }
          }
          if (w == 0 && cl == 0 && on) g.inv[s_r0[gi] + t] = (r > 0 && rsum > 0.0) ? (1.0 / rsum) * ws : 0.0;
          double* zrow = g.g0 + (size_t)max(s_seq[gi], (int64_t)0) * NP;
#pragma unroll
          for (int n = 0; n < CT; ++n) {
            const double gm = rsum > 0.0 ? (al[m][q][n] / rsum) * ws : 0.0;
            *(t == 0 ? zrow + col[n] : dump) = gm;
          }
        } else if (GAMMA) {
          double* grow = g.gamma + (size_t)el * N;
#pragma unroll
          for (int n = 0; n < CT; ++n) {
            const double gm = rsum > 0.0 ? al[m][q][n] / rsum : 0.0;
            *((on && col[n] < N) ? grow + col[n] : dump) = gm;
          }
        }
        if constexpr (COUNTS && !GRAD) {
          // rsum_t = 0 in a sequence that is not OK (live) and where the tags leave no path
          if (w == 0 && cl == 0 && on) g.inv[s_r0[gi] + t] = (r > 0 && rsum > 0.0) ? 1.0 / rsum : 0.0;
          double* zrow = g.g0 + (size_t)max(s_seq[gi], (int64_t)0) * NP;
#pragma unroll
          for (int n = 0; n < CT; ++n) {
            const double gm = rsum > 0.0 ? al[m][q][n] / rsum : 0.0;
            *(t == 0 ? zrow + col[n] : dump) = gm;
          }
        }
        if (more) {  // the next operand u_t = b(o_t) o mask_t o beta^_t
          const double* er = g.et + (size_t)s_ob[r & 3][gi] * NP;
          const int fc = s_fc[r & 3][gi];
#pragma unroll
          for (int n = 0; n < CT; ++n) {
            const double u = ldexp(acc[m][n][q], -e) * er[col[n]];
            xt[cvf::xt_at<G>(col[n], gi)] = (on1 && (fc < 0 || fc == col[n])) ? u : 0.0;
            if constexpr (COUNTS)  // the same operand: row t - 1 of g.urows is u_t
              *(on1 ? g.urows + (size_t)(s_r0[gi] + t - 1) * NP + col[n] : dump) = (fc < 0 || fc == col[n]) ? u : 0.0;
          }
        }
      }
    __syncthreads();  // xt complete; the reduction slots free
    if (!more) break;
  }
}

// ---- N <= 4096: one workgroup per sequence ---------------------------------------------------
// (post_fwd_gen, posterior.hip, and the backward body below)  256 threads, thread j owns the states j, j + 256, ...; x (the step's operand) and y (its
// result) in LDS, A read row by row: consecutive threads read consecutive addresses.  The sums
// run over i = 0 .. N - 1 in order; block reductions as in fit.hip (one fixed tree).
__device__ __forceinline__ void block_argmax(double& v, int& i, double* redv, int* redi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    const bool up = ov > v || (ov == v && oi < i);
    v = up ? ov : v;
    i = up ? oi : i;
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    redv[w] = v;
    redi[w] = i;
  }
  __syncthreads();
  v = redv[0];
  i = redi[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const bool up = redv[k] > v || (redv[k] == v && redi[k] < i);
    v = up ? redv[k] : v;
    i = up ? redi[k] : i;
  }
}

__device__ __forceinline__ double dot_col(const double* __restrict__ x, const double* __restrict__ M, int N, int NP,
                                          int j) {
  double s = 0.0;
  for (int i = 0; i < N; ++i) s += x[i] * M[(size_t)i * NP + j];
  return s;
}

// The backward pass of the plain kernels (post_bwd_gen; COUNTS: post_cnt_bwd_gen, GRAD:
// post_grad_bwd_gen, both as in bwd_mm_body)
template <bool COUNTS, bool GRAD = false>
__device__ __forceinline__ void bwd_gen_body(const PostArgs g) {
  static_assert(COUNTS || !GRAD, "the gradient arm extends the counts arm");
  extern __shared__ double sm[];
  __shared__ double red[4];
  __shared__ int redi[4];
  const int N = g.nstates, NP = g.np, tid = threadIdx.x;
  double* x = sm;
  double* y = sm + NP;
  const int64_t k = g.seq_begin + blockIdx.x;
  const int64_t s = g.order ? g.order[k] : k;
  const int64_t e0 = g.offsets[s];
  const int T = (int)(g.offsets[s + 1] - e0);
  const bool ok = g.status[s] == kSeqOk;
  double ws = 1.0;
  if constexpr (GRAD) ws = g.weight ? g.weight[s] : 1.0;
  for (int t = T - 1; t >= 0; --t) {
    const double* arow = g.rows + (size_t)(e0 - g.elem_base + t) * NP;
    double vm = 0.0, vs = 0.0, bv = -1.0;
    int bi = INT_MAX;
    for (int j = tid; j < NP; j += 256) {
      const double W = t == T - 1 ? 1.0 : dot_col(x, g.at, N, NP, j);
      const double p = ok ? arow[j] * W : 0.0;
      y[j] = W;
      vm = fmax(vm, W);
      vs += p;
      if (p > bv) {
        bv = p;
        bi = j;
      }
    }
    const double rmax = cvf::block_max(vm, red);
    const double rsum = cvf::block_sum(vs, red);
    block_argmax(bv, bi, red, redi);
    const int e = row_exp(rmax);
    if (g.path && tid == 0) g.path[e0 + t] = rsum > 0.0 ? bi : -1;
    if constexpr (GRAD) {
      if (tid == 0) g.inv[e0 - g.elem_base + t] = (t < T - 1 && rsum > 0.0) ? (1.0 / rsum) * ws : 0.0;
    } else if constexpr (COUNTS) {
      if (tid == 0) g.inv[e0 - g.elem_base + t] = (t < T - 1 && rsum > 0.0) ? 1.0 / rsum : 0.0;
    }
    int o = g.obs[e0 + t];
    o = (o < 0 || o >= g.nobs) ? 0 : o;
    const int fc = g.forced ? g.forced[e0 + t] : -1;
    const double* er = g.et + (size_t)o * NP;
    __syncthreads();  // block_argmax's slots read by every thread
    for (int j = tid; j < NP; j += 256) {
      const double W = y[j];
      if constexpr (GRAD) {  // the gradient row of E, straight into the caller's array
        if (g.egrad && j < N)
          g.egrad[(size_t)(e0 + t) * (size_t)g.ld_grad + j] = rsum > 0.0 ? ((ok ? arow[j] * W : 0.0) / rsum) * ws : 0.0;
      } else {
        if (g.gamma && j < N) g.gamma[(size_t)(e0 + t) * N + j] = rsum > 0.0 ? (ok ? arow[j] * W : 0.0) / rsum : 0.0;
      }
      const double u = ldexp(W, -e) * er[j];
      x[j] = (fc < 0 || fc == j) ? u : 0.0;
      if constexpr (GRAD) {
        if (t > 0) g.urows[(size_t)(e0 - g.elem_base + t - 1) * NP + j] = x[j];
        else g.g0[(size_t)s * NP + j] = rsum > 0.0 ? ((ok ? arow[j] * W : 0.0) / rsum) * ws : 0.0;
      } else if constexpr (COUNTS) {
        if (t > 0) g.urows[(size_t)(e0 - g.elem_base + t - 1) * NP + j] = x[j];
        else g.g0[(size_t)s * NP + j] = rsum > 0.0 ? (ok ? arow[j] * W : 0.0) / rsum : 0.0;
      }
    }
    __syncthreads();
  }
}

static inline bool post_args_ok(const PostArgs& g) {
  return g.nstates >= 1 && g.nstates <= kPostMaxStates && g.np == post_padded_states(g.nstates) &&
         g.seq_end >= g.seq_begin && g.seq_end - g.seq_begin < (int64_t)1 << 31;
}

// dynamic LDS of the plain kernels: two vectors of NP
static inline size_t gen_lds(const void* kernel, int np) {
  const size_t lds = (size_t)2 * np * sizeof(double);
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return lds;
}

}  // namespace cvp

#endif  // CV_KERNELS_POST_BWD_H
