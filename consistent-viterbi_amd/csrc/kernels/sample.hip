// sample.hip -- MI355X (gfx950) posterior path sampling (cv_sample_batch, DESIGN.md "Posterior
// sampling"): the backward half of forward filtering, backward sampling.  The forward rows are
// posterior.hip's (post_fwd_mm / post_fwd_gen, [element][NP] in the handle's workspace); this file
// walks them from the last element to the first, one categorical draw per step:
//   sample_wave<C, D>   N <= 256: one wave per (sequence, group of D draws); lane l owns the
//                       C = NP / 64 consecutive states [C l, C l + C)
//   sample_gen          N <= 4096: one workgroup per (sequence, draw); thread k owns the
//                       consecutive states [k CH, k CH + CH), CH = ceil(NP / 256)
//   sample_score        the reference's f64 log10 fold along every sampled path, front to back
// The weights of a step are w_i = alpha^_t[i] A[i][j] (j the state drawn for t + 1; alpha^ alone at
// the last element), f64 products of the zero padded probability-space tables.  The pick is the
// smallest i with w_i > 0 whose inclusive prefix sum exceeds u W, and the largest i with w_i > 0
// when rounding leaves none: a state of weight 0 is never picked.  The prefix sums run in one
// fixed order (the owner's states in sequence, a scan over the owners), so runs repeat bit for
// bit; u comes from sample_rng.h and depends on (seed, sequence, draw, position) only.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sample.h"
#include "sample_rng.h"

namespace cvs {

// per-sequence status values of include/cviterbi.h
constexpr uint8_t kSeqOk = 0, kSeqEmpty = 2, kSeqBadObs = 3;

// v of the DPP source lane; 0.0 where the control has no source lane or the row is masked off
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp0_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)u, CTRL, ROWS, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), CTRL, ROWS, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// inclusive scan over the 64 lanes in lane order: row_shr 1, 2, 4, 8 inside each row of 16, then
// lane 15 of rows 0 / 2 into rows 1 / 3 (row_bcast15) and lane 31 into rows 2 and 3 (row_bcast31)
__device__ __forceinline__ double wave_scan(double v) {
  v += dpp0_f64<0x111, 0xf>(v);
  v += dpp0_f64<0x112, 0xf>(v);
  v += dpp0_f64<0x114, 0xf>(v);
  v += dpp0_f64<0x118, 0xf>(v);
  v += dpp0_f64<0x142, 0xa>(v);
  v += dpp0_f64<0x143, 0xc>(v);
  return v;
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {  // lane: wave-uniform
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = __builtin_amdgcn_readlane((int)u, lane);
  const int hi = __builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

template <int C>
__device__ __forceinline__ void load_states(const double* __restrict__ p, double (&v)[C]) {
  if constexpr (C == 2) {
    const double2 x = *reinterpret_cast<const double2*>(p);
    v[0] = x.x, v[1] = x.y;
  } else if constexpr (C == 4) {
    const double2 x = *reinterpret_cast<const double2*>(p), y = *reinterpret_cast<const double2*>(p + 2);
    v[0] = x.x, v[1] = x.y, v[2] = y.x, v[3] = y.y;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = p[c];
  }
}

// ---- N <= 256: one wave per (sequence, D draws) ----------------------------------------------
// The rows alpha^_t do not depend on the picks: they come through a ring of PF rows issued ahead
// of the chain, once per wave for all of its draws.  The one dependent load of a step and draw is
// the row j of A^T (NP * 8 bytes, L2).  A step: the lane's C products and their running sums, the
// scan of the 64 lane sums, a ballot of (lane sum > 0 and prefix > u W), its first lane; that lane's
// states are resolved in every lane alike and read with one readlane.  The picks of 64 steps stay
// in a register (lane t & 63) and leave as one coalesced store.  The uniforms of 64 steps are
// computed by the 64 lanes at once and read with readlane.
template <int C, int D>
__global__ __launch_bounds__(256) void sample_wave(SampleArgs g) {
  constexpr int NP = 64 * C, PF = 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * 4 + w;
  if (slot >= g.seq_end - g.seq_begin) return;  // wave-uniform; the kernel has no barrier
  const int64_t k = g.seq_begin + slot;
  const int r0 = (int)blockIdx.y * D;
  const int64_t s = g.order ? g.order[k] : k;
  const int64_t e0 = g.offsets[s];
  const int T = (int)(g.offsets[s + 1] - e0);
  if (T <= 0) return;
  int32_t* const path = g.path + e0;
  if (g.status[s] != kSeqOk) {
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (r0 + d < g.draws)
        for (int t = l; t < T; t += 64) path[(size_t)(r0 + d) * g.plane + t] = -1;
    return;
  }
  const double* const rowp = g.rows + (size_t)(e0 - g.elem_base) * NP + C * l;
  const double* const atp = g.at + C * l;
  uint64_t key[D];
  int j[D], preg[D];
  double ureg[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    key[d] = draw_key(g.seed, (uint64_t)(g.seq_base + s), (uint64_t)(r0 + d));
    j[d] = 0;
    preg[d] = -1;
    ureg[d] = 0.0;
  }
  auto step = [&](int t, const double (&al)[C], bool first) {
    const int tl = t & 63;
    if (first || tl == 63) {  // wave-uniform: the uniforms of the positions (t & ~63) + lane
#pragma unroll
      for (int d = 0; d < D; ++d) ureg[d] = key_uniform(key[d], (uint64_t)((t & ~63) + l));
    }
    double av[D][C];
#pragma unroll
    for (int d = 0; d < D; ++d) load_states<C>(atp + (size_t)max(j[d], 0) * NP, av[d]);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      double wt[C], ps[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double pr = al[c] * av[d][c];
        wt[c] = first ? al[c] : pr;
        ps[c] = c ? ps[c - 1] + wt[c] : wt[c];
      }
      const double ls = ps[C - 1];
      const double cs = wave_scan(ls);
      const double thr = readlane_f64(ureg[d], tl) * readlane_f64(cs, 63);
      const bool pos = ls > 0.0;
      const uint64_t m = __ballot(pos && cs > thr), mp = __ballot(pos);
      // the first lane over the threshold; none (rounding): the last lane with a positive weight
      const int L = m ? __builtin_ctzll(m) : 63 - __builtin_clzll(mp | 1);
      const double ex = L > 0 ? readlane_f64(cs, max(L - 1, 0)) : 0.0;  // the sum below lane L's states
      int hit = -1, last = -1;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const bool q = wt[c] > 0.0;
        hit = (hit < 0 && q && ex + ps[c] > thr) ? c : hit;
        last = q ? c : last;
      }
      int i = C * L + __builtin_amdgcn_readlane(hit >= 0 ? hit : last, L);
      // no positive weight at all (tables below the accuracy contract's range): the draw ends
      // here and the rest of its path is -1
      i = (mp == 0 || (!first && j[d] < 0)) ? -1 : i;
      j[d] = i;
      preg[d] = l == tl ? i : preg[d];
    }
    if (tl == 0) {  // wave-uniform: the picks of the positions t .. t + 63
#pragma unroll
      for (int d = 0; d < D; ++d)
        if (r0 + d < g.draws && t + l < T) path[(size_t)(r0 + d) * g.plane + t + l] = preg[d];
    }
  };
  double ring[PF][C];
  int t = T - 1;
#pragma unroll
  for (int p = 0; p < PF; ++p) load_states<C>(rowp + (size_t)max(t - p, 0) * NP, ring[p]);
  bool first = true;
  while (t >= 0) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      if (t >= 0) {
        step(t, ring[p], first);
        first = false;
      }
      load_states<C>(rowp + (size_t)max(t - PF, 0) * NP, ring[p]);
      --t;
    }
  }
}

// ---- N <= 4096: one workgroup per (sequence, draw) ---------------------------------------------
// 256 threads over consecutive state ranges; the thread sums are scanned inside each wave
// (shuffles) and the 4 wave totals added in order through LDS.
__global__ __launch_bounds__(256) void sample_gen(SampleArgs g) {
  __shared__ double s_wt[4];
  __shared__ int s_first[4], s_last[4], s_pick;
  const int NP = g.np, tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int64_t k = g.seq_begin + blockIdx.x;
  const int r = blockIdx.y;
  const int64_t s = g.order ? g.order[k] : k;
  const int64_t e0 = g.offsets[s];
  const int T = (int)(g.offsets[s + 1] - e0);
  if (T <= 0) return;  // workgroup-uniform
  int32_t* const path = g.path + (size_t)r * g.plane + e0;
  if (g.status[s] != kSeqOk) {
    for (int t = tid; t < T; t += 256) path[t] = -1;
    return;
  }
  const int CH = (NP + 255) / 256;
  const int lo = min(tid * CH, NP), hi = min(lo + CH, NP);
  const uint64_t key = draw_key(g.seed, (uint64_t)(g.seq_base + s), (uint64_t)r);
  int j = 0;
  for (int t = T - 1; t >= 0; --t) {
    const bool first = t == T - 1;
    const double* __restrict__ arow = g.rows + (size_t)(e0 - g.elem_base + t) * NP;
    const double* __restrict__ atr = g.at + (size_t)max(j, 0) * NP;
    double ls = 0.0;
    for (int i = lo; i < hi; ++i) ls += first ? arow[i] : arow[i] * atr[i];
    double cs = ls;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double o = __shfl_up(cs, off);
      cs += l >= off ? o : 0.0;
    }
    double exl = __shfl_up(cs, 1);
    exl = l ? exl : 0.0;
    if (l == 63) s_wt[w] = cs;
    __syncthreads();
    const double t0 = s_wt[0], t1 = s_wt[1], t2 = s_wt[2], t3 = s_wt[3];
    const double base = w == 0 ? 0.0 : w == 1 ? t0 : w == 2 ? t0 + t1 : (t0 + t1) + t2;
    const double W = ((t0 + t1) + t2) + t3;
    const double thr = key_uniform(key, (uint64_t)t) * W;
    const bool pos = ls > 0.0;
    const uint64_t m = __ballot(pos && base + cs > thr), mp = __ballot(pos);
    if (l == 0) {
      s_first[w] = m ? 64 * w + __builtin_ctzll(m) : INT_MAX;
      s_last[w] = mp ? 64 * w + 63 - __builtin_clzll(mp) : -1;
    }
    __syncthreads();
    const int fi = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
    const int la = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
    const int owner = fi != INT_MAX ? fi : la;  // -1: no positive weight at all
    if (tid == (owner < 0 ? 0 : owner)) {
      int hit = -1, last = -1;
      const double ex = base + exl;
      double ps = 0.0;
      for (int i = lo; i < hi; ++i) {
        const double wt = first ? arow[i] : arow[i] * atr[i];
        ps += wt;
        const bool q = wt > 0.0;
        hit = (hit < 0 && q && ex + ps > thr) ? i : hit;
        last = q ? i : last;
      }
      const int i = hit >= 0 ? hit : last;
      s_pick = (owner < 0 || (!first && j < 0)) ? -1 : i;
    }
    __syncthreads();
    j = s_pick;
    if (tid == 0) path[t] = j;
  }
}

// ---- the scores: one lane per (sequence, draw), the fold of rescore_f64_lanes -------------------
__global__ __launch_bounds__(64) void sample_score(SampleScoreArgs g) {
  const int64_t slot = g.seq_begin + (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (slot >= g.seq_end) return;
  const int r = blockIdx.y;
  const int64_t seq = g.order ? (int64_t)g.order[slot] : slot;
  double* const out = g.score + (size_t)r * g.nseq + seq;
  const uint8_t st = g.status[seq];
  if (st == kSeqEmpty) return;
  if (st != kSeqOk) {
    *out = st == kSeqBadObs ? __builtin_nan("") : -__builtin_inf();
    return;
  }
  const int64_t e0 = g.offsets[seq];
  const int T = (int)(g.offsets[seq + 1] - e0);
  const int32_t* __restrict__ path = g.path + (size_t)r * g.plane + e0;
  const int32_t* __restrict__ obs = g.obs + e0;
  const int N = g.nstates;
  int pp = path[0];
  bool neg = pp < 0;
  pp = max(pp, 0);
  double d = g.pi64[pp] + g.et64[(size_t)obs[0] * N + pp];
  int t = 1;
  constexpr int U = 8;
  for (; t + U <= T; t += U) {
    int p[U], o[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      p[q] = path[t + q];
      o[q] = obs[t + q];
      neg |= p[q] < 0;
      p[q] = max(p[q], 0);
    }
    double av[U], bv[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      av[q] = g.a64[(size_t)(q ? p[q - 1] : pp) * N + p[q]];
      bv[q] = g.et64[(size_t)o[q] * N + p[q]];
    }
#pragma unroll
    for (int q = 0; q < U; ++q) d = (d + av[q]) + bv[q];
    pp = p[U - 1];
  }
  for (; t < T; ++t) {
    int p = path[t];
    neg |= p < 0;
    p = max(p, 0);
    d = (d + g.a64[(size_t)pp * N + p]) + g.et64[(size_t)obs[t] * N + p];
    pp = p;
  }
  *out = neg ? -__builtin_inf() : d;
}

// ---- launchers -----------------------------------------------------------------------------
template <int C>
static void launch_wave(const SampleArgs& g, unsigned blocks, hipStream_t stream) {
  const int R = g.draws;
  if (R == 1) hipLaunchKernelGGL((sample_wave<C, 1>), dim3(blocks, 1), dim3(256), 0, stream, g);
  else if (R == 2) hipLaunchKernelGGL((sample_wave<C, 2>), dim3(blocks, 1), dim3(256), 0, stream, g);
  else if (R <= 4) hipLaunchKernelGGL((sample_wave<C, 4>), dim3(blocks, 1), dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((sample_wave<C, 8>), dim3(blocks, (unsigned)((R + 7) / 8)), dim3(256), 0, stream, g);
}

hipError_t launch_sample(const SampleArgs& g, bool generic, hipStream_t stream) {
  if (g.nstates < 1 || g.nstates > 4096 || g.np != (g.nstates + 63) / 64 * 64 || g.draws < 1 ||
      g.draws > kSampleMaxDraws || g.seq_end < g.seq_begin || g.seq_end - g.seq_begin >= (int64_t)1 << 31 || !g.rows ||
      !g.path)
    return hipErrorInvalidValue;
  const int64_t n = g.seq_end - g.seq_begin;
  if (n == 0) return hipSuccess;
  if (generic || g.nstates > kSampleWaveStates) {
    hipLaunchKernelGGL(sample_gen, dim3((unsigned)n, (unsigned)g.draws), dim3(256), 0, stream, g);
    return hipGetLastError();
  }
  const unsigned blocks = (unsigned)((n + 3) / 4);
  switch (g.np) {
    case 64: launch_wave<1>(g, blocks, stream); break;
    case 128: launch_wave<2>(g, blocks, stream); break;
    case 192: launch_wave<3>(g, blocks, stream); break;
    default: launch_wave<4>(g, blocks, stream); break;
  }
  return hipGetLastError();
}

hipError_t launch_sample_score(const SampleScoreArgs& g, hipStream_t stream) {
  const int64_t n = g.seq_end - g.seq_begin;
  if (n < 0 || g.draws < 1 || g.draws > kSampleMaxDraws || !g.path || !g.score) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(sample_score, dim3((unsigned)((n + 63) / 64), (unsigned)g.draws), dim3(64), 0, stream, g);
  return hipGetLastError();
}

}  // namespace cvs
