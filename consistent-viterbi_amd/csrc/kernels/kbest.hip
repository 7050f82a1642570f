// kbest.hip -- K-best (list) Viterbi in exact f64: cv_kbest_batch* (include/cviterbi.h).
//
// The contract (row A0, VITERBI association): L_0(j) = [pi[j] + b[j, o_0]] if finite; for t >= 1
// the candidates of state j are x(i, r) = L_{t-1}(i)[r] + a[i, j], L_t(j) is the first K finite
// ones in the order value descending, ties by (i, r) ascending, and b[j, o_t] is added after the
// order is fixed.  fl(x + c) is monotone in x, so every list stays sorted and the K best lists of
// the predecessors determine the K best list of a state.
//
// kbest_fwd<KT, S>: the structure of generic_fwd_ms (trellis.hip) with a list where that kernel
// keeps one value: S sequences per workgroup, one state per thread, a[i][j] loaded once for all
// S.  Each thread holds its state's KT values and back-pointers in registers (compile-time
// indices only); the previous lists sit in LDS as [KT][N] (kb_double_buffered), so a read of
// x(i, r) is one address for the whole wave (a broadcast) and a thread's KT stores go to KT
// conflict-free rows.  Per predecessor the hot path is one add and
// one compare of x(i, 0) against the thread's K-th value; the wave enters the insertion code
// only if some lane passes, and rank r + 1 of the same i is tried only by lanes whose rank r
// went in (the lists are sorted: the rest cannot enter).  Strict > keeps the earlier of two
// equal candidates, which is the (i, r) tie rule.
#include "kbest.h"

#include <algorithm>

#include "trellis.h"

namespace cvkb {
namespace {

using cvk::CVK_SEQ_BADOBS;
using cvk::CVK_SEQ_EMPTY;
using cvk::CVK_SEQ_INFEASIBLE;
using cvk::CVK_SEQ_OK;

// x > v[KT - 1] holds: x goes in front of the first entry below it (behind its equals), the
// rest moves down one rank and the last entry drops out.
template <int KT>
__device__ __forceinline__ void kb_insert(double (&v)[KT], uint32_t (&bp)[KT], double x, uint32_t p) {
  // carried down from the top: each rank keeps the larger of its entry and the carried one (a
  // maximum and a minimum are exact); the back-pointers swap on strict > until x is placed and
  // at every rank below it, so equal entries keep their order
  bool sw = false;
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    sw = sw || x > v[q];
    const double hi = fmax(v[q], x), lo = fmin(v[q], x);
    const uint32_t bh = sw ? p : bp[q], bl = sw ? bp[q] : p;
    v[q] = hi;
    bp[q] = bh;
    x = lo;
    p = bl;
  }
}

template <int KT>
__device__ __forceinline__ void kb_store_bp(uint16_t* dst, const uint32_t (&bp)[KT]) {
  uint32_t w[KT / 2];
#pragma unroll
  for (int q = 0; q < KT / 2; ++q) w[q] = bp[2 * q] | (bp[2 * q + 1] << 16);
  if constexpr (KT == 2) {
    *reinterpret_cast<uint32_t*>(dst) = w[0];
  } else if constexpr (KT == 4) {
    *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int q = 0; q < KT / 8; ++q)
      reinterpret_cast<uint4*>(dst)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
}

// The previous lists in LDS: one row per sequence and two barriers per step (every read, then
// every write) up to KT = 8 -- half the LDS, so twice the workgroups per CU, measured 6-19% faster
// at KT = 4 and 8 (DESIGN.md, K-best) -- and two rows with one barrier at KT = 16, where the
// one-row kernel no longer holds its lists in 128 VGPRs.
constexpr bool kb_double_buffered(int kt) { return kt >= 16; }

constexpr int kCandBlock = 4;  // predecessors whose a[i][j] and x(i, 0) operands are loaded ahead

template <int KT, int S>
__global__ __launch_bounds__(1024) void kbest_fwd(KbestArgs g, int64_t nslots) {
  constexpr bool DB = kb_double_buffered(KT);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* lbuf = reinterpret_cast<double*>(smem_raw);  // [DB ? 2 : 1][S][KT][N]
  const int N = g.nstates;
  const int V = g.nobs;
  const int j = threadIdx.x;
  const bool mine = j < N;  // the last wave's spare lanes only meet the barriers
  const double ninf = -__builtin_inf();
  int64_t e0[S], seq[S];
  int T[S];
  int Tmax = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int64_t k = (int64_t)blockIdx.x * S + s;
    seq[s] = -1;
    T[s] = 0;
    e0[s] = 0;
    if (k < nslots) {
      const int64_t slot = g.seq_begin + k;
      seq[s] = g.order ? (int64_t)g.order[slot] : slot;
      e0[s] = g.offsets[seq[s]];
      T[s] = (int)(g.offsets[seq[s] + 1] - e0[s]);
    }
    Tmax = T[s] > Tmax ? T[s] : Tmax;
  }
  if (Tmax <= 0) return;
  auto row = [&](int buf, int s) -> double* { return lbuf + (size_t)((DB ? buf : 0) * S + s) * KT * N; };
  auto store_last = [&](int s, const double(&v)[KT]) {
    double* out = g.last + (((int64_t)blockIdx.x * S + s) * N + j) * KT;
#pragma unroll
    for (int r = 0; r < KT; ++r) out[r] = v[r];
  };
  int bad = 0;  // bit s: sequence s saw an observation outside [0, V)
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (T[s] <= 0) continue;
    const int o = g.obs[e0[s]];
    const bool ok = (unsigned)o < (unsigned)V;
    bad |= ok ? 0 : 1 << s;
    const int fs = g.forced ? g.forced[e0[s]] : -1;
    if (mine) {
      const double e = ok ? g.et[(size_t)o * N + j] : ninf;
      double v[KT];
      v[0] = g.pi[j] + e;
      if (fs >= 0 && j != fs) v[0] = ninf;
#pragma unroll
      for (int r = 1; r < KT; ++r) v[r] = ninf;
      double* r0 = row(0, s);
#pragma unroll
      for (int r = 0; r < KT; ++r) r0[r * N + j] = v[r];
      if (T[s] == 1) store_last(s, v);
    }
  }
  __syncthreads();
  for (int t = 1; t < Tmax; ++t) {
    int o[S], fs[S];
    bool act[S], ok[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      act[s] = t < T[s];
      o[s] = act[s] ? g.obs[e0[s] + t] : 0;
      ok[s] = (unsigned)o[s] < (unsigned)V;
      if (act[s] && !ok[s]) bad |= 1 << s;
      fs[s] = (act[s] && g.forced) ? g.forced[e0[s] + t] : -1;
    }
    const int pb = (t - 1) & 1, cb = t & 1;
    double v[S][KT];
    uint32_t bp[S][KT];
    if (mine) {
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int r = 0; r < KT; ++r) {
          v[s][r] = ninf;
          bp[s][r] = 0;
        }
      const double* col = g.a + j;
      for (int i0 = 0; i0 < N; i0 += kCandBlock) {
        double av[kCandBlock], p0[kCandBlock][S];
        int ii[kCandBlock];
#pragma unroll
        for (int u = 0; u < kCandBlock; ++u) {
          ii[u] = i0 + u < N ? i0 + u : N - 1;
          // past the last predecessor: a -inf arc, whose candidates never enter
          av[u] = i0 + u < N ? col[(size_t)ii[u] * N] : ninf;
#pragma unroll
          for (int s = 0; s < S; ++s) p0[u][s] = row(pb, s)[ii[u]];
        }
#pragma unroll
        for (int u = 0; u < kCandBlock; ++u) {
#pragma unroll
          for (int s = 0; s < S; ++s) {
            if (!act[s]) continue;
            double x = p0[u][s] + av[u];
            if (x > v[s][KT - 1]) {
              kb_insert<KT>(v[s], bp[s], x, (uint32_t)ii[u] << 4);
              const double* pr = row(pb, s) + ii[u];
#pragma unroll
              for (int r = 1; r < KT; ++r) {
                x = pr[r * N] + av[u];
                if (!(x > v[s][KT - 1])) break;
                kb_insert<KT>(v[s], bp[s], x, ((uint32_t)ii[u] << 4) | (uint32_t)r);
              }
            }
          }
        }
      }
    }
    if constexpr (!DB) __syncthreads();  // one list row per sequence: every read before any write
    if (mine) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (!act[s]) continue;
        // the order is fixed; now the emission (a -inf emission or a forced element that
        // admits another state empties the list)
        const double e = ok[s] ? g.et[(size_t)o[s] * N + j] : ninf;
        const bool shut = fs[s] >= 0 && j != fs[s];
        double* rc = row(cb, s);
#pragma unroll
        for (int r = 0; r < KT; ++r) {
          const double w = shut ? ninf : v[s][r] + e;
          v[s][r] = w;
          rc[r * N + j] = w;
        }
        kb_store_bp<KT>(g.bp + ((e0[s] + t - g.elem_base) * (int64_t)N + j) * KT, bp[s]);
        if (t == T[s] - 1) store_last(s, v[s]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (T[s] > 0 && ((bad >> s) & 1) && threadIdx.x == 0) g.status[seq[s]] = CVK_SEQ_BADOBS;
}

// kbest_select: one wave per sequence.  Every list is sorted (value descending, rank ascending
// among equals), so the next entry of the global order -- value descending, ties by the
// flattened index j * KT + r ascending -- is the head of some state's list: k rounds of a wave
// arg-max over the heads, the first index among equal maxima.
__global__ __launch_bounds__(64) void kbest_select(KbestArgs g) {
  __shared__ uint8_t head[kKbestMaxStates];  // entries already taken from each state's list
  const int lane = threadIdx.x;
  const int64_t slot = g.seq_begin + blockIdx.x;
  const int64_t seq = g.order ? (int64_t)g.order[slot] : slot;
  const int64_t e0 = g.offsets[seq];
  const int T = (int)(g.offsets[seq + 1] - e0);
  const int N = g.nstates, KT = g.kt, K = g.k;
  const double ninf = -__builtin_inf();
  double* score = g.score + seq * K;
  int32_t* end = g.end + seq * K;
  const uint8_t prior = g.status[seq];
  if (T <= 0 || prior == CVK_SEQ_BADOBS) {
    // the bit patterns of -inf and of a quiet NaN, stored as integers: this file is built
    // without NaN semantics (a bare v_max_f64 / v_min_f64 in kb_insert)
    const uint64_t bits = T <= 0 ? 0xfff0000000000000ull : 0x7ff8000000000000ull;
    for (int r = lane; r < K; r += 64) {
      reinterpret_cast<uint64_t*>(score)[r] = bits;
      end[r] = -1;
    }
    if (lane == 0) {
      g.count[seq] = 0;
      g.status[seq] = T <= 0 ? CVK_SEQ_EMPTY : CVK_SEQ_BADOBS;
    }
    return;
  }
  const double* last = g.last + (int64_t)blockIdx.x * N * KT;
  for (int j = lane; j < N; j += 64) head[j] = 0;
  __syncthreads();
  int cnt = 0;
  for (int r = 0; r < K; ++r) {
    double bv = ninf;
    int bi = 0x7fffffff;
    for (int j = lane; j < N; j += 64) {
      const int hd = head[j];
      if (hd < KT) {
        const double v = last[j * KT + hd];
        if (v > bv) {
          bv = v;
          bi = j * KT + hd;
        }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (!(bv > ninf)) break;  // the same in every lane
    if (lane == 0) {
      const int j = bi / KT, hd = bi - j * KT;
      score[r] = bv;
      end[r] = (j << 4) | hd;
      head[j] = (uint8_t)(hd + 1);
    }
    ++cnt;
    __syncthreads();
  }
  for (int r = cnt + lane; r < K; r += 64) {
    score[r] = ninf;
    end[r] = -1;
  }
  if (lane == 0) {
    g.count[seq] = cnt;
    g.status[seq] = cnt > 0 ? CVK_SEQ_OK : CVK_SEQ_INFEASIBLE;
  }
}

// kbest_walk: one thread per (sequence, rank) follows the back-pointers from the last element
// to the first into its plane of path; an unused rank gets -1.
__global__ __launch_bounds__(256) void kbest_walk(KbestArgs g) {
  const int K = g.k, KT = g.kt, N = g.nstates;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t slot = g.seq_begin + idx / K;
  if (slot >= g.seq_end) return;
  const int r = (int)(idx % K);
  const int64_t seq = g.order ? (int64_t)g.order[slot] : slot;
  const int64_t e0 = g.offsets[seq];
  const int T = (int)(g.offsets[seq + 1] - e0);
  int32_t* path = g.path + (int64_t)r * g.plane + e0;
  const int e = g.end[seq * K + r];
  if (e < 0) {
    for (int t = 0; t < T; ++t) path[t] = -1;
    return;
  }
  int j = e >> 4, q = e & 15;
  const uint16_t* bp = g.bp + (e0 - g.elem_base) * (int64_t)N * KT;
  for (int t = T - 1; t >= 0; --t) {
    path[t] = j;
    if (t > 0) {
      const uint32_t p = bp[((int64_t)t * N + j) * KT + q];
      j = (int)(p >> 4);
      q = (int)(p & 15);
    }
  }
}

template <int KT, int S>
hipError_t launch_fwd_ks(const KbestArgs& g, hipStream_t stream) {
  constexpr bool DB = kb_double_buffered(KT);
  const int64_t n = g.seq_end - g.seq_begin;
  const size_t lds = sizeof(double) * (DB ? 2 : 1) * S * KT * (size_t)g.nstates;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&kbest_fwd<KT, S>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const unsigned threads = (unsigned)((g.nstates + 63) / 64 * 64);
  hipLaunchKernelGGL((kbest_fwd<KT, S>), dim3((unsigned)((n + S - 1) / S)), dim3(threads), lds, stream, g, n);
  return hipGetLastError();
}

template <int KT>
hipError_t launch_fwd_k(const KbestArgs& g, int s, hipStream_t stream) {
  // kbest_seqs_per_wg: S = 4 at KT = 2 only, S = 2 up to KT = 8
  if constexpr (KT <= 2)
    if (s >= 4) return launch_fwd_ks<KT, 4>(g, stream);
  if constexpr (KT <= 8)
    if (s >= 2) return launch_fwd_ks<KT, 2>(g, stream);
  return launch_fwd_ks<KT, 1>(g, stream);
}

}  // namespace

// Sequences per workgroup of kbest_fwd: generic_fwd_ms's rule (4 while the launch keeps >= 2
// workgroups per CU of 256 CUs, else fewer) with the list width in it.  S * KT <= 16 keeps the
// lists (3 VGPRs per entry) within 48 VGPRs, so the kernel fits the 128 VGPRs a 1,024-thread
// workgroup leaves a wave without scratch; above KT = 2 at most 2 (at KT = 4 four sequences
// measured 17% slower than two: 128 VGPRs and twice the LDS per workgroup); and the list rows
// of S sequences must fit the LDS (S N KT <= 8,192).
int kbest_seqs_per_wg(int n, int kt, int64_t nseq) {
  int s = 4;
  while (s > 1 && (s * kt > 16 || (kt > 2 && s > 2) || (int64_t)s * n * kt > kKbestMaxCells ||
                   nseq < (int64_t)s * 512))
    s /= 2;
  return s;
}

hipError_t launch_kbest_fwd(const KbestArgs& g, int s, hipStream_t stream) {
  if (g.seq_end <= g.seq_begin) return hipSuccess;
  if (g.nstates < 1 || g.nstates > kKbestMaxStates || g.nstates * g.kt > kKbestMaxCells) return hipErrorInvalidValue;
  if ((int64_t)s * g.nstates * g.kt > kKbestMaxCells) return hipErrorInvalidValue;
  switch (g.kt) {
    case 2: return launch_fwd_k<2>(g, s, stream);
    case 4: return launch_fwd_k<4>(g, s, stream);
    case 8: return launch_fwd_k<8>(g, s, stream);
    case 16: return launch_fwd_k<16>(g, s, stream);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_kbest_select(const KbestArgs& g, hipStream_t stream) {
  const int64_t n = g.seq_end - g.seq_begin;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(kbest_select, dim3((unsigned)n), dim3(64), 0, stream, g);
  return hipGetLastError();
}

hipError_t launch_kbest_walk(const KbestArgs& g, hipStream_t stream) {
  const int64_t n = (g.seq_end - g.seq_begin) * g.k;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(kbest_walk, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g);
  return hipGetLastError();
}

}  // namespace cvkb
