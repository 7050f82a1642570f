// emis.hip -- the staging passes over caller-supplied emission scores: emis_prepare_f64 (below,
// log domain, cv_decode_emissions*) and emis_prepare_lin_f64 (further down, probability space,
// cv_posterior_emissions*).
// emis_prepare_f64: one pass over a chunk of caller-supplied emission scores
// E[e][j] = log10 p(observation e | state j) (cv_decode_emissions*).  It writes the rows in the
// table layout of the decode kernel that will read them -- stride P >= N, columns [N, P) = -inf,
// row r of the chunk at dst + r * P -- and the index array idx[r] = r, so the f64 forward and
// backtrack kernels decode the chunk through their usual (et, obs, nobs) triple, unchanged:
// they read row et + obs[e] * P with obs[e] = e - (first element of the chunk).
//
// Validation is on the 64-bit pattern (no floating compare, so it holds under any fast-math
// flag): NaN and +inf are bad -- staged as -inf, and the sequence that owns the row gets
// CVK_SEQ_BADOBS, which every backtrack preserves -- -0.0 becomes +0.0 (the tables of
// cv_hmm_create never hold a -0.0 either), every other pattern is copied bit for bit.
//
// Bandwidth-bound: a group of 2^lsh lanes owns a row (a whole wave from P = 128 on, so ragged
// sequence lengths never matter: the loop is over rows), 16-byte loads where the row base is
// 16-byte aligned (8-byte loads of the same lines otherwise: `ld` odd or a shifted base) and
// 16-byte stores whenever P is even.
#include "emis.h"

#include <algorithm>

#include "exp10_scaled.h"
#include "trellis.h"

namespace cvem {
namespace {

using u64 = unsigned long long;
struct alignas(16) u64x2 {
  u64 x, y;
};
constexpr u64 kNegInf = 0xfff0000000000000ull, kPosInf = 0x7ff0000000000000ull, kNegZero = 0x8000000000000000ull;

__device__ __forceinline__ u64 clean(u64 u, bool& bad) {
  const bool b = (u << 1) > (kPosInf << 1) || u == kPosInf;  // NaN (either sign) or +inf
  bad |= b;
  return b ? kNegInf : u == kNegZero ? 0ull : u;
}

// VEC: P is even, a lane moves two columns at a time
template <bool VEC>
__global__ __launch_bounds__(256) void emis_prepare_f64(EmisPrepArgs g, int lsh) {
  const int lpr = 1 << lsh;  // lanes per row
  const int sub = (int)threadIdx.x & (lpr - 1);
  const int64_t rows_per_block = 256 >> lsh;
  const int64_t rstep = (int64_t)gridDim.x * rows_per_block;
  const int N = g.nstates, P = g.stride;
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + ((int)threadIdx.x >> lsh); r < g.nrows; r += rstep) {
    const u64* __restrict__ s = reinterpret_cast<const u64*>(g.src + (g.e0 + r) * g.ld);
    u64* __restrict__ d = reinterpret_cast<u64*>(g.dst + r * P);
    if (sub == 0) g.idx[r] = (int32_t)r;
    bool bad = false;
    if constexpr (VEC) {
      const bool aligned = (reinterpret_cast<uintptr_t>(s) & 15) == 0;
      for (int j = 2 * sub; j < P; j += 2 * lpr) {
        u64x2 v{kNegInf, kNegInf};
        if (j + 1 < N) {
          if (aligned) {
            v = *reinterpret_cast<const u64x2*>(s + j);
          } else {
            v.x = s[j];
            v.y = s[j + 1];
          }
          v.x = clean(v.x, bad);
          v.y = clean(v.y, bad);
        } else if (j < N) {
          v.x = clean(s[j], bad);
        }
        *reinterpret_cast<u64x2*>(d + j) = v;
      }
    } else {
      for (int j = sub; j < P; j += lpr) d[j] = j < N ? clean(s[j], bad) : kNegInf;
    }
    if (bad) {
      // the last sequence of the chunk that starts at or before this element (the empty
      // sequences before it start there too and end there)
      const int64_t e = g.e0 + r;
      int64_t lo = g.seq_begin, hi = g.seq_end;
      while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (g.offsets[mid] <= e)
          lo = mid;
        else
          hi = mid;
      }
      g.status[lo] = cvk::CVK_SEQ_BADOBS;
    }
  }
}

// ---- emis_prepare_lin_f64: the probability-space staging of cv_posterior_emissions* ----------
// Row r of the chunk -> dst + r * NP: 10^x 2^-k_r (exp10_scaled.h) with k_r chosen so that the
// row's largest entry lands in [1, 2), zeros in the columns [N, NP) (the posterior kernels'
// masking), idx[r] = r, and k_r added to kshift[sequence of the row] (integer atomics: the sum
// does not depend on the order or on how the rows are grouped).  A row with a NaN, a +inf or a finite |x| >= 2^40 is
// staged as zeros with idx[r] = -1: the posterior kernels' range check reports BADOBS.
//
// Two passes over the row, both through the same loads (the second hits L2 / TCP): the first
// validates on the bit pattern and reduces the row maximum as an order-preserving integer key
// (a bad entry is the largest key, so one reduction carries both), the second evaluates and
// stores.  The lane group of a row is 32 lanes at NP = 64 and the wave from NP = 128 on; the
// reduction is DPP inside a row of 16 lanes and ds_bpermute (no LDS memory) across the rows.
typedef u64 u64v2 __attribute__((ext_vector_type(2)));
constexpr u64 kAbsMask = 0x7fffffffffffffffull;
constexpr u64 kTwo40 = 0x4270000000000000ull;  // 2^40
constexpr long long kBadKey = 0x7fffffffffffffffll;

// the order-preserving key of a score (-0.0 as +0.0); kBadKey for what the contract rejects
__device__ __forceinline__ long long lin_key(u64 u) {
  if (u != kNegInf && (u & kAbsMask) >= kTwo40) return kBadKey;
  if (u == kNegZero) u = 0;
  const long long i = (long long)u;
  return i ^ ((i >> 63) & (long long)kAbsMask);
}
__device__ __forceinline__ double lin_unkey(long long k) {
  return __builtin_bit_cast(double, (u64)(k ^ ((k >> 63) & (long long)kAbsMask)));
}

template <int CTRL>
__device__ __forceinline__ long long max_dpp_i64(long long v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(u64)v, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)((u64)v >> 32), CTRL, 0xf, 0xf, false);
  const long long o = (long long)(((u64)(unsigned)hi << 32) | (unsigned)lo);
  return o > v ? o : v;
}

// the two scores at columns j, j + 1 (the second only when j + 1 < N) -- the caller has j < N.
// ALIGNED is a template parameter, not a select inside one loop (merged into one loop body the
// compiler lowers both cases to the pair of 8-byte loads that is valid for either).
template <bool ALIGNED>
__device__ __forceinline__ u64x2 lin_load(const u64* __restrict__ s, int j, int N) {
  u64x2 v{kNegInf, kNegInf};
  if (j + 1 < N) {
    if constexpr (ALIGNED) {  // one vector load (a struct copy is split into its members)
      const u64v2 t = *reinterpret_cast<const u64v2*>(s + j);
      v.x = t.x;
      v.y = t.y;
    } else {
      v.x = s[j];
      v.y = s[j + 1];
    }
  } else {
    v.x = s[j];
  }
  return v;
}

// the largest key of the lane's columns
template <bool ALIGNED>
__device__ __forceinline__ long long lin_scan(const u64* __restrict__ s, int N, int sub, int lpr) {
  long long key = lin_key(kNegInf);
  for (int j = 2 * sub; j < N; j += 2 * lpr) {
    const u64x2 v = lin_load<ALIGNED>(s, j, N);
    const long long kx = lin_key(v.x), ky = lin_key(v.y);
    key = kx > key ? kx : key;
    key = ky > key ? ky : key;
  }
  return key;
}

// the lane's columns of the staged row; bad: zeros
template <bool ALIGNED>
__device__ __forceinline__ void lin_store(const u64* __restrict__ s, u64* __restrict__ d, int N, int P, int sub, int lpr,
                                          bool bad, int64_t k) {
  for (int j = 2 * sub; j < P; j += 2 * lpr) {
    double ox = 0.0, oy = 0.0;
    if (j < N && !bad) {
      const u64x2 v = lin_load<ALIGNED>(s, j, N);
      ox = cvx::exp10_scaled(__builtin_bit_cast(double, v.x), k);
      oy = cvx::exp10_scaled(__builtin_bit_cast(double, v.y), k);  // -inf beyond N: 0
    }
    *reinterpret_cast<u64x2*>(d + j) = u64x2{__builtin_bit_cast(u64, ox), __builtin_bit_cast(u64, oy)};
  }
}

__global__ __launch_bounds__(256) void emis_prepare_lin_f64(EmisLinArgs g, int lsh) {
  const int lpr = 1 << lsh;  // lanes per row: 32 or 64
  const int sub = (int)threadIdx.x & (lpr - 1);
  const int64_t rows_per_block = 256 >> lsh;
  const int N = g.nstates, P = g.stride;
  // a lane group owns consecutive rows, so it crosses few sequence boundaries: it looks its
  // sequence up (12 dependent loads at 4,096 sequences, one lane, the others waiting) and adds
  // to kshift once per sequence it touches, not once per row
  const int64_t groups = (int64_t)gridDim.x * rows_per_block;
  const int64_t per = (g.nrows + groups - 1) / groups;
  const int64_t r0 = ((int64_t)blockIdx.x * rows_per_block + ((int)threadIdx.x >> lsh)) * per;
  const int64_t r1 = r0 + per < g.nrows ? r0 + per : g.nrows;
  int64_t seq = -1, seq_end = 0, kacc = 0;  // lane sub == 0: the current sequence, its end, its sum of k
  for (int64_t r = r0; r < r1; ++r) {
    const u64* __restrict__ s = reinterpret_cast<const u64*>(g.src + (g.e0 + r) * g.ld);
    u64* __restrict__ d = reinterpret_cast<u64*>(g.dst + r * P);
    const bool aligned = (reinterpret_cast<uintptr_t>(s) & 15) == 0;
    long long key = aligned ? lin_scan<true>(s, N, sub, lpr) : lin_scan<false>(s, N, sub, lpr);
    key = max_dpp_i64<0xB1>(key);   // quad_perm [1,0,3,2]
    key = max_dpp_i64<0x4E>(key);   // quad_perm [2,3,0,1]
    key = max_dpp_i64<0x141>(key);  // row_half_mirror
    key = max_dpp_i64<0x140>(key);  // row_mirror
    {
      const long long o = __shfl_xor(key, 16);
      key = o > key ? o : key;
    }
    if (lsh == 6) {
      const long long o = __shfl_xor(key, 32);
      key = o > key ? o : key;
    }
    const bool bad = key == kBadKey;
    const int64_t k = bad ? 0 : cvx::exp10_row_shift(cvx::exp10_parts(lin_unkey(key)));
    if (aligned)
      lin_store<true>(s, d, N, P, sub, lpr, bad, k);
    else
      lin_store<false>(s, d, N, P, sub, lpr, bad, k);
    if (sub == 0) {
      g.idx[r] = bad ? -1 : (int32_t)r;
      const int64_t e = g.e0 + r;
      if (seq < 0 || e >= seq_end) {
        if (kacc != 0) atomicAdd(reinterpret_cast<u64*>(g.kshift + seq), (u64)kacc);
        kacc = 0;
        // the last sequence of the chunk that starts at or before this element (as above)
        int64_t lo = g.seq_begin, hi = g.seq_end;
        while (hi - lo > 1) {
          const int64_t mid = lo + (hi - lo) / 2;
          if (g.offsets[mid] <= e)
            lo = mid;
          else
            hi = mid;
        }
        seq = lo;
        seq_end = g.offsets[lo + 1];
      }
      kacc += k;
    }
  }
  if (sub == 0 && kacc != 0) atomicAdd(reinterpret_cast<u64*>(g.kshift + seq), (u64)kacc);
}

}  // namespace

hipError_t launch_emis_prepare_lin(const EmisLinArgs& g, int cus, hipStream_t stream) {
  if (g.nrows <= 0) return hipSuccess;
  if (g.nstates < 1 || g.stride < g.nstates || (g.stride & 63) != 0 || g.ld < g.nstates || g.nrows > INT32_MAX ||
      g.seq_end <= g.seq_begin || (reinterpret_cast<uintptr_t>(g.dst) & 15) != 0 || !g.kshift || !g.idx)
    return hipErrorInvalidValue;
  const int lsh = g.stride == 64 ? 5 : 6;
  const int64_t rows_per_block = 256 >> lsh;
  const int64_t need = (g.nrows + rows_per_block - 1) / rows_per_block;
  const unsigned grid = (unsigned)std::min<int64_t>(need, (int64_t)std::max(cus, 1) * 16);
  hipLaunchKernelGGL(emis_prepare_lin_f64, dim3(grid), dim3(256), 0, stream, g, lsh);
  return hipGetLastError();
}

hipError_t launch_emis_prepare(const EmisPrepArgs& g, int cus, hipStream_t stream) {
  if (g.nrows <= 0) return hipSuccess;
  if (g.nstates < 1 || g.stride < g.nstates || g.ld < g.nstates || g.nrows > INT32_MAX ||
      g.seq_end <= g.seq_begin)
    return hipErrorInvalidValue;
  const bool vec = (g.stride & 1) == 0 && (reinterpret_cast<uintptr_t>(g.dst) & 15) == 0;
  const int items = vec ? g.stride / 2 : g.stride;
  int lsh = 0;
  while (lsh < 6 && (1 << lsh) < items) ++lsh;
  const int64_t rows_per_block = 256 >> lsh;
  const int64_t need = (g.nrows + rows_per_block - 1) / rows_per_block;
  const unsigned grid = (unsigned)std::min<int64_t>(need, (int64_t)std::max(cus, 1) * 16);
  if (vec)
    hipLaunchKernelGGL(emis_prepare_f64<true>, dim3(grid), dim3(256), 0, stream, g, lsh);
  else
    hipLaunchKernelGGL(emis_prepare_f64<false>, dim3(grid), dim3(256), 0, stream, g, lsh);
  return hipGetLastError();
}

}  // namespace cvem
