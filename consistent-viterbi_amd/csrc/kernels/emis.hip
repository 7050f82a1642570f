// emis.hip -- emis_prepare_f64: one pass over a chunk of caller-supplied emission scores
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

}  // namespace

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
