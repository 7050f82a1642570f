// bcount.hip -- MI355X (gfx950) kernels of cv_expected_counts_model* (DESIGN.md "Emission counts"):
// the expected emission counts  b_cnt[j][v] = sum over the elements e of OK sequences with
// obs[e] = v of G[e][j],  G[e] = w_s gamma_e the rows the gradient arm of the backward pass stored
// (post_bwd.h).  A scatter by observation with one fixed order of every sum:
//   bcnt_keys      the key of every row of the chunk: its observation, or the discard key V for a
//                  row of a sequence that is not OK (or an observation outside [0, V))
//   (rocPRIM)      stable radix sort of (key, row) over the bits V needs; inclusive scan of the flags
//   bcnt_flags     a run starts where a part of part_rows sorted places starts or the key changes
//   bcnt_gather    one wave per (part, 128 columns): reads the rows of its part in sorted order, 16
//                  bytes per lane, adds them per column in registers and stores every run's sum
//                  whole to part[run]
//   bcnt_fold      acc[v] += the runs of v in ascending run order (the workgroup of v's first run)
//   bcnt_final     b_cnt[j][v] = acc[v][j] after the last chunk (32 x 32 tiles through LDS)
// No atomic adds, global or LDS: the sorted order is a function of the keys alone (the sort is
// stable), the runs of (keys, part_rows), so runs repeat bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "bcount.h"

namespace cvb {

constexpr uint8_t kSeqOk = 0;  // CV_SEQ_OK of include/cviterbi.h
constexpr int kGatherCols = 128;  // columns of a wave of bcnt_gather: 64 lanes x 2
constexpr int kGatherAhead = 8;   // rows in flight per wave
constexpr int kFoldAhead = 16;    // run sums in flight per thread of bcnt_fold

// one thread per row: the row's sequence by bisection of the chunk's offsets, then its key
__global__ __launch_bounds__(256) void bcnt_keys(BcntArgs b) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= b.nrows) return;
  const int64_t e = b.elem_base + r;
  int64_t lo = b.seq_begin, hi = b.seq_end;  // the last s in [lo, hi) with offsets[s] <= e
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (b.offsets[mid] <= e) lo = mid;
    else hi = mid;
  }
  const int32_t o = b.obs[e];
  const bool on = b.status[lo] == kSeqOk && o >= 0 && (int64_t)o < b.nobs;
  b.key_in[r] = on ? (uint32_t)o : (uint32_t)b.nobs;
  b.row_in[r] = (int32_t)r;
}

__global__ __launch_bounds__(256) void bcnt_flags(BcntArgs b) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= b.nrows) return;
  b.run[i] = (i % b.part_rows == 0 || b.key_out[i] != b.key_out[i - 1]) ? 1 : 0;
}

// VEC: g and ld keep every lane's two columns 16-byte aligned.  `runs` is the scanned flag array.
template <bool VEC>
__global__ __launch_bounds__(64) void bcnt_gather(BcntArgs b, const int32_t* __restrict__ runs) {
  const int lane = threadIdx.x, c0 = blockIdx.y * kGatherCols + 2 * lane;
  const int N = b.nstates, NP = b.np;
  const int64_t i0 = (int64_t)blockIdx.x * b.part_rows;
  const int64_t i1 = i0 + b.part_rows < b.nrows ? i0 + b.part_rows : b.nrows;
  const uint32_t discard = (uint32_t)b.nobs;
  const bool in0 = c0 < N, in1 = c0 + 1 < N;
  double a0 = 0.0, a1 = 0.0;
  int32_t cur = 0;  // the run being summed (1-based; 0: none yet)
  uint32_t curkey = discard;
  auto flush = [&] {
    if (cur == 0) return;  // wave-uniform
    if (c0 == 0) b.run_key[cur - 1] = curkey;
    if (curkey != discard && c0 < NP) {
      double* out = b.part + (size_t)(cur - 1) * NP + c0;
      out[0] = a0;
      out[1] = a1;
    }
  };
  for (int64_t i = i0; i < i1; i += kGatherAhead) {
    int32_t rr[kGatherAhead], rn[kGatherAhead];
    uint32_t kk[kGatherAhead];
    double v0[kGatherAhead], v1[kGatherAhead];
#pragma unroll
    for (int q = 0; q < kGatherAhead; ++q) {  // wave-uniform addresses
      const int64_t ii = i + q < i1 ? i + q : i1 - 1;
      rr[q] = b.row_out[ii];
      rn[q] = runs[ii];
      kk[q] = b.key_out[ii];
    }
#pragma unroll
    for (int q = 0; q < kGatherAhead; ++q) {
      v0[q] = 0.0;
      v1[q] = 0.0;
      if (kk[q] == discard || i + q >= i1) continue;  // wave-uniform
      const double* row = b.g + (size_t)rr[q] * (size_t)b.ld + c0;
      if constexpr (VEC) {
        if (in0) {  // c0 + 1 < ld: ld is even and c0 < N <= ld
          const double2 t = *reinterpret_cast<const double2*>(row);
          v0[q] = t.x;
          v1[q] = in1 ? t.y : 0.0;
        }
      } else {
        if (in0) v0[q] = row[0];
        if (in1) v1[q] = row[1];
      }
    }
#pragma unroll
    for (int q = 0; q < kGatherAhead; ++q) {
      if (i + q >= i1) break;  // wave-uniform
      if (rn[q] != cur) {
        flush();
        cur = rn[q];
        curkey = kk[q];
        a0 = 0.0;
        a1 = 0.0;
      }
      if (kk[q] != discard) {
        a0 += v0[q];
        a1 += v1[q];
      }
    }
  }
  flush();
}

// The workgroup of run r works only where r is the first run of its key in the chunk: acc[key] +=
// part[r], part[r + 1], ... while the key stays, one column per thread
__global__ __launch_bounds__(256) void bcnt_fold(BcntArgs b, const int32_t* __restrict__ runs) {
  const int64_t nruns = runs[b.nrows - 1], r = blockIdx.x;
  if (r >= nruns) return;
  const uint32_t k = b.run_key[r];
  if (k == (uint32_t)b.nobs || (r > 0 && b.run_key[r - 1] == k)) return;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= b.np) return;
  double* dst = b.acc + (size_t)k * b.np + c;
  double s = *dst;
  for (int64_t q = r;; q += kFoldAhead) {
    int m = 0;
    while (m < kFoldAhead && q + m < nruns && b.run_key[q + m] == k) ++m;
    double v[kFoldAhead];
#pragma unroll
    for (int u = 0; u < kFoldAhead; ++u) v[u] = u < m ? b.part[(size_t)(q + u) * b.np + c] : 0.0;
#pragma unroll
    for (int u = 0; u < kFoldAhead; ++u)
      if (u < m) s += v[u];
    if (m < kFoldAhead) break;
  }
  *dst = s;
}

__global__ __launch_bounds__(256) void bcnt_final(const double* __restrict__ acc, int64_t nobs, int nstates, int np,
                                                  double* __restrict__ b_cnt) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t v0 = (int64_t)blockIdx.x * 32;
  const int j0 = blockIdx.y * 32;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t v = v0 + ty + 8 * q;
    const int j = j0 + tx;
    tile[ty + 8 * q][tx] = (v < nobs && j < nstates) ? acc[(size_t)v * np + j] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = j0 + ty + 8 * q;
    const int64_t v = v0 + tx;
    if (v < nobs && j < nstates) b_cnt[(size_t)j * (size_t)nobs + v] = tile[tx][ty + 8 * q];
  }
}

static unsigned key_bits(int64_t nobs) {  // bits of the largest key, nobs itself
  unsigned bits = 1;
  while (bits < 32 && ((uint64_t)nobs >> bits) != 0) ++bits;
  return bits;
}

hipError_t bcnt_sort_tmp_bytes(int64_t rows, int64_t nobs, size_t* bytes) {
  if (rows < 0 || rows > INT32_MAX || nobs < 1 || nobs > INT32_MAX || !bytes) return hipErrorInvalidValue;
  size_t a = 0, s = 0;
  uint32_t* k = nullptr;
  int32_t* r = nullptr;
  hipError_t err = rocprim::radix_sort_pairs(nullptr, a, k, k, r, r, (unsigned int)rows, 0u, key_bits(nobs), hipStream_t(0));
  if (err != hipSuccess) return err;
  err = rocprim::inclusive_scan(nullptr, s, r, r, (size_t)rows, rocprim::plus<int32_t>(), hipStream_t(0));
  if (err != hipSuccess) return err;
  *bytes = a > s ? a : s;
  return hipSuccess;
}

hipError_t launch_bcnt_chunk(const BcntArgs& b, hipStream_t stream) {
  if (b.nrows == 0) return hipSuccess;
  if (b.nrows < 0 || b.nrows > INT32_MAX || b.nobs < 1 || b.nobs > INT32_MAX || b.part_rows < 1 || b.np < 64 ||
      b.np % 64 || b.nstates < 1 || b.nstates > b.np || b.ld < b.nstates || b.seq_end <= b.seq_begin)
    return hipErrorInvalidValue;
  if (!b.g || !b.key_in || !b.key_out || !b.row_in || !b.row_out || !b.run || !b.sort_tmp || !b.run_key || !b.part ||
      !b.acc || b.max_runs < bcnt_max_runs(b.nrows, b.part_rows, b.nobs))
    return hipErrorInvalidValue;
  const unsigned rb = (unsigned)((b.nrows + 255) / 256);
  hipLaunchKernelGGL(bcnt_keys, dim3(rb), dim3(256), 0, stream, b);
  size_t bytes = b.sort_tmp_bytes;
  hipError_t err = rocprim::radix_sort_pairs(b.sort_tmp, bytes, b.key_in, b.key_out, b.row_in, b.row_out,
                                             (unsigned int)b.nrows, 0u, key_bits(b.nobs), stream);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(bcnt_flags, dim3(rb), dim3(256), 0, stream, b);
  // the run numbers go to row_in, free since the sort
  int32_t* const runs = b.row_in;
  bytes = b.sort_tmp_bytes;
  err = rocprim::inclusive_scan(b.sort_tmp, bytes, b.run, runs, (size_t)b.nrows, rocprim::plus<int32_t>(), stream);
  if (err != hipSuccess) return err;
  const int64_t parts = (b.nrows + b.part_rows - 1) / b.part_rows;
  const dim3 gg((unsigned)parts, (unsigned)((b.np + kGatherCols - 1) / kGatherCols));
  const bool vec = b.ld % 2 == 0 && reinterpret_cast<uintptr_t>(b.g) % 16 == 0;
  if (vec) hipLaunchKernelGGL(bcnt_gather<true>, gg, dim3(64), 0, stream, b, (const int32_t*)runs);
  else hipLaunchKernelGGL(bcnt_gather<false>, gg, dim3(64), 0, stream, b, (const int32_t*)runs);
  const int64_t most = bcnt_max_runs(b.nrows, b.part_rows, b.nobs);
  hipLaunchKernelGGL(bcnt_fold, dim3((unsigned)most, (unsigned)((b.np + 255) / 256)), dim3(256), 0, stream, b,
                     (const int32_t*)runs);
  return hipGetLastError();
}

hipError_t launch_bcnt_final(const double* acc, int64_t nobs, int nstates, int np, double* b_cnt, hipStream_t stream) {
  if (!acc || !b_cnt || nobs < 1 || nstates < 1 || nstates > np) return hipErrorInvalidValue;
  const int64_t bx = (nobs + 31) / 32;
  if (bx >= (int64_t)1 << 31) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bcnt_final, dim3((unsigned)bx, (unsigned)((nstates + 31) / 32)), dim3(256), 0, stream, acc, nobs,
                     nstates, np, b_cnt);
  return hipGetLastError();
}

}  // namespace cvb
