// gauss.h -- argument blocks and launchers of the Gaussian-emission kernels (gauss.hip) behind
// cv_gauss_emissions* and cv_expected_counts_gauss*.  Internal to libcviterbi; the public boundary
// is include/cviterbi.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvg {

constexpr int kGaussMaxDims = 1024;  // D above this: CV_ELIMIT
constexpr int kGaussDBlock = 32;     // dimensions per register block of gauss_emis (the tables are padded to it)

// dimensions of the per-call tables: D up to 8 / 16 rounds up to that block, else to a multiple of 32
inline int gauss_padded_dims(int D) { return D <= 8 ? 8 : D <= 16 ? 16 : (D + kGaussDBlock - 1) / kGaussDBlock * kGaussDBlock; }
// doubles of the per-call tables: c [N], then mean^T and w^T as [DP][N] (a dimension's states are
// contiguous, so a wave's loads coalesce), then center [DP]
inline size_t gauss_table_doubles(int N, int D) {
  const size_t dp = (size_t)gauss_padded_dims(D);
  return (size_t)N + 2 * dp * (size_t)N + dp;
}

// E[e][j] = c_j - kappa sum_d (x_ed - mean_jd)^2 w_jd, rows [0, nrows)
struct GaussArgs {
  const double* x;  // row r at x + r * ldx, D values
  int64_t ldx, nrows;
  int D, DP;        // DP = gauss_padded_dims(D); table entries of d in [D, DP) are 0
  int nstates;
  const double* c;     // [N]
  const double* mu_t;  // [DP][N]
  const double* w_t;   // [DP][N]
  double* out;         // row r at out + r * ld, N values; columns [N, ld) are never written
  int64_t ld;
};
hipError_t launch_gauss_emis(const GaussArgs& g, int cus, hipStream_t stream);

// ---- the moments of cv_expected_counts_gauss*: M += G^T Phi over a chunk's rows ----------------
constexpr uint64_t kGmPartCap = (uint64_t)256 << 20;  // most bytes of partial tiles
constexpr int kGmMaxParts = 256;                      // most parts by rule (gm_part_rows = 0)
constexpr int kGmMinRows = 1024;                      // fewest rows of a part by rule

// columns of Phi = [1 | y | y^2], padded to a multiple of 16
inline int gm_padded_width(int D) { return (2 * D + 1 + 15) / 16 * 16; }
// rows per part of a chunk of `rows` rows: a function of rows, NP, the width, the tuning key
// gm_part_rows and part_cap (the bytes the call's workspace cap leaves the partial tiles) alone
inline int64_t gm_part_rows(int64_t rows, int np, int wp, int64_t key, uint64_t part_cap) {
  const uint64_t tile = (uint64_t)np * wp * 8;
  const int64_t maxp = (int64_t)((part_cap < kGmPartCap ? part_cap : kGmPartCap) / tile);
  const int64_t fit = maxp > 1 ? maxp : 1, rule = fit < kGmMaxParts ? fit : kGmMaxParts;
  int64_t per = key > 0 ? key : (rows + rule - 1) / rule;
  if (key <= 0 && per < kGmMinRows) per = kGmMinRows;
  if (per < (rows + fit - 1) / fit) per = (rows + fit - 1) / fit;
  return (per + 3) / 4 * 4;
}

struct GmArgs {
  // the chunk: sequences [seq_begin, seq_end) = elements [elem_base, elem_base + nrows)
  const int64_t* offsets;
  const uint8_t* status;  // [nseq]
  int64_t seq_begin, seq_end, elem_base, nrows;
  const double* g;        // row r of the chunk at g + r * ldg, N values: w_s gamma
  int64_t ldg;
  const double* x;        // element e at x + e * ldx, D values
  int64_t ldx;
  const double* center;   // [D]
  int D, wp;              // wp = gm_padded_width(D)
  int nstates, np;
  int32_t* rowok;         // [nrows] scratch: 1 where the row's sequence is CV_SEQ_OK
  int64_t part_rows, nparts;
  double* part;           // [nparts][NP][wp] partial sums, every entry written
  double* acc;            // [NP][wp] the call's accumulator: acc += sum_p part[p], p ascending
};
// acc += the chunk's G^T Phi: the row flags, gm_gemm, then gm_fold
hipError_t launch_gm_chunk(const GmArgs& m, hipStream_t stream);
// after the last chunk: g_cnt [N], m1 [N][D], m2 [N][D] from acc
hipError_t launch_gm_final(const double* acc, int nstates, int D, int wp, double* g_cnt, double* m1, double* m2,
                           hipStream_t stream);

}  // namespace cvg
