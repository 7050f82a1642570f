// posterior.h -- argument block and launchers of the sum-product (forward-backward) kernels
// (posterior.hip) and of the expected-counts and gradient kernels behind them (counts.hip, grad.hip).  Internal to libcviterbi; the public boundary is include/cviterbi.h
// (cv_posterior_batch*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvp {

constexpr int kPostMmStates = 256;    // up to here: the matrix-core kernels (post_*_mm)
constexpr int kPostMaxStates = 4096;  // up to here: the plain kernels (two vectors of NP in LDS)
constexpr int kPostGroup = 32;        // sequences per workgroup of the matrix-core kernels
constexpr int kPostDumpWaves = 4096;

// padded state count of the probability-space tables: 64 / 128 / 192 / 256, then multiples of 64
inline int post_padded_states(int n) { return (n + 63) / 64 * 64; }

struct PostArgs {
  // probability-space tables, zero padded to NP = post_padded_states(N)
  const double* pi;  // [NP]
  const double* a;   // [NP][NP] row-major (from, to)
  const double* at;  // [NP][NP] transposed
  const double* et;  // [V][NP] emission column of each observation
  const int64_t* offsets;  // [nseq + 1] element offsets
  const int32_t* obs;      // indexed by element offset
  const int32_t* forced;   // nullable; indexed like obs
  const int32_t* order;    // nullable: slot k of [seq_begin, seq_end) -> sequence (longest first)
  int64_t seq_begin, seq_end;
  int64_t elem_base;  // element offset that maps to row 0 of rows
  int nstates, np;
  int64_t nobs;
  double* rows;       // [elements][NP] scaled forward rows (null: scoring mode, forward only)
  double* loglik;     // [nseq]
  uint8_t* status;    // [nseq]
  int32_t* path;      // nullable, indexed by element offset
  double* gamma;      // nullable, [element][N]
  double* dump;       // [kPostDumpWaves][64] target of the stores of masked lanes
  // nullable, [nseq]: the binary exponent the emission rows of each sequence were scaled by
  // (their sum of k, emis_prepare_lin_f64), added to the forward pass's exponent sum
  const int64_t* kshift;
  // counts arm of the backward pass (cv_expected_counts*; urows null: the plain pass).  Rows are
  // chunk-local like `rows`: row e belongs to element elem_base + e = step t of its sequence.
  double* urows;  // [elements][NP] u_{t+1} = b(o_{t+1}) o mask_{t+1} o beta^_{t+1}; unwritten at t = T - 1
  double* inv;    // [elements] 1 / rsum_t; 0 at t = T - 1, where rsum_t = 0, and in a sequence that is not OK
  double* g0;     // [nseq][NP] gamma_0 of every OK sequence (the other slots stay unwritten)
  // gradient arm of the counts arm (cv_loglik_grad_emissions*, grad.hip; read by its kernels only):
  // inv, g0 and the gamma rows carry the factor weight[s], and the rows go to egrad, not gamma
  const double* weight;  // nullable, [nseq]: all 1
  double* egrad;         // nullable, row e at egrad + e * ld_grad, N values; the columns beyond stay unwritten
  int64_t ld_grad;       // >= N
};

// ---- expected transition counts (cv_expected_counts*) ----------------------------------------
constexpr uint64_t kXiPartCap = (uint64_t)512 << 20;  // most bytes of partial tiles
constexpr int kXiMaxParts = 256;                      // most parts by rule (xi_part_rows = 0)
constexpr int kXiMinRows = 1024;                      // fewest rows of a part by rule

// rows per GEMM part of a chunk of `rows` rows: a function of rows, NP and the tuning key
// xi_part_rows (and of part_cap, the bytes the call's workspace cap leaves the partial tiles)
inline int64_t post_xi_part_rows(int64_t rows, int np, int64_t key, uint64_t part_cap) {
  const uint64_t tile = (uint64_t)np * np * 8;
  const int64_t maxp = (int64_t)((part_cap < kXiPartCap ? part_cap : kXiPartCap) / tile);
  const int64_t fit = maxp > 1 ? maxp : 1, rule = fit < kXiMaxParts ? fit : kXiMaxParts;
  int64_t per = key > 0 ? key : (rows + rule - 1) / rule;
  if (key <= 0 && per < kXiMinRows) per = kXiMinRows;
  if (per < (rows + fit - 1) / fit) per = (rows + fit - 1) / fit;
  return (per + 3) / 4 * 4;
}

struct XiArgs {
  const double* rows;   // [nrows][NP] alpha^ rows of the chunk
  const double* urows;  // [nrows][NP]
  const double* inv;    // [nrows]
  int64_t nrows, part_rows, nparts;  // part p: rows [p part_rows, min((p + 1) part_rows, nrows))
  int np;
  double* part;  // [nparts][NP][NP] partial sums, every entry written
  double* s;     // [NP][NP] the call's accumulator: s += sum_p part[p], p ascending
};
struct CountsFinalArgs {
  const double* s;   // [NP][NP]
  const double* a;   // [NP][NP] probability-space A
  const double* g0;  // [nseq][NP]
  const uint8_t* status;
  int64_t nseq;
  int nstates, np;
  double* a_cnt;   // [N][N] = A o S
  double* pi_cnt;  // [N] = sum of gamma_0 over the OK sequences: 16 strided runs, s ascending, then one tree
};

// forward pass of the chunk [seq_begin, seq_end): loglik, status, and the rows when g.rows
hipError_t launch_post_fwd(const PostArgs& g, bool generic, hipStream_t stream);
// backward pass over the stored rows: path and / or gamma
hipError_t launch_post_bwd(const PostArgs& g, bool generic, hipStream_t stream);
// the backward pass with the counts arm (g.urows, g.inv, g.g0 set; launch_post_bwd forwards here)
hipError_t launch_post_cnt_bwd(const PostArgs& g, bool generic, hipStream_t stream);
// the counts arm with the gradient arm (g.weight, g.egrad, g.ld_grad read): grad.hip
hipError_t launch_post_grad_bwd(const PostArgs& g, bool generic, hipStream_t stream);
// S += R^T U over the chunk's rows (R = alpha^ o inv): post_xi_gemm, then post_xi_fold
hipError_t launch_post_xi(const XiArgs& x, hipStream_t stream);
// after the last chunk: a_cnt and pi_cnt
hipError_t launch_post_counts_final(const CountsFinalArgs& c, hipStream_t stream);

}  // namespace cvp
