// posterior.h -- argument block and launchers of the sum-product (forward-backward) kernels
// (posterior.hip).  Internal to libcviterbi; the public boundary is include/cviterbi.h
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
};

// forward pass of the chunk [seq_begin, seq_end): loglik, status, and the rows when g.rows
hipError_t launch_post_fwd(const PostArgs& g, bool generic, hipStream_t stream);
// backward pass over the stored rows: path and / or gamma
hipError_t launch_post_bwd(const PostArgs& g, bool generic, hipStream_t stream);

}  // namespace cvp
