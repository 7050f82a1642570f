// emis.h -- staging of caller-supplied emission scores (emis.hip): cv_decode_emissions* and
// cv_posterior_emissions*.
// Internal to libcviterbi; the public boundary is include/cviterbi.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvem {

// One chunk of dense emission rows -> the table layout of the decode kernel that reads them.
// Row r of the chunk is element e0 + r of the caller's array (src + (e0 + r) * ld, N scores).
struct EmisPrepArgs {
  const double* src;       // [sum T][ld] log10 scores E[e][j], rows 8-byte aligned
  int64_t ld;              // row stride in doubles (>= nstates)
  int64_t e0;              // first element of the chunk
  int64_t nrows;           // elements of the chunk
  int nstates;             // N
  int stride;              // P >= N: the decode kernel's table stride; columns [N, P) = -inf
  double* dst;             // [nrows][P] staged rows (16-byte aligned)
  int32_t* idx;            // [nrows] idx[r] = r: the chunk-relative observation index
  const int64_t* offsets;  // [nseq_total + 1] element offsets (device)
  int64_t seq_begin, seq_end;  // the chunk's sequences: their elements are [e0, e0 + nrows)
  uint8_t* status;         // [nseq_total], zeroed by the caller: CVK_SEQ_BADOBS where a row of
                           // the sequence holds a NaN or +inf (staged as -inf)
};

// emis_prepare_f64 on `stream`; cus sizes the grid (a flat grid-stride loop over the rows)
hipError_t launch_emis_prepare(const EmisPrepArgs& g, int cus, hipStream_t stream);

// One chunk of dense emission rows -> the probability-space rows of the posterior kernels:
// dst[r][j] = 10^src[e0 + r][j] 2^-k_r (exp10_scaled.h), k_r the integer that puts the row's
// largest entry into [1, 2) (0 for a row that is all -inf), columns [N, NP) = 0.
struct EmisLinArgs {
  const double* src;       // as EmisPrepArgs
  int64_t ld, e0, nrows;
  int nstates;             // N
  int stride;              // NP = post_padded_states(N): a multiple of 64
  double* dst;             // [nrows][NP] staged rows (16-byte aligned)
  int32_t* idx;            // [nrows] idx[r] = r, or -1 where the row holds a NaN, a +inf or a finite
                           // |score| >= 2^40 (staged as zeros): the posterior kernels' own range
                           // check then reports CV_SEQ_BADOBS
  const int64_t* offsets;  // [nseq_total + 1] element offsets (device)
  int64_t seq_begin, seq_end;
  int64_t* kshift;         // [nseq_total], zeroed by the caller: += k_r of the sequence's good rows
};

// emis_prepare_lin_f64 on `stream`; cus sizes the grid (each lane group takes a run of consecutive rows)
hipError_t launch_emis_prepare_lin(const EmisLinArgs& g, int cus, hipStream_t stream);

}  // namespace cvem
