// sample.h -- argument block and launchers of the posterior path sampler (sample.hip): forward
// filtering (posterior.hip's forward pass), backward sampling over the stored rows.  Internal to
// libcviterbi; the public boundary is include/cviterbi.h (cv_sample_batch*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvs {

constexpr int kSampleMaxDraws = 64;    // R of one call
constexpr int kSampleWaveStates = 256; // up to here: one wave per (sequence, draw group)
constexpr int kSampleMaxGroup = 8;     // draws one wave carries

struct SampleArgs {
  const double* at;        // [NP][NP] A^T in probability space, zero padded (PostArgs::at)
  const double* rows;      // [elements][NP] scaled forward rows of the chunk (PostArgs::rows)
  const int64_t* offsets;  // [nseq + 1]
  const int32_t* order;    // nullable: slot -> sequence (longest first)
  int64_t seq_begin, seq_end;
  int64_t elem_base;       // element offset of row 0 of rows
  int nstates, np;
  const uint8_t* status;   // [nseq] of the forward pass: only CV_SEQ_OK sequences are sampled
  int32_t* path;           // [R][plane], indexed by element offset inside a plane
  int64_t plane;           // L = offsets[nseq]
  int draws;               // R
  uint64_t seed;
  int64_t seq_base;
};

// the walk of every (sequence, draw) of the chunk [seq_begin, seq_end); a sequence that is not
// CV_SEQ_OK gets -1 in every plane
hipError_t launch_sample(const SampleArgs& g, bool generic, hipStream_t stream);

struct SampleScoreArgs {
  const int32_t* path;     // [R][plane]
  int64_t plane;
  int draws;
  const int32_t* obs;
  const int64_t* offsets;
  const int32_t* order;
  int64_t seq_begin, seq_end;
  int64_t nseq;            // stride of a score plane
  int nstates;
  const double* pi64;      // log10 tables of the f64 decode: [N], [N][N], [V][N]
  const double* a64;
  const double* et64;
  const uint8_t* status;
  double* score;           // [R][nseq]
};

// score[r][s] = the f64 log10 fold along plane r's path of sequence s (front to back); NaN for
// CV_SEQ_BADOBS, -inf for CV_SEQ_INFEASIBLE, nothing for CV_SEQ_EMPTY
hipError_t launch_sample_score(const SampleScoreArgs& g, hipStream_t stream);

}  // namespace cvs
