// bcount.h -- argument block and launchers of the expected emission counts (bcount.hip) behind
// cv_expected_counts_model*.  Internal to libcviterbi; the public boundary is include/cviterbi.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvb {

constexpr int kBcntMaxParts = 4096;  // most parts of a chunk by rule (bcnt_part_rows = 0)
constexpr int kBcntMinRows = 64;     // fewest rows of a part by rule

// rows per part of a chunk's sorted row list: a function of the chunk's rows, NP and the tuning
// key bcnt_part_rows alone (NP: the rule keeps a part's reads at 32 KiB or more)
inline int64_t bcnt_part_rows(int64_t rows, int np, int64_t key) {
  if (key > 0) return key;
  int64_t per = (rows + kBcntMaxParts - 1) / kBcntMaxParts;
  const int64_t least = np >= 512 ? kBcntMinRows / 2 : kBcntMinRows;
  return per < least ? least : per;
}
// most runs a chunk of `rows` rows can have: a run starts where a part starts or the key changes
// (the keys are 0 .. V, V the discard key)
inline int64_t bcnt_max_runs(int64_t rows, int64_t part_rows, int64_t nobs) {
  const int64_t parts = (rows + part_rows - 1) / part_rows;
  return parts + (nobs + 1 < rows ? nobs + 1 : rows);
}

struct BcntArgs {
  // the chunk: sequences [seq_begin, seq_end) = elements [elem_base, elem_base + nrows)
  const int64_t* offsets;
  const int32_t* obs;      // indexed by element offset
  const uint8_t* status;   // [nseq]
  int64_t seq_begin, seq_end, elem_base, nrows;
  int64_t nobs;            // V: keys 0 .. V - 1, the discard key V
  int nstates, np;
  const double* g;         // row r of the chunk (element elem_base + r) at g + r * ld, N values: w_s gamma
  int64_t ld;
  int64_t part_rows;
  // scratch of the chunk
  uint32_t *key_in, *key_out;  // [nrows]
  int32_t *row_in, *row_out;   // [nrows] the permutation: row_out[i] is the row at sorted place i
  int32_t* run;                // [nrows] 1-based run number of sorted place i (flags before the scan)
  void* sort_tmp;              // rocPRIM's scratch for the sort and the scan
  size_t sort_tmp_bytes;
  int64_t max_runs;
  uint32_t* run_key;           // [max_runs] the key of every run
  double* part;                // [max_runs][NP] the sum of every run
  double* acc;                 // [V][NP] the call's accumulator
};

// bytes of sort_tmp for a chunk of at most `rows` rows
hipError_t bcnt_sort_tmp_bytes(int64_t rows, int64_t nobs, size_t* bytes);
// acc += the chunk's rows by observation: keys, stable sort, runs, run sums, fold
hipError_t launch_bcnt_chunk(const BcntArgs& b, hipStream_t stream);
// after the last chunk: b_cnt[j * V + v] = acc[v][j]
hipError_t launch_bcnt_final(const double* acc, int64_t nobs, int nstates, int np, double* b_cnt, hipStream_t stream);

}  // namespace cvb
