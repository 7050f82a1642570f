// batchplan.hpp -- host planning of a batch call (batchplan.cpp): the offsets check, the split of
// a CSR batch into chunks of whole sequences under a workspace cap, and the longest-first order
// inside each chunk.  Integer arithmetic on caller-controlled offsets and caps only: no device
// call, no HIP header (tools/sanitize/san_driver.cpp runs it under ASan + UBSan).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace cvplan {

using Chunk = std::pair<int64_t, int64_t>;  // sequences [first, second), original order

// The checks every batch entry makes on (nseq, offsets).  false: `msg` holds the message of the
// caller's CV_EINVAL.
bool check_offsets(int64_t nseq, const int64_t* offsets, char (&msg)[64]);

// false: every sequence has the length of the first (nseq >= 1).
bool varlen(const int64_t* offsets, int64_t nseq);

// Equal shares (posterior, K-best): the fewest chunks of at most elem_cap elements each, filled
// to equal shares of the batch rather than full chunks and a remainder, so every launch fills
// the device alike.  A sequence longer than elem_cap is a chunk of its own.
struct Shares {
  uint64_t max_elems;  // of any chunk
  int64_t max_seqs;
};
Shares split_equal_shares(const int64_t* offsets, int64_t nseq, uint64_t elem_cap, std::vector<Chunk>& chunks);

// The decode's split: chunks pipelined over two streams out of a double-buffered workspace
// (each gets half the cap) unless `serial`.
struct Pipeline {
  uint64_t per_elem_all;  // workspace bytes per element (> 0)
  uint64_t cap;           // workspace bytes
  bool serial;
  uint64_t max_chunks;  // pipelined: at least min(max_chunks, nseq / 2048) chunks
  int64_t unit;         // sequences of one round of workgroups (> 0): (64 | group) * CUs
};
void split_pipelined(const int64_t* offsets, int64_t nseq, const Pipeline& p, std::vector<Chunk>& chunks);
Shares measure(const int64_t* offsets, const std::vector<Chunk>& chunks);

// order[c.first, c.second) of every chunk c = its sequences longest first, ties by ascending
// index (the stable order, hence unique: a counting sort on the lengths, a stable sort where
// the longest is too long for one).  npair (nullable, [chunks.size()]): then equal-length
// neighbours are paired first -- slots [c.first, c.first + 2 * npair[ci]) hold the pairs -- and
// the leftovers follow, still longest first.  scratch is the caller's, kept between calls.
void longest_first(const int64_t* offsets, const std::vector<Chunk>& chunks, int32_t* order, int64_t* npair,
                   std::vector<int64_t>& scratch);

}  // namespace cvplan
