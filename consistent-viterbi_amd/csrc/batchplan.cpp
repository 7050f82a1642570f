// batchplan.cpp -- see batchplan.hpp.
#include "batchplan.hpp"

#include <algorithm>
#include <cstdio>
#include <numeric>

namespace cvplan {

namespace {

inline int64_t len(const int64_t* offsets, int64_t s) { return offsets[s + 1] - offsets[s]; }

// Greedy fill in the original order: a chunk closes before the sequence that would take it over
// elem_cap or over target elements (never empty), or at 2^30 sequences.
void greedy(const int64_t* offsets, int64_t nseq, uint64_t elem_cap, uint64_t target, std::vector<Chunk>& chunks) {
  chunks.clear();
  for (int64_t s0 = 0; s0 < nseq;) {
    int64_t s1 = s0;
    uint64_t elems = 0;
    while (s1 < nseq && s1 - s0 < (1 << 30)) {
      const uint64_t T = (uint64_t)len(offsets, s1);
      if (s1 > s0 && (elems + T > elem_cap || elems + T > target)) break;
      elems += T;
      ++s1;
    }
    chunks.emplace_back(s0, s1);
    s0 = s1;
  }
}

}  // namespace

bool check_offsets(int64_t nseq, const int64_t* offsets, char (&msg)[64]) {
  msg[0] = 0;
  if (nseq < 0) return std::snprintf(msg, sizeof msg, "nseq < 0"), false;
  if (!offsets) return std::snprintf(msg, sizeof msg, "offsets is NULL"), false;
  if (offsets[0] < 0) return std::snprintf(msg, sizeof msg, "offsets[0] < 0"), false;
  for (int64_t s = 0; s < nseq; ++s) {
    const int64_t T = len(offsets, s);
    if (T < 0) return std::snprintf(msg, sizeof msg, "offsets not non-decreasing at %lld", (long long)s), false;
    if (T > INT32_MAX) return std::snprintf(msg, sizeof msg, "sequence %lld too long", (long long)s), false;
  }
  return true;
}

bool varlen(const int64_t* offsets, int64_t nseq) {
  const int64_t T0 = len(offsets, 0);
  for (int64_t s = 1; s < nseq; ++s)
    if (len(offsets, s) != T0) return true;
  return false;
}

Shares measure(const int64_t* offsets, const std::vector<Chunk>& chunks) {
  Shares m{0, 0};
  for (const Chunk& c : chunks) {
    m.max_elems = std::max<uint64_t>(m.max_elems, (uint64_t)(offsets[c.second] - offsets[c.first]));
    m.max_seqs = std::max<int64_t>(m.max_seqs, c.second - c.first);
  }
  return m;
}

Shares split_equal_shares(const int64_t* offsets, int64_t nseq, uint64_t elem_cap, std::vector<Chunk>& chunks) {
  elem_cap = std::max<uint64_t>(elem_cap, 1);
  const uint64_t total_elems = (uint64_t)(offsets[nseq] - offsets[0]);
  const uint64_t nchunks = std::max<uint64_t>(1, (total_elems + elem_cap - 1) / elem_cap);
  const uint64_t target = std::max<uint64_t>(1, (total_elems + nchunks - 1) / nchunks);
  greedy(offsets, nseq, elem_cap, target, chunks);
  return measure(offsets, chunks);
}

void split_pipelined(const int64_t* offsets, int64_t nseq, const Pipeline& p, std::vector<Chunk>& chunks) {
  const uint64_t total_elems = (uint64_t)(offsets[nseq] - offsets[0]);
  const uint64_t half_cap = std::max<uint64_t>(p.serial ? p.cap : p.cap / 2, p.per_elem_all);
  uint64_t nchunks = std::max<uint64_t>(1, (total_elems * p.per_elem_all + half_cap - 1) / half_cap);
  if (!p.serial) nchunks = std::max<uint64_t>(nchunks, std::min<uint64_t>(p.max_chunks, (uint64_t)(nseq / 2048)));
  const uint64_t target = std::max<uint64_t>(1, (total_elems + nchunks - 1) / nchunks);
  const uint64_t elem_cap = std::max<uint64_t>(half_cap / p.per_elem_all, 1);
  greedy(offsets, nseq, elem_cap, target, chunks);
  // Equal lengths: whole rounds of workgroups (`unit` sequences) per chunk, so only the last
  // chunk ends on a partly filled round (a chunk's launch waits for the last).
  const int64_t T0 = len(offsets, 0);
  if (T0 <= 0 || chunks.size() <= 1 || varlen(offsets, nseq)) return;
  const int64_t cap_seqs = (int64_t)std::min<uint64_t>(std::max<uint64_t>(elem_cap / (uint64_t)T0, 1), INT64_MAX);
  int64_t per = (nseq + (int64_t)chunks.size() - 1) / (int64_t)chunks.size();
  per = ((per + p.unit - 1) / p.unit) * p.unit;
  if (per > cap_seqs) per = cap_seqs >= p.unit ? (cap_seqs / p.unit) * p.unit : cap_seqs;
  chunks.clear();
  for (int64_t s0 = 0; s0 < nseq; s0 += per) chunks.emplace_back(s0, std::min(nseq, s0 + per));
}

void longest_first(const int64_t* offsets, const std::vector<Chunk>& chunks, int32_t* order, int64_t* npair,
                   std::vector<int64_t>& scratch) {
  for (size_t ci = 0; ci < chunks.size(); ++ci) {
    const Chunk& c = chunks[ci];
    int32_t* const b = order + c.first;
    int32_t* const e = order + c.second;
    // a counting sort on the lengths (a comparison sort of 16,384 sequences cost ~1 ms of host
    // time per call), a stable sort for very long lengths
    int64_t maxlen = 0;
    for (int64_t x = c.first; x < c.second; ++x) maxlen = std::max(maxlen, len(offsets, x));
    if (maxlen <= 4 * (c.second - c.first) + (1 << 16)) {
      std::vector<int64_t>& pos = scratch;
      pos.assign((size_t)maxlen + 2, 0);
      for (int64_t x = c.first; x < c.second; ++x) ++pos[(size_t)(maxlen - len(offsets, x)) + 1];
      for (size_t k = 1; k < pos.size(); ++k) pos[k] += pos[k - 1];
      for (int64_t x = c.first; x < c.second; ++x) b[pos[(size_t)(maxlen - len(offsets, x))]++] = (int32_t)x;
    } else {
      std::iota(b, e, (int32_t)c.first);
      std::stable_sort(b, e, [&](int32_t x, int32_t y) { return len(offsets, x) > len(offsets, y); });
    }
    if (!npair) continue;
    std::vector<int64_t>& tail = scratch;  // the leftovers, in order (the buckets are done with)
    tail.clear();
    int32_t* out = b;
    for (const int32_t* it = b; it != e;) {
      if (it + 1 != e && len(offsets, it[0]) == len(offsets, it[1])) {
        *out++ = *it++;
        *out++ = *it++;
      } else {
        tail.push_back(*it++);
      }
    }
    npair[ci] = (out - b) / 2;
    for (int64_t x : tail) *out++ = (int32_t)x;
  }
}

}  // namespace cvplan
