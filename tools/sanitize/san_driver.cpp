// san_driver.cpp -- host-only AddressSanitizer + UndefinedBehaviorSanitizer run of the C++
// host units that parse untrusted input or do wide integer arithmetic:
//   hmm_json.cpp  the hmm.json reader/writer (malformed files, nulls, round trips)
//   csp.cpp       exact term accumulation (add_exact), pair lists, the component search
//   hostscan.cpp  the constrained decode's component scan vs a scalar loop (both builds)
//   batchplan.cpp the batch planner (chunk splits, longest-first order) vs plain loops, hand-
//                 worked splits, offsets and caps at the edge of 64 bits
//   exact_fixed.h nearbyint(x * 2^64) limbs for f32 and f64 vs an __int128 reference
// Built with g++ -fsanitize=address,undefined (tools/sanitize/Makefile); runs in the
// container, never on the GPU box.  Exit status 0 = every check passed with no sanitizer
// report (UBSan is built with -fno-sanitize-recover, so any report aborts).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../consistent-viterbi_amd/csrc/batchplan.hpp"
#include "../../consistent-viterbi_amd/csrc/csp.hpp"
#include "../../consistent-viterbi_amd/csrc/exact_fixed.h"
#include "../../consistent-viterbi_amd/csrc/hmm_json.hpp"
#include "../../consistent-viterbi_amd/csrc/hostscan.hpp"

static int g_fail = 0;
static int g_csp_feasible = 0;  // CSP trials with a feasible optimum (compared)
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

// reference: round-half-even of x * 2^64 in plain double arithmetic (the scaling by 2^64 is
// exact; nearbyint rounds half to even in the default mode; |y| >= 2^52 is already integral
// and converts to __int128 exactly)
static __int128 ref_units(double x) {
  const double y = std::ldexp(x, 64);
  return (__int128)(std::fabs(y) >= 0x1p52 ? y : std::nearbyint(y));
}

static __int128 limbs_value(const int64_t* l) {
  const __int128 B = (__int128)1 << 32;
  return (__int128)l[0] + (__int128)l[1] * B + (__int128)l[2] * (B * B) + (__int128)l[3] * (B * B * B);
}

static void check_exact_fixed() {
  std::mt19937_64 rng(7);
  std::vector<double> xs = {0.0, -0.0, -1.0, -0.5, -0x1p-64, -0x1p-65, -0x1.8p-65, -0x1p-66, -3.0 * 0x1p-66,
                            -0x1p31, -0x1.fffffffffffffp31, 0x1p31, -1e-300, -4.9e-324, -2.2250738585072014e-308};
  for (int i = 0; i < 200000; ++i) {
    const double m = std::ldexp((double)(rng() >> 11), -53);
    const int e = (int)(rng() % 100) - 70;
    xs.push_back(-std::ldexp(m, e));
  }
  for (double x : xs) {
    if (!cvx::term_in_range(x)) continue;
    int64_t l[4];
    cvx::fixed64_limbs(x, l);
    CHECK(limbs_value(l) == ref_units(x));
    const float f = (float)x;
    if (cvx::term_in_range((double)f)) {
      int64_t lf[4];
      cvx::fixed64_limbs(f, lf);
      CHECK(limbs_value(lf) == ref_units((double)f));
    }
  }
  CHECK(!cvx::term_in_range(-0x1p32) && !cvx::term_in_range(0x1p32) && !cvx::term_in_range(-INFINITY));
  CHECK(cvx::term_in_range(-0x1.fffffffffffffp31));
}

static void check_add_exact() {
  int64_t limbs[4] = {0, 0, 0, 0}, ninf = 0;
  __int128 want = 0;
  std::mt19937_64 rng(11);
  for (int i = 0; i < 100000; ++i) {
    const double x = -std::ldexp((double)(rng() >> 11), -22);  // up to ~2^31 in magnitude
    CHECK(cvcsp::add_exact(limbs, &ninf, x));
    want += ref_units(x);
  }
  CHECK(limbs_value(limbs) == want);
  CHECK(cvcsp::add_exact(limbs, &ninf, -INFINITY) && ninf == 1);
  CHECK(cvcsp::add_exact(limbs, &ninf, -INFINITY + 0.0f) && ninf == 2);
  // out of range: rejected, nothing added (a huge finite "impossible" value)
  CHECK(!cvcsp::add_exact(limbs, &ninf, -1e30));
  CHECK(!cvcsp::add_exact(limbs, &ninf, -1e30f));
  CHECK(!cvcsp::add_exact(limbs, &ninf, -3.4e38f));
  CHECK(limbs_value(limbs) == want && ninf == 2);
}

static void check_csp() {
  // pair list + index
  const int64_t off[4] = {0, 4, 7, 10};
  const int32_t comp[10] = {-1, 2, 0, 2, 1, -1, 0, 3, 3, -1};
  const std::vector<int32_t> p = cvcsp::component_pairs(3, off, comp);
  CHECK(p == (std::vector<int32_t>{0, 1, 0, 2}));
  CHECK(cvcsp::pair_index(p.data(), 2, 0, 2) == 1 && cvcsp::pair_index(p.data(), 2, 1, 2) == -1);
  // exact search vs brute force on random small problems, with limb carries
  std::mt19937_64 rng(3);
  const __int128 M = 0xffffffff;
  for (int trial = 0; trial < 60; ++trial) {
    const int N = 2 + (int)(rng() % 3), ncomp = 2 + (int)(rng() % 2);
    std::vector<int32_t> pairs;
    for (int c1 = 0; c1 < ncomp; ++c1)
      for (int c2 = c1 + 1; c2 < ncomp; ++c2)
        if (rng() & 1) pairs.push_back(c1), pairs.push_back(c2);
    const int64_t npairs = (int64_t)pairs.size() / 2;
    std::vector<int64_t> part((size_t)cvcsp::partial_words(N, ncomp, npairs), 0);
    std::vector<__int128> U((size_t)ncomp * N), P((size_t)npairs * N * N);
    std::vector<uint8_t> Ud((size_t)ncomp * N, 0), Pd((size_t)npairs * N * N, 0);
    auto put = [&](int64_t* w, __int128 v) {
      w[0] += (int64_t)(v & M);
      w[1] += (int64_t)((v >> 32) & M);
      w[2] += (int64_t)((v >> 64) & M);
      w[3] += (int64_t)(v >> 96);
    };
    for (int c = 0; c < ncomp; ++c) {
      int64_t* u = part.data() + (size_t)c * cvcsp::unary_words(N);
      u[5 * N] = 1;
      for (int s = 0; s < N; ++s) {
        for (int k = 0; k < 3; ++k) {
          const __int128 v = ((__int128)(int64_t)(rng() >> 2) << (rng() % 40)) - ((__int128)1 << 88);
          put(u + 4 * s, v);
          U[(size_t)c * N + s] += v;
        }
        if (rng() % 7 == 0) u[4 * N + s] += 1, Ud[(size_t)c * N + s] = 1;
      }
    }
    for (int64_t q = 0; q < npairs; ++q) {
      int64_t* w = part.data() + (size_t)ncomp * cvcsp::unary_words(N) + (size_t)q * cvcsp::pair_words(N);
      w[5 * N * N] = 1;
      for (int e = 0; e < N * N; ++e) {
        const __int128 v = (__int128)(int64_t)(rng() >> 4) - ((__int128)1 << 70);
        put(w + 4 * e, v);
        P[(size_t)q * N * N + e] = v;
        if (rng() % 9 == 0) w[4 * N * N + e] += 1, Pd[(size_t)q * N * N + e] = 1;
      }
    }
    std::vector<int32_t> got((size_t)ncomp, -2);
    const cvcsp::SolveResult r = cvcsp::solve(N, ncomp, pairs.data(), npairs, part.data(), got.data(), 1000000);
    CHECK(!r.limit_hit);
    // brute force over every assignment, lexicographically smallest among the maxima, groups
    // merged (the whole problem as one group gives the same per-component optimum only when
    // connected; compare objective values instead)
    bool have = false;
    __int128 best = 0;
    std::vector<int> st((size_t)ncomp, 0), arg;
    for (int64_t code = 0, tot = (int64_t)std::pow(N, ncomp); code < tot; ++code) {
      int64_t c2 = code;
      for (int c = ncomp - 1; c >= 0; --c) st[(size_t)c] = (int)(c2 % N), c2 /= N;
      bool ok = true;
      __int128 v = 0;
      for (int c = 0; c < ncomp && ok; ++c) {
        ok = !Ud[(size_t)c * N + st[(size_t)c]];
        v += U[(size_t)c * N + st[(size_t)c]];
      }
      for (int64_t q = 0; q < npairs && ok; ++q) {
        const size_t e = (size_t)q * N * N + (size_t)st[(size_t)pairs[2 * q]] * N + st[(size_t)pairs[2 * q + 1]];
        ok = !Pd[e];
        v += P[e];
      }
      if (ok && (!have || v > best)) have = true, best = v, arg = st;
    }
    if (have) {
      ++g_csp_feasible;
      bool all = true;
      __int128 v = 0;
      for (int c = 0; c < ncomp; ++c) all &= got[(size_t)c] >= 0;
      if (all) {
        for (int c = 0; c < ncomp; ++c) v += U[(size_t)c * N + got[(size_t)c]];
        for (int64_t q = 0; q < npairs; ++q)
          v += P[(size_t)q * N * N + (size_t)got[(size_t)pairs[2 * q]] * N + got[(size_t)pairs[2 * q + 1]]];
      }
      CHECK(all && v == best);
    }
  }
}

// cvscan::scan_sequence / constrained_positions vs the scalar definition: random lengths
// (incl. 0 and non-multiples of 16), sparse / dense constrained elements, out-of-range values
static void check_hostscan() {
  std::mt19937_64 rng(7);
  for (int trial = 0; trial < 20000; ++trial) {
    const int64_t n = (int64_t)(rng() % 300);
    const int32_t ncomp = 1 + (int32_t)(rng() % 9);
    std::vector<int32_t> c((size_t)n, -1);
    const int mode = (int)(rng() % 4);
    for (int64_t k = 0; k < n; ++k) {
      const uint64_t x = rng() % 1000;
      if (mode >= 1 && x < (mode == 1 ? 5u : mode == 2 ? 300u : 1000u)) c[(size_t)k] = (int32_t)(rng() % ncomp);
    }
    if (n > 0 && rng() % 8 == 0)  // an out-of-range value somewhere
      c[(size_t)(rng() % n)] = (rng() % 2) ? ncomp + (int32_t)(rng() % 3) : -2 - (int32_t)(rng() % 3);
    int64_t bad = -1;
    bool any = false;
    std::vector<int64_t> pos;
    for (int64_t k = 0; k < n; ++k) {
      if (bad < 0 && (c[(size_t)k] < -1 || c[(size_t)k] >= ncomp)) bad = k;
      if (c[(size_t)k] >= 0) any = true;
    }
    const cvscan::SeqScan r = cvscan::scan_sequence(c.data(), n, ncomp);
    CHECK(r.bad == bad);
    if (bad >= 0) continue;
    CHECK(r.constrained == any);
    for (int64_t k = 0; k < n; ++k)
      if (c[(size_t)k] >= 0) pos.push_back(1000 + k);
    std::vector<int64_t> got;
    cvscan::constrained_positions(c.data(), n, 1000, got);
    CHECK(got == pos);
  }
}

// ---- batchplan.cpp --------------------------------------------------------------------------
using Chunks = std::vector<cvplan::Chunk>;

static std::vector<int64_t> offsets_of(const std::vector<int64_t>& lengths, int64_t base = 0) {
  std::vector<int64_t> off(lengths.size() + 1, base);
  for (size_t s = 0; s < lengths.size(); ++s) off[s + 1] = off[s] + lengths[s];
  return off;
}

// contiguous, non-empty, covering [0, nseq); over elem_cap elements only as a single sequence
static void check_chunks(const Chunks& ch, const std::vector<int64_t>& off, uint64_t elem_cap) {
  const int64_t nseq = (int64_t)off.size() - 1;
  CHECK(!ch.empty() && ch.front().first == 0 && ch.back().second == nseq);
  for (size_t i = 0; i < ch.size(); ++i) {
    CHECK(ch[i].first < ch[i].second);
    if (i) CHECK(ch[i].first == ch[i - 1].second);
    const uint64_t elems = (uint64_t)(off[(size_t)ch[i].second] - off[(size_t)ch[i].first]);
    CHECK(elems <= elem_cap || ch[i].second - ch[i].first == 1);
  }
}

// the order of every chunk against std::stable_sort of the identity and, with pairing, against
// a greedy scan of that sorted list (pairs of equal-length neighbours first, leftovers after)
static void check_order(const Chunks& ch, const std::vector<int64_t>& off, std::vector<int64_t>& scratch) {
  const size_t nseq = off.size() - 1;
  auto len = [&](int32_t x) { return off[(size_t)x + 1] - off[(size_t)x]; };
  std::vector<int32_t> plain(nseq, -1), paired(nseq, -1);
  std::vector<int64_t> npair(ch.size(), -1);
  cvplan::longest_first(off.data(), ch, plain.data(), nullptr, scratch);
  cvplan::longest_first(off.data(), ch, paired.data(), npair.data(), scratch);
  for (size_t ci = 0; ci < ch.size(); ++ci) {
    const size_t b = (size_t)ch[ci].first, e = (size_t)ch[ci].second;
    std::vector<int32_t> ref(e - b);
    std::iota(ref.begin(), ref.end(), (int32_t)b);
    std::stable_sort(ref.begin(), ref.end(), [&](int32_t x, int32_t y) { return len(x) > len(y); });
    CHECK(std::equal(ref.begin(), ref.end(), plain.begin() + (long)b));
    std::vector<int32_t> pairs, tail;
    for (size_t i = 0; i < ref.size();) {
      if (i + 1 < ref.size() && len(ref[i]) == len(ref[i + 1])) {
        pairs.push_back(ref[i]), pairs.push_back(ref[i + 1]);
        i += 2;
      } else {
        tail.push_back(ref[i++]);
      }
    }
    CHECK(npair[ci] == (int64_t)pairs.size() / 2);
    if (npair[ci] != (int64_t)pairs.size() / 2) continue;
    for (size_t i = 0; i + 1 < pairs.size(); i += 2) CHECK(len(paired[b + i]) == len(paired[b + i + 1]));
    for (size_t i = b + pairs.size(); i + 1 < e; ++i)  // the tail: longest first, ties by index
      CHECK(len(paired[i]) > len(paired[i + 1]) || (len(paired[i]) == len(paired[i + 1]) && paired[i] < paired[i + 1]));
    CHECK(std::equal(pairs.begin(), pairs.end(), paired.begin() + (long)b));
    CHECK(std::equal(tail.begin(), tail.end(), paired.begin() + (long)(b + pairs.size())));
  }
}

// the decode's split as plain loops: equal shares of the batch under half the cap (the whole cap
// when serial), then, for equal lengths, whole rounds of `unit` sequences per chunk
static Chunks ref_pipelined(const std::vector<int64_t>& off, const cvplan::Pipeline& p) {
  const int64_t nseq = (int64_t)off.size() - 1;
  const uint64_t total = (uint64_t)(off.back() - off.front());
  const uint64_t half_cap = std::max<uint64_t>(p.serial ? p.cap : p.cap / 2, p.per_elem_all);
  uint64_t nchunks = std::max<uint64_t>(1, (total * p.per_elem_all + half_cap - 1) / half_cap);
  if (!p.serial) nchunks = std::max<uint64_t>(nchunks, std::min<uint64_t>(p.max_chunks, (uint64_t)(nseq / 2048)));
  const uint64_t target = std::max<uint64_t>(1, (total + nchunks - 1) / nchunks);
  const uint64_t elem_cap = std::max<uint64_t>(half_cap / p.per_elem_all, 1);
  Chunks ch;
  uint64_t elems = 0;
  int64_t s0 = 0;
  for (int64_t s = 0; s < nseq; ++s) {
    const uint64_t T = (uint64_t)(off[(size_t)s + 1] - off[(size_t)s]);
    if (s > s0 && (elems + T > elem_cap || elems + T > target)) ch.emplace_back(s0, s), s0 = s, elems = 0;
    elems += T;
  }
  ch.emplace_back(s0, nseq);
  const int64_t T0 = off[1] - off[0];
  bool uniform = T0 > 0;
  for (int64_t s = 1; s < nseq; ++s) uniform &= off[(size_t)s + 1] - off[(size_t)s] == T0;
  if (!uniform || ch.size() == 1) return ch;
  const int64_t cap_seqs = (int64_t)std::min<uint64_t>(std::max<uint64_t>(elem_cap / (uint64_t)T0, 1), INT64_MAX / 2);
  int64_t per = (nseq + (int64_t)ch.size() - 1) / (int64_t)ch.size();
  while (per % p.unit) ++per;
  if (per > cap_seqs) per = cap_seqs >= p.unit ? cap_seqs - cap_seqs % p.unit : cap_seqs;
  ch.clear();
  for (s0 = 0; s0 < nseq; s0 += per) ch.emplace_back(s0, std::min(nseq, s0 + per));
  return ch;
}

static void check_batchplan() {
  char msg[64];
  const int64_t good[3] = {2, 2, 5}, down[3] = {0, 4, 3}, neg[2] = {-1, 3}, longer[2] = {0, (int64_t)INT32_MAX + 1};
  CHECK(cvplan::check_offsets(2, good, msg) && cvplan::check_offsets(0, good, msg));
  CHECK(!cvplan::check_offsets(-1, good, msg) && !std::strcmp(msg, "nseq < 0"));
  CHECK(!cvplan::check_offsets(1, nullptr, msg) && !std::strcmp(msg, "offsets is NULL"));
  CHECK(!cvplan::check_offsets(1, neg, msg) && !std::strcmp(msg, "offsets[0] < 0"));
  CHECK(!cvplan::check_offsets(2, down, msg) && !std::strcmp(msg, "offsets not non-decreasing at 1"));
  CHECK(!cvplan::check_offsets(1, longer, msg) && !std::strcmp(msg, "sequence 0 too long"));

  // hand-worked splits
  Chunks ch;
  std::vector<int64_t> scratch;
  const std::vector<int64_t> five = offsets_of({5, 3, 4, 2, 6});
  const cvplan::Shares sh = cvplan::split_equal_shares(five.data(), 5, 8, ch);
  CHECK((ch == Chunks{{0, 1}, {1, 3}, {3, 4}, {4, 5}}) && sh.max_elems == 7 && sh.max_seqs == 2);
  for (int64_t unit : {1, 2, 64, 16384}) {
    cvplan::split_pipelined(five.data(), 5, {4, 64, true, 8, unit}, ch);
    CHECK((ch == Chunks{{0, 2}, {2, 4}, {4, 5}}));
    cvplan::split_pipelined(five.data(), 5, {4, 64, false, 8, unit}, ch);
    CHECK((ch == Chunks{{0, 1}, {1, 3}, {3, 4}, {4, 5}}));
  }
  const std::vector<int64_t> ten = offsets_of(std::vector<int64_t>(10, 4));
  cvplan::split_pipelined(ten.data(), 10, {4, 64, true, 8, 3}, ch);
  CHECK((ch == Chunks{{0, 3}, {3, 6}, {6, 9}, {9, 10}}));
  cvplan::split_pipelined(ten.data(), 10, {4, 64, true, 8, 4}, ch);
  CHECK((ch == Chunks{{0, 4}, {4, 8}, {8, 10}}));

  // properties over seeded random batches
  std::mt19937_64 rng(13);
  for (int trial = 0; trial < 4000; ++trial) {
    const int64_t nseq = 1 + (int64_t)(rng() % 300);
    const int mode = (int)(rng() % 6);  // 0: all zero, 1: all equal, 2: few distinct lengths, else ragged
    const int64_t same = 1 + (int64_t)(rng() % 70);
    std::vector<int64_t> lengths((size_t)nseq);
    for (int64_t& T : lengths) T = mode == 0 ? 0 : mode == 1 ? same : mode == 2 ? 3 * (int64_t)(rng() % 4) : (int64_t)(rng() % 71);
    const std::vector<int64_t> off = offsets_of(lengths, (int64_t)(rng() % 1000));
    const uint64_t total = (uint64_t)(off.back() - off.front());
    CHECK(cvplan::check_offsets(nseq, off.data(), msg));
    bool ragged = false;
    for (int64_t T : lengths) ragged |= T != lengths[0];
    CHECK(cvplan::varlen(off.data(), nseq) == ragged);

    const uint64_t elem_cap = rng() % 4 == 0 ? rng() % 3 : rng() % (total + 10);
    const cvplan::Shares got = cvplan::split_equal_shares(off.data(), nseq, elem_cap, ch);
    check_chunks(ch, off, std::max<uint64_t>(elem_cap, 1));
    uint64_t max_elems = 0;
    int64_t max_seqs = 0;
    for (const auto& c : ch) {
      uint64_t elems = 0;
      for (int64_t s = c.first; s < c.second; ++s) elems += (uint64_t)lengths[(size_t)s];
      max_elems = std::max(max_elems, elems);
      max_seqs = std::max(max_seqs, c.second - c.first);
    }
    CHECK(got.max_elems == max_elems && got.max_seqs == max_seqs);
    if (elem_cap >= std::max<uint64_t>(total, 1)) CHECK(ch.size() == 1);
    check_order(ch, off, scratch);

    cvplan::Pipeline p;
    p.per_elem_all = 1 + rng() % 64;
    p.cap = rng() % 4 == 0 ? rng() % (2 * p.per_elem_all) : rng() % (2 * (total + 10) * p.per_elem_all);
    p.serial = rng() % 2;
    p.max_chunks = 1 + rng() % 8;
    p.unit = 1 + (int64_t)(rng() % 130);
    cvplan::split_pipelined(off.data(), nseq, p, ch);
    CHECK(ch == ref_pipelined(off, p));
    const uint64_t half_cap = std::max<uint64_t>(p.serial ? p.cap : p.cap / 2, p.per_elem_all);
    check_chunks(ch, off, half_cap / p.per_elem_all);
    if (half_cap / p.per_elem_all >= std::max<uint64_t>(total, 1)) CHECK(ch.size() == 1);
    const cvplan::Shares m = cvplan::measure(off.data(), ch);
    CHECK(m.max_elems <= std::max<uint64_t>(half_cap / p.per_elem_all, 70) && m.max_seqs >= 1);
    check_order(ch, off, scratch);
  }

  // both sides of the counting-sort threshold (longest <= 4 n + 65,536): n = 6
  for (int64_t longest : {(int64_t)65560, (int64_t)65561, (int64_t)70000}) {
    const std::vector<int64_t> off = offsets_of({7, longest, 7, 0, longest, 9});
    check_order(Chunks{{0, 6}}, off, scratch);
    check_order(Chunks{{0, 2}, {2, 6}}, off, scratch);
  }

  // offsets near INT64_MAX / per_elem and a cap of UINT64_MAX: no signed overflow
  for (uint64_t per_elem : {(uint64_t)1, (uint64_t)2, (uint64_t)2048, (uint64_t)1 << 20}) {
    const int64_t top = (int64_t)((uint64_t)INT64_MAX / per_elem);
    for (const std::vector<int64_t>& off :
         {std::vector<int64_t>{top - 40, top - 30, top - 30, top - 5, top}, std::vector<int64_t>{0, top / 2, top},
          std::vector<int64_t>{0, top / 4, top / 2, 3 * (top / 4), top}}) {
      const int64_t nseq = (int64_t)off.size() - 1;
      for (uint64_t cap : {UINT64_MAX, UINT64_MAX / 2, per_elem, (uint64_t)0})
        for (bool serial : {false, true}) {
          cvplan::split_pipelined(off.data(), nseq, {per_elem, cap, serial, 8, 64 * 256}, ch);
          check_chunks(ch, off, std::max<uint64_t>(std::max<uint64_t>(serial ? cap : cap / 2, per_elem) / per_elem, 1));
          check_order(ch, off, scratch);
          cvplan::split_equal_shares(off.data(), nseq, cap / per_elem, ch);
          check_chunks(ch, off, std::max<uint64_t>(cap / per_elem, 1));
        }
    }
  }
}

static void check_json() {
  const std::string good =
      "{\"a\":{\"v\":1,\"dim\":[2,2],\"data\":[-0.1549019599857432,-0.5228787452803376,null,0.0]},"
      "\"b\":{\"v\":1,\"dim\":[2],\"data\":[{\"v\":1,\"dim\":[3,1],\"data\":[-0.3010299956639812,-0.3010299956639812,null]},"
      "{\"v\":1,\"dim\":[3,1],\"data\":[null,-0.47712125471966244,-0.17609125905568124]}]},"
      "\"pi\":{\"v\":1,\"dim\":[2],\"data\":[-0.3010299956639812,-0.3010299956639812]}}";
  cvh::HmmJson h;
  std::string err;
  CHECK(cvh::parse_hmm_json(good, h, err));
  CHECK(h.nstates == 2 && h.bdims.size() == 2 && h.a.size() == 4 && h.b.size() == 6);
  CHECK(std::isinf(h.a[2]) && h.a[2] < 0 && std::isinf(h.b[2]));
  const std::string round = cvh::format_hmm_json(h.nstates, h.bdims, h.pi.data(), h.a.data(), h.b.data());
  cvh::HmmJson h2;
  CHECK(cvh::parse_hmm_json(round, h2, err));
  CHECK(std::memcmp(h.a.data(), h2.a.data(), 32) == 0 && std::memcmp(h.b.data(), h2.b.data(), 48) == 0);
  // malformed inputs: every prefix of the good file, bad shapes, bad tokens -- rejected
  // without a sanitizer report
  for (size_t n = 0; n < good.size(); ++n) {
    cvh::HmmJson x;
    CHECK(!cvh::parse_hmm_json(good.substr(0, n), x, err));
  }
  const char* bad[] = {"{", "{\"a\":1}", "[]", "{\"a\":{\"v\":1,\"dim\":[2,2],\"data\":[1,2,3]},\"b\":{\"dim\":[0],\"data\":[]},"
                       "\"pi\":{\"v\":1,\"dim\":[2],\"data\":[0,0]}}", "{\"a\":{\"v\":1,\"dim\":[-1,2],\"data\":[]}}",
                       "{\"a\":{\"v\":1,\"dim\":[99999999999,99999999999],\"data\":[]}}", "nul", "\"\\u12", "1e99999",
                       "{\"a\":{\"v\":1,\"dim\":[1,1],\"data\":[nan]}}"};
  for (const char* b : bad) {
    cvh::HmmJson x;
    CHECK(!cvh::parse_hmm_json(b, x, err));
  }
  // random byte flips of the good file: whatever the parser says, no sanitizer report
  std::mt19937_64 rng(5);
  for (int i = 0; i < 3000; ++i) {
    std::string s = good;
    for (int k = 0; k < 3; ++k) s[rng() % s.size()] = (char)(rng() & 0x7f);
    cvh::HmmJson x;
    (void)cvh::parse_hmm_json(s, x, err);
  }
}

int main() {
  check_hostscan();
  check_batchplan();
  check_exact_fixed();
  check_add_exact();
  check_csp();
  check_json();
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  CHECK(g_csp_feasible >= 20);
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("sanitizer driver: all checks passed (%d feasible CSP trials vs brute force)\n", g_csp_feasible);
  return 0;
}
