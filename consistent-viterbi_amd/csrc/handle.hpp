// handle.hpp -- the HMM handle (struct cv_hmm) and the host scaffolding shared by the translation
// units behind include/cviterbi.h: cviterbi.cpp (the handle and its table builders, the
// constrained, chain, solver, fit and timing entries; the definitions of everything declared here
// but the decode core), decode.cpp (the decode / K-best / dense-emission entries; decode_device and
// decode_host_locked) and evaluate.cpp (the posterior / sampling / counts / gradient entries).
// Internal: nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/cviterbi.h"
#include "tuning.h"

// the handle's lock plus its tuning snapshot as the calling thread's current tuning (tuning.h)
#define CV_LOCK(h)                             \
  std::lock_guard<std::mutex> lk((h)->mu);     \
  cvk::TuningScope tuning_scope((h)->tuning)

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return cvi::set_err(CV_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                          __LINE__);                                                           \
  } while (0)

namespace cvi {

// the calling thread's message (cv_last_error) and the status to return with it
cv_status set_err(cv_status st, const char* fmt, ...);

// device bytes this process's library holds now / at most (cv_device_memory)
extern std::atomic<int64_t> g_dev_cur, g_dev_peak;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) {
      (void)hipFree(p);
      g_dev_cur -= (int64_t)bytes;
    }
    p = nullptr;
    bytes = 0;
  }
  cv_status ensure(size_t n) {
    if (n <= bytes && p) return CV_OK;
    release();
    if (n == 0) n = 16;
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return set_err(CV_ENOMEM, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
    }
    bytes = n;
    const int64_t cur = g_dev_cur += (int64_t)n;
    int64_t pk = g_dev_peak.load();
    while (cur > pk && !g_dev_peak.compare_exchange_weak(pk, cur)) {
    }
    return CV_OK;
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

constexpr uint64_t kDefaultWorkspace = 8ull << 30;
constexpr uint64_t kDefaultWorkspaceT64 = 64ull << 30;  // config 5 resume decode in one chunk: 3% faster than 40 GiB

// A grow-only pinned host buffer (hipHostMalloc) for small device-to-host results read right
// after a synchronize (the parallel chain's scores, statuses and certificates: two direct
// copies instead of three through the runtime's pageable staging).
struct PinnedHost {
  void* p = nullptr;
  size_t cap = 0;
  PinnedHost() = default;
  PinnedHost(const PinnedHost&) = delete;
  PinnedHost& operator=(const PinnedHost&) = delete;
  ~PinnedHost() { release(); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  bool ensure(size_t bytes) {
    if (cap >= bytes && p) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = std::max<size_t>(bytes, 4096);
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    cap = want;
    return true;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

// Pinned, double-buffered host staging of a decode call's longest-first order: the call
// writes slot k only after that slot's previous copy has completed (its event), so the
// copy is truly asynchronous and the host never waits for the stream's earlier work
struct OrderStage {
  int32_t* p[2] = {nullptr, nullptr};
  size_t cap[2] = {0, 0};
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool pending[2] = {false, false};
  int slot = 0;
  OrderStage() = default;
  OrderStage(const OrderStage&) = delete;
  OrderStage& operator=(const OrderStage&) = delete;
  ~OrderStage() {
    for (int k = 0; k < 2; ++k) {
      if (pending[k]) (void)hipEventSynchronize(ev[k]);
      if (p[k]) (void)hipHostFree(p[k]);
      if (ev[k]) (void)hipEventDestroy(ev[k]);
    }
  }
  // the current slot, at least n entries, free to write (nullptr: allocation failed)
  int32_t* acquire(size_t n) {
    const int k = slot;
    if (pending[k]) {
      if (hipEventSynchronize(ev[k]) != hipSuccess) return nullptr;
      pending[k] = false;
    }
    if (!ev[k] && hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) return nullptr;
    if (cap[k] < n) {
      if (p[k]) (void)hipHostFree(p[k]);
      p[k] = nullptr;
      cap[k] = 0;
      const size_t want = std::max<size_t>(n, 4096);
      if (hipHostMalloc((void**)&p[k], want * 4, hipHostMallocDefault) != hipSuccess) return nullptr;
      cap[k] = want;
    }
    return p[k];
  }
  // after the copy out of the current slot is enqueued on `stream`
  hipError_t release(hipStream_t stream) {
    const hipError_t e = hipEventRecord(ev[slot], stream);
    pending[slot] = e == hipSuccess;
    slot ^= 1;
    return e;
  }
};

}  // namespace cvi

struct cv_hmm {
  using DevBuf = cvi::DevBuf;
  using PinnedHost = cvi::PinnedHost;
  using OrderStage = cvi::OrderStage;

  int N = 0, D = 0;
  std::vector<int64_t> bdims;
  int64_t V = 0;
  std::vector<double> pi, a, b;  // host log10, canonical (-0.0 -> +0.0); b state-major [N*V]
  int device = 0;
  int cus = 0;                      // compute units of the device (workgroup rounds)
  hipStream_t stream = nullptr;     // default stream of the handle
  hipStream_t bt_stream = nullptr;  // backtrack stream (overlaps the next chunk's forward)
  std::mutex mu;
  // tuning keys and test hooks (tuning.h): the environment at cv_hmm_create, then
  // cv_hmm_set_tuning only; every locked host API call makes it the thread's current tuning
  cvk::Tuning tuning;

  // trellis kernel tables (f32, padded to NP)
  int np = 0;
  DevBuf t_aimg, t_pi, t_et, t_at, t_arm;  // t_arm: row-major A (one-wave kernel)
  // one-wave kernel (N <= 64): tables padded to npw = 16 * ceil(N / 16) states
  int npw = 0;
  DevBuf w_arm, w_pi, w_et, w_at;
  DevBuf t_aimg_T, t_pi0;  // reversed (backward) pass: VALU image of a^T, pi = 0
  // f64 tables (generic f64 kernel + re-scoring): pi[N], a[N*N], et[V][N]
  bool f64_ready = false;
  DevBuf d_pi64, d_a64, d_et64;
  DevBuf d_at64;  // [N][N] a^T, f64: the constrained decode's suffix pass for N > 256

  // exact-f64 trellis tables (trellis_fwd_f64 / backtrack_f64), padded to np64 = 64*ceil(N/64)
  int np64 = 0;
  bool t64_ready = false;
  DevBuf q_a, q_at, q_pi, q_et;
  DevBuf q_at32;            // f32(a^T), uploaded when t64_nonpos
  bool t64_nonpos = false;  // every finite pi/a/b entry in [-2^80, 0] (NONPOS backtrack test)
  int nonpos_cache = -1;    // model_nonpos(): the same predicate without the t64 tables (any N)
  double arc_max = -1.0;    // max finite |pi| or |a|, plus max finite |b| (< 0: not computed yet)
  double cert_rho_cap = 0.0;  // the parallel chain's certified backtrack (T64BtArgs::rho_cap)
  // sparse low planes (tuning key t64_lo_every): the resolver's device counter block
  // ([kT64StatSlots + 1][kT64StatWords] u64; the last slot holds the call's lo_every and
  // sequence count) and its pinned host copy, made asynchronously after each plain batch decode
  // on the f64 trellis, so it holds the last such call that has FINISHED.  t64_lo_off: the
  // sticky guard -- a call that replayed densely more than once per 64 sequences (tie-heavy
  // models) or failed a self-check pins the handle to full rows
  DevBuf t64_stats;
  PinnedHost t64_stats_pin;
  bool t64_lo_off = false;
  // certified fixed-point first pass (tuning key t64_fixed_first, fixed_first_decode): the int32
  // tables in the f32 trellis tables' layouts, built once per handle (fx_state -1: not looked at
  // yet, 0: the model is outside the pass's range, 1: ready); the per-sequence certificates and
  // their pinned host copy; the compact batch of the uncertified sequences.  fx_pinned: the
  // sticky guard -- a call that left more than 1 in 8 sequences uncertified pins the handle to
  // the f64 kernels.  fx_last: engaged, certified, fallback, pinned (cv_last_fixed_first_stats)
  int fx_state = -1;
  DevBuf fx_aimg, fx_pi, fx_et, fx_at;
  double fx_gain = 0.0;
  DevBuf fx_cert, fx_idx, fx_obs2, fx_path2, fx_score2, fx_status2;
  PinnedHost fx_cert_pin;
  std::vector<int64_t> fx_idx_host;
  bool fx_pinned = false;
  int64_t fx_last[4] = {0, 0, 0, 0};
  // certified f32 round-up first pass (tuning key t64_f32ru_first): the shifted, rounded-up f32
  // tables in the same layouts, the shifts ca [N] and cb [V] in f64 (ru_state as fx_state); the
  // shifts mu_t and losing candidates r_t per element and E per sequence of the last call.
  // fx_last_kind: which first pass the last call took (0 none, 1 integer, 2 round-up)
  int ru_state = -1;
  DevBuf ru_aimg, ru_pi, ru_et, ru_at, ru_ca, ru_cb;
  double ru_ks = 0.0;
  DevBuf ru_mu, ru_r, ru_e;
  int fx_last_kind = 0;
  DevBuf q_pi0;  // the reversed (suffix) pass: pi = 0 for the N states, -inf padding
  // f32 generic tables
  bool g32_ready = false;
  DevBuf d_pi32, d_a32, d_et32;
  DevBuf d_at32;  // [N][N] a^T f32 (generic_bt_rows)
  // probability-space tables of the posterior kernels (10^x, zero padded to pnp states; built on
  // first use): pi[pnp], a[pnp][pnp], a^T, et[V][pnp], and the dump rows of masked stores
  int pnp = 0;
  DevBuf p_pi, p_a, p_at, p_et, p_dump;
  // posterior workspace: the scaled forward rows of one chunk, the longest-first order, and the
  // host API's gamma staging
  DevBuf ps_rows, ps_order, st_gamma;
  DevBuf ps_kshift;  // cv_posterior_emissions*: each sequence's sum of row-scale exponents (int64)
  // cv_expected_counts*: the GEMM's partial tiles, the call's NP x NP accumulator, gamma_0 of every
  // sequence, and the host API's staging of pi_cnt [N] and a_cnt [N][N]
  DevBuf ps_xi_part, ps_xi_s, ps_g0, st_cnt;
  DevBuf ps_bc_acc, ps_bc_sort, ps_bc_part;  // cv_expected_counts_model*: [V][NP] accumulator, sort scratch, run sums
  // cv_gauss_emissions* / cv_expected_counts_gauss*: the call's tables (c, mean^T, w^T, center) and
  // their pinned staging; the moment GEMM's partial tiles, its [NP][2D + 1 padded] accumulator and
  // the chunk's row flags
  DevBuf ps_gauss, ps_gm_part, ps_gm_acc, ps_gm_ok;
  OrderStage gs_pin;
  PinnedHost sm_pin;  // cv_sample_batch: the log-likelihoods and score planes on their way to the caller
  OrderStage ps_pin;
  // K-best workspace: the u16 back-pointers of one chunk, each sequence's last lists, the
  // longest-first order, the ranks' end points, and the host API's count staging
  DevBuf kb_bp, kb_last, kb_order, kb_end, st_count;
  OrderStage kb_pin;
  // workspace
  DevBuf ws_main, ws_last, ws_order;
  // a second decode workspace + stream: the constrained decode's unconstrained sequences run
  // on it beside the terms pass (constrained decode)
  struct SideWs {
    DevBuf main, last, order, idx, obs2, path2, res2;
    std::vector<int32_t> order_host;
    OrderStage order_pin;
    hipEvent_t ws_done = nullptr;  // the last decode_device call on this workspace has finished
    bool ws_rec = false;
    std::vector<int64_t> idx_host;
    std::vector<hipEvent_t> ev;
    hipStream_t stream = nullptr;  // lowest priority: fills what the constrained work leaves idle
    hipStream_t hi = nullptr;      // highest priority: the constrained work itself
    hipEvent_t start = nullptr, done = nullptr, after = nullptr;
  } side;
  DevBuf st_off, st_obs, st_path, st_score, st_status, st_forced;
  DevBuf st_emis;  // cv_decode_emissions: the host array's rows, compact ([elements][N])
  DevBuf cs_ranges, cs_delta, cs_g, cs_mu, cs_start, cs_zero, cs_queue;  // constrained-decode scratch
  DevBuf cs_wrows;  // the wide generic_ext's rows ([slot][2][N], N > 10,240)
  DevBuf cs_comp, cs_words;  // device exact unary sums: per-sequence components, output words
  DevBuf cs_flag;            // device exact sums: out-of-range term flag
  DevBuf cs_seg;             // segment-table rows (cs_delta keeps the prefix rows t_1)
  // resume flow of the constrained decode: stored prefix rows, forced row t_1 per constrained
  // sequence, the compact suffix batch and its index arrays
  DevBuf rs_rows, rs_rowbase, rs_resume, rs_start, rs_off2, rs_ridx, rs_slot, rs_obs2, rs_frc2, rs_path2;
  // certified suffix trace (f64): the suffix pass's rows, their per-slot bases, the slot flags
  DevBuf rs_srows, rs_srowbase, rs_cert;
  hipEvent_t rs_ev = nullptr;  // prefix backtrack done / staging done
  std::vector<int32_t> order_host;
  OrderStage order_pin;
  // the last decode_device call on the main workspace has finished (recorded on its stream;
  // the next call waits for it on ITS stream, so calls on different streams never share the
  // workspace while it is in use)
  hipEvent_t ws_done = nullptr;
  bool ws_rec = false;
  std::vector<float> host_dl, host_mu;  // constrained-decode term rows (kept: no per-call page faults)
  std::vector<int64_t> sort_pos;        // counting-sort buckets of the longest-first order
  // timing events of the last call
  std::vector<hipEvent_t> ev;  // 4 per chunk: fwd start/end (main stream), bt start/end
  std::vector<uint8_t> ev_nobt;  // per chunk of ev: nothing ran between its bt events (bt_ms reads 0)
  int64_t last_launches = 0;
  size_t last_ev_base = 0;  // first event of the last call in ev
  // cv_timing_begin/end: every decode call's events kept (appended) until cv_timing_end
  bool acc_on = false, acc_overflow = false;
  size_t acc_used = 0;
  int32_t last_kernel = 0;
  int32_t last_np = 0;
  int32_t last_mt = -1;
  uint64_t last_explored = 0;
  int64_t last_traced = 0;  // constrained sequences the last resume flow certified (suffix trace)
  // the last cv_decode_superseq_cp: parallel chain ran (1/0), sequences certified, sequences in
  // serial-chain runs, runs, certified folds done by the quantised sum, sequences taken from
  // speculative parallel re-decodes, such batches
  // speculative parallel re-decodes, such batches, candidate paths fetched packed for the walk,
  // walk steps that waited for the whole path copy
  int64_t last_chain[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // the parallel chain's per-call device arrays, kept between calls (grow-only): a
  // config-4-sized call allocated and freed ~0.4 GB of them each time (hipFree synchronises)
  struct ChainBufs {
    DevBuf off, obs, path, res, cert, ebin, q, ends, gid, gpath;
    // serial runs and speculative batches (kept, so no hipFree -- a device-wide sync -- lands
    // while the second part's forward pass runs)
    DevBuf first, rpsi, rows, small, rpath, soff, sobs, spath, sres, sinit, slast, spsi;
  } chainb;
  // the chain's own stream (high priority: its walk-side kernels -- end states, quantised folds,
  // gathers, runs, speculative batches -- run beside the second part's forward pass) and the
  // events closing each part's decode
  hipStream_t chain_stream = nullptr;
  std::vector<hipEvent_t> part_ev;
  // the parallel chain's path copy: per decode chunk, behind that chunk's backtrack (chunk_ev),
  // on a non-blocking stream of its own, from a host thread of its own
  std::vector<hipEvent_t> chunk_ev;
  std::vector<hipEvent_t> emis_ev;  // dense emissions: chunk k's rows staged (on bt_stream, beside chunk k-1)
  hipStream_t copy_stream = nullptr;
  PinnedHost chain_pin;  // the chain's scores, statuses and certificates on their way to the host
  PinnedHost chain_gpin;  // the chain's gathered candidate paths and speculative results (16 MiB)
  // the chain's later parts' observations and its path copy's two-chunk ring, staged through
  // pinned memory: the DMA engines move them, where a pageable copy runs blit kernels beside
  // the forward passes (tuning keys chain_pin_obs / chain_pin_path)
  PinnedHost chain_obs_pin, chain_ring[2];
  hipEvent_t ring_ev[2] = {nullptr, nullptr};

  ~cv_hmm() {
    for (auto e : ring_ev)
      if (e) (void)hipEventDestroy(e);
    for (auto e : ev) (void)hipEventDestroy(e);
    for (auto e : side.ev) (void)hipEventDestroy(e);
    if (side.start) (void)hipEventDestroy(side.start);
    if (side.done) (void)hipEventDestroy(side.done);
    if (side.after) (void)hipEventDestroy(side.after);
    if (side.stream) (void)hipStreamDestroy(side.stream);
    if (side.hi) (void)hipStreamDestroy(side.hi);
    if (rs_ev) (void)hipEventDestroy(rs_ev);
    if (ws_done) (void)hipEventDestroy(ws_done);
    if (side.ws_done) (void)hipEventDestroy(side.ws_done);
    if (stream) (void)hipStreamDestroy(stream);
    if (bt_stream) (void)hipStreamDestroy(bt_stream);
    for (auto e : chunk_ev) (void)hipEventDestroy(e);
    for (auto e : emis_ev) (void)hipEventDestroy(e);
    for (auto e : part_ev) (void)hipEventDestroy(e);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (chain_stream) (void)hipStreamDestroy(chain_stream);
  }
};

namespace cvi {

cv_status upload(DevBuf& buf, const void* src, size_t bytes);
// The default delta-workspace cap when the caller leaves opts.workspace_bytes at 0: `base`,
// clamped to 3/4 of what the device can still give the workspace being sized (`held` = its
// current bytes, reclaimable).
uint64_t default_workspace_cap(uint64_t held, uint64_t base);
cv_status set_device(cv_hmm* h);
cv_opts default_opts();
// The model's device tables by kernel family, each built on first use: the f32 trellis (and its
// one-wave form), the f64 tables of the generic kernel and the re-scoring, a^T for the generic
// rows mode (f64 / f32), the exact-f64 trellis, the f32 generic kernel.
cv_status ensure_trellis_tables(cv_hmm* h);
cv_status ensure_f64_tables(cv_hmm* h);
cv_status ensure_at64(cv_hmm* h);
cv_status ensure_at32(cv_hmm* h);
cv_status ensure_t64_tables(cv_hmm* h);
cv_status ensure_g32_tables(cv_hmm* h);
// Every finite pi/a/b entry in [-2^80, 0] (log-probabilities), and tuning key t64_nonpos on.
bool model_nonpos(cv_hmm* h);
// ev[i], created on first use (nullptr: hipEventCreate failed)
hipEvent_t get_event(std::vector<hipEvent_t>& ev, size_t i);

// Host worker threads for the O(elements) loops of the host API: min(16, hardware threads),
// tuning key host_threads overrides.
int host_threads();

// f(t, lo, hi) over [0, n) split into contiguous ranges, one per worker (t = worker index).
template <typename F>
void parallel_ranges(int64_t n, F&& f, int64_t min_per_thread = 1 << 16) {
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), n / std::max<int64_t>(min_per_thread, 1)));
  if (nt <= 1) {
    f(0, (int64_t)0, n);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt);
  for (int t = 0; t < nt; ++t) th.emplace_back([&, t] { f(t, n * t / nt, n * (t + 1) / nt); });
  for (auto& x : th) x.join();
}

// First index k in [lo, hi) with bad(k), or -1 (parallel scan; the smallest index wins).
template <typename P>
int64_t first_bad(int64_t lo, int64_t hi, P&& bad) {
  std::vector<int64_t> first((size_t)host_threads(), -1);
  parallel_ranges(hi - lo, [&](int t, int64_t a, int64_t b) {
    for (int64_t k = lo + a; k < lo + b; ++k)
      if (bad(k)) {
        first[t] = k;
        return;
      }
  });
  for (int64_t f : first)
    if (f >= 0) return f;  // workers hold ascending ranges
  return -1;
}

cv_status check_batch(int64_t nseq, const int64_t* offsets);

// ---- scaffolding shared by the device cores (decode_device, posterior_device, kbest_device) ----
// The host copy of the offsets, checked: the caller's, or fetched from the device into `off_copy`.
cv_status host_offsets(int64_t nseq, const int64_t*& offsets_host, const int64_t* offsets_dev,
                       std::vector<int64_t>& off_copy, hipStream_t stream);
// The longest-first order of a call on its way to the device, through the pinned stage.
cv_status upload_order(DevBuf& dev, OrderStage& stage, const int32_t* order_host, int64_t nseq, hipStream_t stream,
                       const int32_t** order_dev);
// The decode workspace a core call runs on: the handle's main one, or the side workspace of a
// decode running beside another decode_device call of the same handle on another stream.
struct DecodeWs {
  DevBuf &main, &last, &order;
  std::vector<int32_t>& order_host;
  OrderStage& order_pin;
  std::vector<hipEvent_t>& ev;
  hipEvent_t& ws_done;  // the last core call on this workspace has finished
  bool& ws_rec;
};
inline DecodeWs decode_ws(cv_hmm* h, bool side) {
  auto& s = h->side;
  if (side) return {s.main, s.last, s.order, s.order_host, s.order_pin, s.ev, s.ws_done, s.ws_rec};
  return {h->ws_main, h->ws_last, h->ws_order, h->order_host, h->order_pin, h->ev, h->ws_done, h->ws_rec};
}
// The nev timing events of a call, evv[*eb ...]: from 0 (each call overwrites the last), or
// appended after the calls already timed since cv_timing_begin.  side_ws: the side workspace's
// own events, no bookkeeping.
cv_status reserve_events(cv_hmm* h, bool side_ws, size_t nev, size_t* eb);
// The end of a core call whose last work is on `stream`: its nev events are kept (cv_timing_begin)
// and the workspace's ws_done follows it.
cv_status end_call(cv_hmm* h, bool side_ws, size_t nev, hipStream_t stream);

// The kernels index per-element arrays by absolute element e, while a chunk's (or a staged
// slice's) storage p starts at its first element e0: the pointer q with q[e * width] =
// p[(e - e0) * width].
template <typename T>
T* rebased(T* p, int64_t e0, size_t width = 1) {
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) - (uintptr_t)e0 * width * sizeof(T));
}

// Caller-supplied emission scores (cv_decode_emissions*): a dense device array, row e (element
// index of the CSR offsets) at p + e * ld, N log10 scores each.
// chunk_local (cv_expected_counts_gauss*): p and ld are unused; the rows of a chunk are computed
// into a workspace of the plan whose row 0 is the chunk's first element.
struct EmisSrc {
  const double* p;
  int64_t ld;
  bool chunk_local = false;
};

// The options of decode_device beyond a plain decode; every caller names only what it sets.
struct DecodeReq {
  const void* resume_rows = nullptr;  // the constrained decode's resume rows (the kernel's real type)
  // the handle's second workspace (h->side), no timing / last-call bookkeeping -- a decode
  // running beside another decode_device call of the same handle on another stream
  bool side_ws = false;
  // the parallel CPSolver chain (row-A0 f64 trellis or the f64 generic rows mode): each chunk's
  // backtrack computes its certificates (or a cp_cert pass reads its rows and paths) -> [nseq][2]
  double* cp_cert = nullptr;
  const double* cp_init = nullptr;  // the chain's speculative re-decodes: start offsets in,
  double* cp_last = nullptr;        // last values out
  // h->chunk_ev[i] is recorded after chunk i's backtrack (its paths written, before any
  // certificate pass) and its sequence range [s0, s1) appended
  std::vector<std::pair<int64_t, int64_t>>* chunks_out = nullptr;
  // cv_decode_emissions* (f64 only; the caller has checked the options, emissions_opts_ok): the
  // emissions of every element come from this dense array instead of the handle's b through
  // obs_dev (ignored, may be null); each chunk's rows are staged beside its delta rows
  const EmisSrc* emis = nullptr;
  // cv_decode_batch[_device] only: the f64 trellis may keep sparse low planes (tuning key
  // t64_lo_every) and records the resolver's counters (cv_last_t64_stats)
  bool batch_api = false;
};
// Core device-side decode (decode.cpp).  All pointers are device pointers except offsets_host.
cv_status decode_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host, const int64_t* offsets_dev,
                        const int32_t* obs_dev, const cv_opts& o, int32_t* path_dev, double* score_dev,
                        uint8_t* status_dev, hipStream_t stream, const DecodeReq& rq = DecodeReq{});
// Host-pointer decode (decode.cpp); the caller holds h->mu and has selected the device.
cv_status decode_host_locked(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs, cv_opts o,
                             int32_t* path_out, double* score_out, uint8_t* status_out, bool obs_staged = false,
                             bool forced_staged = false, bool batch_api = false);

// CV_EINFEASIBLE for the first sequence of a fetched batch with status CV_SEQ_INFEASIBLE:
// "sequence <s> <what>".
cv_status report_infeasible(int64_t nseq, const uint8_t* status, const char* what);

// One host-pointer batch call (cv_decode_batch, cv_posterior_batch, cv_kbest_batch,
// cv_decode_emissions, cv_posterior_emissions) through the handle's staging buffers; the caller
// holds h->mu and has selected the device.  stage() checks the caller's arrays and only then enqueues the copies from
// them; the entry runs its core on the st_* buffers and fetches the results.  obs / path / forced
// are indexed by absolute element offset: the element slice is [base, total).
struct HostBatch {
  cv_hmm* h;
  int64_t nseq;
  const int64_t* offsets;
  const int32_t* obs;  // null: this call stages no observations
  hipStream_t stream;
  int64_t base = 0, total = 0;
  hipError_t err = hipSuccess;  // of the result copies (finish)

  size_t plane() const { return (size_t)std::max<int64_t>(total, 1); }

  // Sizes st_path (`planes` element planes), st_score (`width` per sequence) and st_status too.
  // check_obs: the host range check (decode only; posterior and K-best report CV_SEQ_BADOBS from
  // the device).  forced_host: o.forced is the caller's host array -> checked, staged and
  // rewritten to the device copy (false: it is a validated device array already).
  cv_status stage(cv_opts& o, size_t planes, size_t width, bool check_obs = false, bool forced_host = true) {
    cv_status st = check_batch(nseq, offsets);
    if (st != CV_OK) return st;
    base = offsets[0], total = offsets[nseq];
    const int32_t* ob = check_obs ? obs : nullptr;
    const int32_t* fr = forced_host ? o.forced : nullptr;
    const int64_t V = h->V, N = h->N;
    int64_t k;
    if (ob && (k = first_bad(base, total, [&](int64_t i) { return ob[i] < 0 || ob[i] >= V; })) >= 0)
      return set_err(CV_EINVAL, "obs[%lld] = %d out of range [0,%lld)", (long long)k, ob[k], (long long)V);
    if (fr && (k = first_bad(base, total, [&](int64_t i) { return fr[i] < -1 || fr[i] >= N; })) >= 0)
      return set_err(CV_EINVAL, "forced[%lld] = %d out of range [-1,%d)", (long long)k, fr[k], h->N);
    if ((st = h->st_off.ensure((size_t)(nseq + 1) * 8)) != CV_OK) return st;
    if (obs && (st = h->st_obs.ensure(plane() * 4)) != CV_OK) return st;
    if (planes && (st = h->st_path.ensure(plane() * planes * 4)) != CV_OK) return st;
    if ((st = h->st_score.ensure((size_t)nseq * width * 8)) != CV_OK) return st;
    if ((st = h->st_status.ensure((size_t)nseq)) != CV_OK) return st;
    if (fr && (st = h->st_forced.ensure(plane() * 4)) != CV_OK) return st;
    HIP_TRY(hipMemcpyAsync(h->st_off.p, offsets, (size_t)(nseq + 1) * 8, hipMemcpyHostToDevice, stream));
    const size_t n = (size_t)(total - base) * 4;
    if (obs && n) HIP_TRY(hipMemcpyAsync(h->st_obs.as<int32_t>() + base, obs + base, n, hipMemcpyHostToDevice, stream));
    if (fr && n) HIP_TRY(hipMemcpyAsync(h->st_forced.as<int32_t>() + base, fr + base, n, hipMemcpyHostToDevice, stream));
    if (fr) o.forced = h->st_forced.as<int32_t>();
    return CV_OK;
  }
  // After stage(): the caller's dense emission rows (cv_decode_emissions, cv_posterior_emissions),
  // the N scores of each row compact on the device (the columns beyond N are never read).
  cv_status stage_emis(const double* emis, int64_t ld, EmisSrc* src) {
    const int64_t N = h->N, rows = total - base;
    cv_status st = h->st_emis.ensure((size_t)std::max<int64_t>(rows, 1) * N * 8);
    if (st != CV_OK) return st;
    if (rows > 0)
      HIP_TRY(hipMemcpy2DAsync(h->st_emis.p, (size_t)N * 8, emis + base * ld, (size_t)ld * 8, (size_t)N * 8,
                               (size_t)rows, hipMemcpyHostToDevice, stream));
    // row e of the staging at p + e * N: the staging holds the elements from `base` on
    *src = EmisSrc{rebased(h->st_emis.as<const double>(), base, (size_t)N), N};
    return CV_OK;
  }
  // a failed core's work is waited for before the caller sees its status
  cv_status fail(cv_status st) const {
    (void)hipStreamSynchronize(stream);
    return st;
  }
  // the element slice of plane r of buf (`width` T per element) -> the same slice of out
  template <typename T>
  void fetch_elems(T* out, const DevBuf& buf, size_t width = 1, size_t r = 0) {
    const size_t at = (r * (size_t)total + (size_t)base) * width, n = (size_t)(total - base) * width * sizeof(T);
    if (err == hipSuccess && n) err = hipMemcpyAsync(out + at, buf.as<T>() + at, n, hipMemcpyDeviceToHost, stream);
  }
  // nseq items of `width` T
  template <typename T>
  void fetch_seqs(T* out, const DevBuf& buf, size_t width = 1) {
    if (err == hipSuccess) err = hipMemcpyAsync(out, buf.p, (size_t)nseq * width * sizeof(T), hipMemcpyDeviceToHost, stream);
  }
  // n T from a device address of the staging
  template <typename T>
  void fetch_n(T* out, const T* dev, size_t n) {
    if (err == hipSuccess) err = hipMemcpyAsync(out, dev, n * sizeof(T), hipMemcpyDeviceToHost, stream);
  }
  // the results are in the caller's arrays
  cv_status finish() {
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    return err == hipSuccess ? CV_OK : set_err(CV_EDEVICE, "copying the results back failed: %s", hipGetErrorString(err));
  }
};

}  // namespace cvi
