// decode.cpp -- the decode entries of the C ABI (include/cviterbi.h): cv_decode_batch,
// cv_kbest_batch, cv_decode_emissions and their _device twins, cv_viterbi_decode, the certified
// first passes of the exact f64 batch decode (cv_last_fixed_first_stats, cv_last_first_pass_kind,
// cv_f32ru_trace*) and cv_last_t64_stats.
//
// One core, decode_device, in four parts: the choice (plan_decode: options and model -> the arm
// that runs, with every option check), the layout (lay_out: chunks, workspace, order, sparse low
// planes), a forward and a backtrack step per arm, and the chunk loop.  The loop's protocol --
// the f0 / f1 / b0 / b1 events of a chunk, the forward of chunk k + 1 beside the backtrack of
// chunk k out of a double-buffered workspace -- is run_chunks, which the first passes share
// (fixed_first_decode); the integer and the round-up pass are one chunk body over FixPass /
// RuPass.  The constrained decode, the chain and the solver (cviterbi.cpp) enter through
// decode_device and DecodeReq.  The handle and the shared scaffolding: handle.hpp.
//
// There is deliberately no CPU decode path here: every decode runs the HIP kernels
// in kernels/trellis.hip and fails with CV_EDEVICE if no gfx950 device is usable.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <type_traits>
#include <utility>
#include <vector>

#include "batchplan.hpp"
#include "handle.hpp"
#include "kernels/emis.h"
#include "kernels/kbest.h"
#include "kernels/trellis.h"
#include "kernels/trellis64.h"

using namespace cvi;

namespace {

// The batch of a call: device pointers except offsets_host.
struct Batch {
  int64_t nseq;
  const int64_t* offsets_host;
  const int64_t* offsets_dev;
  const int32_t* obs_dev;
};
// Where its results go (device).
struct Results {
  int32_t* path;
  double* score;
  uint8_t* status;
};

// ---- the pipelined chunk protocol ------------------------------------------------------------
// Chunk ci records its four events ev[4 ci ...] = f0, f1 (around its forward pass, on `stream`)
// and b0, b1 (around its backtrack, on `bts`).  Not serial: bts is a second stream, the backtrack
// of chunk ci waits for f1 and runs beside the forward of chunk ci + 1, which reuses the workspace
// half of chunk ci - 1 and so waits for that chunk's b1; `stream` joins the last b1 at the end.
// Serial: bts is `stream` and nothing waits.
struct ChunkPipe {
  hipStream_t stream, bts;
  bool serial;
  const hipEvent_t* ev;
  size_t nchunks;
  bool* bts_pending = nullptr;  // the caller's failure join of bts, if it keeps one: work is on bts that `stream` has not joined
  int64_t* done = nullptr;      // chunks run so far
};

// forward(ci) between f0 and f1, staged(ci) right after f1, backtrack(ci) between b0 and b1.
template <typename Fwd, typename Staged, typename Bt>
cv_status run_chunks(const ChunkPipe& p, Fwd&& forward, Staged&& staged, Bt&& backtrack) {
  cv_status st;
  for (size_t ci = 0; ci < p.nchunks; ++ci) {
    const hipEvent_t f0 = p.ev[4 * ci], f1 = p.ev[4 * ci + 1], b0 = p.ev[4 * ci + 2], b1 = p.ev[4 * ci + 3];
    if (!p.serial && ci >= 2) HIP_TRY(hipStreamWaitEvent(p.stream, p.ev[4 * (ci - 2) + 3], 0));  // buffer reuse
    HIP_TRY(hipEventRecord(f0, p.stream));
    if ((st = forward(ci)) != CV_OK) return st;
    HIP_TRY(hipEventRecord(f1, p.stream));
    if ((st = staged(ci)) != CV_OK) return st;
    if (!p.serial) {
      HIP_TRY(hipStreamWaitEvent(p.bts, f1, 0));
      if (p.bts_pending) *p.bts_pending = true;
    }
    HIP_TRY(hipEventRecord(b0, p.bts));
    if ((st = backtrack(ci)) != CV_OK) return st;
    HIP_TRY(hipEventRecord(b1, p.bts));
    if (p.done) *p.done = (int64_t)ci + 1;
  }
  // the caller's stream sees every chunk complete
  if (!p.serial) {
    HIP_TRY(hipStreamWaitEvent(p.stream, p.ev[4 * (p.nchunks - 1) + 3], 0));
    if (p.bts_pending) *p.bts_pending = false;
  }
  return CV_OK;
}

// Work enqueued on a second stream is joined by the caller's stream later in the call; if the call
// fails before that, it is waited for here, so no kernel of a failed call is left running on a
// stream the caller does not see.
struct StreamJoin {
  hipStream_t s;
  bool pending = false;
  ~StreamJoin() {
    if (pending) (void)hipStreamSynchronize(s);
  }
};

// The fields every "f64 fold along the path" argument set shares (RescoreArgs, FixScoreArgs,
// RuScoreArgs).
template <typename Args>
void fold_fields(const cv_hmm* h, const Batch& bt, const int32_t* path, Args* ra) {
  ra->path = path;
  ra->obs = bt.obs_dev;
  ra->offsets = bt.offsets_dev;
  ra->nstates = h->N;
  ra->pi64 = h->d_pi64.as<double>();
  ra->a64 = h->d_a64.as<double>();
  ra->et64 = h->d_et64.as<double>();
}

// ---- dense emissions -------------------------------------------------------------------------
// What a decode kernel reads its emissions through: row et + obs[e] * stride, obs[e] < nobs.
struct EmisView {
  const double* et;
  const int32_t* obs;
  int nobs;
};

// Stages the dense rows of the chunk of sequences c (elements [e0, e1)) at the table stride of
// the kernel that will decode them: `staged` ([e1 - e0][stride] f64, 16-byte aligned) takes the
// rows and idx[e - e0] = e - e0 ([e1 - e0] int32); both must live until the chunk's backtrack has
// run.  emis_prepare_f64 (emis.hip) runs on `stream`; a NaN or +inf sets status BADOBS.
cv_status stage_emissions(const cv_hmm* h, const EmisSrc& src, const Batch& bt, const cvplan::Chunk& c, int stride,
                          double* staged, int32_t* idx, uint8_t* status_dev, hipStream_t stream) {
  const int64_t e0 = bt.offsets_host[c.first], e1 = bt.offsets_host[c.second];
  if (e1 - e0 > INT32_MAX) return set_err(CV_ELIMIT, "chunk of %lld elements of dense emissions", (long long)(e1 - e0));
  cvem::EmisPrepArgs g{};
  g.src = src.p;
  g.ld = src.ld;
  g.e0 = e0;
  g.nrows = e1 - e0;
  g.nstates = h->N;
  g.stride = stride;
  g.dst = staged;
  g.idx = idx;
  g.offsets = bt.offsets_dev;
  g.seq_begin = c.first;
  g.seq_end = c.second;
  g.status = status_dev;
  const hipError_t err = cvem::launch_emis_prepare(g, h->cus, stream);
  if (err != hipSuccess) return set_err(CV_EDEVICE, "emission staging launch failed: %s", hipGetErrorString(err));
  return CV_OK;
}

// The resolver's counters as cv_last_t64_stats reports them, from the pinned copy: lo_every,
// events, scans, rows descended, dense replays, self-check mismatches, largest need-set,
// sequences (zeros before the first such call has finished).
void t64_stats_sum(const cv_hmm* h, int64_t (&out)[8]) {
  for (int64_t& v : out) v = 0;
  const volatile uint64_t* p = static_cast<const volatile uint64_t*>(h->t64_stats_pin.p);
  if (!p) return;
  for (int sl = 0; sl < cvk::kT64StatSlots; ++sl) {
    const volatile uint64_t* w = p + (size_t)sl * cvk::kT64StatWords;
    out[1] += (int64_t)w[cvk::T64_STAT_EVENTS];
    out[2] += (int64_t)w[cvk::T64_STAT_SCANS];
    out[3] += (int64_t)w[cvk::T64_STAT_LEVELS];
    out[4] += (int64_t)w[cvk::T64_STAT_OVERFLOWS];
    out[5] += (int64_t)w[cvk::T64_STAT_MISMATCHES];
    out[6] = std::max<int64_t>(out[6], (int64_t)w[cvk::T64_STAT_MAXNEED]);
  }
  const volatile uint64_t* meta = p + (size_t)cvk::kT64StatSlots * cvk::kT64StatWords;
  out[0] = (int64_t)(meta[0] & 0xffffffffu);
  out[7] = (int64_t)(meta[1] & 0xffffffffu);
}
constexpr size_t kT64StatBytes = (size_t)(cvk::kT64StatSlots + 1) * cvk::kT64StatWords * 8;

// ---- decode_device, part 1: the choice -------------------------------------------------------
enum class Arm {
  kTrellis,      // f32 trellis, a workgroup per sequence or pair: trellis_fwd[2]_f32 + backtrack
  kTrellisWave,  // f32 trellis, N <= 64: one wave per sequence, forward and backtrack fused
  kT64,          // exact f64 trellis: trellis_fwd_f64 + backtrack_f64
  kT64Cp,        // its CP form: trellis_cp_f64 (argmax in the forward pass) + generic_backtrack<double>
  kGeneric64,    // generic f64 kernels
  kGeneric32,    // generic f32 kernels
};

struct DecodePlan {
  Arm arm = Arm::kGeneric64;
  bool gen_rows = false;    // generic: the delta rows kept, argmax recomputed along the path (psi mode otherwise)
  bool gen_global = false;  // generic: wide (two rows per sequence in global memory, states over many workgroups)
  bool serial = false;      // the chunks back to back on one stream
  int group = 1;            // sequences per forward workgroup of the f32 trellis
  bool cert_fused = false;  // the chain's certificates inside the f64 backtrack, no second pass
  int32_t kernel = 0, np = 0, mt = -1;  // what last_kernel / last_np / last_mt report

  bool trellis() const { return arm == Arm::kTrellis || arm == Arm::kTrellisWave; }
  bool t64() const { return arm == Arm::kT64 || arm == Arm::kT64Cp; }
  bool f64() const { return t64() || arm == Arm::kGeneric64; }
  int real_bytes() const { return f64() ? 8 : 4; }
};

// (handle, options, nseq, request) -> the arm that runs, with every option check in the order a
// caller can observe.  Between the checks it fetches and checks the offsets (bt->offsets_host, into
// off_copy when the caller gave none) and builds the tables the arm reads.
cv_status plan_decode(cv_hmm* h, const cv_opts& o, const DecodeReq& rq, Batch* bt, std::vector<int64_t>& off_copy,
                      hipStream_t stream, DecodePlan* plan) {
  DecodePlan& p = *plan;
  const int64_t nseq = bt->nseq;
  if (o.dtype != CV_DTYPE_F32 && o.dtype != CV_DTYPE_F64) return set_err(CV_EINVAL, "bad dtype %d", o.dtype);
  if (o.assoc < CV_ASSOC_VITERBI || o.assoc > CV_ASSOC_DECODE) return set_err(CV_EINVAL, "bad assoc %d", o.assoc);
  const bool trellis_ok = o.dtype == CV_DTYPE_F32 && o.assoc == CV_ASSOC_VITERBI &&
                          cvk::trellis_padded_states(h->N) != 0;
  bool use_trellis;
  if (o.kernel == CV_KERNEL_TRELLIS) {
    if (!trellis_ok)
      return set_err(CV_EUNSUPPORTED, "trellis kernel needs dtype f32, assoc VITERBI and N <= 256");
    use_trellis = true;
  } else if (o.kernel == CV_KERNEL_GENERIC || o.kernel == CV_KERNEL_AUTO || o.kernel == CV_KERNEL_TRELLIS_F64) {
    use_trellis = o.kernel == CV_KERNEL_AUTO && trellis_ok;
  } else {
    return set_err(CV_EINVAL, "bad kernel %d", o.kernel);
  }
  // exact f64, row-A0 association, N <= 256, no forced states: trellis_fwd_f64 (one wave per
  // S sequences) unless the generic kernel is asked for
  // VITERBI (row A0), DECODE (row 0 = 0.0) and DP ((a + b) + d) share trellis_fwd_f64 +
  // backtrack_f64; CP runs
  // trellis_cp_f64 (argmax in the forward pass) + generic_backtrack<double>
  // forced states / resume rows (the constrained decode): row A0 only (trellis_fwd_f64 EXT)
  // 256 < N <= 512 (cvk::t64_batch_states): VITERBI (forced states too) / DECODE / DP, where
  // the padded NP = 512 trellis beats the generic kernels: N >= 384 or >= 8,192 sequences
  // (4,096 x 128: N = 384 15.3 vs 15.8 ms, N = 320 15.4 vs 12.3; 16,384 x 128: N = 320 34.1
  // vs 46.7 ms, N = 512 35.8 vs 84.0 -- profiles/r04_large_n.txt); CV_T64_512=1 forces it
  // What the f64 trellis SUPPORTS (an explicit CV_KERNEL_TRELLIS_F64 request gets it) is wider
  // than what AUTO picks: 256 < N <= 512 only for N >= 384 or >= 8,192 sequences, 512 < N <=
  // 1,024 only above N = 724 (cvk::t64_batch_states; the generic kernels win below)
  const bool t512_pick = h->tuning.t64_512 == 1 || h->N >= 384 || nseq >= 8192;
  const bool small_ok = (o.assoc == CV_ASSOC_VITERBI || o.assoc == CV_ASSOC_DECODE || o.assoc == CV_ASSOC_CP ||
                         o.assoc == CV_ASSOC_DP) &&
                        (!(o.forced || rq.resume_rows) || o.assoc == CV_ASSOC_VITERBI) && cvk::t64_padded_states(h->N) != 0;
  const bool big_ok = cvk::t64_support_states(h->N) >= 512 &&
                      (o.assoc == CV_ASSOC_VITERBI || ((o.assoc == CV_ASSOC_DECODE || o.assoc == CV_ASSOC_DP) && !o.forced)) &&
                      !rq.resume_rows && !rq.cp_init && !rq.cp_last;
  const bool big_pick = cvk::t64_batch_states(h->N) >= 512 && (t512_pick || h->N > 512);
  const bool t64_ok = o.dtype == CV_DTYPE_F64 && (small_ok || big_ok);
  if (o.kernel == CV_KERNEL_TRELLIS_F64 && !t64_ok)
    return set_err(CV_EUNSUPPORTED,
                   "f64 trellis kernel needs dtype f64 and N <= 1024; above N = 256 only the VITERBI, DECODE and DP "
                   "associations, forced states only with VITERBI (N=%d, assoc %d)",
                   h->N, o.assoc);
  const bool use_t64 = !use_trellis && t64_ok &&
                       (o.kernel == CV_KERNEL_TRELLIS_F64 ||
                        (o.kernel == CV_KERNEL_AUTO && !(o.flags & CV_FLAG_NO_T64) && (small_ok || big_pick)));
  // above generic_max_states (10,240 f64 / 20,480 f32) the generic decode runs wide (two rows
  // per sequence in global memory, states over many workgroups, psi mode); psi is u16
  if (!use_trellis && !use_t64 && h->N > cvk::kGenericGlobalMaxStates)
    return set_err(CV_EUNSUPPORTED, "N=%d exceeds the generic kernel's u16 back-pointer range (N <= %d)", h->N,
                   cvk::kGenericGlobalMaxStates);
  const bool f64 = o.dtype == CV_DTYPE_F64;
  // (the chain's certificates read the rows mode's rows: no wide decode for them below the limit)
  p.gen_global = !use_trellis && !use_t64 &&
                 (h->N > cvk::generic_max_states(f64 ? 8 : 4) ||
                  (!rq.cp_cert && cvk::generic_wide(h->N, f64 ? 8 : 4, nseq, o.assoc == CV_ASSOC_CP)));

  cv_status st = host_offsets(nseq, bt->offsets_host, bt->offsets_dev, off_copy, stream);
  if (st != CV_OK) return st;

  const bool need_f64 = (o.rescore_f64 && !f64) || f64;
  if (use_trellis && (st = ensure_trellis_tables(h)) != CV_OK) return st;
  if (need_f64 && (st = ensure_f64_tables(h)) != CV_OK) return st;
  if (!use_trellis && !f64 && (st = ensure_g32_tables(h)) != CV_OK) return st;
  if (use_t64 && (st = ensure_t64_tables(h)) != CV_OK) return st;

  // CV_FLAG_MFMA_TRELLIS (bit 0) and the MFMA tile bits 8-15 belonged to the retired
  // MFMA-assisted f32 trellis (slower than the all-VALU one on gfx950: DESIGN.md §3)
  if ((o.flags & 0x1u) || ((o.flags >> 8) & 0xFF))
    return set_err(CV_EUNSUPPORTED, "the MFMA-assisted trellis was retired (flags 0x%x)", o.flags);
  // N <= 64: one wave per sequence, forward and backtrack fused (trellis_wave_f32) on tables
  // padded to npw = 16 * ceil(N / 16); its chunks run back to back on one stream (nothing to
  // overlap)
  const bool wave = use_trellis && h->npw > 0 && !(o.flags & CV_FLAG_NO_WAVE);
  p.arm = use_trellis ? (wave ? Arm::kTrellisWave : Arm::kTrellis)
          : use_t64   ? (o.assoc == CV_ASSOC_CP ? Arm::kT64Cp : Arm::kT64)
                      : (f64 ? Arm::kGeneric64 : Arm::kGeneric32);
  p.kernel = use_trellis ? CV_KERNEL_TRELLIS : use_t64 ? CV_KERNEL_TRELLIS_F64 : CV_KERNEL_GENERIC;
  p.np = use_trellis ? (wave ? h->npw : h->np) : use_t64 ? h->np64 : 0;
  p.mt = p.gen_global ? 0 : -1;  // GENERIC: 0 = wide (states over workgroups)
  // generic kernels: rows mode (the delta rows, argmax recomputed along the path) for every
  // association but CP (whose values need the argmax in the forward pass); A/B knob
  // tuning key generic_rows = 0 (psi mode, bit-identical).  4,096 x 128 sequences:
  // N = 300 14.9 -> 11.5 ms, N = 512 28.7 -> 21.5 ms, N = 1,024 163 -> 139 ms
  // (profiles/r04_large_n.txt)
  p.gen_rows = !use_trellis && !use_t64 && !p.gen_global && o.assoc != CV_ASSOC_CP && h->tuning.generic_rows != 0;
  // Chunks (contiguous in the original order) are pipelined over two streams: the forward
  // pass of chunk k+1 runs while chunk k backtracks, out of a double-buffered workspace.
  // At least ~2,048 sequences per chunk (8 per CU), at most 8 chunks unless the
  // workspace cap forces more.
  // t64 runs serial: its 212-VGPR forward waves fill each SIMD exactly twice per launch and
  // saturate the VALU; a co-running backtrack cost more than it hid (config 4: 159.8 ms with a
  // persistent one-wave-per-SIMD backtrack vs 152.4 ms serial, profiles/r02_ab_t64_overlap.txt)
  p.serial = (o.flags & CV_FLAG_SERIAL) != 0 || wave || use_t64 || rq.side_ws;
  // Sequences per forward workgroup: 2 (trellis_fwd2_f32, equal-length pairs; default) or 1
  // (trellis_fwd_f32: leftovers, N not a multiple of 64).
  const bool plain = use_trellis && !wave && cvk::trellis_pair_supported(h->np);
  p.group = (!plain || (o.flags & CV_FLAG_NO_PAIR)) ? 1 : 2;
  // the parallel chain's certificates inside the backtrack (NONPOS row A0, NP <= 256; dense
  // emissions may be positive: the general f64 interval test): no second pass over every row
  // (tuning key chain_cert_fused = 0: the cp_cert_f64 pass)
  p.cert_fused = p.arm == Arm::kT64 && rq.cp_cert && h->t64_nonpos && !rq.emis && o.assoc != CV_ASSOC_DP &&
                 o.assoc != CV_ASSOC_DECODE && h->np64 <= 256 && h->tuning.chain_cert_fused != 0;
  return CV_OK;
}

// ---- part 2: the layout ----------------------------------------------------------------------
// The chunks of a call and what each gets of the workspace: buffer half b of ws.main holds a
// chunk's rows ([max_elems] x bytes per element), then one staging area (two under emis_overlap)
// of dense emission rows ([max_elems][estride] f64) and their index array; half b of ws.last its
// last rows (generic kernels, f64 CP trellis).
struct DecodeLayout {
  std::vector<cvplan::Chunk> chunks;
  std::vector<int64_t> npair;  // group == 2: chunk slots [first, first + 2 npair) hold equal-length pairs
  bool varlen = false;
  bool eov = false;  // tuning key emis_overlap engaged
  int nbuf = 1, estride = 0;
  size_t rows_bytes = 0, stage_bytes = 0, idx_bytes = 0, buf_bytes = 0, last_bytes = 0;
  int64_t max_seqs = 0;
  const int32_t* order_dev = nullptr;
  bool t64_stats_on = false;  // cv_last_t64_stats follows this call
  int lo_every = 1;           // sparse low planes of the f64 trellis rows
};

cv_status lay_out(cv_hmm* h, const DecodeWs& ws, const cv_opts& o, const DecodeReq& rq, const Batch& bt,
                  const DecodePlan& p, hipStream_t stream, DecodeLayout* layout) {
  DecodeLayout& l = *layout;
  const EmisSrc* const emis = rq.emis;
  const bool use_t64 = p.t64();
  const int64_t* offsets_host = bt.offsets_host;
  cv_status st;
  // Per-element workspace bytes: trellis keeps f32 delta rows [NP]; generic keeps u16 psi [N].
  // f64 trellis: 2 KiB of delta per element at N = 256 and >= 16,384 sequences per launch for
  // 8 sequences per wave, so its default cap is larger (HBM3E: 288 GB per GPU)
  const uint64_t cap = o.workspace_bytes ? o.workspace_bytes
                                         : default_workspace_cap(ws.main.bytes, use_t64 ? kDefaultWorkspaceT64 : kDefaultWorkspace);
  // (an option check, here because it has always followed the status memset of a non-empty call)
  if (rq.cp_cert && !use_t64 && !(p.gen_rows && p.f64()))
    return set_err(CV_EUNSUPPORTED, "chain certificates need the f64 trellis or the generic kernels' rows mode");
  if (p.gen_rows && (st = p.f64() ? ensure_at64(h) : ensure_at32(h)) != CV_OK) return st;
  const uint64_t per_elem = p.trellis() ? (uint64_t)p.np * 4
                           : p.arm == Arm::kT64 ? (uint64_t)h->np64 * 8
                           : p.gen_rows ? (uint64_t)h->N * p.real_bytes()
                                        : (uint64_t)h->N * 2;
  // dense emissions: a chunk's staged rows [elements][estride] f64 and its index array follow
  // its delta rows in the same buffer, so the cap covers them and they live as long
  l.estride = use_t64 ? h->np64 : h->N;
  const uint64_t stage_per_elem = emis ? (uint64_t)l.estride * 8 + 4 : 0;
  const int v = h->tuning.max_chunks;  // tuning key max_chunks (bit-identical): pipeline depth
  const uint64_t max_chunks = (uint64_t)(v >= 1 && v <= 64 ? v : 8);
  // the batch split under the cap at per_elem_all workspace bytes per element
  auto split = [&](const uint64_t per_elem_all) {
    cvplan::split_pipelined(offsets_host, bt.nseq,
                            {per_elem_all, cap, p.serial, max_chunks, (use_t64 ? 64 : p.group) * (int64_t)std::max(h->cus, 1)},
                            l.chunks);
  };
  split(per_elem + stage_per_elem);
  // Tuning key emis_overlap = 1 (bit-identical; off by default): dense emissions on the f64
  // trellis (its chunks run back to back on one stream), more than one chunk: chunk k+1 is staged
  // on the second stream beside chunk k's forward pass -- the staging is bound by bandwidth, the
  // forward by the VALU -- into a SECOND staging buffer, so the batch is split again with 8P + 4
  // bytes per element more under the same cap (a batch that fits one chunk is never split for
  // it).  12,288 x 512 at N = 256: 2% faster at three chunks each, but under one cap the finer
  // split decides: 57.0 vs 39.8 ms and 38.8 vs 49.3 ms at two caps (profiles/emissions_bench.txt)
  l.eov = emis && use_t64 && !rq.side_ws && l.chunks.size() > 1 && h->tuning.emis_overlap != 0;
  if (l.eov) split(per_elem + 2 * stage_per_elem);
  const cvplan::Shares largest = cvplan::measure(offsets_host, l.chunks);
  const uint64_t max_elems = std::max<uint64_t>(largest.max_elems, 1);
  l.max_seqs = largest.max_seqs;
  l.nbuf = (l.chunks.size() > 1 && !p.serial) ? 2 : 1;
  l.varlen = cvplan::varlen(offsets_host, bt.nseq);
  auto up256 = [](uint64_t n) { return (size_t)((n + 255) / 256 * 256); };
  l.rows_bytes = up256(max_elems * per_elem);
  l.stage_bytes = emis ? up256(max_elems * l.estride * 8) : 0;
  l.idx_bytes = emis ? up256(max_elems * 4) : 0;
  l.buf_bytes = l.rows_bytes + (l.eov ? 2 : 1) * (l.stage_bytes + l.idx_bytes);
  // gen_global: each sequence's two rows follow the chunk's last rows ([max_seqs][2][N])
  l.last_bytes = ((size_t)l.max_seqs * h->N * p.real_bytes() * (p.gen_global ? 3 : 1) + 255) / 256 * 256;
  if ((st = ws.main.ensure(l.buf_bytes * l.nbuf)) != CV_OK) return st;
  if (!p.trellis() && (st = ws.last.ensure(l.last_bytes * l.nbuf)) != CV_OK) return st;
  const bool pairing = p.group == 2;
  l.npair.assign(l.chunks.size(), 0);
  if (l.varlen) {
    // longest-first schedule inside each chunk so the tail of the grid is short sequences;
    // with pairing, equal-length neighbours are paired first and leftovers go last
    ws.order_host.resize((size_t)bt.nseq);
    cvplan::longest_first(offsets_host, l.chunks, ws.order_host.data(), pairing ? l.npair.data() : nullptr, h->sort_pos);
    if ((st = upload_order(ws.order, ws.order_pin, ws.order_host.data(), bt.nseq, stream, &l.order_dev)) != CV_OK)
      return st;
  }

  // Sparse low planes (trellis64.h row contract): only where the forward and the backtrack are
  // the plain NONPOS row-A0 pair and nothing else reads the rows -- no forced states, resume rows,
  // chain certificates or chunk events, dense emissions, DPSolver / viterbi::decode rows -- at
  // NP = 128 / 192 / 256.  Every other decode writes and reads full rows.
  l.t64_stats_on = rq.batch_api && p.arm == Arm::kT64 && !rq.side_ws;
  if (l.t64_stats_on) {
    if (!h->t64_stats_pin.p) {
      if (!h->t64_stats_pin.ensure(kT64StatBytes)) return set_err(CV_ENOMEM, "pinned f64 trellis counters failed");
      std::memset(h->t64_stats_pin.p, 0, kT64StatBytes);
    }
    if ((st = h->t64_stats.ensure(kT64StatBytes)) != CV_OK) return st;
    int64_t last[8];
    t64_stats_sum(h, last);  // the previous call's counters if it has finished (no wait: else older ones)
    if (last[0] > 1 && (last[4] * 64 > last[7] || last[5] > 0)) h->t64_lo_off = true;
    const bool plain_pair = o.assoc == CV_ASSOC_VITERBI && !o.forced && !rq.resume_rows && !rq.cp_cert && !rq.cp_init &&
                            !rq.cp_last && !rq.chunks_out && !emis && h->t64_nonpos &&
                            (h->np64 == 128 || h->np64 == 192 || h->np64 == 256);
    if (plain_pair && !h->t64_lo_off)
      l.lo_every = std::min(std::max(h->tuning.t64_lo_every, 1), cvk::kT64LoEveryMax);
    HIP_TRY(hipMemsetAsync(h->t64_stats.p, 0, kT64StatBytes, stream));
    uint32_t* meta = h->t64_stats.as<uint32_t>() + (size_t)cvk::kT64StatSlots * cvk::kT64StatWords * 2;
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(meta), l.lo_every, 1, stream));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(meta + 2), (int)bt.nseq, 1, stream));
  }
  return CV_OK;
}

// ---- part 3: a forward and a backtrack step per arm ------------------------------------------
// What a step reads of the call ...
struct DecodeCall {
  cv_hmm* h;
  const cv_opts& o;
  const DecodeReq& rq;
  Batch bt;
  Results out;
  const DecodePlan& plan;
  const DecodeLayout& lay;
};
// ... and of the chunk it runs, by value.
struct ChunkRun {
  cvplan::Chunk c;      // its sequences (slots of the order) [first, second)
  int64_t n;            // how many
  int64_t elem_base;    // the element its rows start at
  int64_t npairs;       // f32 trellis: equal-length pairs at the front of the chunk
  unsigned char* rows;  // its half of ws.main
  unsigned char* last;  // its half of ws.last
  double* stage_rows;   // dense emissions: its staged rows and their index array ...
  int32_t* stage_idx;
  EmisView ev;          // ... which replace (table, obs_dev, V) in its kernels
  hipStream_t stream, bts;
  int bt_reserve;       // LDS the backtrack reserves so that one workgroup per CU runs beside the next forward
};

ChunkRun chunk_run(const DecodeCall& d, const DecodeWs& ws, size_t ci, hipStream_t stream, hipStream_t bts) {
  const DecodeLayout& l = d.lay;
  ChunkRun k{};
  k.c = l.chunks[ci];
  k.n = k.c.second - k.c.first;
  k.elem_base = d.bt.offsets_host[k.c.first];
  k.npairs = d.plan.group == 2 ? (l.varlen ? l.npair[ci] : k.n / 2) : 0;
  const size_t buf = l.nbuf == 2 ? ci % 2 : 0;
  k.rows = ws.main.as<unsigned char>() + buf * l.buf_bytes;
  k.last = ws.last.as<unsigned char>() + buf * l.last_bytes;
  if (d.rq.emis) {
    unsigned char* sb = k.rows + l.rows_bytes + (l.eov ? ci % 2 : 0) * (l.stage_bytes + l.idx_bytes);
    k.stage_rows = reinterpret_cast<double*>(sb);
    k.stage_idx = reinterpret_cast<int32_t*>(sb + l.stage_bytes);
    // the kernels index obs by absolute element
    k.ev = EmisView{k.stage_rows, rebased<const int32_t>(k.stage_idx, k.elem_base),
                    (int)(d.bt.offsets_host[k.c.second] - k.elem_base)};
  }
  k.stream = stream;
  k.bts = bts;
  // overlap mode: at most ONE backtrack workgroup (one 64-VGPR wave per SIMD) per CU, so
  // the next forward workgroup (4 waves x 104 VGPRs per SIMD) always
  // finds its registers free: reserve 100 KiB of LDS (2 x 100 > 160 KiB)
  // the last chunk's backtrack has the device to itself: full occupancy
  k.bt_reserve = (d.plan.serial || ci + 1 == l.chunks.size()) ? 0 : 100 * 1024;
  return k;
}

cvk::BacktrackArgs trellis_bt_args(const DecodeCall& d, const ChunkRun& k) {
  const cv_hmm* h = d.h;
  cvk::BacktrackArgs ba{};
  ba.delta = reinterpret_cast<const float*>(k.rows);
  ba.delta_elem_base = k.elem_base;
  ba.at = h->t_at.as<float>();
  ba.offsets = d.bt.offsets_dev;
  ba.obs = d.bt.obs_dev;
  ba.order = d.lay.order_dev;
  ba.seq_begin = k.c.first;
  ba.seq_end = k.c.second;
  ba.nstates = h->N;
  ba.path = d.out.path;
  ba.score = d.out.score;
  ba.score32 = nullptr;
  ba.status = d.out.status;
  return ba;
}

hipError_t forward_trellis(const DecodeCall& d, const ChunkRun& k) {
  const cv_hmm* h = d.h;
  cvk::TrellisFwdArgs fa{};
  fa.a_img = h->t_aimg.as<float>();
  fa.pi = h->t_pi.as<float>();
  fa.et = h->t_et.as<float>();
  fa.offsets = d.bt.offsets_dev;
  fa.obs = d.bt.obs_dev;
  fa.order = d.lay.order_dev;
  fa.seq_begin = k.c.first;
  fa.delta = reinterpret_cast<float*>(k.rows);
  fa.delta_elem_base = k.elem_base;
  fa.status = d.out.status;
  fa.nobs = (int)h->V;
  fa.forced = d.o.forced;
  fa.resume_rows = static_cast<const float*>(d.rq.resume_rows);
  if (d.plan.arm == Arm::kTrellisWave) {
    fa.a_img = h->w_arm.as<float>();
    fa.pi = h->w_pi.as<float>();
    fa.et = h->w_et.as<float>();
    cvk::BacktrackArgs ba = trellis_bt_args(d, k);
    ba.at = h->w_at.as<float>();
    return cvk::launch_trellis_wave(h->npw, fa, ba, k.n, k.stream);
  }
  hipError_t err = cvk::launch_trellis_fwd2(h->np, fa, k.npairs, k.stream);
  if (err == hipSuccess && k.n > 2 * k.npairs) {
    fa.seq_begin = k.c.first + 2 * k.npairs;
    err = cvk::launch_trellis_fwd(h->np, fa, k.n - 2 * k.npairs, k.stream);
  }
  return err;
}

// wave: the backtrack ran fused with the forward
hipError_t backtrack_trellis(const DecodeCall& d, const ChunkRun& k) {
  const cv_hmm* h = d.h;
  hipError_t err = d.plan.arm == Arm::kTrellisWave
                       ? hipSuccess
                       : cvk::launch_trellis_bt(h->np, trellis_bt_args(d, k), k.n, k.bts, k.bt_reserve);
  if (err == hipSuccess && d.o.rescore_f64) {
    cvk::RescoreArgs ra{};
    fold_fields(h, d.bt, d.out.path, &ra);
    ra.order = d.lay.order_dev;
    ra.seq_begin = k.c.first;
    ra.seq_end = k.c.second;
    ra.status = d.out.status;
    ra.score = d.out.score;
    err = cvk::launch_rescore_f64(ra, k.n, k.bts, k.bt_reserve);
  }
  return err;
}

// kT64 and kT64Cp; sets what last_mt reports of the launch
hipError_t forward_t64(const DecodeCall& d, const ChunkRun& k) {
  cv_hmm* h = d.h;
  const cv_opts& o = d.o;
  const bool t64cp = d.plan.arm == Arm::kT64Cp, side_ws = d.rq.side_ws;
  const int64_t n = k.n;
  cvk::T64FwdArgs fa{};
  fa.a = h->q_a.as<double>();
  fa.pi = h->q_pi.as<double>();
  fa.et = h->q_et.as<double>();
  fa.offsets = d.bt.offsets_dev;
  fa.obs = d.bt.obs_dev;
  fa.order = d.lay.order_dev;
  fa.seq_begin = k.c.first;
  fa.nslots = n;
  fa.delta = reinterpret_cast<double*>(k.rows);
  fa.delta_elem_base = k.elem_base;
  fa.status = d.out.status;
  fa.nobs = (int)h->V;
  fa.zero_init = o.assoc == CV_ASSOC_DECODE ? 1 : 0;
  fa.dp_assoc = o.assoc == CV_ASSOC_DP ? 1 : 0;
  fa.forced = o.forced;
  fa.resume_rows = static_cast<const double*>(d.rq.resume_rows);
  fa.lo_every = d.lay.lo_every;
  if (d.rq.emis) fa.et = k.ev.et, fa.obs = k.ev.obs, fa.nobs = k.ev.nobs;
  const int spw = cvk::t64_seqs_per_wave(n, h->cus, h->np64);
  // the S actually launched: CP / DP, NP = 1,024 and forced NP = 512 run S <= 4 (launch_t64_fwd)
  if (!side_ws)
    h->last_mt = t64cp ? cvk::t64_cp_seqs_per_wave(spw, n, cvk::t64_cp_waves(h->np64, n))
                       : (fa.dp_assoc || h->np64 == 1024 || (h->np64 == 512 && o.forced)) ? std::min(spw, 4) : spw;
  {  // eight-wave workgroups: equal lengths (within 1/8), or >= 2 rounds of 64 x CUs
     // (ragged T in [32, 1024], chunks of 32,768: 158 vs 168 ms; one round, 16,384: 65.5
     // vs 56 ms -- profiles/r03_ab_wg.txt)
    int64_t tmin = INT64_MAX, tmax = 0;
    for (int64_t sq = k.c.first; sq < k.c.second; ++sq) {
      const int64_t T = d.bt.offsets_host[sq + 1] - d.bt.offsets_host[sq];
      tmin = std::min(tmin, T);
      tmax = std::max(tmax, T);
    }
    fa.wg_ok = (8 * tmin >= 7 * tmax || n >= 2 * 64 * (int64_t)std::max(h->cus, 1)) ? 1 : 0;
  }
  fa.nstates = h->N;  // (kT64: the N <= 48 one-wave kernel, the few-sequence layout)
  if (t64cp) {
    fa.psi = reinterpret_cast<uint16_t*>(k.rows);
    fa.last_row = reinterpret_cast<double*>(k.last);
    fa.cp_init = d.rq.cp_init;  // the parallel chain's speculative re-decodes (start offsets)
    fa.cp_last = d.rq.cp_last;
    return cvk::launch_t64_cp_fwd(h->np64, spw, fa, n, k.stream);
  }
  if (!side_ws && cvk::t64_few_launch(h->np64, fa, n)) h->last_mt = 0;
  return cvk::launch_t64_fwd(h->np64, spw, fa, n, k.stream);
}

// the f64 trellis backtrack of one chunk (backtrack_f64)
hipError_t backtrack_t64(const DecodeCall& d, const ChunkRun& k) {
  const cv_hmm* h = d.h;
  const cv_opts& o = d.o;
  cvk::T64BtArgs ba{};
  ba.delta = reinterpret_cast<const double*>(k.rows);
  ba.delta_elem_base = k.elem_base;
  ba.at = h->q_at.as<double>();
  ba.offsets = d.bt.offsets_dev;
  ba.order = d.lay.order_dev;
  ba.seq_begin = k.c.first;
  ba.seq_end = k.c.second;
  ba.nstates = h->N;
  ba.path = d.out.path;
  ba.score = d.out.score;  // the f64 delta is already the reference score: no re-score
  ba.status = d.out.status;
  ba.dp_assoc = o.assoc == CV_ASSOC_DP ? 1 : 0;
  ba.decode_bt = o.assoc == CV_ASSOC_DECODE ? 1 : 0;
  ba.obs = d.bt.obs_dev;
  ba.et = h->q_et.as<double>();
  ba.at32 = h->t64_nonpos ? h->q_at32.as<float>() : nullptr;
  ba.lo_every = d.lay.lo_every;
  ba.a = h->q_a.as<double>();
  ba.stats = h->t64_stats.as<unsigned long long>();
  if (d.rq.emis) {  // densities may be positive: the general f64 interval test
    ba.at32 = nullptr;
    ba.et = k.ev.et, ba.obs = k.ev.obs;
  }
  if (d.plan.cert_fused) {
    ba.cert = d.rq.cp_cert;
    ba.rho_cap = h->cert_rho_cap;
  }
  return cvk::launch_t64_bt(h->np64, ba, k.n, k.bts);
}

// The tables of the generic kernels by real type.
template <typename REAL>
struct GenericTables {
  const REAL *pi, *a, *et, *at;
};
template <typename REAL>
GenericTables<REAL> generic_tables(const cv_hmm* h) {
  if constexpr (std::is_same_v<REAL, double>)
    return {h->d_pi64.as<double>(), h->d_a64.as<double>(), h->d_et64.as<double>(), h->d_at64.as<double>()};
  else
    return {h->d_pi32.as<float>(), h->d_a32.as<float>(), h->d_et32.as<float>(), h->d_at32.as<float>()};
}

template <typename REAL>
hipError_t forward_generic(const DecodeCall& d, const ChunkRun& k) {
  const cv_hmm* h = d.h;
  const GenericTables<REAL> tab = generic_tables<REAL>(h);
  cvk::GenericFwdArgs<REAL> fa{};
  fa.a = tab.a;
  fa.pi = tab.pi;
  fa.et = tab.et;
  fa.offsets = d.bt.offsets_dev;
  fa.obs = d.bt.obs_dev;
  fa.order = d.lay.order_dev;
  fa.seq_begin = k.c.first;
  fa.nstates = h->N;
  fa.nobs = (int)h->V;
  fa.assoc = d.o.assoc;
  fa.psi = reinterpret_cast<uint16_t*>(k.rows);
  fa.psi_elem_base = k.elem_base;
  fa.last_row = reinterpret_cast<REAL*>(k.last);
  fa.status = d.out.status;
  fa.forced = d.o.forced;
  if constexpr (std::is_same_v<REAL, double>) {
    fa.cp_init = d.rq.cp_init;  // the parallel chain's speculative re-decodes (N > 256)
    fa.cp_last = d.rq.cp_last;
    if (d.rq.emis) fa.et = k.ev.et, fa.obs = k.ev.obs, fa.nobs = k.ev.nobs;
  }
  if (d.plan.gen_rows) fa.rows = reinterpret_cast<REAL*>(k.rows);
  if (d.plan.gen_global) {  // wide: the chunk's rows after its last rows, one launch per step
    fa.grows = reinterpret_cast<REAL*>(k.last) + (size_t)d.lay.max_seqs * h->N;
    for (int64_t sq = k.c.first; sq < k.c.second; ++sq)
      fa.wide_steps = std::max<int64_t>(fa.wide_steps, d.bt.offsets_host[sq + 1] - d.bt.offsets_host[sq]);
  }
  return cvk::launch_generic_fwd<REAL>(fa, k.n, k.stream);
}

// the generic kernels', and behind the f64 CP trellis (psi mode)
template <typename REAL>
hipError_t backtrack_generic(const DecodeCall& d, const ChunkRun& k) {
  const cv_hmm* h = d.h;
  const GenericTables<REAL> tab = generic_tables<REAL>(h);
  cvk::GenericBtArgs<REAL> ba{};
  ba.psi = reinterpret_cast<const uint16_t*>(k.rows);
  ba.psi_elem_base = k.elem_base;
  ba.last_row = reinterpret_cast<const REAL*>(k.last);
  ba.offsets = d.bt.offsets_dev;
  ba.order = d.lay.order_dev;
  ba.seq_begin = k.c.first;
  ba.seq_end = k.c.second;
  ba.nstates = h->N;
  ba.path = d.out.path;
  ba.score = d.out.score;
  ba.status = d.out.status;
  ba.obs = d.bt.obs_dev;
  // the f64 kernel's own score is already reference numerics
  ba.rescore_f64 = (std::is_same_v<REAL, float> && d.o.rescore_f64) ? 1 : 0;
  ba.decode_bt = d.o.assoc == CV_ASSOC_DECODE ? 1 : 0;
  ba.pi64 = h->d_pi64.as<double>();
  ba.a64 = h->d_a64.as<double>();
  ba.et64 = h->d_et64.as<double>();
  if (d.plan.gen_rows) {
    ba.rows = reinterpret_cast<const REAL*>(k.rows);
    ba.at = tab.at;
    ba.et = tab.et;
    ba.assoc = d.o.assoc;
    ba.nobs = (int)h->V;
  }
  if constexpr (std::is_same_v<REAL, double>)
    if (d.rq.emis) ba.et64 = ba.et = k.ev.et, ba.obs = k.ev.obs, ba.nobs = k.ev.nobs;
  return d.plan.gen_rows ? cvk::launch_generic_bt_rows<REAL>(ba, k.n, k.bts) : cvk::launch_generic_bt<REAL>(ba, k.n, k.bts);
}

// The chain's certificate pass over the chunk's f64 rows and paths, by the a^T table of its kernel:
// the f64 trellis's padded one, or the plain one of the generic rows mode (N > 256).
hipError_t certify(const DecodeCall& d, const ChunkRun& k) {
  const cv_hmm* h = d.h;
  const bool t64 = d.plan.arm == Arm::kT64;
  cvk::CpCert64Args ca{};
  ca.delta = reinterpret_cast<const double*>(k.rows);
  ca.delta_elem_base = k.elem_base;
  ca.at = t64 ? h->q_at.as<double>() : h->d_at64.as<double>();
  ca.offsets = d.bt.offsets_dev;
  ca.order = d.lay.order_dev;
  ca.seq_begin = k.c.first;
  ca.seq_end = k.c.second;
  ca.nstates = h->N;
  ca.path = d.out.path;
  ca.status = d.out.status;
  ca.out = d.rq.cp_cert;
  return t64 ? cvk::launch_cp_cert(h->np64, ca, k.bts) : cvk::launch_cp_cert_plain(ca, k.bts);
}

hipError_t forward(const DecodeCall& d, const ChunkRun& k) {
  switch (d.plan.arm) {
    case Arm::kTrellis:
    case Arm::kTrellisWave: return forward_trellis(d, k);
    case Arm::kT64:
    case Arm::kT64Cp: return forward_t64(d, k);
    case Arm::kGeneric64: return forward_generic<double>(d, k);
    default: return forward_generic<float>(d, k);
  }
}

hipError_t backtrack(const DecodeCall& d, const ChunkRun& k) {
  switch (d.plan.arm) {
    case Arm::kTrellis:
    case Arm::kTrellisWave: return backtrack_trellis(d, k);
    case Arm::kT64: return backtrack_t64(d, k);
    case Arm::kT64Cp:
    case Arm::kGeneric64: return backtrack_generic<double>(d, k);
    default: return backtrack_generic<float>(d, k);
  }
}

}  // namespace

// ---- part 4: the loop ------------------------------------------------------------------------
// Core device-side decode.  All pointers are device pointers except offsets_host.
cv_status cvi::decode_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host, const int64_t* offsets_dev,
                             const int32_t* obs_dev, const cv_opts& o, int32_t* path_dev, double* score_dev,
                             uint8_t* status_dev, hipStream_t stream, const DecodeReq& rq) {
  const bool side_ws = rq.side_ws;
  const EmisSrc* const emis = rq.emis;
  const DecodeWs ws = decode_ws(h, side_ws);
  Batch bt{nseq, offsets_host, offsets_dev, obs_dev};
  std::vector<int64_t> off_copy;
  DecodePlan plan;
  cv_status st = plan_decode(h, o, rq, &bt, off_copy, stream, &plan);
  if (st != CV_OK) return st;
  int64_t launches_done = 0;
  if (!side_ws) {
    h->last_launches = 0;
    h->last_kernel = plan.kernel;
    h->last_np = plan.np;
    h->last_mt = plan.mt;
  }
  if (nseq == 0) return CV_OK;
  // the workspace of the previous call on this handle may still be in use on another stream
  if (ws.ws_rec) HIP_TRY(hipStreamWaitEvent(stream, ws.ws_done, 0));
  HIP_TRY(hipMemsetAsync(status_dev, 0, (size_t)nseq, stream));
  DecodeLayout lay;
  if ((st = lay_out(h, ws, o, rq, bt, plan, stream, &lay)) != CV_OK) return st;
  const DecodeCall d{h, o, rq, bt, Results{path_dev, score_dev, status_dev}, plan, lay};

  const hipStream_t bts = plan.serial ? stream : h->bt_stream;
  const size_t nchunks = lay.chunks.size(), nev = 4 * nchunks;
  size_t eb;
  if ((st = reserve_events(h, side_ws, nev, &eb)) != CV_OK) return st;
  // a staging pass enqueued on the second stream (emis_overlap) is joined by the forward pass of
  // its chunk; see StreamJoin
  StreamJoin stage_join{h->bt_stream};
  auto stage = [&](const ChunkRun& k, hipStream_t s) {
    return stage_emissions(h, *emis, bt, k.c, lay.estride, k.stage_rows, k.stage_idx, status_dev, s);
  };
  ChunkPipe pipe{stream, bts, plan.serial, &ws.ev[eb], nchunks};
  pipe.done = side_ws ? &launches_done : &h->last_launches;
  st = run_chunks(
      pipe,
      [&](size_t ci) -> cv_status {
        const ChunkRun k = chunk_run(d, ws, ci, stream, bts);
        if (lay.eov && ci > 0) {  // staged beside the previous chunk's forward
          HIP_TRY(hipStreamWaitEvent(stream, h->emis_ev[ci], 0));
          stage_join.pending = false;
        } else if (emis) {
          const cv_status se = stage(k, stream);
          if (se != CV_OK) return se;
        }
        const hipError_t err = forward(d, k);
        if (err != hipSuccess) return set_err(CV_EDEVICE, "forward launch failed: %s", hipGetErrorString(err));
        return CV_OK;
      },
      [&](size_t ci) -> cv_status {
        if (!lay.eov || ci + 1 >= nchunks) return CV_OK;
        // chunk ci - 1 has finished with the other staging buffer at f0
        if (!get_event(h->emis_ev, ci + 1)) return set_err(CV_EDEVICE, "hipEventCreate failed");
        HIP_TRY(hipStreamWaitEvent(h->bt_stream, pipe.ev[4 * ci], 0));
        stage_join.pending = true;
        const cv_status se = stage(chunk_run(d, ws, ci + 1, stream, bts), h->bt_stream);
        if (se != CV_OK) return se;
        HIP_TRY(hipEventRecord(h->emis_ev[ci + 1], h->bt_stream));
        return CV_OK;
      },
      [&](size_t ci) -> cv_status {
        const ChunkRun k = chunk_run(d, ws, ci, stream, bts);
        hipError_t err = backtrack(d, k);
        // DecodeReq::chunks_out: the chunk's paths are written at this point of `bts`
        if (err == hipSuccess && plan.f64() && rq.chunks_out) {
          hipEvent_t ce = get_event(h->chunk_ev, rq.chunks_out->size());
          if (!ce) return set_err(CV_EDEVICE, "hipEventCreate failed");
          HIP_TRY(hipEventRecord(ce, bts));
          rq.chunks_out->push_back(k.c);
        }
        if (err == hipSuccess && plan.f64() && rq.cp_cert && !plan.cert_fused) err = certify(d, k);
        if (err != hipSuccess) return set_err(CV_EDEVICE, "backtrack launch failed: %s", hipGetErrorString(err));
        return CV_OK;
      });
  if (st != CV_OK) return st;
  if (lay.t64_stats_on)  // the counters follow the last backtrack (t64 chunks run on `stream`); nobody waits for them
    HIP_TRY(hipMemcpyAsync(h->t64_stats_pin.p, h->t64_stats.p, kT64StatBytes, hipMemcpyDeviceToHost, stream));
  return end_call(h, side_ws, nev, stream);
}

namespace {

// ---- K-best (list) Viterbi: cv_kbest_batch* ---------------------------------------------------
// Core of cv_kbest_batch*: all pointers are device pointers except offsets_host.  Chunks of whole
// sequences (original order) whose u16 back-pointers (N * KT * 2 bytes per element) fit the
// workspace cap run forward, select and walk on `stream`.
cv_status kbest_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host, const int64_t* offsets_dev,
                       const int32_t* obs_dev, int32_t k, const cv_opts& o, int32_t* path_dev, double* score_dev,
                       int32_t* count_dev, uint8_t* status_dev, hipStream_t stream) {
  if (o.dtype == CV_DTYPE_F32) return set_err(CV_EUNSUPPORTED, "the K-best path is f64 only");
  if (o.dtype != CV_DTYPE_F64) return set_err(CV_EINVAL, "bad dtype %d", o.dtype);
  if (o.assoc != CV_ASSOC_VITERBI)
    return set_err(CV_EINVAL, "the K-best path covers the VITERBI association only (assoc %d)", o.assoc);
  if (o.kernel != CV_KERNEL_AUTO && o.kernel != CV_KERNEL_GENERIC)
    return set_err(CV_EINVAL, "K-best kernel must be AUTO or GENERIC (kernel %d)", o.kernel);
  if (k < 1 || k > cvkb::kKbestMaxK) return set_err(CV_EINVAL, "k = %d outside [1, %d]", k, cvkb::kKbestMaxK);
  const int N = h->N, KT = cvkb::kbest_width(k);
  if (N > cvkb::kKbestMaxStates)
    return set_err(CV_EUNSUPPORTED, "the K-best kernels cover N <= %d (N=%d)", cvkb::kKbestMaxStates, N);
  if (N * KT > cvkb::kKbestMaxCells)
    return set_err(CV_EUNSUPPORTED, "the K-best kernels cover N * KT <= %d (N=%d, k=%d: list width KT=%d)",
                   cvkb::kKbestMaxCells, N, k, KT);
  std::vector<int64_t> off_copy;
  cv_status st = host_offsets(nseq, offsets_host, offsets_dev, off_copy, stream);
  if (st != CV_OK) return st;
  if ((st = ensure_f64_tables(h)) != CV_OK) return st;
  const int S = cvkb::kbest_seqs_per_wg(N, KT, nseq);
  h->last_launches = 0;
  h->last_kernel = CV_KERNEL_GENERIC;
  h->last_np = KT;
  h->last_mt = S;
  if (nseq == 0) return CV_OK;
  if (h->ws_rec) HIP_TRY(hipStreamWaitEvent(stream, h->ws_done, 0));
  HIP_TRY(hipMemsetAsync(status_dev, 0, (size_t)nseq, stream));

  const uint64_t per_elem = (uint64_t)N * KT * 2;
  const uint64_t cap = o.workspace_bytes ? o.workspace_bytes : default_workspace_cap(h->kb_bp.bytes, kDefaultWorkspace);
  const uint64_t elem_cap = cap / per_elem;
  for (int64_t s = 0; s < nseq; ++s) {
    const uint64_t T = (uint64_t)(offsets_host[s + 1] - offsets_host[s]);
    if (T > elem_cap)
      return set_err(CV_ENOMEM, "sequence %lld needs %llu bytes of back-pointers (T=%llu, N=%d, KT=%d), workspace cap %llu",
                     (long long)s, (unsigned long long)(T * per_elem), (unsigned long long)T, N, KT,
                     (unsigned long long)cap);
  }
  std::vector<cvplan::Chunk> chunks;
  const cvplan::Shares largest = cvplan::split_equal_shares(offsets_host, nseq, elem_cap, chunks);
  if ((st = h->kb_bp.ensure((size_t)std::max<uint64_t>(largest.max_elems, 1) * per_elem)) != CV_OK) return st;
  if ((st = h->kb_last.ensure((size_t)largest.max_seqs * N * KT * 8)) != CV_OK) return st;
  if ((st = h->kb_end.ensure((size_t)nseq * k * 4)) != CV_OK) return st;
  // longest first inside each chunk (stable), so a workgroup's sequences have similar lengths
  const int32_t* order_dev = nullptr;
  if (cvplan::varlen(offsets_host, nseq)) {
    if (nseq > INT32_MAX) return set_err(CV_EINVAL, "too many sequences (%lld)", (long long)nseq);
    h->order_host.resize((size_t)nseq);
    cvplan::longest_first(offsets_host, chunks, h->order_host.data(), nullptr, h->sort_pos);
    if ((st = upload_order(h->kb_order, h->kb_pin, h->order_host.data(), nseq, stream, &order_dev)) != CV_OK) return st;
  }
  const size_t nev = 4 * chunks.size();
  size_t eb;
  if ((st = reserve_events(h, false, nev, &eb)) != CV_OK) return st;
  for (size_t ci = 0; ci < chunks.size(); ++ci) {
    const auto& c = chunks[ci];
    cvkb::KbestArgs g{};
    g.pi = h->d_pi64.as<double>();
    g.a = h->d_a64.as<double>();
    g.et = h->d_et64.as<double>();
    g.offsets = offsets_dev;
    g.obs = obs_dev;
    g.forced = o.forced;
    g.order = order_dev;
    g.seq_begin = c.first;
    g.seq_end = c.second;
    g.elem_base = offsets_host[c.first];
    g.nstates = N;
    g.nobs = (int)h->V;
    g.k = k;
    g.kt = KT;
    g.bp = h->kb_bp.as<uint16_t>();
    g.last = h->kb_last.as<double>();
    g.end = h->kb_end.as<int32_t>();
    g.plane = offsets_host[nseq];
    g.path = path_dev;
    g.score = score_dev;
    g.count = count_dev;
    g.status = status_dev;
    hipEvent_t f0 = h->ev[eb + 4 * ci], f1 = h->ev[eb + 4 * ci + 1], b0 = h->ev[eb + 4 * ci + 2], b1 = h->ev[eb + 4 * ci + 3];
    HIP_TRY(hipEventRecord(f0, stream));
    hipError_t err = cvkb::launch_kbest_fwd(g, S, stream);
    if (err != hipSuccess) return set_err(CV_EDEVICE, "K-best forward launch failed: %s", hipGetErrorString(err));
    HIP_TRY(hipEventRecord(f1, stream));
    HIP_TRY(hipEventRecord(b0, stream));
    err = cvkb::launch_kbest_select(g, stream);
    if (err == hipSuccess) err = cvkb::launch_kbest_walk(g, stream);
    if (err != hipSuccess) return set_err(CV_EDEVICE, "K-best select / walk launch failed: %s", hipGetErrorString(err));
    HIP_TRY(hipEventRecord(b1, stream));
    h->last_launches = (int64_t)ci + 1;
  }
  return end_call(h, false, nev, stream);
}

// ---- certified fixed-point first pass of the exact f64 batch decode -------------------------
// (tuning key t64_fixed_first; DESIGN.md "Certified fixed-point first pass")
int32_t fix_quantise(double x) {  // max(rint(x / q), F); -inf -> F.  x <= 0
  const double r = std::nearbyint(std::ldexp(x, -cvk::kFixQLog2));
  return r > (double)cvk::kFixFloor ? (int32_t)r : cvk::kFixFloor;
}

// The register image of ensure_trellis_tables (a_img) of the entries A(i, j).
template <typename T, typename F>
std::vector<T> trellis_image(int np, F&& A) {
  const int R = np / 8;
  std::vector<T> img((size_t)np * np);
  for (int w = 0; w < np / 16; ++w)
    for (int q = 0; q < R / 2; ++q)
      for (int lane = 0; lane < 64; ++lane) {
        const int rg = lane & 7, cp = lane >> 3, j0 = 16 * w + 2 * cp, r0 = rg * R + 2 * q;
        T* dst = &img[(((size_t)w * (R / 2) + q) * 64 + lane) * 4];
        dst[0] = A(r0, j0);
        dst[1] = A(r0, j0 + 1);
        dst[2] = A(r0 + 1, j0);
        dst[3] = A(r0 + 1, j0 + 1);
      }
  return img;
}

// W: the largest finite |pi| + |a| + |b|, what the f64 recurrence's rounding per step scales with
double model_wmax(const cv_hmm* h) {
  double wmax = 0.0;
  for (const std::vector<double>* v : {&h->pi, &h->a, &h->b}) {
    double m = 0.0;
    for (double x : *v)
      if (std::isfinite(x)) m = std::max(m, std::fabs(x));
    wmax += m;
  }
  return wmax;
}

// The int32 tables, once per handle.  fx_state = 0: the model is outside the pass's range (a
// positive entry, or a padded state count the integer pair kernel does not cover).
cv_status ensure_fix_tables(cv_hmm* h) {
  if (h->fx_state >= 0) return CV_OK;
  const int np = cvk::trellis_padded_states(h->N);
  if (!cvk::fix_supported(np) || !model_nonpos(h)) {
    h->fx_state = 0;
    return CV_OK;
  }
  const int N = h->N;
  const int64_t V = h->V;
  const int32_t F = cvk::kFixFloor;
  auto A = [&](int i, int j) -> int32_t { return (i < N && j < N) ? fix_quantise(h->a[(size_t)i * N + j]) : F; };
  const std::vector<int32_t> img = trellis_image<int32_t>(np, A);
  std::vector<int32_t> pi((size_t)np, F), at((size_t)np * np, F), et((size_t)V * np, F);
  for (int j = 0; j < N; ++j) pi[(size_t)j] = fix_quantise(h->pi[(size_t)j]);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) at[(size_t)j * np + i] = A(i, j);
  parallel_ranges(N, [&](int, int64_t lo, int64_t hi) {
    for (int64_t j = lo; j < hi; ++j)
      for (int64_t o = 0; o < V; ++o) et[(size_t)o * np + j] = fix_quantise(h->b[(size_t)j * V + o]);
  }, std::max<int64_t>(1, 4096 / std::max<int64_t>(V, 1)));
  // the f64 recurrence's own rounding, which a certificate has to cover besides the quantisation:
  // at step t at most 2.02 u (t + 1) W; in units of q and summed over the steps it stays below
  // gain * (t + 1)^2
  h->fx_gain = 1.01 * 2.02 * std::ldexp(1.0, -53 - cvk::kFixQLog2) * model_wmax(h);
  cv_status st;
  if ((st = upload(h->fx_aimg, img.data(), img.size() * 4)) != CV_OK) return st;
  if ((st = upload(h->fx_pi, pi.data(), pi.size() * 4)) != CV_OK) return st;
  if ((st = upload(h->fx_at, at.data(), at.size() * 4)) != CV_OK) return st;
  if ((st = upload(h->fx_et, et.data(), et.size() * 4)) != CV_OK) return st;
  h->fx_state = 1;
  return CV_OK;
}

// ---- certified f32 round-up first pass (tuning key t64_f32ru_first) ------------------------
// The smallest float >= x + y, the real sum: the two-sum gives the f64 add's exact remainder.
// (tools/probe_f32ru.py ru_sum64; the tables hold no +inf and no NaN)
float ru_sum32(double x, double y) {
  const double s = x + y;
  if (!std::isfinite(s)) return (float)s;
  const double bb = s - x;
  const double e = (x - (s - bb)) + (y - bb);
  float f = (float)s;
  if ((double)f < s || ((double)f == s && e > 0.0)) f = std::nextafter(f, std::numeric_limits<float>::infinity());
  return f;
}
double ru_grid(double x) {  // a multiple of 2^-16 near x; a maximum of -inf alone -> 0
  return std::isfinite(x) ? std::nearbyint(x * 65536.0) / 65536.0 : 0.0;
}

// The shifted f32 tables, once per handle (DESIGN.md "Certified f32 round-up first pass"):
// ca_j = grid(max_i a[i,j]), a' = RU(a - ca_j), cb_o = grid(max_j (b[j,o] + ca_j)),
// b'' = RU(b + (ca_j - cb_o)), pi' = RU(pi - ca_j).  ru_state = 0: outside the pass's range.
cv_status ensure_ru_tables(cv_hmm* h) {
  if (h->ru_state >= 0) return CV_OK;
  const int np = cvk::trellis_padded_states(h->N);
  if (!cvk::fix_supported(np) || !model_nonpos(h)) {
    h->ru_state = 0;
    return CV_OK;
  }
  const int N = h->N;
  const int64_t V = h->V;
  const float ninf = -std::numeric_limits<float>::infinity();
  std::vector<double> ca((size_t)N), cb((size_t)V);
  for (int j = 0; j < N; ++j) {
    double m = -INFINITY;
    for (int i = 0; i < N; ++i) m = std::max(m, h->a[(size_t)i * N + j]);
    ca[(size_t)j] = ru_grid(m);
  }
  for (int64_t o = 0; o < V; ++o) {
    double m = -INFINITY;
    for (int j = 0; j < N; ++j) m = std::max(m, h->b[(size_t)j * V + o] + ca[(size_t)j]);
    cb[(size_t)o] = ru_grid(m);
  }
  double smax = 0.0;
  for (double x : ca) smax = std::max(smax, std::fabs(x));
  for (double x : cb) smax = std::max(smax, std::fabs(x));
  if (!(smax < 1073741824.0)) {  // ca - cb would not be exact on the grid
    h->ru_state = 0;
    return CV_OK;
  }
  auto A = [&](int i, int j) -> float {
    return (i < N && j < N) ? ru_sum32(h->a[(size_t)i * N + j], -ca[(size_t)j]) : ninf;
  };
  const std::vector<float> img = trellis_image<float>(np, A);
  std::vector<float> pi((size_t)np, ninf), at((size_t)np * np, ninf), et((size_t)V * np, ninf);
  for (int j = 0; j < N; ++j) pi[(size_t)j] = ru_sum32(h->pi[(size_t)j], -ca[(size_t)j]);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) at[(size_t)j * np + i] = A(i, j);
  parallel_ranges(N, [&](int, int64_t lo, int64_t hi) {
    for (int64_t j = lo; j < hi; ++j)
      for (int64_t o = 0; o < V; ++o)
        et[(size_t)o * np + j] = ru_sum32(h->b[(size_t)j * V + o], ca[(size_t)j] - cb[(size_t)o]);
  }, std::max<int64_t>(1, 4096 / std::max<int64_t>(V, 1)));
  h->ru_ks = 4.0 * std::ldexp(1.0, -53) * model_wmax(h);
  cv_status st;
  if ((st = upload(h->ru_aimg, img.data(), img.size() * 4)) != CV_OK) return st;
  if ((st = upload(h->ru_pi, pi.data(), pi.size() * 4)) != CV_OK) return st;
  if ((st = upload(h->ru_at, at.data(), at.size() * 4)) != CV_OK) return st;
  if ((st = upload(h->ru_et, et.data(), et.size() * 4)) != CV_OK) return st;
  if ((st = upload(h->ru_ca, ca.data(), ca.size() * 8)) != CV_OK) return st;
  if ((st = upload(h->ru_cb, cb.data(), cb.size() * 8)) != CV_OK) return st;
  h->ru_state = 1;
  return CV_OK;
}

// What the two first passes differ in -- tables, argument structs, launchers -- once per pass.
// args(): the three argument sets of a call with the pass's own fields filled.
struct FixPass {
  using Row = int32_t;
  cvk::FixFwdArgs fa{};
  cvk::FixBtArgs ba{};
  cvk::FixScoreArgs ra{};
  static void tables(const cv_hmm* h, cvk::FixFwdArgs* fa, cvk::FixBtArgs* ba) {
    fa->a_img = h->fx_aimg.as<int32_t>();
    fa->pi = h->fx_pi.as<int32_t>();
    fa->et = h->fx_et.as<int32_t>();
    ba->at = h->fx_at.as<int32_t>();
  }
  explicit FixPass(const cv_hmm* h) {
    tables(h, &fa, &ba);
    ba.gain = h->fx_gain;
  }
  static constexpr auto launch_fwd = cvk::launch_fix_fwd2;
  static constexpr auto launch_bt = cvk::launch_fix_bt;
  static constexpr auto launch_score = cvk::launch_fix_score;
};
struct RuPass {
  using Row = float;
  cvk::RuFwdArgs fa{};
  cvk::RuBtArgs ba{};
  cvk::RuScoreArgs ra{};
  static void tables(const cv_hmm* h, cvk::RuFwdArgs* fa, cvk::RuBtArgs* ba) {
    fa->a_img = h->ru_aimg.as<float>();
    fa->pi = h->ru_pi.as<float>();
    fa->et = h->ru_et.as<float>();
    ba->at = h->ru_at.as<float>();
  }
  explicit RuPass(const cv_hmm* h) {
    tables(h, &fa, &ba);
    ra.mu = fa.mu = h->ru_mu.as<float>();
    ra.r = ba.r = h->ru_r.as<float>();
    ra.e_last = ba.e_last = h->ru_e.as<float>();
    ra.ca = h->ru_ca.as<double>();
    ra.cb = h->ru_cb.as<double>();
    ra.ks = h->ru_ks;
  }
  static constexpr auto launch_fwd = cvk::launch_ru_fwd2;
  static constexpr auto launch_bt = cvk::launch_ru_bt;
  static constexpr auto launch_score = cvk::launch_ru_score;
};

// What fixed_first_decode has laid out for its chunks.
struct FirstPassRun {
  const std::vector<cvplan::Chunk>& chunks;
  const std::vector<int64_t>& npair;
  bool varlen;
  int np, nbuf;
  size_t buf_bytes;
  const int32_t* order_dev;
};

// The chunks of a first pass: the forward on the paired slots, then the certificate backtrack and
// the f64 fold along the candidate paths.
template <typename Pass>
cv_status first_pass_chunks(cv_hmm* h, Pass pass, const FirstPassRun& run, const Batch& bt, const Results& out,
                            const ChunkPipe& pipe) {
  uint8_t* const cert_dev = h->fx_cert.as<uint8_t>();
  pass.fa.offsets = pass.ba.offsets = bt.offsets_dev;
  pass.fa.obs = bt.obs_dev;
  pass.fa.order = pass.ba.order = run.order_dev;
  pass.fa.cert = pass.ba.cert = pass.ra.cert = cert_dev;
  pass.fa.nobs = (int)h->V;
  pass.ba.path = out.path;
  fold_fields(h, bt, out.path, &pass.ra);
  pass.ra.score = out.score;
  pass.ra.status = out.status;
  // chunk ci: its sequences, its pairs, its rows in the workspace
  struct Slot {
    cvplan::Chunk c;
    int64_t np2;
    typename Pass::Row* rows;
    int64_t row_base;
  };
  auto slot = [&](size_t ci) {
    const cvplan::Chunk c = run.chunks[ci];
    return Slot{c, run.varlen ? run.npair[ci] : (c.second - c.first) / 2,
                reinterpret_cast<typename Pass::Row*>(h->ws_main.as<unsigned char>() + (run.nbuf == 2 ? ci % 2 : 0) * run.buf_bytes),
                bt.offsets_host[c.first]};
  };
  return run_chunks(
      pipe,
      [&](size_t ci) -> cv_status {
        const Slot s = slot(ci);
        auto fa = pass.fa;
        fa.seq_begin = s.c.first;
        fa.rows = s.rows;
        fa.row_elem_base = s.row_base;
        const hipError_t err = Pass::launch_fwd(run.np, fa, s.np2, pipe.stream);
        if (err != hipSuccess) return set_err(CV_EDEVICE, "first-pass forward launch failed: %s", hipGetErrorString(err));
        return CV_OK;
      },
      [](size_t) { return CV_OK; },
      [&](size_t ci) -> cv_status {
        const Slot s = slot(ci);
        // beside the next chunk's forward: one backtrack / score workgroup per CU (launch_fix_bt); the
        // last chunk's have the device to themselves
        const int reserve = (pipe.serial || ci + 1 == pipe.nchunks) ? 0 : 100 * 1024;
        auto ba = pass.ba;
        ba.rows = s.rows;
        ba.row_elem_base = s.row_base;
        ba.seq_begin = s.c.first;
        ba.seq_end = s.c.first + 2 * s.np2;  // the paired slots: only their rows exist
        hipError_t err = Pass::launch_bt(run.np, ba, pipe.bts, reserve);
        if (err == hipSuccess) {
          auto ra = pass.ra;
          ra.seq_begin = s.c.first;
          ra.seq_end = s.c.second;
          err = Pass::launch_score(ra, pipe.bts, reserve);
        }
        if (err != hipSuccess) return set_err(CV_EDEVICE, "fixed-point backtrack launch failed: %s", hipGetErrorString(err));
        return CV_OK;
      });
}

// The plain row-A0 f64 batch decode through a certified first pass, the integer or the f32
// round-up one by the call's size and the two keys.  *done = false: the call is not
// the pass's (options, model, batch size, the handle's guard) and nothing has been written; the
// caller runs the f64 kernels.  Otherwise every sequence has its result: the certified ones from
// the integer rows (path) and the f64 fold along it (score), the others -- uncertified, unpaired,
// empty, with a bad observation -- from the f64 kernels on a compact batch, scattered back.  The
// uncertified list is read on the host, so the call waits for the stream once.
cv_status fixed_first_decode(cv_hmm* h, int64_t nseq, const int64_t* offsets_host, const int64_t* offsets_dev,
                             const int32_t* obs_dev, const cv_opts& o, int32_t* path_dev, double* score_dev,
                             uint8_t* status_dev, hipStream_t stream, bool* done) {
  *done = false;
  h->fx_last[0] = h->fx_last[1] = h->fx_last[2] = 0;
  h->fx_last[3] = h->fx_pinned ? 1 : 0;
  h->fx_last_kind = 0;
  // kRu (the f32 round-up pass) for a call of at least t64_f32ru_first elements, kFix (the integer
  // pass) for one below that and at least t64_fixed_first
  enum FirstPass { kNone = 0, kFix = 1, kRu = 2 };
  const int64_t min_fix = h->tuning.t64_fixed_first, min_ru = h->tuning.t64_f32ru_first;
  const bool fix_open = min_fix > 0 && h->fx_state != 0, ru_open = min_ru > 0 && h->ru_state != 0;
  if ((!fix_open && !ru_open) || h->fx_pinned || nseq < 2 || nseq > INT32_MAX) return CV_OK;
  if (o.dtype != CV_DTYPE_F64 || o.assoc != CV_ASSOC_VITERBI || o.forced || o.flags != 0 ||
      (o.kernel != CV_KERNEL_AUTO && o.kernel != CV_KERNEL_TRELLIS_F64))
    return CV_OK;
  std::vector<int64_t> off_copy;
  cv_status st = host_offsets(nseq, offsets_host, offsets_dev, off_copy, stream);
  if (st != CV_OK) return st;
  const int64_t elems = offsets_host[nseq] - offsets_host[0];
  FirstPass pass = kNone;
  if (ru_open && elems >= min_ru) {
    if ((st = ensure_ru_tables(h)) != CV_OK) return st;
    if (h->ru_state == 1) pass = kRu;
  }
  if (pass == kNone && fix_open && elems >= min_fix) {
    if ((st = ensure_fix_tables(h)) != CV_OK) return st;
    if (h->fx_state == 1) pass = kFix;
  }
  if (pass == kNone) return CV_OK;
  if ((st = ensure_f64_tables(h)) != CV_OK) return st;
  const int np = cvk::trellis_padded_states(h->N);

  // chunks of whole sequences under the workspace cap, 4 * np bytes of rows per element; inside a
  // chunk equal-length neighbours of the longest-first order are paired, the leftovers fall back
  const uint64_t per_elem = (uint64_t)np * 4;
  const uint64_t cap = o.workspace_bytes ? o.workspace_bytes : default_workspace_cap(h->ws_main.bytes, kDefaultWorkspaceT64);
  // Tuning key t64_fixed_chunks (bit-identical): k > 0, the default: the chunks are pipelined over
  // two streams as the f32 trellis's are -- at least min(k, nseq / 2048) of them out of a
  // double-buffered workspace, chunk k's certificate backtrack and score on bt_stream beside the
  // forward of chunk k + 1; 0: the chunks back to back on the caller's stream, one under the cap
  const int fchunks = h->tuning.t64_fixed_chunks;
  const bool one_stream = fchunks <= 0;
  std::vector<cvplan::Chunk> chunks;
  cvplan::split_pipelined(offsets_host, nseq,
                          {per_elem, cap, one_stream, one_stream ? 8u : (uint64_t)std::min(fchunks, 64),
                           2 * (int64_t)std::max(h->cus, 1)},
                          chunks);
  const cvplan::Shares largest = cvplan::measure(offsets_host, chunks);
  const bool serial = one_stream || chunks.size() == 1;  // a single chunk has no forward to run beside
  const int nbuf = serial ? 1 : 2;
  const size_t buf_bytes = ((std::max<uint64_t>(largest.max_elems, 1) * per_elem + 255) / 256) * 256;
  if ((st = h->ws_main.ensure(buf_bytes * nbuf)) != CV_OK) return st;
  if ((st = h->fx_cert.ensure((size_t)nseq)) != CV_OK) return st;
  if (!h->fx_cert_pin.ensure((size_t)nseq)) return set_err(CV_ENOMEM, "pinned certificate copy failed");
  if (h->ws_rec) HIP_TRY(hipStreamWaitEvent(stream, h->ws_done, 0));
  const bool varlen = cvplan::varlen(offsets_host, nseq);
  std::vector<int64_t> npair(chunks.size(), 0);
  const int32_t* order_dev = nullptr;
  if (varlen) {
    h->order_host.resize((size_t)nseq);
    cvplan::longest_first(offsets_host, chunks, h->order_host.data(), npair.data(), h->sort_pos);
    if ((st = upload_order(h->ws_order, h->order_pin, h->order_host.data(), nseq, stream, &order_dev)) != CV_OK) return st;
  }
  if (pass == kRu) {  // the shifts and losing candidates, by element like the path; E by sequence
    const size_t ne = (size_t)std::max<int64_t>(offsets_host[nseq], 1);
    if ((st = h->ru_mu.ensure(ne * 4)) != CV_OK) return st;
    if ((st = h->ru_r.ensure(ne * 4)) != CV_OK) return st;
    if ((st = h->ru_e.ensure((size_t)nseq * 4)) != CV_OK) return st;
  }
  HIP_TRY(hipMemsetAsync(h->fx_cert.p, 0, (size_t)nseq, stream));

  // this call's launches -- the integer chunks, then the fallback's -- are timed as one call
  const bool acc_was = h->acc_on;
  const size_t acc_base = acc_was ? h->acc_used : 0;
  if (!acc_was) h->acc_on = true, h->acc_used = 0;
  struct AccRestore {
    cv_hmm* h;
    bool was;
    ~AccRestore() {
      if (!was) h->acc_on = false, h->acc_used = 0;
    }
  } acc_restore{h, acc_was};
  const size_t nev = 4 * chunks.size();
  size_t eb;
  if ((st = reserve_events(h, false, nev, &eb)) != CV_OK) return st;
  StreamJoin bt_join{h->bt_stream};
  ChunkPipe pipe{stream, serial ? stream : h->bt_stream, serial, &h->ev[eb], chunks.size()};
  pipe.bts_pending = &bt_join.pending;
  const FirstPassRun run{chunks, npair, varlen, np, nbuf, buf_bytes, order_dev};
  const Batch bt{nseq, offsets_host, offsets_dev, obs_dev};
  const Results out{path_dev, score_dev, status_dev};
  // the caller's stream sees every chunk's paths, scores and certificates at its end
  st = pass == kRu ? first_pass_chunks(h, RuPass(h), run, bt, out, pipe) : first_pass_chunks(h, FixPass(h), run, bt, out, pipe);
  if (st != CV_OK) return st;
  if ((st = end_call(h, false, nev, stream)) != CV_OK) return st;
  HIP_TRY(hipMemcpyAsync(h->fx_cert_pin.p, h->fx_cert.p, (size_t)nseq, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));

  const uint8_t* cert = h->fx_cert_pin.as<uint8_t>();
  std::vector<int64_t>& ix = h->fx_idx_host;  // cstart [nfb], off2 [nfb + 1], perm [nfb]
  int64_t nfb = 0, nfail = 0;  // not certified; of them, the pass ran to a failed certificate (2)
  for (int64_t s = 0; s < nseq; ++s) nfb += cert[s] != 1, nfail += cert[s] == 2;
  h->fx_last[0] = 1;
  h->fx_last_kind = (int)pass;
  h->fx_last[1] = nseq - nfb;
  h->fx_last[2] = nfb;
  h->fx_last[3] = 0;
  if (nfail * 8 > nseq - nfb + nfail) {  // the guard: this model's margins are below the quantisation; f64 from now on
    h->fx_pinned = true;
    h->fx_last[1] = 0, h->fx_last[2] = nseq, h->fx_last[3] = 1;
    if (acc_was) h->acc_used = acc_base;  // the f64 decode of the whole batch is what the call reports
    return CV_OK;
  }
  *done = true;
  h->last_kernel = CV_KERNEL_TRELLIS_F64;
  h->last_np = np;
  h->last_mt = 2;
  if (nfb > 0) {
    ix.resize((size_t)(3 * nfb + 1));
    int64_t *cstart = ix.data(), *off2 = cstart + nfb, *perm = off2 + nfb + 1;
    int64_t k = 0;
    off2[0] = 0;
    for (int64_t s = 0; s < nseq; ++s)
      if (cert[s] != 1) {
        cstart[k] = offsets_host[s];
        off2[k + 1] = off2[k] + (offsets_host[s + 1] - offsets_host[s]);
        perm[k++] = s;
      }
    const int64_t elems2 = off2[nfb];
    if ((st = h->fx_idx.ensure(ix.size() * 8)) != CV_OK) return st;
    if ((st = h->fx_obs2.ensure((size_t)std::max<int64_t>(elems2, 1) * 4)) != CV_OK) return st;
    if ((st = h->fx_path2.ensure((size_t)std::max<int64_t>(elems2, 1) * 4)) != CV_OK) return st;
    if ((st = h->fx_score2.ensure((size_t)nfb * 8)) != CV_OK) return st;
    if ((st = h->fx_status2.ensure((size_t)nfb)) != CV_OK) return st;
    HIP_TRY(hipMemcpyAsync(h->fx_idx.p, ix.data(), ix.size() * 8, hipMemcpyHostToDevice, stream));
    const int64_t *d_cstart = h->fx_idx.as<int64_t>(), *d_off2 = d_cstart + nfb, *d_perm = d_off2 + nfb + 1;
    hipError_t err = cvk::launch_compact_suffix(d_cstart, d_off2, obs_dev, nullptr, nullptr, h->fx_obs2.as<int32_t>(),
                                                nullptr, nfb, stream);
    if (err != hipSuccess) return set_err(CV_EDEVICE, "fallback gather launch failed: %s", hipGetErrorString(err));
    DecodeReq rq;
    rq.batch_api = true;
    if ((st = decode_device(h, nfb, off2, d_off2, h->fx_obs2.as<int32_t>(), o, h->fx_path2.as<int32_t>(),
                            h->fx_score2.as<double>(), h->fx_status2.as<uint8_t>(), stream, rq)) != CV_OK)
      return st;
    err = cvk::launch_scatter_suffix(d_cstart, d_off2, d_perm, h->fx_path2.as<int32_t>(), h->fx_score2.as<double>(),
                                     h->fx_status2.as<uint8_t>(), path_dev, score_dev, status_dev, nfb, stream);
    if (err != hipSuccess) return set_err(CV_EDEVICE, "fallback scatter launch failed: %s", hipGetErrorString(err));
    // the fallback's buffers are read by the scatter: the next call on the handle waits for it
    if ((st = end_call(h, false, 0, stream)) != CV_OK) return st;
  }
  h->last_ev_base = acc_base;
  h->last_launches = (int64_t)((h->acc_used - acc_base) / 4);
  return CV_OK;
}

}  // namespace

// Host-pointer decode; caller holds h->mu and has selected the device.
// obs_staged: h->st_obs already holds the (validated) observations of [offsets[0],
// offsets[nseq]); forced_staged: o.forced is a validated DEVICE array indexed like obs.
cv_status cvi::decode_host_locked(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs, cv_opts o,
                                  int32_t* path_out, double* score_out, uint8_t* status_out, bool obs_staged,
                                  bool forced_staged, bool batch_api) {
  cv_status st;
  if (nseq == 0) return CV_OK;
  HostBatch hb{h, nseq, offsets, obs_staged ? nullptr : obs, o.stream ? (hipStream_t)o.stream : h->stream};
  if ((st = hb.stage(o, 1, 1, true, !forced_staged)) != CV_OK) return st;
  DecodeReq rq;
  rq.batch_api = batch_api;
  bool done = false;
  if (batch_api && !forced_staged)
    st = fixed_first_decode(h, nseq, offsets, h->st_off.as<int64_t>(), h->st_obs.as<int32_t>(), o,
                            h->st_path.as<int32_t>(), h->st_score.as<double>(), h->st_status.as<uint8_t>(), hb.stream,
                            &done);
  if (st == CV_OK && !done)
    st = decode_device(h, nseq, offsets, h->st_off.as<int64_t>(), h->st_obs.as<int32_t>(), o, h->st_path.as<int32_t>(),
                       h->st_score.as<double>(), h->st_status.as<uint8_t>(), hb.stream, rq);
  if (st != CV_OK) return hb.fail(st);
  hb.fetch_elems(path_out, h->st_path);
  hb.fetch_seqs(score_out, h->st_score);
  hb.fetch_seqs(status_out, h->st_status);
  return hb.finish();
}

namespace {

// what cv_decode_emissions* accepts of the options (no handle needed)
cv_status emissions_opts_ok(const cv_opts& o) {
  if (o.dtype == CV_DTYPE_F32) return set_err(CV_EUNSUPPORTED, "dense emissions are decoded in f64 only");
  if (o.dtype != CV_DTYPE_F64) return set_err(CV_EINVAL, "bad dtype %d", o.dtype);
  if (o.kernel == CV_KERNEL_TRELLIS)
    return set_err(CV_EUNSUPPORTED, "dense emissions: the f32 trellis kernel does not apply (AUTO, GENERIC or TRELLIS_F64)");
  return CV_OK;
}

}  // namespace

// ===================================================================================
extern "C" {

CV_API cv_status cv_decode_batch_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                        const int64_t* offsets_dev, const int32_t* obs_dev, const cv_opts* opts,
                                        int32_t* path_dev, double* score_dev, uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq > 0 && (!offsets_dev || !obs_dev || !path_dev || !score_dev || !status_dev))
    return set_err(CV_EINVAL, "null device buffer");
  CV_LOCK(h);
  cv_status st = set_device(h);
  if (st != CV_OK) return st;
  const cv_opts o = opts ? *opts : default_opts();
  hipStream_t stream = o.stream ? (hipStream_t)o.stream : h->stream;
  bool done = false;
  st = fixed_first_decode(h, nseq, offsets_host, offsets_dev, obs_dev, o, path_dev, score_dev, status_dev, stream, &done);
  if (st != CV_OK || done) return st;
  DecodeReq rq;
  rq.batch_api = true;
  return decode_device(h, nseq, offsets_host, offsets_dev, obs_dev, o, path_dev, score_dev, status_dev, stream, rq);
}

CV_API cv_status cv_decode_batch(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                 const cv_opts* opts, int32_t* path_out, double* score_out, uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || (nseq > 0 && (!offsets || !obs || !path_out || !score_out || !status_out)))
    return set_err(CV_EINVAL, "null argument");
  CV_LOCK(h);
  cv_status st = set_device(h);
  if (st != CV_OK) return st;
  return decode_host_locked(h, nseq, offsets, obs, opts ? *opts : default_opts(), path_out, score_out, status_out,
                            false, false, true);
}

CV_API cv_status cv_viterbi_decode(cv_hmm* h, int64_t T, const int32_t* obs, int32_t* path_out) {
  if (!h || T < 0 || (T > 0 && (!obs || !path_out))) return set_err(CV_EINVAL, "bad argument");
  if (T == 0) return CV_OK;
  const int64_t off[2] = {0, T};
  double score;
  uint8_t status;
  cv_opts o;
  cv_opts_init(&o);
  o.dtype = CV_DTYPE_F64;
  o.assoc = CV_ASSOC_DECODE;
  o.rescore_f64 = 0;
  return cv_decode_batch(h, 1, off, obs, &o, path_out, &score, &status);
}

CV_API cv_status cv_kbest_batch_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                       const int64_t* offsets_dev, const int32_t* obs_dev, int32_t k,
                                       const cv_opts* opts, int32_t* path_dev, double* score_dev,
                                       int32_t* count_dev, uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (k < 1 || k > cvkb::kKbestMaxK) return set_err(CV_EINVAL, "k = %d outside [1, %d]", k, cvkb::kKbestMaxK);
  if (nseq > 0 && (!offsets_dev || !obs_dev || !path_dev || !score_dev || !count_dev || !status_dev))
    return set_err(CV_EINVAL, "null device buffer");
  CV_LOCK(h);
  cv_status st = set_device(h);
  if (st != CV_OK) return st;
  const cv_opts o = opts ? *opts : default_opts();
  hipStream_t stream = o.stream ? (hipStream_t)o.stream : h->stream;
  return kbest_device(h, nseq, offsets_host, offsets_dev, obs_dev, k, o, path_dev, score_dev, count_dev, status_dev,
                      stream);
}

CV_API cv_status cv_kbest_batch(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs, int32_t k,
                                const cv_opts* opts, int32_t* path_out, double* score_out, int32_t* count_out,
                                uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (k < 1 || k > cvkb::kKbestMaxK) return set_err(CV_EINVAL, "k = %d outside [1, %d]", k, cvkb::kKbestMaxK);
  if (nseq < 0 || (nseq > 0 && (!offsets || !obs || !path_out || !score_out || !count_out || !status_out)))
    return set_err(CV_EINVAL, "null argument");
  CV_LOCK(h);
  cv_status st = set_device(h);
  if (st != CV_OK) return st;
  cv_opts o = opts ? *opts : default_opts();
  if (nseq == 0) return CV_OK;
  // the observations are range-checked on the device (CV_SEQ_BADOBS), as in the _device variant
  HostBatch hb{h, nseq, offsets, obs, o.stream ? (hipStream_t)o.stream : h->stream};
  if ((st = hb.stage(o, (size_t)k, (size_t)k)) != CV_OK) return st;
  if ((st = h->st_count.ensure((size_t)nseq * 4)) != CV_OK) return st;
  st = kbest_device(h, nseq, offsets, h->st_off.as<int64_t>(), h->st_obs.as<int32_t>(), k, o, h->st_path.as<int32_t>(),
                    h->st_score.as<double>(), h->st_count.as<int32_t>(), h->st_status.as<uint8_t>(), hb.stream);
  if (st != CV_OK) return hb.fail(st);
  for (int32_t r = 0; r < k; ++r)  // plane r of the staging and of path_out: offsets[nseq] elements each
    hb.fetch_elems(path_out, h->st_path, 1, (size_t)r);
  hb.fetch_seqs(score_out, h->st_score, (size_t)k);
  hb.fetch_seqs(count_out, h->st_count);
  hb.fetch_seqs(status_out, h->st_status);
  if ((st = hb.finish()) != CV_OK) return st;
  return report_infeasible(nseq, status_out, "has no path of finite score");
}

// ---- decode of caller-supplied emission scores: cv_decode_emissions* -------------------------
CV_API cv_status cv_decode_emissions_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                            const int64_t* offsets_dev, const double* emis_dev, int64_t ld,
                                            const cv_opts* opts, int32_t* path_dev, double* score_dev,
                                            uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (nseq > 0 && (!offsets_dev || !emis_dev || !path_dev || !score_dev || !status_dev))
    return set_err(CV_EINVAL, "null device buffer");
  if (ld < h->N) return set_err(CV_EINVAL, "ld = %lld is less than N = %d", (long long)ld, h->N);
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = emissions_opts_ok(o);
  if (st != CV_OK) return st;
  CV_LOCK(h);
  if ((st = set_device(h)) != CV_OK) return st;
  hipStream_t stream = o.stream ? (hipStream_t)o.stream : h->stream;
  const EmisSrc src{emis_dev, ld};
  DecodeReq rq;
  rq.emis = &src;
  return decode_device(h, nseq, offsets_host, offsets_dev, nullptr, o, path_dev, score_dev, status_dev, stream, rq);
}

CV_API cv_status cv_decode_emissions(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* emis, int64_t ld,
                                     const cv_opts* opts, int32_t* path_out, double* score_out, uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || (nseq > 0 && (!offsets || !emis || !path_out || !score_out || !status_out)))
    return set_err(CV_EINVAL, "null argument");
  if (ld < h->N) return set_err(CV_EINVAL, "ld = %lld is less than N = %d", (long long)ld, h->N);
  cv_opts o = opts ? *opts : default_opts();
  cv_status st = emissions_opts_ok(o);
  if (st != CV_OK) return st;
  CV_LOCK(h);
  if ((st = set_device(h)) != CV_OK) return st;
  if (nseq == 0) return CV_OK;
  HostBatch hb{h, nseq, offsets, nullptr, o.stream ? (hipStream_t)o.stream : h->stream};
  if ((st = hb.stage(o, 1, 1)) != CV_OK) return st;
  EmisSrc src;
  if ((st = hb.stage_emis(emis, ld, &src)) != CV_OK) return st;
  DecodeReq rq;
  rq.emis = &src;
  st = decode_device(h, nseq, offsets, h->st_off.as<int64_t>(), nullptr, o, h->st_path.as<int32_t>(),
                     h->st_score.as<double>(), h->st_status.as<uint8_t>(), hb.stream, rq);
  if (st != CV_OK) return hb.fail(st);
  hb.fetch_elems(path_out, h->st_path);
  hb.fetch_seqs(score_out, h->st_score);
  hb.fetch_seqs(status_out, h->st_status);
  return hb.finish();
}

// ---- what the last decode did ------------------------------------------------------------------
CV_API int32_t cv_last_t64_stats(const cv_hmm* h, int64_t* out, int32_t n) {
  if (!h || n < 0 || (n > 0 && !out)) {
    set_err(CV_EINVAL, "bad argument");
    return -1;
  }
  int64_t v[8];
  t64_stats_sum(h, v);
  for (int32_t q = 0; q < n && q < 8; ++q) out[q] = v[q];
  return 8;
}

CV_API int32_t cv_last_fixed_first_stats(const cv_hmm* h, int64_t* out, int32_t n) {
  if (!h || n < 0 || (n > 0 && !out)) {
    set_err(CV_EINVAL, "bad argument");
    return -1;
  }
  for (int32_t q = 0; q < n && q < 4; ++q) out[q] = h->fx_last[q];
  return 4;
}

CV_API int32_t cv_last_first_pass_kind(const cv_hmm* h) {
  if (!h) {
    set_err(CV_EINVAL, "null handle");
    return -1;
  }
  return h->fx_last_kind;
}

// The round-up pass's forward and certificate backtrack on nseq sequences of one length T,
// everything they store copied out: what tests compare with the numpy model bit for bit.
CV_API cv_status cv_f32ru_trace(cv_hmm* h, int64_t nseq, int64_t T, const int32_t* obs, float* rows, float* mu,
                                float* r, float* e_last, int32_t* path) {
  if (nseq < 2 || T < 1 || nseq * T > (1 << 22)) return set_err(CV_EINVAL, "bad batch shape");
  std::vector<int64_t> off((size_t)nseq + 1);
  for (int64_t s = 0; s <= nseq; ++s) off[(size_t)s] = s * T;
  return cv_f32ru_trace_ragged(h, nseq, off.data(), obs, rows, mu, r, e_last, path);
}

// The same on sequences of several lengths: sequences 2k and 2k + 1 are a pair and have one length.
CV_API cv_status cv_f32ru_trace_ragged(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                       float* rows, float* mu, float* r, float* e_last, int32_t* path) {
  if (!h || !offsets || !obs || !rows || !mu || !r || !e_last || !path) return set_err(CV_EINVAL, "null argument");
  if (nseq < 2 || nseq > (1 << 22) || offsets[0] != 0) return set_err(CV_EINVAL, "bad batch shape");
  for (int64_t s = 0; s < nseq; ++s) {
    const int64_t len = offsets[s + 1] - offsets[s];
    if (len < 1 || offsets[s + 1] > (1 << 22)) return set_err(CV_EINVAL, "bad batch shape");
    if ((s & 1) && len != offsets[s] - offsets[s - 1]) return set_err(CV_EINVAL, "a pair of two lengths");
  }
  CV_LOCK(h);
  cv_status st = set_device(h);
  if (st != CV_OK) return st;
  const size_t ne = (size_t)offsets[nseq];
  for (size_t e = 0; e < ne; ++e)
    if (obs[e] < 0 || obs[e] >= h->V) return set_err(CV_EINVAL, "observation out of range");
  if ((st = ensure_ru_tables(h)) != CV_OK) return st;
  if (h->ru_state != 1) return set_err(CV_EINVAL, "the model is outside the round-up pass's range");
  const int np = cvk::trellis_padded_states(h->N);
  const std::vector<int64_t> off(offsets, offsets + nseq + 1);
  DevBuf d_off, d_obs, d_rows, d_mu, d_r, d_e, d_path, d_cert;
  if ((st = upload(d_off, off.data(), off.size() * 8)) != CV_OK) return st;
  if ((st = upload(d_obs, obs, ne * 4)) != CV_OK) return st;
  if ((st = d_rows.ensure(ne * np * 4)) != CV_OK) return st;
  if ((st = d_mu.ensure(ne * 4)) != CV_OK) return st;
  if ((st = d_r.ensure(ne * 4)) != CV_OK) return st;
  if ((st = d_e.ensure((size_t)nseq * 4)) != CV_OK) return st;
  if ((st = d_path.ensure(ne * 4)) != CV_OK) return st;
  if ((st = d_cert.ensure((size_t)nseq)) != CV_OK) return st;
  hipStream_t stream = h->stream;
  HIP_TRY(hipMemsetAsync(d_cert.p, 0, (size_t)nseq, stream));
  HIP_TRY(hipMemsetAsync(d_mu.p, 0, ne * 4, stream));
  HIP_TRY(hipMemsetAsync(d_r.p, 0, ne * 4, stream));
  HIP_TRY(hipMemsetAsync(d_rows.p, 0, ne * np * 4, stream));  // an odd count leaves its last sequence alone
  HIP_TRY(hipMemsetAsync(d_path.p, 0, ne * 4, stream));
  HIP_TRY(hipMemsetAsync(d_e.p, 0, (size_t)nseq * 4, stream));
  cvk::RuFwdArgs fa{};
  cvk::RuBtArgs ba{};
  RuPass::tables(h, &fa, &ba);
  fa.offsets = ba.offsets = d_off.as<int64_t>();
  fa.obs = d_obs.as<int32_t>();
  fa.rows = d_rows.as<float>();
  fa.mu = d_mu.as<float>();
  fa.cert = ba.cert = d_cert.as<uint8_t>();
  fa.nobs = (int)h->V;
  hipError_t err = cvk::launch_ru_fwd2(np, fa, nseq / 2, stream);
  ba.rows = fa.rows;
  ba.seq_end = nseq - (nseq & 1);
  ba.path = d_path.as<int32_t>();
  ba.r = d_r.as<float>();
  ba.e_last = d_e.as<float>();
  if (err == hipSuccess) err = cvk::launch_ru_bt(np, ba, stream, 0);
  if (err != hipSuccess) return set_err(CV_EDEVICE, "round-up pass launch failed: %s", hipGetErrorString(err));
  HIP_TRY(hipStreamSynchronize(stream));
  std::vector<float> padded(ne * (size_t)np);
  HIP_TRY(hipMemcpy(padded.data(), d_rows.p, padded.size() * 4, hipMemcpyDeviceToHost));
  for (size_t e = 0; e < ne; ++e) std::memcpy(rows + e * (size_t)h->N, &padded[e * (size_t)np], (size_t)h->N * 4);
  HIP_TRY(hipMemcpy(mu, d_mu.p, ne * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(r, d_r.p, ne * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(e_last, d_e.p, (size_t)nseq * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(path, d_path.p, ne * 4, hipMemcpyDeviceToHost));
  return CV_OK;
}

}  // extern "C"
