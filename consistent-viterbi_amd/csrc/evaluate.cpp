// evaluate.cpp -- the evaluation (sum-product) entries of the C ABI (include/cviterbi.h):
// cv_posterior_batch, cv_sample_batch, cv_posterior_emissions, cv_expected_counts,
// cv_expected_counts_emissions, cv_loglik_grad_emissions, cv_expected_counts_model,
// cv_gauss_emissions, cv_expected_counts_gauss and their _device twins.  One core
// (posterior_device: a workspace plan, the arms of a chunk, a short loop), one path for the _device
// entries and one for the host entries; each exported function is its argument checks and a filled
// request.  The handle and the shared scaffolding: handle.hpp.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "batchplan.hpp"
#include "handle.hpp"
#include "kernels/bcount.h"
#include "kernels/emis.h"
#include "kernels/gauss.h"
#include "kernels/posterior.h"
#include "kernels/sample.h"

using namespace cvi;

namespace {

// Probability-space tables of the posterior kernels: p = 10^x by the host's correctly rounded
// pow (-inf -> 0 exactly), zero padded to pnp states so the kernels never test a row or column
// against N; the emission column of each observation is contiguous ([V][pnp]).
cv_status ensure_post_tables(cv_hmm* h) {
  const int np = cvp::post_padded_states(h->N);
  if (h->pnp == np) return CV_OK;
  const int N = h->N;
  const int64_t V = h->V;
  auto p10 = [](double x) { return x == -INFINITY ? 0.0 : std::pow(10.0, x); };
  std::vector<double> pi((size_t)np, 0.0), a((size_t)np * np, 0.0), at((size_t)np * np, 0.0), et((size_t)V * np, 0.0);
  for (int i = 0; i < N; ++i) pi[(size_t)i] = p10(h->pi[(size_t)i]);
  parallel_ranges(N, [&](int, int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i)
      for (int j = 0; j < N; ++j) {
        const double v = p10(h->a[(size_t)i * N + j]);
        a[(size_t)i * np + j] = v;
        at[(size_t)j * np + i] = v;
      }
  }, std::max<int64_t>(1, 4096 / N));
  parallel_ranges(N, [&](int, int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i)
      for (int64_t o = 0; o < V; ++o) et[(size_t)o * np + i] = p10(h->b[(size_t)i * V + o]);
  }, std::max<int64_t>(1, 4096 / std::max<int64_t>(V, 1)));
  cv_status st;
  if ((st = upload(h->p_pi, pi.data(), pi.size() * 8)) != CV_OK) return st;
  if ((st = upload(h->p_a, a.data(), a.size() * 8)) != CV_OK) return st;
  if ((st = upload(h->p_at, at.data(), at.size() * 8)) != CV_OK) return st;
  if ((st = upload(h->p_et, et.data(), et.size() * 8)) != CV_OK) return st;
  if ((st = h->p_dump.ensure((size_t)cvp::kPostDumpWaves * 64 * 8)) != CV_OK) return st;
  h->pnp = np;
  return CV_OK;
}

// What the posterior path accepts of the options and the model (no device needed).
cv_status posterior_opts_ok(const cv_hmm* h, const cv_opts& o) {
  if (o.dtype == CV_DTYPE_F32) return set_err(CV_EUNSUPPORTED, "the posterior path is f64 only");
  if (o.dtype != CV_DTYPE_F64) return set_err(CV_EINVAL, "bad dtype %d", o.dtype);
  if (o.assoc != CV_ASSOC_VITERBI)
    return set_err(CV_EINVAL, "the posterior path reads the model as the VITERBI association (assoc %d)", o.assoc);
  if (o.kernel != CV_KERNEL_AUTO && o.kernel != CV_KERNEL_GENERIC)
    return set_err(CV_EINVAL, "posterior kernel must be AUTO or GENERIC (kernel %d)", o.kernel);
  if (h->N > cvp::kPostMaxStates)
    return set_err(CV_EUNSUPPORTED, "the posterior kernels cover N <= %d (N=%d)", cvp::kPostMaxStates, h->N);
  return CV_OK;
}

// cv_sample_batch*: what the sampler puts in place of the backward pass of a chunk
struct SampleReq {
  int32_t draws;
  uint64_t seed;
  int64_t seq_base;
  int32_t* path;  // device, [draws][offsets[nseq]]
  double* score;  // device, [draws][nseq], nullable
};
// cv_expected_counts_gauss*: the Gaussian arm of the counts request (gauss.hip).  The density kernel
// fills a chunk-local workspace the staging reads (EmisSrc::chunk_local), and the rows w_s gamma of
// the gradient arm meet Phi = [1 | y | y^2] in the moment GEMM
struct GaussReq {
  const double* x;    // device, element e at x + e * ldx, D values
  int64_t ldx;
  int D;
  const double* tab;  // device: the call's tables (cvg::gauss_table_doubles)
  double *g_cnt, *m1, *m2;  // device, [N], [N][D], [N][D]
};
// cv_expected_counts*: the counts arm of the backward pass and the kernels behind it
struct CountsReq {
  double* pi_cnt;  // device, [N]
  double* a_cnt;   // device, [N][N]
  // cv_loglik_grad_emissions*: the gradient arm (grad.hip) -- every term times its sequence's weight,
  // the gamma rows (then the gradient of E) at the caller's stride; PostReq::gamma is null in such a call
  bool grad = false;
  const double* weight = nullptr;  // device, [nseq]; null: all 1
  double* egrad = nullptr;         // device, nullable, row e at egrad + e * ld_grad
  int64_t ld_grad = 0;
  // cv_expected_counts_model*: the expected emission counts of the discrete model (bcount.hip), with
  // grad set -- the rows w_s gamma the gradient arm stores are what the scatter by observation adds.
  // egrad (ld_grad = N) is then the caller's gamma; null: a chunk-local workspace takes the rows
  double* b_cnt = nullptr;  // device, nullable, [N][V]
  // cv_expected_counts_gauss*: with grad set and egrad as for b_cnt; PostReq::emis is chunk-local
  const GaussReq* gauss = nullptr;
};
// What one call asks of posterior_device, filled by field name: the outputs (device pointers), the
// stream, and at most one of each mode -- dense emissions, the sampler, the counts arm.
struct PostReq {
  double* loglik = nullptr;  // [nseq]
  int32_t* path = nullptr;   // nullable, [offsets[nseq]]
  double* gamma = nullptr;   // nullable, [offsets[nseq]][N]
  uint8_t* status = nullptr;
  hipStream_t stream = nullptr;
  const EmisSrc* emis = nullptr;
  const SampleReq* smp = nullptr;
  const CountsReq* cnt = nullptr;
};

// The batch of a call: device pointers except offsets_host.
struct Batch {
  int64_t nseq;
  const int64_t* offsets_host;
  const int64_t* offsets_dev;
  const int32_t* obs_dev;
};

// The workspace of a call: chunks of whole sequences whose per-element rows fit the cap, and
// ps_rows carved into [max_elems][NP] forward rows (store), [max_elems][NP] U rows (counts),
// [max_elems][NP] staged emission rows (emis), [max_elems][NP] rows w_s gamma (emission counts or
// Gaussian moments without the caller's gamma), [max_elems][NP] log10 densities (Gaussian),
// [max_elems] inv (counts), [max_elems] int32 observation indices (emis); NP * 8 is a multiple of
// 512.  A pointer is null when its mode is off.
struct PostPlan {
  bool store = false;  // any row is kept: everything but the scoring mode
  bool bc_ws = false;  // emission counts, Gaussian moments: the rows w_s gamma go to the workspace
  uint64_t row_bytes = 0, per_elem = 0, part_cap = 0, gm_cap = 0, max_elems = 0;
  std::vector<cvplan::Chunk> chunks;
  double *ws_rows = nullptr, *ws_urows = nullptr, *ws_emis = nullptr, *ws_g = nullptr, *ws_dens = nullptr, *ws_inv = nullptr;
  int32_t* ws_idx = nullptr;
};

cv_status plan_workspace(cv_hmm* h, const Batch& bt, const cv_opts& o, const PostReq& rq, PostPlan* plan) {
  PostPlan& p = *plan;
  const CountsReq* cnt = rq.cnt;
  const EmisSrc* emis = rq.emis;
  const int np = h->pnp;
  const int64_t* offsets_host = bt.offsets_host;
  cv_status st;
  p.store = rq.path || rq.gamma || rq.smp || cnt;
  const GaussReq* gs = cnt ? cnt->gauss : nullptr;
  p.bc_ws = cnt && (cnt->b_cnt || gs) && !cnt->egrad;
  const uint64_t row_bytes = p.row_bytes = (uint64_t)np * 8;
  // counts: the U row and inv of every element beside its forward row
  const uint64_t per_elem = p.per_elem =
      (p.store ? row_bytes : 0) + (cnt ? row_bytes + 8 : 0) + (emis ? row_bytes + 4 : 0) + (p.bc_ws ? row_bytes : 0) + (gs ? row_bytes : 0);
  if (per_elem == 0) {
    p.chunks.emplace_back(0, bt.nseq);
  } else {
    // 2 KiB of rows per element at N = 256: the f64 trellis's default cap (HBM3E: 288 GB per GPU)
    uint64_t cap = o.workspace_bytes ? o.workspace_bytes : default_workspace_cap(h->ps_rows.bytes, kDefaultWorkspaceT64);
    // ... and the GEMM's partial tiles, under the same cap: at most cvp::kXiPartCap, and half of a
    // cap that is smaller than twice that
    if (cnt) {
      const uint64_t most = std::min<uint64_t>(cvp::kXiPartCap, (uint64_t)cvp::kXiMaxParts * np * row_bytes);
      p.part_cap = cap >= 2 * most ? most : cap / 2;
      cap -= p.part_cap;
    }
    // ... and the moment GEMM's, by the same rule on what is left
    if (gs) {
      const uint64_t most = std::min<uint64_t>(cvg::kGmPartCap, (uint64_t)cvg::kGmMaxParts * cvg::gm_padded_width(gs->D) * row_bytes);
      p.gm_cap = cap >= 2 * most ? most : cap / 2;
      cap -= p.gm_cap;
    }
    uint64_t elem_cap = cap / per_elem;
    if (emis) {  // the staged rows of a sequence cannot be split, and a chunk is indexed by int32
      elem_cap = std::min<uint64_t>(elem_cap, INT32_MAX);
      for (int64_t s = 0; s < bt.nseq; ++s) {
        const uint64_t T = (uint64_t)(offsets_host[s + 1] - offsets_host[s]);
        if (T > INT32_MAX) return set_err(CV_ELIMIT, "sequence %lld: %llu elements of dense emissions", (long long)s, (unsigned long long)T);
        if (T > elem_cap)
          return set_err(CV_ENOMEM, "sequence %lld needs %llu bytes of staged emissions and rows (T=%llu, NP=%d), workspace cap %llu",
                         (long long)s, (unsigned long long)(T * per_elem), (unsigned long long)T, np, (unsigned long long)cap);
      }
    }
    p.max_elems = std::max<uint64_t>(cvplan::split_equal_shares(offsets_host, bt.nseq, elem_cap, p.chunks).max_elems, 1);
    if ((st = h->ps_rows.ensure((size_t)(p.max_elems * per_elem))) != CV_OK) return st;
  }
  double* ws_next = h->ps_rows.as<double>();
  auto take_rows = [&](bool on, uint64_t width) {
    double* const q = on ? ws_next : nullptr;
    if (on) ws_next += p.max_elems * width;
    return q;
  };
  p.ws_rows = take_rows(p.store, (uint64_t)np);
  p.ws_urows = take_rows(cnt != nullptr, (uint64_t)np);
  p.ws_emis = take_rows(emis != nullptr, (uint64_t)np);
  p.ws_g = take_rows(p.bc_ws, (uint64_t)np);
  p.ws_dens = take_rows(gs != nullptr, (uint64_t)np);
  p.ws_inv = take_rows(cnt != nullptr, 1);
  p.ws_idx = emis ? reinterpret_cast<int32_t*>(ws_next) : nullptr;
  return CV_OK;
}

// What the counts arm keeps between its preparation and its chunks.
struct CountsArm {
  int64_t xi_key = 0;  // tuning key xi_part_rows
  int64_t bc_key = 0;  // tuning key bcnt_part_rows
  cvb::BcntArgs bq{};  // emission counts: what every chunk's launch shares
  int64_t gm_key = 0;  // tuning key gm_part_rows
};

// Counts: the GEMM's partial tiles of the largest chunk, the accumulator ps_xi_s (zeroed here) and
// gamma_0 of every sequence.
cv_status prepare_counts(cv_hmm* h, const Batch& bt, const PostPlan& plan, hipStream_t stream, CountsArm* arm) {
  const int np = h->pnp;
  cv_status st;
  arm->xi_key = cvk::tuning().xi_part_rows;
  int64_t most_parts = 1;
  for (const auto& c : plan.chunks) {
    const int64_t rows = bt.offsets_host[c.second] - bt.offsets_host[c.first];
    const int64_t per = cvp::post_xi_part_rows(rows, np, arm->xi_key, plan.part_cap);
    most_parts = std::max(most_parts, (rows + per - 1) / per);
  }
  if ((st = h->ps_xi_part.ensure((size_t)most_parts * np * plan.row_bytes)) != CV_OK) return st;
  if ((st = h->ps_xi_s.ensure((size_t)np * plan.row_bytes)) != CV_OK) return st;
  if ((st = h->ps_g0.ensure((size_t)bt.nseq * plan.row_bytes)) != CV_OK) return st;
  HIP_TRY(hipMemsetAsync(h->ps_xi_s.p, 0, (size_t)np * plan.row_bytes, stream));
  return CV_OK;
}

// Emission counts: the sort's scratch and the run sums of the largest chunk, the accumulator
// ps_bc_acc (zeroed here).
cv_status prepare_emission_counts(cv_hmm* h, const Batch& bt, const PostPlan& plan, const PostReq& rq, CountsArm* arm) {
  const int np = h->pnp;
  const uint64_t max_elems = plan.max_elems, row_bytes = plan.row_bytes;
  cv_status st;
  arm->bc_key = cvk::tuning().bcnt_part_rows;
  cvb::BcntArgs& bq = arm->bq;
  if (max_elems > INT32_MAX) return set_err(CV_ELIMIT, "emission counts: a chunk of %llu elements", (unsigned long long)max_elems);
  int64_t most_runs = 1;
  for (const auto& c : plan.chunks) {
    const int64_t rows = bt.offsets_host[c.second] - bt.offsets_host[c.first];
    most_runs = std::max(most_runs, cvb::bcnt_max_runs(rows, cvb::bcnt_part_rows(rows, np, arm->bc_key), h->V));
  }
  size_t tmp = 0;
  hipError_t qe = cvb::bcnt_sort_tmp_bytes((int64_t)max_elems, h->V, &tmp);
  if (qe != hipSuccess) return set_err(CV_EDEVICE, "emission-count sort sizing failed: %s", hipGetErrorString(qe));
  auto up = [](size_t n) { return (n + 255) / 256 * 256; };
  const size_t plane = up((size_t)max_elems * 4), tmp_b = up(tmp), keys_b = up((size_t)most_runs * 4);
  if ((st = h->ps_bc_sort.ensure(5 * plane + tmp_b + keys_b)) != CV_OK) return st;
  if ((st = h->ps_bc_part.ensure((size_t)most_runs * row_bytes)) != CV_OK) return st;
  if ((st = h->ps_bc_acc.ensure((size_t)h->V * row_bytes)) != CV_OK) return st;
  HIP_TRY(hipMemsetAsync(h->ps_bc_acc.p, 0, (size_t)h->V * row_bytes, rq.stream));
  char* const sp = h->ps_bc_sort.as<char>();
  bq.key_in = reinterpret_cast<uint32_t*>(sp);
  bq.key_out = reinterpret_cast<uint32_t*>(sp + plane);
  bq.row_in = reinterpret_cast<int32_t*>(sp + 2 * plane);
  bq.row_out = reinterpret_cast<int32_t*>(sp + 3 * plane);
  bq.run = reinterpret_cast<int32_t*>(sp + 4 * plane);
  bq.sort_tmp = sp + 5 * plane;
  bq.sort_tmp_bytes = tmp_b;
  bq.run_key = reinterpret_cast<uint32_t*>(sp + 5 * plane + tmp_b);
  bq.max_runs = most_runs;
  bq.part = h->ps_bc_part.as<double>();
  bq.acc = h->ps_bc_acc.as<double>();
  bq.offsets = bt.offsets_dev;
  bq.obs = bt.obs_dev;
  bq.status = rq.status;
  bq.nobs = h->V;
  bq.nstates = h->N;
  bq.np = np;
  return CV_OK;
}

// Gaussian moments: the partial tiles of the largest chunk, the row flags, the accumulator ps_gm_acc
// (zeroed here).
cv_status prepare_gauss(cv_hmm* h, const Batch& bt, const PostPlan& plan, const PostReq& rq, CountsArm* arm) {
  const int np = h->pnp, wp = cvg::gm_padded_width(rq.cnt->gauss->D);
  cv_status st;
  arm->gm_key = cvk::tuning().gm_part_rows;
  int64_t most_parts = 1;
  for (const auto& c : plan.chunks) {
    const int64_t rows = bt.offsets_host[c.second] - bt.offsets_host[c.first];
    const int64_t per = cvg::gm_part_rows(rows, np, wp, arm->gm_key, plan.gm_cap);
    most_parts = std::max(most_parts, (rows + per - 1) / per);
  }
  if ((st = h->ps_gm_part.ensure((size_t)most_parts * wp * plan.row_bytes)) != CV_OK) return st;
  if ((st = h->ps_gm_acc.ensure((size_t)wp * plan.row_bytes)) != CV_OK) return st;
  if ((st = h->ps_gm_ok.ensure((size_t)plan.max_elems * 4)) != CV_OK) return st;
  HIP_TRY(hipMemsetAsync(h->ps_gm_acc.p, 0, (size_t)wp * plan.row_bytes, rq.stream));
  return CV_OK;
}

// The device tables of a Gaussian call inside h->ps_gauss (cvg::gauss_table_doubles).
struct GaussTab {
  const double *c, *mu_t, *w_t, *center;
};
GaussTab gauss_tab(const double* tab, int N, int D) {
  const size_t dp = (size_t)cvg::gauss_padded_dims(D);
  return GaussTab{tab, tab + N, tab + N + dp * (size_t)N, tab + N + 2 * dp * (size_t)N};
}

// The density kernel over `nrows` rows of x into out (row stride ld).
cv_status launch_density(cv_hmm* h, const double* tab, const double* x, int64_t ldx, int D, int64_t nrows, double* out,
                         int64_t ld, hipStream_t stream) {
  const GaussTab t = gauss_tab(tab, h->N, D);
  cvg::GaussArgs ga{};
  ga.x = x;
  ga.ldx = ldx;
  ga.nrows = nrows;
  ga.D = D;
  ga.DP = cvg::gauss_padded_dims(D);
  ga.nstates = h->N;
  ga.c = t.c;
  ga.mu_t = t.mu_t;
  ga.w_t = t.w_t;
  ga.out = out;
  ga.ld = ld;
  const hipError_t err = cvg::launch_gauss_emis(ga, h->cus, stream);
  if (err != hipSuccess) return set_err(CV_EDEVICE, "Gaussian density launch failed: %s", hipGetErrorString(err));
  return CV_OK;
}

// Dense emissions: the chunk's rows staged in probability space behind its forward rows; g then
// reads them as its emission table, one row per element.  A chunk-local source (the Gaussian arm)
// is first filled by the density kernel: row 0 of its workspace is element e0.
cv_status stage_chunk_emissions(cv_hmm* h, const PostReq& rq, const PostPlan& plan, const Batch& bt, cvp::PostArgs* g) {
  const int64_t e0 = bt.offsets_host[g->seq_begin], e1 = bt.offsets_host[g->seq_end];
  cvem::EmisLinArgs eg{};
  eg.src = rq.emis->p;
  eg.ld = rq.emis->ld;
  if (rq.emis->chunk_local) {
    const GaussReq* gs = rq.cnt->gauss;
    const cv_status st = launch_density(h, gs->tab, gs->x + (size_t)e0 * (size_t)gs->ldx, gs->ldx, gs->D, e1 - e0,
                                        plan.ws_dens, h->pnp, rq.stream);
    if (st != CV_OK) return st;
    eg.src = rebased<const double>(plan.ws_dens, e0, (size_t)h->pnp);
    eg.ld = h->pnp;
  }
  eg.e0 = e0;
  eg.nrows = e1 - e0;
  eg.nstates = h->N;
  eg.stride = h->pnp;
  eg.dst = plan.ws_emis;
  eg.idx = plan.ws_idx;
  eg.offsets = bt.offsets_dev;
  eg.seq_begin = g->seq_begin;
  eg.seq_end = g->seq_end;
  eg.kshift = h->ps_kshift.as<int64_t>();
  const hipError_t err = cvem::launch_emis_prepare_lin(eg, h->cus, rq.stream);
  if (err != hipSuccess) return set_err(CV_EDEVICE, "emission staging launch failed: %s", hipGetErrorString(err));
  g->et = plan.ws_emis;
  g->obs = rebased<const int32_t>(plan.ws_idx, e0);
  g->nobs = e1 - e0;
  g->kshift = h->ps_kshift.as<int64_t>();
  return CV_OK;
}

// The sampler in place of the chunk's backward pass: the walk over the stored rows, then the
// scores of its paths when asked.
cv_status sample_chunk(cv_hmm* h, const PostReq& rq, const Batch& bt, const cvp::PostArgs& g, bool generic) {
  const SampleReq* smp = rq.smp;
  cvs::SampleArgs sg{};
  sg.at = g.at;
  sg.rows = g.rows;
  sg.offsets = bt.offsets_dev;
  sg.order = g.order;
  sg.seq_begin = g.seq_begin;
  sg.seq_end = g.seq_end;
  sg.elem_base = g.elem_base;
  sg.nstates = h->N;
  sg.np = h->pnp;
  sg.status = rq.status;
  sg.path = smp->path;
  sg.plane = bt.offsets_host[bt.nseq];
  sg.draws = smp->draws;
  sg.seed = smp->seed;
  sg.seq_base = smp->seq_base;
  hipError_t err = cvs::launch_sample(sg, generic, rq.stream);
  if (err == hipSuccess && smp->score) {
    cvs::SampleScoreArgs ss{};
    ss.path = smp->path;
    ss.plane = sg.plane;
    ss.draws = smp->draws;
    ss.obs = bt.obs_dev;
    ss.offsets = bt.offsets_dev;
    ss.order = g.order;
    ss.seq_begin = g.seq_begin;
    ss.seq_end = g.seq_end;
    ss.nseq = bt.nseq;
    ss.nstates = h->N;
    ss.pi64 = h->d_pi64.as<double>();
    ss.a64 = h->d_a64.as<double>();
    ss.et64 = h->d_et64.as<double>();
    ss.status = rq.status;
    ss.score = smp->score;
    err = cvs::launch_sample_score(ss, rq.stream);
  }
  if (err != hipSuccess) return set_err(CV_EDEVICE, "sampling launch failed: %s", hipGetErrorString(err));
  return CV_OK;
}

// Counts after the chunk's backward pass: the count GEMM and its fold into ps_xi_s, the scatter
// of the rows w_s gamma by observation (emission counts), and after the last chunk the kernels
// that write pi_cnt, a_cnt and b_cnt.
cv_status counts_chunk(cv_hmm* h, const PostReq& rq, const PostPlan& plan, const CountsArm& arm, const Batch& bt,
                       const cvp::PostArgs& g, bool last) {
  const CountsReq* cnt = rq.cnt;
  const int np = h->pnp;
  cvp::XiArgs x{};
  x.rows = plan.ws_rows;
  x.urows = plan.ws_urows;
  x.inv = plan.ws_inv;
  x.nrows = bt.offsets_host[g.seq_end] - bt.offsets_host[g.seq_begin];
  x.part_rows = cvp::post_xi_part_rows(x.nrows, np, arm.xi_key, plan.part_cap);
  x.nparts = (x.nrows + x.part_rows - 1) / x.part_rows;
  x.np = np;
  x.part = h->ps_xi_part.as<double>();
  x.s = h->ps_xi_s.as<double>();
  hipError_t err = cvp::launch_post_xi(x, rq.stream);
  if (err == hipSuccess && last) {
    cvp::CountsFinalArgs f{};
    f.s = x.s;
    f.a = g.a;
    f.g0 = g.g0;
    f.status = rq.status;
    f.nseq = bt.nseq;
    f.nstates = h->N;
    f.np = np;
    f.a_cnt = cnt->a_cnt;
    f.pi_cnt = cnt->pi_cnt;
    err = cvp::launch_post_counts_final(f, rq.stream);
  }
  if (err == hipSuccess && cnt->b_cnt) {
    cvb::BcntArgs b = arm.bq;
    b.seq_begin = g.seq_begin;
    b.seq_end = g.seq_end;
    b.elem_base = g.elem_base;
    b.nrows = x.nrows;
    b.ld = g.ld_grad;
    b.g = plan.bc_ws ? plan.ws_g : cnt->egrad + (size_t)g.elem_base * (size_t)h->N;
    b.part_rows = cvb::bcnt_part_rows(b.nrows, np, arm.bc_key);
    err = cvb::launch_bcnt_chunk(b, rq.stream);
    if (err == hipSuccess && last) err = cvb::launch_bcnt_final(arm.bq.acc, h->V, h->N, np, cnt->b_cnt, rq.stream);
  }
  if (err == hipSuccess && cnt->gauss) {
    const GaussReq* gs = cnt->gauss;
    cvg::GmArgs m{};
    m.offsets = bt.offsets_dev;
    m.status = rq.status;
    m.seq_begin = g.seq_begin;
    m.seq_end = g.seq_end;
    m.elem_base = g.elem_base;
    m.nrows = x.nrows;
    m.g = plan.bc_ws ? plan.ws_g : cnt->egrad + (size_t)g.elem_base * (size_t)h->N;
    m.ldg = g.ld_grad;
    m.x = gs->x;
    m.ldx = gs->ldx;
    m.center = gauss_tab(gs->tab, h->N, gs->D).center;
    m.D = gs->D;
    m.wp = cvg::gm_padded_width(gs->D);
    m.nstates = h->N;
    m.np = np;
    m.rowok = h->ps_gm_ok.as<int32_t>();
    m.part_rows = cvg::gm_part_rows(m.nrows, np, m.wp, arm.gm_key, plan.gm_cap);
    m.nparts = (m.nrows + m.part_rows - 1) / m.part_rows;
    m.part = h->ps_gm_part.as<double>();
    m.acc = h->ps_gm_acc.as<double>();
    err = cvg::launch_gm_chunk(m, rq.stream);
    if (err == hipSuccess && last) err = cvg::launch_gm_final(m.acc, h->N, gs->D, m.wp, gs->g_cnt, gs->m1, gs->m2, rq.stream);
  }
  if (err != hipSuccess) return set_err(CV_EDEVICE, "expected-counts launch failed: %s", hipGetErrorString(err));
  return CV_OK;
}

// Core of the family: all pointers are device pointers except offsets_host.  Chunks of whole
// sequences (original order) whose forward rows fit the workspace cap run forward then backward
// on rq.stream; scoring mode (no path, no gamma) is one forward launch with no rows.
// rq.emis (cv_posterior_emissions*): the emissions of every element come from this dense array
// of log10 scores instead of the handle's b through obs_dev (ignored, may be null).  Each chunk's
// rows are staged behind its forward rows (8 NP + 4 bytes per element more, under the same cap --
// so the scoring mode is chunked too) and stay there until its backward pass has run; the
// sequences' row-scale exponents go to ps_kshift.
// rq.smp (cv_sample_batch*): the rows are stored and each chunk's backward pass is replaced by the
// sampler; planning, order and events are unchanged, so a sampling call chunks and times exactly
// like a posterior call.
// rq.cnt (cv_expected_counts*): the backward pass runs with its counts arm (8 NP + 8 bytes per
// element more: the U row and 1 / rsum) and counts_chunk follows it inside the chunk's backward
// events, so bt_ms covers the counts.  With cnt->grad (cv_loglik_grad_emissions*) the backward
// pass is the gradient arm's; nothing else differs.  cnt->b_cnt (cv_expected_counts_model*; with
// cnt->grad, the handle's own b): the rows w_s gamma of the gradient arm go to cnt->egrad (the
// caller's gamma, stride N) or, when that is null, to a chunk-local workspace (8 NP bytes per
// element more, under the cap).  cnt->gauss (cv_expected_counts_gauss*; with cnt->grad and a
// chunk-local rq.emis): each chunk's log10 densities are computed into a workspace of their own
// (8 NP bytes per element more) before the staging reads them, and the rows w_s gamma -- placed as
// for b_cnt -- meet Phi = [1 | y | y^2] in the moment GEMM (its partial tiles under the cap too).
cv_status posterior_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host, const int64_t* offsets_dev,
                           const int32_t* obs_dev, const cv_opts& o, const PostReq& rq) {
  const CountsReq* cnt = rq.cnt;
  const hipStream_t stream = rq.stream;
  cv_status st = posterior_opts_ok(h, o);
  if (st != CV_OK) return st;
  if (rq.smp && rq.smp->score && (st = ensure_f64_tables(h)) != CV_OK) return st;
  const bool generic = o.kernel == CV_KERNEL_GENERIC || h->N > cvp::kPostMmStates;
  std::vector<int64_t> off_copy;
  if ((st = host_offsets(nseq, offsets_host, offsets_dev, off_copy, stream)) != CV_OK) return st;
  if ((st = ensure_post_tables(h)) != CV_OK) return st;
  const int np = h->pnp;
  h->last_launches = 0;
  h->last_kernel = generic ? CV_KERNEL_GENERIC : CV_KERNEL_AUTO;
  h->last_np = np;
  h->last_mt = generic ? -1 : cvp::kPostGroup;
  if (nseq == 0 && cnt) {  // overwritten, not accumulated: an empty batch counts nothing
    HIP_TRY(hipMemsetAsync(cnt->pi_cnt, 0, (size_t)h->N * 8, stream));
    HIP_TRY(hipMemsetAsync(cnt->a_cnt, 0, (size_t)h->N * h->N * 8, stream));
    if (cnt->b_cnt) HIP_TRY(hipMemsetAsync(cnt->b_cnt, 0, (size_t)h->N * (size_t)h->V * 8, stream));
    if (cnt->gauss) {
      HIP_TRY(hipMemsetAsync(cnt->gauss->g_cnt, 0, (size_t)h->N * 8, stream));
      HIP_TRY(hipMemsetAsync(cnt->gauss->m1, 0, (size_t)h->N * cnt->gauss->D * 8, stream));
      HIP_TRY(hipMemsetAsync(cnt->gauss->m2, 0, (size_t)h->N * cnt->gauss->D * 8, stream));
    }
  }
  if (nseq == 0) return CV_OK;
  if (h->ws_rec) HIP_TRY(hipStreamWaitEvent(stream, h->ws_done, 0));

  const bool bc = cnt && cnt->b_cnt;
  if (bc && (rq.emis || !cnt->grad || !obs_dev || rq.gamma || (cnt->egrad && cnt->ld_grad != h->N)))
    return set_err(CV_EINTERNAL, "emission counts: the discrete model under the gradient arm only");
  const bool gs = cnt && cnt->gauss;
  if (gs && (bc || !rq.emis || !rq.emis->chunk_local || !cnt->grad || rq.gamma || (cnt->egrad && cnt->ld_grad != h->N)))
    return set_err(CV_EINTERNAL, "Gaussian moments: chunk-local densities under the gradient arm only");
  if (!gs && rq.emis && rq.emis->chunk_local) return set_err(CV_EINTERNAL, "chunk-local emissions without their source");
  if (bc && h->V > INT32_MAX) return set_err(CV_ELIMIT, "emission counts cover V <= %d (V=%lld)", INT32_MAX, (long long)h->V);
  const Batch bt{nseq, offsets_host, offsets_dev, obs_dev};
  PostPlan plan;
  if ((st = plan_workspace(h, bt, o, rq, &plan)) != CV_OK) return st;
  CountsArm arm;
  if (cnt && (st = prepare_counts(h, bt, plan, stream, &arm)) != CV_OK) return st;
  if (bc && (st = prepare_emission_counts(h, bt, plan, rq, &arm)) != CV_OK) return st;
  if (gs && (st = prepare_gauss(h, bt, plan, rq, &arm)) != CV_OK) return st;
  if (rq.emis) {
    if ((st = h->ps_kshift.ensure((size_t)nseq * 8)) != CV_OK) return st;
    HIP_TRY(hipMemsetAsync(h->ps_kshift.p, 0, (size_t)nseq * 8, stream));
  }
  // longest first inside each chunk (stable), so a group's sequences have similar lengths
  const std::vector<cvplan::Chunk>& chunks = plan.chunks;
  const int32_t* order_dev = nullptr;
  if (cvplan::varlen(offsets_host, nseq)) {
    if (nseq > INT32_MAX) return set_err(CV_EINVAL, "too many sequences (%lld)", (long long)nseq);
    h->order_host.resize((size_t)nseq);
    cvplan::longest_first(offsets_host, chunks, h->order_host.data(), nullptr, h->sort_pos);
    if ((st = upload_order(h->ps_order, h->ps_pin, h->order_host.data(), nseq, stream, &order_dev)) != CV_OK) return st;
  }
  const size_t nev = 4 * chunks.size();
  size_t eb;
  if ((st = reserve_events(h, false, nev, &eb)) != CV_OK) return st;
  // scoring mode: no backward launch, and cv_last_timing says so exactly (bt_ms = 0)
  if (!plan.store) std::fill(h->ev_nobt.begin() + (ptrdiff_t)(eb / 4), h->ev_nobt.begin() + (ptrdiff_t)(eb / 4 + chunks.size()), (uint8_t)1);
  for (size_t ci = 0; ci < chunks.size(); ++ci) {
    const auto& c = chunks[ci];
    cvp::PostArgs g{};
    g.pi = h->p_pi.as<double>();
    g.a = h->p_a.as<double>();
    g.at = h->p_at.as<double>();
    g.et = h->p_et.as<double>();
    g.offsets = offsets_dev;
    g.obs = obs_dev;
    g.forced = o.forced;
    g.order = order_dev;
    g.seq_begin = c.first;
    g.seq_end = c.second;
    g.elem_base = offsets_host[c.first];
    g.nstates = h->N;
    g.np = np;
    g.nobs = h->V;
    g.rows = plan.ws_rows;
    g.loglik = rq.loglik;
    g.status = rq.status;
    g.path = rq.path;
    g.gamma = rq.gamma;
    g.dump = h->p_dump.as<double>();
    if (cnt) {
      g.urows = plan.ws_urows;
      g.inv = plan.ws_inv;
      g.g0 = h->ps_g0.as<double>();
      g.weight = cnt->weight;
      g.egrad = cnt->egrad;
      g.ld_grad = cnt->ld_grad;
      if (plan.bc_ws) {
        g.egrad = rebased(plan.ws_g, g.elem_base, (size_t)np);
        g.ld_grad = np;
      }
    }
    hipEvent_t f0 = h->ev[eb + 4 * ci], f1 = h->ev[eb + 4 * ci + 1], b0 = h->ev[eb + 4 * ci + 2], b1 = h->ev[eb + 4 * ci + 3];
    HIP_TRY(hipEventRecord(f0, stream));
    if (rq.emis && (st = stage_chunk_emissions(h, rq, plan, bt, &g)) != CV_OK) return st;
    hipError_t err = cvp::launch_post_fwd(g, generic, stream);
    if (err != hipSuccess) return set_err(CV_EDEVICE, "posterior forward launch failed: %s", hipGetErrorString(err));
    HIP_TRY(hipEventRecord(f1, stream));
    HIP_TRY(hipEventRecord(b0, stream));
    if (rq.smp) {
      if ((st = sample_chunk(h, rq, bt, g, generic)) != CV_OK) return st;
    } else if (plan.store) {
      err = cnt && cnt->grad ? cvp::launch_post_grad_bwd(g, generic, stream) : cvp::launch_post_bwd(g, generic, stream);
      if (err != hipSuccess) return set_err(CV_EDEVICE, "posterior backward launch failed: %s", hipGetErrorString(err));
    }
    if (cnt && (st = counts_chunk(h, rq, plan, arm, bt, g, ci + 1 == chunks.size())) != CV_OK) return st;
    HIP_TRY(hipEventRecord(b1, stream));
    h->last_launches = (int64_t)ci + 1;
  }
  return end_call(h, false, nev, stream);
}

cv_status sample_draws_ok(int32_t draws) {
  if (draws < 1 || draws > cvs::kSampleMaxDraws)
    return set_err(CV_EINVAL, "draws = %d outside [1, %d]", draws, cvs::kSampleMaxDraws);
  return CV_OK;
}

// The checks of the dense entries that need no device, made before any copy from the caller's arrays.
cv_status posterior_emissions_args_ok(const cv_hmm* h, int64_t ld, const cv_opts& o) {
  if (ld < h->N) return set_err(CV_EINVAL, "ld = %lld is less than N = %d", (long long)ld, h->N);
  return posterior_opts_ok(h, o);
}

hipStream_t call_stream(const cv_hmm* h, const cv_opts& o) { return o.stream ? (hipStream_t)o.stream : h->stream; }

// A _device entry after its argument checks: the handle's lock and tuning, the device, the stream
// of the options, the core.  The forward pass always writes the log-likelihoods: to the staging
// when the caller asks for none (cv_sample_batch_device).
cv_status device_entry(cv_hmm* h, int64_t nseq, const int64_t* offsets_host, const int64_t* offsets_dev,
                       const int32_t* obs_dev, const cv_opts& o, PostReq rq) {
  CV_LOCK(h);
  cv_status st = set_device(h);
  if (st != CV_OK) return st;
  rq.stream = call_stream(h, o);
  if (!rq.loglik && nseq > 0) {
    if ((st = h->st_score.ensure((size_t)nseq * 8)) != CV_OK) return st;
    rq.loglik = h->st_score.as<double>();
  }
  return posterior_device(h, nseq, offsets_host, offsets_dev, obs_dev, o, rq);
}

// The argument checks of the Gaussian entries, made before any device work.
cv_status gauss_args_ok(const cv_hmm* h, int64_t ldx, int64_t D, const double* mean, const double* var) {
  if (D < 1) return set_err(CV_EINVAL, "D = %lld is less than 1", (long long)D);
  if (D > cvg::kGaussMaxDims) return set_err(CV_ELIMIT, "the Gaussian kernels cover D <= %d (D=%lld)", cvg::kGaussMaxDims, (long long)D);
  if (ldx < D) return set_err(CV_EINVAL, "ldx = %lld is less than D = %lld", (long long)ldx, (long long)D);
  if (!mean || !var) return set_err(CV_EINVAL, "null mean or var");
  const int64_t n = (int64_t)h->N * D;
  int64_t k = first_bad(0, n, [&](int64_t i) { return !std::isfinite(mean[i]); });
  if (k >= 0) return set_err(CV_EINVAL, "mean[%lld][%lld] is not finite", (long long)(k / D), (long long)(k % D));
  k = first_bad(0, n, [&](int64_t i) { return !(var[i] >= 1e-300 && var[i] <= 1e300); });
  if (k >= 0)
    return set_err(CV_EINVAL, "var[%lld][%lld] = %g is outside [1e-300, 1e300]", (long long)(k / D), (long long)(k % D), var[k]);
  return CV_OK;
}

// The tables of a Gaussian call, in f64 on the host: w = 1 / var (one division per entry), c_j =
// -1/2 sum_d log10(2 pi var_jd) in ascending d, mean and w transposed to [DP][N] and zero padded,
// center [DP] (null: zeros).  Through the pinned stage to h->ps_gauss on `stream`, behind the last
// call that used the workspaces.
cv_status upload_gauss_tables(cv_hmm* h, int D, const double* mean, const double* var, const double* center,
                              hipStream_t stream, const double** tab) {
  const size_t N = (size_t)h->N, dp = (size_t)cvg::gauss_padded_dims(D), n = cvg::gauss_table_doubles(h->N, D);
  cv_status st = h->ps_gauss.ensure(n * 8);
  if (st != CV_OK) return st;
  double* const pin = reinterpret_cast<double*>(h->gs_pin.acquire(2 * n));
  if (!pin) return set_err(CV_ENOMEM, "pinned staging of %zu table entries failed", n);
  std::memset(pin, 0, n * 8);
  double *c = pin, *mu_t = pin + N, *w_t = mu_t + dp * N, *cen = w_t + dp * N;
  constexpr double kTwoPi = 6.283185307179586476925;
  parallel_ranges((int64_t)N, [&](int, int64_t lo, int64_t hi) {
    for (int64_t j = lo; j < hi; ++j) {
      double sum = 0.0;
      for (int d = 0; d < D; ++d) {
        const double v = var[(size_t)j * D + d];
        sum += std::log10(kTwoPi * v);
        mu_t[(size_t)d * N + j] = mean[(size_t)j * D + d];
        w_t[(size_t)d * N + j] = 1.0 / v;
      }
      c[j] = -0.5 * sum;
    }
  }, std::max<int64_t>(1, 65536 / D));
  for (int d = 0; center && d < D; ++d) cen[d] = center[d];
  if (h->ws_rec) HIP_TRY(hipStreamWaitEvent(stream, h->ws_done, 0));
  HIP_TRY(hipMemcpyAsync(h->ps_gauss.p, pin, n * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(h->gs_pin.release(stream));
  *tab = h->ps_gauss.as<const double>();
  return CV_OK;
}

// What a host entry wants back in the caller's arrays (null: not asked).
struct HostOut {
  double* loglik;
  uint8_t* status;
  int32_t* path = nullptr;
  double* gamma = nullptr;  // the gamma rows; with grad, the rows the gradient arm stores in their place
  int64_t gamma_ld = 0;     // 0: compact rows of N; else the caller's stride (its columns beyond N stay untouched)
  // pi_cnt set: the counts arm; b_cnt: the emission counts too.  grad: the gradient arm, weight
  // (host, [nseq], null: all 1) times every term of its sequence
  double *pi_cnt = nullptr, *a_cnt = nullptr, *b_cnt = nullptr;
  bool grad = false;
  const double* weight = nullptr;
  // cv_expected_counts_gauss (g_cnt set; with grad): the observation vectors x (host, element e at
  // x + e * ldx), the model's rows and the center (nullable), and the moments back
  const double *x = nullptr, *mean = nullptr, *var = nullptr, *center = nullptr;
  int64_t ldx = 0;
  int D = 0;
  double *g_cnt = nullptr, *m1 = nullptr, *m2 = nullptr;
};

// A host entry after its argument checks: the batch through the handle's staging (HostBatch;
// obs or the dense rows emis, whichever is given), the core on the st_* buffers, the results
// back, and CV_EINFEASIBLE for the first sequence of likelihood 0.  The counts ride in st_cnt as
// [pi N][a N * N][b N * V if asked][g_cnt N, m1 N * D, m2 N * D if asked][weight nseq if given],
// gamma compact in st_gamma; the rows of x compact in st_emis.
cv_status host_entry(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs, const double* emis,
                     int64_t ld, cv_opts o, const HostOut& out) {
  CV_LOCK(h);
  cv_status st = set_device(h);
  if (st != CV_OK) return st;
  const size_t N = (size_t)h->N, V = (size_t)h->V;
  if (nseq == 0) {  // the counts are overwritten, not accumulated
    if (out.pi_cnt) std::fill(out.pi_cnt, out.pi_cnt + N, 0.0);
    if (out.a_cnt) std::fill(out.a_cnt, out.a_cnt + N * N, 0.0);
    if (out.b_cnt) std::fill(out.b_cnt, out.b_cnt + N * V, 0.0);
    if (out.g_cnt) std::fill(out.g_cnt, out.g_cnt + N, 0.0);
    if (out.g_cnt) std::fill(out.m1, out.m1 + N * (size_t)out.D, 0.0);
    if (out.g_cnt) std::fill(out.m2, out.m2 + N * (size_t)out.D, 0.0);
    return CV_OK;
  }
  // the observations are range-checked on the device (CV_SEQ_BADOBS), as in the _device variants
  HostBatch hb{h, nseq, offsets, obs, call_stream(h, o)};
  if ((st = hb.stage(o, out.path ? 1 : 0, 1)) != CV_OK) return st;
  if (out.gamma && (st = h->st_gamma.ensure(hb.plane() * N * 8)) != CV_OK) return st;
  const size_t ND = N * (size_t)out.D, nb = out.b_cnt ? N * V : out.g_cnt ? N + 2 * ND : 0;
  if (out.pi_cnt && (st = h->st_cnt.ensure((N + N * N + nb + (out.weight ? (size_t)nseq : 0)) * 8)) != CV_OK) return st;
  EmisSrc src{};
  if (emis && (st = hb.stage_emis(emis, ld, &src)) != CV_OK) return st;
  GaussReq gs{};
  if (out.g_cnt) {
    const size_t Dd = (size_t)out.D, xrows = (size_t)(hb.total - hb.base);
    if ((st = h->st_emis.ensure(std::max<size_t>(xrows, 1) * Dd * 8)) != CV_OK) return st;
    if (xrows > 0)
      HIP_TRY(hipMemcpy2DAsync(h->st_emis.p, Dd * 8, out.x + (size_t)hb.base * (size_t)out.ldx, (size_t)out.ldx * 8, Dd * 8,
                               xrows, hipMemcpyHostToDevice, hb.stream));
    gs.x = rebased(h->st_emis.as<const double>(), hb.base, Dd);
    gs.ldx = out.D;
    gs.D = out.D;
    if ((st = upload_gauss_tables(h, out.D, out.mean, out.var, out.center, hb.stream, &gs.tab)) != CV_OK) return st;
    src.chunk_local = true;
  }
  double* const gamma_dev = out.gamma ? h->st_gamma.as<double>() : nullptr;
  CountsReq cnt{nullptr, nullptr};
  if (out.pi_cnt) {
    cnt.pi_cnt = h->st_cnt.as<double>();
    cnt.a_cnt = cnt.pi_cnt + N;
    if (out.b_cnt) cnt.b_cnt = cnt.a_cnt + N * N;
    if (out.g_cnt) {
      gs.g_cnt = cnt.a_cnt + N * N;
      gs.m1 = gs.g_cnt + N;
      gs.m2 = gs.m1 + ND;
      cnt.gauss = &gs;
    }
    if (out.weight) {
      double* const wd = cnt.a_cnt + N * N + nb;
      HIP_TRY(hipMemcpyAsync(wd, out.weight, (size_t)nseq * 8, hipMemcpyHostToDevice, hb.stream));
      cnt.weight = wd;
    }
    if (out.grad) {
      cnt.grad = true;
      cnt.egrad = gamma_dev;
      cnt.ld_grad = (int64_t)N;
    }
  }
  PostReq rq;
  rq.loglik = h->st_score.as<double>();
  rq.path = out.path ? h->st_path.as<int32_t>() : nullptr;
  rq.gamma = out.grad ? nullptr : gamma_dev;
  rq.status = h->st_status.as<uint8_t>();
  rq.stream = hb.stream;
  rq.emis = emis || out.g_cnt ? &src : nullptr;
  rq.cnt = out.pi_cnt ? &cnt : nullptr;
  st = posterior_device(h, nseq, offsets, h->st_off.as<int64_t>(), obs ? h->st_obs.as<int32_t>() : nullptr, o, rq);
  if (st != CV_OK) return hb.fail(st);
  if (out.path) hb.fetch_elems(out.path, h->st_path);
  const size_t rows = (size_t)(hb.total - hb.base);
  if (out.gamma && !out.gamma_ld) hb.fetch_elems(out.gamma, h->st_gamma, N);
  if (out.gamma && out.gamma_ld && rows && hb.err == hipSuccess)
    hb.err = hipMemcpy2DAsync(out.gamma + (size_t)hb.base * (size_t)out.gamma_ld, (size_t)out.gamma_ld * 8,
                              gamma_dev + (size_t)hb.base * N, N * 8, N * 8, rows, hipMemcpyDeviceToHost, hb.stream);
  hb.fetch_seqs(out.loglik, h->st_score);
  hb.fetch_seqs(out.status, h->st_status);
  if (out.pi_cnt) hb.fetch_n(out.pi_cnt, cnt.pi_cnt, N);
  if (out.pi_cnt) hb.fetch_n(out.a_cnt, cnt.a_cnt, N * N);
  if (out.b_cnt) hb.fetch_n(out.b_cnt, cnt.b_cnt, N * V);
  if (out.g_cnt) hb.fetch_n(out.g_cnt, (const double*)gs.g_cnt, N);
  if (out.g_cnt) hb.fetch_n(out.m1, (const double*)gs.m1, ND);
  if (out.g_cnt) hb.fetch_n(out.m2, (const double*)gs.m2, ND);
  if ((st = hb.finish()) != CV_OK) return st;
  return report_infeasible(nseq, out.status, "has likelihood 0");
}

}  // namespace

extern "C" {

CV_API cv_status cv_posterior_batch_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                           const int64_t* offsets_dev, const int32_t* obs_dev, const cv_opts* opts,
                                           double* loglik_dev, int32_t* path_dev, double* gamma_dev,
                                           uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (nseq > 0 && (!offsets_dev || !obs_dev || !loglik_dev || !status_dev))
    return set_err(CV_EINVAL, "null device buffer");
  PostReq rq;
  rq.loglik = loglik_dev;
  rq.path = path_dev;
  rq.gamma = gamma_dev;
  rq.status = status_dev;
  return device_entry(h, nseq, offsets_host, offsets_dev, obs_dev, opts ? *opts : default_opts(), rq);
}

// The options are checked by the core, after the empty batch has returned.
CV_API cv_status cv_posterior_batch(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                    const cv_opts* opts, double* loglik_out, int32_t* path_out, double* gamma_out,
                                    uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || (nseq > 0 && (!offsets || !obs || !loglik_out || !status_out)))
    return set_err(CV_EINVAL, "null argument");
  HostOut out{loglik_out, status_out};
  out.path = path_out;
  out.gamma = gamma_out;
  return host_entry(h, nseq, offsets, obs, nullptr, 0, opts ? *opts : default_opts(), out);
}

// ---- posterior path sampling: cv_sample_batch* -------------------------------------------------
// Forward filtering, backward sampling: the core's plan with the sampler in place of the backward pass.
CV_API cv_status cv_sample_batch_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                        const int64_t* offsets_dev, const int32_t* obs_dev, int32_t draws,
                                        uint64_t seed, int64_t seq_base, const cv_opts* opts, int32_t* path_dev,
                                        double* score_dev, double* loglik_dev, uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  cv_status st = sample_draws_ok(draws);
  if (st != CV_OK) return st;
  if (nseq > 0 && (!offsets_dev || !obs_dev || !path_dev || !status_dev)) return set_err(CV_EINVAL, "null device buffer");
  const SampleReq smp{draws, seed, seq_base, path_dev, score_dev};
  PostReq rq;
  rq.loglik = loglik_dev;
  rq.status = status_dev;
  rq.smp = &smp;
  return device_entry(h, nseq, offsets_host, offsets_dev, obs_dev, opts ? *opts : default_opts(), rq);
}

// Its own result path: the scores come back through pinned staging, so that an empty sequence's
// slots of score_out stay untouched.  The options are checked by the core, after the empty batch
// has returned.
CV_API cv_status cv_sample_batch(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs, int32_t draws,
                                 uint64_t seed, int64_t seq_base, const cv_opts* opts, int32_t* path_out,
                                 double* score_out, double* loglik_out, uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  cv_status st = sample_draws_ok(draws);
  if (st != CV_OK) return st;
  if (nseq < 0 || (nseq > 0 && (!offsets || !obs || !path_out || !status_out))) return set_err(CV_EINVAL, "null argument");
  CV_LOCK(h);
  if ((st = set_device(h)) != CV_OK) return st;
  cv_opts o = opts ? *opts : default_opts();
  if (nseq == 0) return CV_OK;
  const size_t R = (size_t)draws, B = (size_t)nseq;
  // the observations are range-checked on the device (CV_SEQ_BADOBS), as in the _device variant
  HostBatch hb{h, nseq, offsets, obs, call_stream(h, o)};
  // st_score: [nseq] log-likelihoods, then the [R][nseq] score planes
  if ((st = hb.stage(o, R, R + 1)) != CV_OK) return st;
  double* const ll_dev = h->st_score.as<double>();
  const SampleReq smp{draws, seed, seq_base, h->st_path.as<int32_t>(), score_out ? ll_dev + B : nullptr};
  PostReq rq;
  rq.loglik = ll_dev;
  rq.status = h->st_status.as<uint8_t>();
  rq.stream = hb.stream;
  rq.smp = &smp;
  st = posterior_device(h, nseq, offsets, h->st_off.as<int64_t>(), h->st_obs.as<int32_t>(), o, rq);
  if (st != CV_OK) return hb.fail(st);
  for (size_t r = 0; r < R; ++r)  // plane r of the staging and of path_out: offsets[nseq] elements each
    hb.fetch_elems(path_out, h->st_path, 1, r);
  const size_t nsc = (score_out ? R * B : 0) + B;
  if (!h->sm_pin.ensure(nsc * 8)) return hb.fail(set_err(CV_ENOMEM, "pinned staging of %zu scores failed", nsc));
  double* const pin = h->sm_pin.as<double>();
  if (hb.err == hipSuccess) hb.err = hipMemcpyAsync(pin, ll_dev, nsc * 8, hipMemcpyDeviceToHost, hb.stream);
  hb.fetch_seqs(status_out, h->st_status);
  if ((st = hb.finish()) != CV_OK) return st;
  if (loglik_out) std::memcpy(loglik_out, pin, B * 8);
  for (size_t s = 0; score_out && s < B; ++s)
    if (status_out[s] != CV_SEQ_EMPTY)
      for (size_t r = 0; r < R; ++r) score_out[r * B + s] = pin[B + r * B + s];
  return report_infeasible(nseq, status_out, "has likelihood 0");
}

// ---- evaluation under caller-supplied emission scores: cv_posterior_emissions* ----------------
CV_API cv_status cv_posterior_emissions_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                               const int64_t* offsets_dev, const double* emis_dev, int64_t ld,
                                               const cv_opts* opts, double* loglik_dev, int32_t* path_dev,
                                               double* gamma_dev, uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (nseq > 0 && (!offsets_dev || !emis_dev || !loglik_dev || !status_dev))
    return set_err(CV_EINVAL, "null device buffer");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_emissions_args_ok(h, ld, o);
  if (st != CV_OK) return st;
  const EmisSrc src{emis_dev, ld};
  PostReq rq;
  rq.loglik = loglik_dev;
  rq.path = path_dev;
  rq.gamma = gamma_dev;
  rq.status = status_dev;
  rq.emis = &src;
  return device_entry(h, nseq, offsets_host, offsets_dev, nullptr, o, rq);
}

CV_API cv_status cv_posterior_emissions(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* emis,
                                        int64_t ld, const cv_opts* opts, double* loglik_out, int32_t* path_out,
                                        double* gamma_out, uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || (nseq > 0 && (!offsets || !emis || !loglik_out || !status_out)))
    return set_err(CV_EINVAL, "null argument");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_emissions_args_ok(h, ld, o);
  if (st != CV_OK) return st;
  HostOut out{loglik_out, status_out};
  out.path = path_out;
  out.gamma = gamma_out;
  return host_entry(h, nseq, offsets, nullptr, emis, ld, o, out);
}

// ---- expected counts for EM: cv_expected_counts* -----------------------------------------------
// The posterior entries with the counts request in place of the path: pi_cnt [N] and a_cnt [N][N].
CV_API cv_status cv_expected_counts_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                           const int64_t* offsets_dev, const int32_t* obs_dev, const cv_opts* opts,
                                           double* loglik_dev, double* pi_cnt_dev, double* a_cnt_dev, double* gamma_dev,
                                           uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (!pi_cnt_dev || !a_cnt_dev) return set_err(CV_EINVAL, "null device buffer");
  if (nseq > 0 && (!offsets_dev || !obs_dev || !loglik_dev || !status_dev)) return set_err(CV_EINVAL, "null device buffer");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_opts_ok(h, o);
  if (st != CV_OK) return st;
  const CountsReq cnt{pi_cnt_dev, a_cnt_dev};
  PostReq rq;
  rq.loglik = loglik_dev;
  rq.gamma = gamma_dev;
  rq.status = status_dev;
  rq.cnt = &cnt;
  return device_entry(h, nseq, offsets_host, offsets_dev, obs_dev, o, rq);
}

CV_API cv_status cv_expected_counts(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                    const cv_opts* opts, double* loglik_out, double* pi_cnt_out, double* a_cnt_out,
                                    double* gamma_out, uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || !pi_cnt_out || !a_cnt_out) return set_err(CV_EINVAL, "null argument");
  if (nseq > 0 && (!offsets || !obs || !loglik_out || !status_out)) return set_err(CV_EINVAL, "null argument");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_opts_ok(h, o);
  if (st != CV_OK) return st;
  HostOut out{loglik_out, status_out};
  out.gamma = gamma_out;
  out.pi_cnt = pi_cnt_out;
  out.a_cnt = a_cnt_out;
  return host_entry(h, nseq, offsets, obs, nullptr, 0, o, out);
}

CV_API cv_status cv_expected_counts_emissions_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                                     const int64_t* offsets_dev, const double* emis_dev, int64_t ld,
                                                     const cv_opts* opts, double* loglik_dev, double* pi_cnt_dev,
                                                     double* a_cnt_dev, double* gamma_dev, uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (!pi_cnt_dev || !a_cnt_dev) return set_err(CV_EINVAL, "null device buffer");
  if (nseq > 0 && (!offsets_dev || !emis_dev || !loglik_dev || !status_dev)) return set_err(CV_EINVAL, "null device buffer");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_emissions_args_ok(h, ld, o);
  if (st != CV_OK) return st;
  const EmisSrc src{emis_dev, ld};
  const CountsReq cnt{pi_cnt_dev, a_cnt_dev};
  PostReq rq;
  rq.loglik = loglik_dev;
  rq.gamma = gamma_dev;
  rq.status = status_dev;
  rq.emis = &src;
  rq.cnt = &cnt;
  return device_entry(h, nseq, offsets_host, offsets_dev, nullptr, o, rq);
}

CV_API cv_status cv_expected_counts_emissions(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* emis,
                                              int64_t ld, const cv_opts* opts, double* loglik_out, double* pi_cnt_out,
                                              double* a_cnt_out, double* gamma_out, uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || !pi_cnt_out || !a_cnt_out) return set_err(CV_EINVAL, "null argument");
  if (nseq > 0 && (!offsets || !emis || !loglik_out || !status_out)) return set_err(CV_EINVAL, "null argument");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_emissions_args_ok(h, ld, o);
  if (st != CV_OK) return st;
  HostOut out{loglik_out, status_out};
  out.gamma = gamma_out;
  out.pi_cnt = pi_cnt_out;
  out.a_cnt = a_cnt_out;
  return host_entry(h, nseq, offsets, nullptr, emis, ld, o, out);
}

// ---- likelihood gradients under emission scores: cv_loglik_grad_emissions* ---------------------
// The dense expected-counts entries with the gradient request: per-sequence weights (null: all 1)
// and the gradient rows of E at the caller's stride in place of gamma.
CV_API cv_status cv_loglik_grad_emissions_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                                 const int64_t* offsets_dev, const double* emis_dev, int64_t ld,
                                                 const double* weight_dev, const cv_opts* opts, double* loglik_dev,
                                                 double* pi_grad_dev, double* a_grad_dev, double* emis_grad_dev,
                                                 int64_t ld_grad, uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (!pi_grad_dev || !a_grad_dev) return set_err(CV_EINVAL, "null device buffer");
  if (nseq > 0 && (!offsets_dev || !emis_dev || !loglik_dev || !status_dev)) return set_err(CV_EINVAL, "null device buffer");
  if (emis_grad_dev && ld_grad < h->N)
    return set_err(CV_EINVAL, "ld_grad = %lld is less than N = %d", (long long)ld_grad, h->N);
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_emissions_args_ok(h, ld, o);
  if (st != CV_OK) return st;
  const EmisSrc src{emis_dev, ld};
  CountsReq cnt{pi_grad_dev, a_grad_dev};
  cnt.grad = true;
  cnt.weight = weight_dev;
  cnt.egrad = emis_grad_dev;
  cnt.ld_grad = ld_grad;
  PostReq rq;
  rq.loglik = loglik_dev;
  rq.status = status_dev;
  rq.emis = &src;
  rq.cnt = &cnt;
  return device_entry(h, nseq, offsets_host, offsets_dev, nullptr, o, rq);
}

// Host arrays: the gradient rows are staged compact and copied back at the caller's stride.
CV_API cv_status cv_loglik_grad_emissions(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* emis, int64_t ld,
                                          const double* weight, const cv_opts* opts, double* loglik_out,
                                          double* pi_grad_out, double* a_grad_out, double* emis_grad_out,
                                          int64_t ld_grad, uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || !pi_grad_out || !a_grad_out) return set_err(CV_EINVAL, "null argument");
  if (nseq > 0 && (!offsets || !emis || !loglik_out || !status_out)) return set_err(CV_EINVAL, "null argument");
  if (emis_grad_out && ld_grad < h->N)
    return set_err(CV_EINVAL, "ld_grad = %lld is less than N = %d", (long long)ld_grad, h->N);
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_emissions_args_ok(h, ld, o);
  if (st != CV_OK) return st;
  HostOut out{loglik_out, status_out};
  out.gamma = emis_grad_out;
  out.gamma_ld = ld_grad;
  out.pi_cnt = pi_grad_out;
  out.a_cnt = a_grad_out;
  out.grad = true;
  out.weight = weight;
  return host_entry(h, nseq, offsets, nullptr, emis, ld, o, out);
}

// ---- expected counts of the whole discrete model: cv_expected_counts_model* --------------------
// cv_expected_counts* with per-sequence weights (null: all 1) and the emission counts b_cnt [N][V]:
// the gradient arm on the handle's own b, its rows w_s gamma scattered by observation (bcount.hip).
CV_API cv_status cv_expected_counts_model_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                                 const int64_t* offsets_dev, const int32_t* obs_dev,
                                                 const double* weight_dev, const cv_opts* opts, double* loglik_dev,
                                                 double* pi_cnt_dev, double* a_cnt_dev, double* b_cnt_dev,
                                                 double* gamma_dev, uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (!pi_cnt_dev || !a_cnt_dev || !b_cnt_dev) return set_err(CV_EINVAL, "null device buffer");
  if (nseq > 0 && (!offsets_dev || !obs_dev || !loglik_dev || !status_dev)) return set_err(CV_EINVAL, "null device buffer");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_opts_ok(h, o);
  if (st != CV_OK) return st;
  CountsReq cnt{pi_cnt_dev, a_cnt_dev};
  cnt.grad = true;
  cnt.weight = weight_dev;
  cnt.egrad = gamma_dev;
  cnt.ld_grad = h->N;
  cnt.b_cnt = b_cnt_dev;
  PostReq rq;
  rq.loglik = loglik_dev;
  rq.status = status_dev;
  rq.cnt = &cnt;
  return device_entry(h, nseq, offsets_host, offsets_dev, obs_dev, o, rq);
}

CV_API cv_status cv_expected_counts_model(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                          const double* weight, const cv_opts* opts, double* loglik_out,
                                          double* pi_cnt_out, double* a_cnt_out, double* b_cnt_out, double* gamma_out,
                                          uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || !pi_cnt_out || !a_cnt_out || !b_cnt_out) return set_err(CV_EINVAL, "null argument");
  if (nseq > 0 && (!offsets || !obs || !loglik_out || !status_out)) return set_err(CV_EINVAL, "null argument");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = posterior_opts_ok(h, o);
  if (st != CV_OK) return st;
  HostOut out{loglik_out, status_out};
  out.gamma = gamma_out;
  out.pi_cnt = pi_cnt_out;
  out.a_cnt = a_cnt_out;
  out.b_cnt = b_cnt_out;
  out.grad = true;
  out.weight = weight;
  return host_entry(h, nseq, offsets, obs, nullptr, 0, o, out);
}

// ---- Gaussian emissions: cv_gauss_emissions*, cv_expected_counts_gauss* ------------------------
CV_API cv_status cv_gauss_emissions_device(cv_hmm* h, int64_t nrows, const double* x_dev, int64_t ldx, int64_t D,
                                           const double* mean, const double* var, const cv_opts* opts,
                                           double* emis_dev, int64_t ld) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nrows < 0) return set_err(CV_EINVAL, "nrows < 0");
  if (ld < h->N) return set_err(CV_EINVAL, "ld = %lld is less than N = %d", (long long)ld, h->N);
  cv_status st = gauss_args_ok(h, ldx, D, mean, var);
  if (st != CV_OK) return st;
  if (nrows > 0 && (!x_dev || !emis_dev)) return set_err(CV_EINVAL, "null device buffer");
  if (nrows == 0) return CV_OK;
  const cv_opts o = opts ? *opts : default_opts();
  CV_LOCK(h);
  if ((st = set_device(h)) != CV_OK) return st;
  const hipStream_t stream = call_stream(h, o);
  const double* tab = nullptr;
  if ((st = upload_gauss_tables(h, (int)D, mean, var, nullptr, stream, &tab)) != CV_OK) return st;
  if ((st = launch_density(h, tab, x_dev, ldx, (int)D, nrows, emis_dev, ld, stream)) != CV_OK) return st;
  return end_call(h, false, 0, stream);  // the tables stay in use until here
}

// Host arrays: the rows of x go compact to st_emis, the scores come back at the caller's stride.
CV_API cv_status cv_gauss_emissions(cv_hmm* h, int64_t nrows, const double* x, int64_t ldx, int64_t D,
                                    const double* mean, const double* var, double* emis_out, int64_t ld) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nrows < 0) return set_err(CV_EINVAL, "nrows < 0");
  if (ld < h->N) return set_err(CV_EINVAL, "ld = %lld is less than N = %d", (long long)ld, h->N);
  cv_status st = gauss_args_ok(h, ldx, D, mean, var);
  if (st != CV_OK) return st;
  if (nrows > 0 && (!x || !emis_out)) return set_err(CV_EINVAL, "null argument");
  if (nrows == 0) return CV_OK;
  CV_LOCK(h);
  if ((st = set_device(h)) != CV_OK) return st;
  const hipStream_t stream = h->stream;
  const size_t N = (size_t)h->N, Dd = (size_t)D, rows = (size_t)nrows;
  if ((st = h->st_emis.ensure(rows * Dd * 8)) != CV_OK) return st;
  if ((st = h->st_gamma.ensure(rows * N * 8)) != CV_OK) return st;
  if (h->ws_rec) HIP_TRY(hipStreamWaitEvent(stream, h->ws_done, 0));
  HIP_TRY(hipMemcpy2DAsync(h->st_emis.p, Dd * 8, x, (size_t)ldx * 8, Dd * 8, rows, hipMemcpyHostToDevice, stream));
  const double* tab = nullptr;
  if ((st = upload_gauss_tables(h, (int)D, mean, var, nullptr, stream, &tab)) == CV_OK)
    st = launch_density(h, tab, h->st_emis.as<const double>(), D, (int)D, nrows, h->st_gamma.as<double>(), (int64_t)N, stream);
  if (st == CV_OK) st = end_call(h, false, 0, stream);
  if (st != CV_OK) {
    (void)hipStreamSynchronize(stream);
    return st;
  }
  HIP_TRY(hipMemcpy2DAsync(emis_out, (size_t)ld * 8, h->st_gamma.p, N * 8, N * 8, rows, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return CV_OK;
}

// The gradient arm under densities computed per chunk, plus the moments: the counts request with
// its Gaussian arm.
CV_API cv_status cv_expected_counts_gauss_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                                 const int64_t* offsets_dev, const double* x_dev, int64_t ldx, int64_t D,
                                                 const double* mean, const double* var, const double* weight_dev,
                                                 const double* center, const cv_opts* opts, double* loglik_dev,
                                                 double* pi_cnt_dev, double* a_cnt_dev, double* g_cnt_dev,
                                                 double* m1_dev, double* m2_dev, double* gamma_dev, uint8_t* status_dev) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0) return set_err(CV_EINVAL, "nseq < 0");
  if (!pi_cnt_dev || !a_cnt_dev || !g_cnt_dev || !m1_dev || !m2_dev) return set_err(CV_EINVAL, "null device buffer");
  if (nseq > 0 && (!offsets_dev || !x_dev || !loglik_dev || !status_dev)) return set_err(CV_EINVAL, "null device buffer");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = gauss_args_ok(h, ldx, D, mean, var);
  if (st != CV_OK) return st;
  if ((st = posterior_opts_ok(h, o)) != CV_OK) return st;
  CV_LOCK(h);
  if ((st = set_device(h)) != CV_OK) return st;
  GaussReq gs{x_dev, ldx, (int)D, nullptr, g_cnt_dev, m1_dev, m2_dev};
  const hipStream_t stream = call_stream(h, o);
  if (nseq > 0 && (st = upload_gauss_tables(h, (int)D, mean, var, center, stream, &gs.tab)) != CV_OK) return st;
  EmisSrc src{};
  src.chunk_local = true;
  CountsReq cnt{pi_cnt_dev, a_cnt_dev};
  cnt.grad = true;
  cnt.weight = weight_dev;
  cnt.egrad = gamma_dev;
  cnt.ld_grad = h->N;
  cnt.gauss = &gs;
  PostReq rq;
  rq.loglik = loglik_dev;
  rq.status = status_dev;
  rq.stream = stream;
  rq.emis = &src;
  rq.cnt = &cnt;
  return posterior_device(h, nseq, offsets_host, offsets_dev, nullptr, o, rq);
}

CV_API cv_status cv_expected_counts_gauss(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* x, int64_t ldx,
                                          int64_t D, const double* mean, const double* var, const double* weight,
                                          const double* center, const cv_opts* opts, double* loglik_out,
                                          double* pi_cnt_out, double* a_cnt_out, double* g_cnt_out, double* m1_out,
                                          double* m2_out, double* gamma_out, uint8_t* status_out) {
  if (!h) return set_err(CV_EINVAL, "null handle");
  if (nseq < 0 || !pi_cnt_out || !a_cnt_out || !g_cnt_out || !m1_out || !m2_out) return set_err(CV_EINVAL, "null argument");
  if (nseq > 0 && (!offsets || !x || !loglik_out || !status_out)) return set_err(CV_EINVAL, "null argument");
  const cv_opts o = opts ? *opts : default_opts();
  cv_status st = gauss_args_ok(h, ldx, D, mean, var);
  if (st != CV_OK) return st;
  if ((st = posterior_opts_ok(h, o)) != CV_OK) return st;
  HostOut out{loglik_out, status_out};
  out.gamma = gamma_out;
  out.pi_cnt = pi_cnt_out;
  out.a_cnt = a_cnt_out;
  out.grad = true;
  out.weight = weight;
  out.x = x;
  out.ldx = ldx;
  out.D = (int)D;
  out.mean = mean;
  out.var = var;
  out.center = center;
  out.g_cnt = g_cnt_out;
  out.m1 = m1_out;
  out.m2 = m2_out;
  return host_entry(h, nseq, offsets, nullptr, nullptr, 0, o, out);
}

}  // extern "C"
