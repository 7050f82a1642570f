/*
 * cviterbi.h -- C ABI of the MI355X-native consistent-viterbi decode path.
 *
 * This is the drop-in boundary for the reference's viterbi_solver forward pass over
 * hmm::HMM (AlexandreDubray/consistent-viterbi).  The reference is a Rust crate with
 * no FFI of its own; every entry point below names the Rust item it replaces, so a
 * Rust `extern "C"` binding can stand in for it.  Plain pointers and
 * sizes only; no torch or HIP types in the signatures (streams are opaque void*).
 *
 * Conventions
 *  - Probabilities are log10 doubles, -inf for zero (src/hmm/hmm.rs:192-205); JSON
 *    `null` reads as -inf (hmm.rs:248-264).
 *  - a[from*N + to] (hmm.rs:220-226), b[state*V + obs] with obs flattened row-major
 *    over bdims exactly as ndarray indexes `b[state][&obs[..]]` (hmm.rs:228-230).
 *  - Sequences are CSR: offsets[nseq+1] (int64, element offsets), obs[offsets[nseq]]
 *    (int32 flattened observation indices).  Paths are int32 per element.
 *  - Functions return cv_status; cv_last_error() has a message for the calling thread.
 *    Nothing aborts (the reference panics: cp.rs:87, dp.rs:184-186, unwraps).
 */
#ifndef CVITERBI_H
#define CVITERBI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CV_API __attribute__((visibility("default")))
#define CV_ABI_VERSION 1

typedef enum cv_status {
  CV_OK = 0,
  CV_EINVAL = 1,        /* bad argument (shape, range, NaN/+inf log-prob, obs out of range) */
  CV_EDEVICE = 2,       /* HIP runtime error or no usable gfx950 device */
  CV_ENOMEM = 3,        /* host or device allocation failed */
  CV_EINFEASIBLE = 4,   /* at least one sequence has no finite-probability path */
  CV_EIO = 5,           /* file could not be read / written */
  CV_EPARSE = 6,        /* malformed hmm.json */
  CV_EUNSUPPORTED = 7,  /* valid request this build does not implement */
  CV_EINTERNAL = 8,
  CV_ELIMIT = 9         /* search limit reached (constrained decode: branch-and-bound nodes) */
} cv_status;

/* per-sequence status_out values */
enum { CV_SEQ_OK = 0, CV_SEQ_INFEASIBLE = 1, CV_SEQ_EMPTY = 2, CV_SEQ_BADOBS = 3 };

/* arithmetic type of the trellis recurrence */
enum { CV_DTYPE_F32 = 0, CV_DTYPE_F64 = 1 };

/* association of the recurrence:
 *  VITERBI  d' = max_i(d[i] + a[i,j]) + b[j,o]      viterbi.rs:13-18 order, pi init cp.rs:66-68
 *  CP       d' = d[psi] + (a[psi,j] + b[j,o])       CPSolver::init_viterbi cp.rs:63-83
 *  DP       d' = max_i((a[i,j] + b[j,o]) + d[i])    DPSolver::solve dp.rs:127-182 (first index)
 *  DECODE   VITERBI with row 0 = 0.0                viterbi::decode viterbi.rs:5-32 */
enum { CV_ASSOC_VITERBI = 0, CV_ASSOC_CP = 1, CV_ASSOC_DP = 2, CV_ASSOC_DECODE = 3 };

/* kernel choice: AUTO picks TRELLIS (register-resident A, f32, VITERBI, N <= 256) when it
 * applies, then TRELLIS_F64 (exact f64: any association for N <= 256, forced states with
 * VITERBI only; one wave per 2/4/8 sequences, A streamed from L2.  Above 256, VITERBI /
 * DECODE / DP without forced states (VITERBI with them) as pairs of waves at NP = 512 or quads
 * at NP = 1,024; AUTO takes NP = 512 for N >= 384 or >= 8,192 sequences and NP = 1,024 for
 * N > 724, tuning keys t64_512 / t64_1024; an explicit TRELLIS_F64 gets it for any N <= 1,024),
 * else GENERIC (f32/f64, any association, N <= 65535: one workgroup per sequence with two rows
 * of N in LDS, or above N = 1024 -- always above 20480 f32 / 10240 f64 -- wide: one launch per
 * step, each sequence's states over ceil(N / 256) workgroups, rows in global memory). */
enum { CV_KERNEL_AUTO = 0, CV_KERNEL_TRELLIS = 1, CV_KERNEL_GENERIC = 2, CV_KERNEL_TRELLIS_F64 = 3 };

/* cv_opts.flags */
/* bit 0 and bits 8-15 are reserved (they selected the retired MFMA-assisted f32 trellis,
 * measured slower than the all-VALU one on gfx950; setting them is CV_EUNSUPPORTED) */
#define CV_FLAG_SERIAL 0x2u       /* one stream, fewest chunks: no forward/backtrack overlap */
#define CV_FLAG_NO_PAIR 0x4u      /* one sequence per forward workgroup (A/B knob; bit-identical) */
#define CV_FLAG_NO_WAVE 0x8u      /* N <= 64: the workgroup kernels instead of one wave per sequence
                                     with the backtrack fused (A/B knob; bit-identical) */
#define CV_FLAG_NO_T64 0x10u     /* f64: the generic kernel instead of TRELLIS_F64 (A/B knob;
                                     bit-identical) */

typedef struct cv_hmm cv_hmm;
typedef struct cv_solver cv_solver;

/* Model description; arrays are copied.  Replaces the fields of struct HMM<D>
 * (hmm.rs:10-18: a: Array2<f64>, b: Array1<ArrayD<f64>>, pi: Array1<f64>). */
typedef struct cv_hmm_desc {
  int32_t nstates;       /* N */
  int32_t ndims;         /* D (const generic of HMM<D>) */
  const int64_t* bdims;  /* [D] shape of each state's emission array (hmm.rs:225) */
  const double* pi;      /* [N]   log10 */
  const double* a;       /* [N*N] log10, from-major */
  const double* b;       /* [N*V] log10, V = prod(bdims) */
  int32_t device;        /* HIP device ordinal */
} cv_hmm_desc;

typedef struct cv_opts {
  int32_t dtype;         /* CV_DTYPE_F64 (default: the reference's arithmetic, hmm.rs:10-18;
                            paths and scores bit-identical to the f64 recurrence) or
                            CV_DTYPE_F32 (the f32 trellis, ~2x faster, paths may differ) */
  int32_t assoc;         /* CV_ASSOC_VITERBI (default) */
  int32_t kernel;        /* CV_KERNEL_AUTO (default) */
  int32_t rescore_f64;   /* 1 (default): score_out = f64 re-score of the decoded path with
                            the VITERBI association (what the f64 reference computes along
                            that path); 0: the kernel's own score (f32 widened for F32) */
  void* stream;          /* hipStream_t for the *_device entry points; NULL = handle stream */
  uint64_t workspace_bytes; /* delta/psi workspace cap; 0 = default (8 GiB; 64 GiB for TRELLIS_F64) */
  uint32_t flags;        /* CV_FLAG_* (0 = defaults) */
  const int32_t* forced; /* [sum T] nullable: -1 = free, s >= 0 = state s forced at that element
                            (host pointer for cv_decode_batch, device pointer for *_device) */
} cv_opts;

typedef struct cv_timing {
  double fwd_ms;         /* forward kernel(s), device time, last decode call */
  double bt_ms;          /* backtrack (+ f64 re-score) kernel(s) */
  double total_ms;       /* first kernel start to last kernel end (device) */
  int64_t launches;      /* forward launches (chunks) */
  int32_t kernel;        /* CV_KERNEL_TRELLIS, _TRELLIS_F64 or _GENERIC actually used */
  int32_t padded_states; /* NP of the trellis kernel (0 for generic) */
  int32_t mfma_tiles;    /* TRELLIS_F64: sequences per forward wave (last chunk), 0 = the few-sequence
                            layout (two per 16-wave workgroup, key t64_few); GENERIC: 0 wide
                            (each step over many workgroups, N > 10240 f64 / 20480 f32), else -1;
                            -1 otherwise (the field name is kept for ABI stability) */
} cv_timing;

typedef struct cv_superseq_desc {
  /* The super-sequence of viterbi_solver/utils.rs:49-58 in element order: sequences
   * concatenated (after reordering), each element carrying MetaElements fields. */
  int64_t nseq;
  const int64_t* offsets;    /* [nseq+1] */
  const int32_t* obs;        /* [offsets[nseq]] flattened observation index (value) */
  const int64_t* seq_id;     /* [nseq] original sequence id (MetaElements::seq) or NULL = 0..nseq-1 */
  const int32_t* component;  /* [elements] constraint_component, -1 = none; NULL = none */
  const uint8_t* active;     /* [elements] active_cstr; NULL = all inactive */
} cv_superseq_desc;

/* ---- library ---------------------------------------------------------------------- */
CV_API const char* cv_last_error(void);
CV_API const char* cv_version(void);
CV_API int32_t cv_abi_version(void);
CV_API int32_t cv_device_count(void);
/* Device memory this process's library holds (handles' tables and workspaces, call buffers):
 * now and at most since load (either pointer may be NULL). */
CV_API cv_status cv_device_memory(int64_t* current_bytes, int64_t* peak_bytes);
CV_API void cv_opts_init(cv_opts* opts);

/* ---- hmm::HMM (src/hmm/hmm.rs) ------------------------------------------------------- */
/* HMM struct construction (hmm.rs:10-18). */
CV_API cv_status cv_hmm_create(const cv_hmm_desc* desc, cv_hmm** out);
/* HMM::from_json (hmm.rs:242-245 + null->-inf parsers 248-264). */
CV_API cv_status cv_hmm_from_json(const char* path, int32_t device, cv_hmm** out);
/* HMM::write (hmm.rs:236-240): serde_json layout, -inf written as null. */
CV_API cv_status cv_hmm_write_json(const cv_hmm* h, const char* path);
CV_API void cv_hmm_destroy(cv_hmm* h);
/* HMM::nstates (hmm.rs:207-209). */
/* ---- tuning keys (per handle) ------------------------------------------------------------
 * Layout, schedule and A/B choices of the kernels, and the test hooks that force a code path.
 * None changes a decode's result: every key is bit-identical in paths, scores and statuses (the
 * fitting keys bw_*: to the fitting tolerance, see the end of the list).  Each handle
 * holds ONE snapshot, taken at cv_hmm_create / cv_hmm_from_json from the environment
 * (variable CV_<KEY> in upper case, e.g. CV_T64_S=4 for "t64_s"; integers) over the defaults
 * below, and changed afterwards only by cv_hmm_set_tuning: an environment variable set after
 * the handle exists changes nothing, and no kernel launch reads the environment.  The
 * handle-less cv_hmm_fit_* read the environment once per call.
 *   trace 0               1: host phase stamps on stderr
 *   host_threads 0        host worker threads (0: min(16, hardware threads))
 *   t64_nonpos 1          0: the general f64 backtrack interval test (and no parallel chain)
 *   generic_rows 1        0: generic kernels in psi mode (inline argmax) instead of rows mode
 *   max_chunks 8          f32 trellis pipeline depth (1..64)
 *   emis_overlap 0        1: cv_decode_emissions* on the f64 trellis, more than one chunk: the next chunk
 *                         staged on a second stream beside the current forward pass, out of a second
 *                         staging buffer under the same cap (2% faster at equal chunks; the cap then
 *                         splits the batch into more chunks, which can cost far more: DESIGN.md)
 *   host_sums 0           1: the constrained decode's exact unary sums on the host
 *   no_trace / no_resume / no_side 0   1: no certified suffix trace / resume flow / side-stream decode
 *   chain_par 1           0: cv_decode_superseq_cp runs the serial chain kernel
 *   chain_old 0           1: the one-thread-per-state chain kernel at any N
 *   chain_par_force 0     m > 0: every m-th sequence of the parallel chain taken as uncertified
 *   chain_spec 1          0: no speculative re-decode in the parallel chain
 *   chain_spec_kernel 0   the parallel chain's speculative re-decodes where N <= 256: 0 the serial chain
 *                         kernel's layout batched (one sequence per CU) after the forward passes and
 *                         cp_spec_psi (one sequence per workgroup, ~20 KiB of LDS) beside them;
 *                         1 trellis_cp_f64; 2 the generic CP kernel (always so above N = 256)
 *   chain_copy_overlap 1  0: the parallel chain in one decode chunk, its path copy before the walk
 *   chain_cert_fused 1    0: the chain's certificates by their own pass (cp_cert_f64), not the backtrack
 *   chain_parts 1         0: the parallel chain's decode in one part; 1: where N <= 256 and the batch
 *                         spans more than a forward round, a large first part then chain_tail small
 *                         parts (each walked beside the next part's forward pass); 2: one round each
 *   chain_tail 2, chain_tail_div 2       chain_parts = 1: the number of small parts, and a small
 *                         part's size as a forward round (64 sequences per CU) / chain_tail_div
 *   chain_spec_prio 3     issue priority (s_setprio 1..3; 0 the default) of the parallel chain's
 *                         speculative batches beside a forward pass
 *   chain_pin_obs 0, chain_pin_path 0   1: the parallel chain's later parts' observations / its
 *                         path copy through pinned staging (82 MiB of pinned host memory per handle)
 *                         instead of the runtime's pageable copies (measured neutral; the pageable
 *                         default keeps a first call ~20-70 ms shorter)
 *   t64_s 0               f64 trellis sequences per wave 2 / 4 / 6 / 8 (0: by batch)
 *   t64_512 / t64_1024 -1 NP = 512 / 1,024 batch kernel: -1 auto, 0 never, 1 always
 *   t64_wg 1              0: one wave per workgroup instead of eight-wave units
 *   t64_wg_force 0        1: eight-wave units whatever the batch's lengths
 *   t64_rs 1 / t64_w2 1   0: no row-split / no pair-of-waves small-batch layout
 *   t64_few -1            f64 row A0 at 192 < N <= 256: the few-sequence forward (one CU per two
 *                         sequences, A streamed from L2 once per workgroup-step): -1 auto, 0 never,
 *                         1 whenever supported
 *   t64_wave 1            0: N <= 64 on the lock-step kernel, not one wave per sequence; 2: N <= 48
 *                         on the 64-state one-wave kernel
 *   t64_bal 8             steps between SIMD-balancing updates (0: off)
 *   t64_cp_s 0            trellis_cp_f64 sequences per wave 1 / 2 / 4 (0: by batch)
 *   t64_cp_w 0            trellis_cp_f64 waves splitting the columns: 1 never, > 1 always (0: up to
 *                         4,096 sequences, NP >= 128); t64_cp_pf 0: its A rows in flight 32 (16)
 *   t64_bt_pf 0           backtrack_f64 rows in flight 2 / 4 / 8 / 16 / 32 (0: by NP).  Any value is
 *                         accepted: the deepest of these depths not above the request that the layout
 *                         has (32 at NP = 64 only, at most 16 up to NP = 256 and for the sparse low
 *                         planes, 8 at NP = 512, 4 at NP = 1,024); a request below 2: by NP
 *   t64_lo_every 8        cv_decode_batch[_device], f64 row A0 on log-probability models, 64 < N <= 256:
 *                         the forward pass writes the low words of its delta rows at every K-th row
 *                         and the last row only (K <= 16; 1: at every row, the earlier behaviour), and
 *                         the backtrack recomputes the few exact values a near tie on another row
 *                         needs (cv_last_t64_stats).  A handle whose call replayed rows densely more
 *                         than once per 64 sequences (models full of exact ties) runs at 1 from then on
 *   t64_fixed_first 16777216   cv_decode_batch[_device], f64 row A0 without forced states on
 *                         log-probability models, 224 < N <= 256: a call of at least this many elements
 *                         (sum of lengths) first decodes in 32-bit fixed point and keeps every sequence
 *                         whose path that pass certifies as the f64 decode's own; the others run on the
 *                         f64 kernels (cv_last_fixed_first_stats).  Such a call waits for its stream
 *                         once.  A handle that left more than 1 in 8 sequences of a call uncertified
 *                         stays on the f64 kernels from then on.  0: never (the earlier behaviour)
 *   t64_f32ru_first 16777216   the same calls: one of at least this many elements takes the
 *                         certified f32 round-up first pass instead (every f32 add rounded toward +inf,
 *                         so every row is an upper bound; the f64 fold along the path certifies it);
 *                         a call below it follows t64_fixed_first.  Same counters, guard and fallback
 *                         (cv_last_first_pass_kind says which pass ran).  0: never
 *   t64_f32ru_mu_every 4  that pass's forward shifts every row by a per-sequence prediction of the
 *                         drift per step and takes the row maximum, which corrects it, at every K-th
 *                         step only: the nearest of K = 1 / 4 / 8 (<= 0: the default).  The rows and
 *                         shifts it stores differ with K; what a decode returns does not
 *   t64_fixed_chunks 8    either pass in chunks pipelined over two streams: at least
 *                         min(this, sequences / 2048) chunks (<= 64) out of a double-buffered workspace
 *                         (each chunk half the workspace cap), a chunk's certificate backtrack and score
 *                         beside the next chunk's forward.  0: the chunks back to back on the caller's
 *                         stream, one chunk where the batch fits the cap (the earlier schedule)
 *   generic_s 0           generic kernels' sequences per workgroup 1 / 2 / 4 (0: by batch)
 *   generic_split 0, generic_split_k 0   1: K threads per state (generic_fwd_split), its K
 *   generic_wide 1, generic_wide_min 0   0: never wide / > 0: wide from this N
 *   generic_prio 0        1: generic_fwd_ms waves at issue priority 3 (the parallel chain sets it
 *                         for its speculative batch beside the last part's forward pass)
 *   wide_s 0              wide decode sequences per workgroup 1 / 2 / 4 (0: by batch)
 *   ext_wide_min 0        > 0: the constrained terms passes wide from this N
 *   chain_wide 1, chain_wide_min 0       the wide serial chain step: 0 never / from this N
 *   f32_onebar 1          0: two barriers per step in the f32 pair trellis
 *   bw_global 0, bw_perseq 0, bw_gemm_path 0   Baum-Welch: global scratch from N = 257 /
 *                         per-sequence E-step kernels / the xi GEMM path at every N
 *   bw_chunk_elems 0      Baum-Welch: > 0 the most elements (alpha / beta rows) of a chunk of
 *                         sequences, instead of the device-memory rule; a longer sequence is still a
 *                         chunk of its own (test hook: several chunks on a small corpus)
 *   bw_max_waves 0        Baum-Welch, N <= 64: > 0 the most backward waves (0: 8 per compute unit);
 *                         each walks ceil(pairs / waves) pairs of sequences (test hook)
 *   xi_part_rows 0        cv_expected_counts*: > 0 the rows per part of the count GEMM, rounded up to a
 *                         multiple of 4 (0: by rule, from the chunk's rows and NP); a test hook: several
 *                         parts from a small input.  Not bit-identical: it regroups the sums of
 *                         non-negative terms; the counts hold their bound under every value
 *   bcnt_part_rows 0      cv_expected_counts_model*: > 0 the sorted rows per part of the emission-count
 *                         gather (0: by rule, from the chunk's rows and NP); a test hook: segments over many
 *                         parts from a small input.  Not bit-identical: it regroups the sums; b_cnt holds
 *                         its bound under every value
 *   gm_part_rows 0        cv_expected_counts_gauss*: > 0 the rows per part of the moment GEMM, rounded up
 *                         to a multiple of 4 (0: by rule, from the chunk's rows, NP and D); a test hook:
 *                         several parts from a small input.  Not bit-identical: it regroups the sums;
 *                         g_cnt, m1 and m2 hold their bounds under every value
 * The bw_* keys are not bit-identical: the E-step sums are f64 atomic adds in arrival order, so
 * they hold to the fitting tolerance (1e-9 on the log10 parameters) instead.
 * Unknown keys and values outside int32 are CV_EINVAL.  cv_tuning_key(i) lists the keys
 * (NULL past the last). */
/* Frees the handle's decode workspaces (delta rows, the posterior and sampling paths' forward rows, the K-best back-pointers and last lists, the
 * constrained decode's and the parallel chain's per-call buffers, pinned staging), which are otherwise kept grow-only between calls
 * so repeated calls do not reallocate: e.g. ~1 GB of chain buffers (observations, paths, the
 * speculative batches' psi rows) and 18 MiB of pinned staging plus the 34-69 GB delta workspace
 * after a config-4-sized cv_decode_superseq_cp / cv_decode_batch.  The model tables
 * stay; the next call allocates what it needs again, and cv_device_memory is back at what the
 * tables alone take.  Waits for the handle's streams and, on the caller's stream of the last
 * *_device call, for that call's end: releasing while such a call is in flight is safe. */
CV_API cv_status cv_hmm_release_workspaces(cv_hmm* h);
CV_API cv_status cv_hmm_set_tuning(cv_hmm* h, const char* key, int64_t value);
CV_API cv_status cv_hmm_get_tuning(const cv_hmm* h, const char* key, int64_t* value);
CV_API const char* cv_tuning_key(int32_t i);

CV_API int32_t cv_hmm_nstates(const cv_hmm* h);
CV_API int64_t cv_hmm_nobs(const cv_hmm* h);                   /* V = prod(bdims) */
CV_API int32_t cv_hmm_ndims(const cv_hmm* h);
CV_API cv_status cv_hmm_bdims(const cv_hmm* h, int64_t* bdims_out /*[D]*/);
/* flatten one D-dim observation value ([usize; D]) to the index used everywhere else. */
CV_API cv_status cv_obs_flatten(const cv_hmm* h, const int64_t* value /*[D]*/, int64_t* flat_out);
/* HMM::init_prob (hmm.rs:211-213) */
CV_API double cv_hmm_init_prob(const cv_hmm* h, int32_t state, int64_t obs);
/* HMM::init_probs (hmm.rs:215-218) -> out[N] */
CV_API cv_status cv_hmm_init_probs(const cv_hmm* h, int64_t obs, double* out);
/* HMM::transition_prob (hmm.rs:220-222) */
CV_API double cv_hmm_transition_prob(const cv_hmm* h, int32_t from, int32_t to, int64_t obs);
/* HMM::transitions_to (hmm.rs:224-226) -> out[N] = a[:, to] */
CV_API cv_status cv_hmm_transitions_to(const cv_hmm* h, int32_t to, double* out);
/* HMM::emit_prob (hmm.rs:228-230) */
CV_API double cv_hmm_emit_prob(const cv_hmm* h, int32_t state, int64_t obs);
/* HMM::emit_probs (hmm.rs:232-234) -> out[N] */
CV_API cv_status cv_hmm_emit_probs(const cv_hmm* h, int64_t obs, double* out);

/* ---- batch decode: the trellis forward pass + backtrack -------------------------------
 * Replaces, per sequence, the dense forward of CPSolver::init_viterbi (cp.rs:63-83) /
 * viterbi::decode (viterbi.rs:9-23) / DPSolver::solve (dp.rs:127-182) plus the backtrack
 * (cp.rs:85-93, viterbi.rs:24-31, dp.rs:71-89).  Host pointers; synchronous. */
CV_API cv_status cv_decode_batch(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                 const cv_opts* opts, int32_t* path_out, double* score_out,
                                 uint8_t* status_out);
/* Same on device-resident buffers, enqueued on opts->stream (or the handle's stream);
 * returns after enqueueing (no host synchronisation, so consecutive calls queue ahead).
 * Consecutive calls on one handle may use different streams: each waits, on its own stream,
 * for the previous call's workspace.  offsets_host (nullable) is a host copy of offsets used
 * for chunking; without it the offsets are copied back once.  Observation indices are
 * range-checked on the device: a bad one sets status CV_SEQ_BADOBS. */
CV_API cv_status cv_decode_batch_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                        const int64_t* offsets_dev, const int32_t* obs_dev,
                                        const cv_opts* opts, int32_t* path_dev, double* score_dev,
                                        uint8_t* status_dev);
/* Counters of the sparse low-plane backtrack (tuning key t64_lo_every) of the last
 * cv_decode_batch[_device] call on the f64 trellis that has FINISHED on this handle (they are
 * copied to the host behind the call's kernels; no synchronisation here -- after cv_decode_batch,
 * or once the stream of cv_decode_batch_device has been synchronised, they are that call's).
 * Length-checked: writes min(n, count) words to out and returns count (8 now; later versions may
 * append words), -1 on a bad argument.  Words: 0 the lo_every the call ran with (1: every row
 * full -- the key, a decode the sparse rows do not cover, or the handle's guard); 1 near-tie
 * events at rows without low words; 2 threshold scans and 3 rows descended resolving them;
 * 4 dense replays (a need-set above 8 states); 5 failed self-checks (always 0; such an event is
 * replayed densely, so the result is exact all the same, and the handle then stays at 1);
 * 6 the largest need-set; 7 the call's sequences. */
CV_API int32_t cv_last_t64_stats(const cv_hmm* h, int64_t* out, int32_t n);
/* Counters of the certified fixed-point first pass (tuning key t64_fixed_first) of the last
 * cv_decode_batch[_device] call on this handle.  Length-checked like cv_last_t64_stats: writes
 * min(n, count) words and returns count (4 now), -1 on a bad argument.  Words: 0 whether the call
 * took the pass (1) or ran on the f64 kernels alone (0); 1 sequences whose path the pass
 * certified; 2 sequences decoded by the f64 kernels (1 + 2 = the call's sequences when word 0
 * is 1); 3 whether the handle's guard has pinned it to the f64 kernels. */
CV_API int32_t cv_last_fixed_first_stats(const cv_hmm* h, int64_t* out, int32_t n);
/* Which certified first pass the last cv_decode_batch[_device] call on this handle ran (word 0 of
 * cv_last_fixed_first_stats is 1 exactly where this is not 0): 0 none, 1 the 32-bit
 * fixed-point pass (t64_fixed_first), 2 the f32 round-up pass (t64_f32ru_first); -1 on a null
 * handle. */
CV_API int32_t cv_last_first_pass_kind(const cv_hmm* h);
/* Test hook of the f32 round-up pass: its forward and certificate backtrack on nseq >= 2
 * sequences of one length T (nseq * T <= 2^22; the last of an odd count is left out as in a
 * decode, its outputs 0), observations in range, and everything they store
 * copied to the host: rows [nseq * T][N], the shifts mu and the losing candidates r [nseq * T]
 * (element 0 of a sequence is 0), e_last [nseq], path [nseq * T]. */
CV_API cv_status cv_f32ru_trace(cv_hmm* h, int64_t nseq, int64_t T, const int32_t* obs, float* rows, float* mu,
                                float* r, float* e_last, int32_t* path);
/* Test hook too, not part of the decoding API: the same on sequences of several lengths (offsets
 * [nseq + 1] from 0, every length at least 1; at most 2^22 elements):
 * sequences 2k and 2k + 1 are run as a pair and must have one length.  rows [elements][N]; mu, r
 * and path by element. */
CV_API cv_status cv_f32ru_trace_ragged(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                       float* rows, float* mu, float* r, float* e_last, int32_t* path);
/* Device timings of the last decode call on this handle (synchronizes its events). */
CV_API cv_status cv_last_timing(cv_hmm* h, cv_timing* out);
/* Device timings summed over EVERY decode call on this handle from cv_timing_begin to
 * cv_timing_end (no synchronisation in between, so a timed loop can enqueue ahead; the end
 * call synchronizes the events).  launches = chunk launches in all; total_ms = first kernel
 * start to last kernel end.  CV_ELIMIT beyond 16,384 chunk launches. */
CV_API cv_status cv_timing_begin(cv_hmm* h);
CV_API cv_status cv_timing_end(cv_hmm* h, cv_timing* out);
/* Consistency-constrained decode (the intended semantics of the reference's constrained
 * solvers, opti.rs:101-111 / dp.rs:157-164 / cp.rs:95-126): every element with
 * component[e] >= 0 takes the common state of its component, and the total log-likelihood
 * is maximised.  The objective splits at the constrained positions of each sequence
 * (cfn.rs:11-34 pattern): one position gives the max-marginal mu(s) = delta + beta; several
 * give alpha(s_1) + sum_k M_k(s_k, s_k+1) + beta(s_m) with segment tables M_k (start in s at
 * t_k with score 0, run to t_k+1) -- all computed by the trellis kernels.  Summed over
 * sequences as exact integers (units of 2^-64: independent of order and sharding) this is
 * a weighted CSP with unary and pairwise terms, solved exactly per connected group of
 * components by branch and bound (ties: lexicographically smallest state vector in
 * component order); then a forced decode.  Row-A0 (VITERBI) association, every term,
 * segment table and the final decode in opts->dtype: CV_DTYPE_F64 (default; the reference's
 * precision, cp.rs:95-126 / dp.rs:147-166 compute in f64: trellis_fwd_f64 for N <= 256, the
 * generic kernels up to N = 65535, wide above 10240) or CV_DTYPE_F32 (the f32 trellis, N <= 256, scores f64
 * re-scored).  A term outside the exact unit (|score| >= 2^32) is
 * CV_EINVAL.  comp_state_out[ncomp] gets s_c (-1: no active element, or no feasible assignment
 * of its group); objective_out = sum of the per-sequence scores.  CV_ELIMIT if the search
 * exceeds its node limit.  Host pointers; synchronous. */
CV_API cv_status cv_decode_constrained(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                       const int32_t* component, int32_t ncomp, const cv_opts* opts,
                                       int32_t* path_out, double* score_out, uint8_t* status_out,
                                       int32_t* comp_state_out, double* objective_out);
/* The same on device-resident inputs/outputs (offsets_dev/obs_dev in HBM, path_dev/score_dev/
 * status_dev written there; offsets_host and component stay on the host: the search's
 * structure is host work).  Observation indices are range-checked on the device before any
 * term is computed (CV_EINVAL, as the host API).  Enqueued on opts->stream (or the handle's
 * stream); synchronous: returns after the decode has finished. */
CV_API cv_status cv_decode_constrained_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                              const int64_t* offsets_dev, const int32_t* obs_dev,
                                              const int32_t* component, int32_t ncomp, const cv_opts* opts,
                                              int32_t* path_dev, double* score_dev, uint8_t* status_dev,
                                              int32_t* comp_state_out, double* objective_out);
/* Constrained sequences whose final forced path the last constrained decode on this handle
 * took from the certified suffix trace (f64, one constrained element, log-probability models:
 * the path after t1 read off the terms pass's suffix rows, with a rounding-error margin that
 * proves it is the forced decode's own path) instead of a second forward pass; 0 when the
 * trace was off (tuning key no_trace, f32, no kept rows). */
CV_API cv_status cv_last_suffix_traced(const cv_hmm* h, int64_t* out);
/* The same decode split at its one exchange step, for a batch sharded over processes/GPUs:
 * 0. cv_constrained_pairs (host only) on the FULL batch: the sorted component pairs (c1 < c2)
 *    that are consecutive constrained elements of some sequence -- the layout every rank
 *    agrees on.  pairs_out may be null to query *npairs_out.
 * 1. cv_constrained_partials: this shard's exact terms as CV_PARTIAL_WORDS int64 words that
 *    ADD across shards (one all-reduce SUM).  Per component: 4N base-2^32 limbs (state-major)
 *    of the unary sum in units of 2^-64, N counts of -inf terms, 1 count of constrained
 *    elements; then per pair: 4N^2 limbs (entry s1*N+s2), N^2 -inf counts, 1 count.
 * 2. cv_constrained_select (host only): the exact search on the reduced partials;
 *    explored = (component, state) candidates scored.
 * 3. cv_decode_forced_components: the shard's final decode with every constrained element
 *    forced to comp_state[component[e]]; objective_out = the shard's sum of scores.
 * cv_decode_constrained == 0 + 1 + 2 + 3 on one process. */
#define CV_PARTIAL_WORDS(nstates, ncomp, npairs) \
  ((int64_t)(ncomp) * (5 * (int64_t)(nstates) + 1) + (int64_t)(npairs) * (5 * (int64_t)(nstates) * (nstates) + 1))
CV_API cv_status cv_constrained_pairs(int64_t nseq, const int64_t* offsets, const int32_t* component, int32_t ncomp,
                                      int32_t* pairs_out, int64_t cap_pairs, int64_t* npairs_out);
CV_API cv_status cv_constrained_partials(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                         const int32_t* component, int32_t ncomp, int64_t npairs,
                                         const int32_t* pairs, const cv_opts* opts, int64_t* partials_out);
CV_API cv_status cv_constrained_select(int32_t nstates, int32_t ncomp, int64_t npairs, const int32_t* pairs,
                                       const int64_t* partials, int32_t* comp_state_out, uint64_t* explored_out);
CV_API cv_status cv_decode_forced_components(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                             const int32_t* component, int32_t ncomp, const int32_t* comp_state,
                                             const cv_opts* opts, int32_t* path_out, double* score_out,
                                             uint8_t* status_out, double* objective_out);
/* Steps 1-3 in ONE call on a shard, the exchange made by the caller's callback: after this
 * shard's partials are computed, exchange(words, nwords, ctx) must replace words[0, nwords)
 * by their SUM over all shards (e.g. an all-reduce; return 0 on success) -- then the search
 * and the shard's final decode run here, which lets the decode reuse the terms pass's prefix
 * rows (the resume flow) like cv_decode_constrained.  pairs = cv_constrained_pairs of the
 * FULL batch.  Every rank must reach the callback: it is called even for an empty shard.
 * exchange == NULL: a single process (words already total).  Host pointers; synchronous.
 * objective_out = the shard's sum of scores. */
typedef int32_t (*cv_exchange_fn)(int64_t* words, int64_t nwords, void* ctx);
CV_API cv_status cv_decode_constrained_exchange(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                                const int32_t* component, int32_t ncomp, int64_t npairs,
                                                const int32_t* pairs, cv_exchange_fn exchange, void* ctx,
                                                const cv_opts* opts, int32_t* path_out, double* score_out,
                                                uint8_t* status_out, int32_t* comp_state_out,
                                                uint64_t* explored_out, double* objective_out);
/* viterbi::decode (viterbi.rs:5): one sequence, reference decode() semantics (row 0 = 0.0,
 * f64), path only. */
CV_API cv_status cv_viterbi_decode(cv_hmm* h, int64_t T, const int32_t* obs, int32_t* path_out);
/* CPSolver::solve without active constraints, exactly (cp.rs:133-143: init_viterbi cp.rs:63-83
 * + backtrack cp.rs:85-93 over the super-sequence of utils.rs:62-103): the nseq sequences are
 * decoded as ONE chain in order -- at a sequence start the predecessor term is pi[j]
 * (utils.rs:24-38), so later sequences carry the running total and round exactly as the
 * reference does (a per-sequence decode can differ from it at near ties).  f64, first-index
 * argmax, CP association.  path_out[offsets[nseq] - offsets[0]] in super-sequence order;
 * objective_out = the chain's final maximum (main.rs:129's first number).  Log-probability
 * models (finite entries in [-2^80, 0]), any N: every sequence is decoded on its own by the
 * batch path's f64 row-A0 decode in parallel and certified to be the chain's path at the chain's running
 * total (a rounding-error margin), the running total folded on the host, and only the
 * uncertified sequences (near ties at that magnitude) re-decoded from their predicted offsets
 * or re-run through the serial chain kernel -- bit-identical to the serial chain
 * (cv_last_superseq_stats).  Otherwise serial over
 * elements on the GPU (one workgroup; above N = 1024 one launch per element with the states
 * over workgroups), as the reference is on the CPU.  N <= 65535.
 * CV_EINFEASIBLE when the maximum is -inf. */
CV_API cv_status cv_decode_superseq_cp(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                       int32_t* path_out, double* objective_out);
/* How the last cv_decode_superseq_cp on this handle ran (out[9]): out[0] = 1 when the PARALLEL
 * chain ran (every finite entry of the model in [-2^80, 0], every sequence feasible:
 * each sequence decoded on its own by the f64 trellis and certified to be the chain's own path
 * at the chain's running total), 0 for the serial chain; out[1] = sequences
 * certified, out[2] = sequences the serial chain kernel re-ran, out[3] = such runs, out[4] =
 * certified sequences folded by one quantised add, out[5] = uncertified sequences settled by
 * the parallel re-decode from their exact offsets (speculation), out[6] = such batches, out[7] =
 * sequences whose paths the host walk fetched packed while the whole path copy ran beside it,
 * out[8] = walk steps that had to wait for that copy (a prediction miss; 0 when it held). */
CV_API cv_status cv_last_superseq_stats(const cv_hmm* h, int64_t* out);

/* ---- evaluation: sequence log-likelihood and posterior state marginals -------------------
 * The sum-product counterpart of cv_decode_batch on the standard HMM, the model read as the
 * row-A0 (VITERBI) association reads it with table entries p = 10^x (-inf = 0):
 *   P(o, s) = pi[s_0] b[s_0, o_0] prod_t a[s_t-1, s_t] b[s_t, o_t].
 * Per sequence: loglik_out[k] = log10 sum_s P(o, s); gamma_out[e * N + j] = P(s_t = j | o) for
 * element e (element-major, N per element); path_out[e] = the first index of max_j gamma
 * (posterior / max-marginal decoding).  path_out and gamma_out are nullable: with both NULL
 * only the forward pass runs and no row is stored (scoring mode); otherwise the scaled forward
 * rows go to the handle's workspace (NP * 8 bytes per element, NP = N rounded up to a multiple
 * of 64; chunks of whole sequences under opts->workspace_bytes, 0 = default 64 GiB;
 * cv_hmm_release_workspaces frees them) and one backward pass writes the argmax, and gamma
 * only when asked for.
 * opts: dtype CV_DTYPE_F64 (CV_DTYPE_F32 is CV_EUNSUPPORTED); assoc CV_ASSOC_VITERBI (others
 * CV_EINVAL); kernel CV_KERNEL_AUTO (N <= 256: 32 sequences per workgroup in lock step, each
 * step a product on the f64 matrix cores) or CV_KERNEL_GENERIC (one workgroup per sequence, an
 * A/B knob and the kernel of every N > 256), CV_KERNEL_TRELLIS* is CV_EINVAL; forced as in
 * cv_decode_batch: a forced element admits only its state, loglik becomes the joint
 * log10 P(o, forced tags) and gamma is conditioned on the tags.  N <= 4096 (above:
 * CV_EUNSUPPORTED).
 * status_out: CV_SEQ_OK; CV_SEQ_EMPTY (loglik 0); CV_SEQ_BADOBS (an observation outside
 * [0, V), checked on the device by both variants: loglik NaN, path -1, gamma rows 0; the call
 * itself still returns CV_OK); CV_SEQ_INFEASIBLE (likelihood 0: loglik -inf, path -1, gamma
 * rows 0).  No sequence disturbs another.  The host variant returns CV_EINFEASIBLE, after
 * writing every output, when a sequence is infeasible.
 * Numerics: the probability-space tables are built once per handle on first use (they count
 * in cv_device_memory until cv_hmm_destroy), 10^x to within 2 ulp; entries below 10^-300 are
 * outside the accuracy contract (they underflow gradually).  Every step rescales its row by
 * an exact power of two, so |loglik - exact| <= 2 T (N + 8) u / ln 10 + 4 T u max(1, S) and
 * |gamma - exact| <= 4 T (N + 8) u gamma + 1e-290 with u = 2^-53 (Posterior).
 * Results are bit-identical between two calls and between the two variants.
 * cv_last_timing: fwd_ms the forward pass, bt_ms the backward pass, kernel CV_KERNEL_AUTO (the
 * matrix-core kernel; mfma_tiles = its 32 sequences per workgroup) or CV_KERNEL_GENERIC,
 * padded_states NP.  Host pointers; synchronous. */
CV_API cv_status cv_posterior_batch(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                    const cv_opts* opts, double* loglik_out, int32_t* path_out,
                                    double* gamma_out, uint8_t* status_out);
/* The same on device-resident buffers, with cv_decode_batch_device's contract: enqueued on
 * opts->stream (or the handle's stream), returns after enqueueing (so it reports CV_OK where
 * the host variant reports CV_EINFEASIBLE: read status_dev); offsets_host (nullable) is a host
 * copy of the offsets; opts->forced is a device pointer. */
CV_API cv_status cv_posterior_batch_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                           const int64_t* offsets_dev, const int32_t* obs_dev, const cv_opts* opts,
                                           double* loglik_dev, int32_t* path_dev, double* gamma_dev,
                                           uint8_t* status_dev);

/* ---- evaluation: posterior path sampling (forward filtering, backward sampling) ------------
 * `draws` = R whole paths per sequence from P(path | observations, tags), the model read exactly
 * as cv_posterior_batch reads it (VITERBI association, p = 10^x, a forced element admits one
 * state).  The forward pass is cv_posterior_batch's (the scaled rows alpha^_t in the handle's
 * workspace); draw r of sequence s then walks back from the last element:
 *   t = T-1: weights w_i = alpha^_t[i];
 *   t < T-1: w_i = alpha^_t[i] * A[i][j] (one f64 product), j the state already drawn for t+1 --
 *     the emission and the mask of t+1 are constant in i and drop out;
 *   pick: with W = sum_i w_i and the inclusive prefix sums c_i in state order, the smallest i with
 *     w_i > 0 and c_i > u W; if rounding leaves none, the largest i with w_i > 0.  The association
 *     order of the sums is the kernel's own and fixed, so results repeat bit for bit.  A state
 *     with w_i = 0 is never picked, whatever the rounding: every returned path has a finite
 *     joint score (unlike cv_posterior_batch's path, the per-element argmax of gamma, which can
 *     cross a zero transition).
 * u = u(seed, S, r, t), S = seq_base + s, t the position in the sequence, is a counter-based
 * uniform on [0, 1), all arithmetic mod 2^64, G = 0x9E3779B97F4A7C15:
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   k = mix(seed + G); k = mix(k ^ S); k = mix(k + G (r + 1)); z = mix(k ^ (t * 0xD1B54A32D192ED03))
 *   u = (z >> 11) * 2^-53
 * e.g. u(0, 0, 0, 0) = 0x1.da202e598192dp-1, u(1, 2, 3, 4) = 0x1.cfd7060f11400p-6.  A draw depends
 * on (seed, S, r) and the sequence alone -- not on the batch around it, the chunking, R or the
 * variant: the first R' planes of an R-draw call are the R'-draw call; sequence s of a batch is
 * the same sequence sampled alone with seq_base = s; a multi-GPU caller shards with seq_base.
 * CV_KERNEL_AUTO and CV_KERNEL_GENERIC may pick differently (their forward rows differ in the
 * last bits); both meet the accuracy contract:
 *   with F the exact conditional CDF given the state drawn at t+1, the picked i satisfies
 *   F_(i-1) - eps <= u <= F_i + eps, eps(T, N) = 4 (T + 1) (N + 8) 2^-53
 * (forward rows within 2 T (N + 8) u relative, N + 2 roundings in each of the numerator and the
 * denominator; DESIGN.md, Posterior sampling).
 * Outputs, with L = offsets[nseq]: path_out is draw-major, plane r (path_out + r * L) a whole path
 * array in cv_decode_batch's layout; score_out[r * nseq + s] (nullable; draw-major too, so every
 * plane is a cv_decode_batch-shaped result) is the reference's f64 fold along the sampled path,
 *   d = pi[s_0] + b[s_0, o_0], then d = (d + a[s_t-1, s_t]) + b[s_t, o_t],
 * bit for bit what cv_kbest_batch reports for the same path; loglik_out[s] (nullable) as
 * cv_posterior_batch.  1 <= draws <= 64 (else CV_EINVAL).
 * status_out as cv_posterior_batch: CV_SEQ_BADOBS (paths -1, scores NaN, loglik NaN);
 * CV_SEQ_INFEASIBLE (paths -1, scores -inf, loglik -inf; the host variant returns
 * CV_EINFEASIBLE after writing every output); CV_SEQ_EMPTY (loglik 0; no path element exists and
 * the sequence's score_out slots are not written).  No sequence disturbs another.
 * opts exactly as cv_posterior_batch: dtype CV_DTYPE_F64, assoc CV_ASSOC_VITERBI, kernel
 * CV_KERNEL_AUTO (N <= 256: one wave per sequence and group of up to 8 draws) or CV_KERNEL_GENERIC
 * (one workgroup per sequence and draw; every N > 256), forced, stream, workspace_bytes (the
 * rows: NP * 8 bytes per element, chunks of whole sequences).  N <= 4096.
 * cv_last_timing: fwd_ms the forward pass, bt_ms sampling plus scoring, the rest as for
 * cv_posterior_batch.  cv_hmm_release_workspaces frees the rows and the staging.
 * Host pointers; synchronous. */
CV_API cv_status cv_sample_batch(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                 int32_t draws, uint64_t seed, int64_t seq_base, const cv_opts* opts,
                                 int32_t* path_out /*[draws][L]*/, double* score_out /*[draws][nseq], nullable*/,
                                 double* loglik_out /*[nseq], nullable*/, uint8_t* status_out /*[nseq]*/);
/* The same on device-resident buffers, with cv_posterior_batch_device's contract: enqueued on
 * opts->stream (or the handle's stream), returns after enqueueing (so it reports CV_OK where
 * the host variant reports CV_EINFEASIBLE: read status_dev); offsets_host (nullable) is a host
 * copy of the offsets; opts->forced is a device pointer. */
CV_API cv_status cv_sample_batch_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                        const int64_t* offsets_dev, const int32_t* obs_dev, int32_t draws,
                                        uint64_t seed, int64_t seq_base, const cv_opts* opts, int32_t* path_dev,
                                        double* score_dev, double* loglik_dev, uint8_t* status_dev);

/* ---- K-best (list) Viterbi decoding, exact f64 --------------------------------------------
 * The k best paths of every sequence under the row-A0 (VITERBI) association in f64, with their
 * scores.  The score of a path s is the reference's fold along it:
 *   d = pi[s_0] + b[s_0, o_0], then d = (d + a[s_t-1, s_t]) + b[s_t, o_t];
 * a path whose score is -inf is not a path.  fl(x + c) is monotone in x, so the K best lists of
 * the predecessors determine the K best list of a state and the recurrence is well defined:
 *   L_0(j) = [pi[j] + b[j, o_0]] if finite, else empty;
 *   t >= 1: the candidates of state j are x(i, r) = L_t-1(i)[r] + a[i, j] over all states i and
 *     ranks r; L_t(j) is the first K FINITE candidates in the order value descending, ties by
 *     (i, r) ascending (a stable descending sort of the candidates laid out at index i * K + r);
 *     b[j, o_t] is then added to each -- the order is fixed before the emission is added -- and
 *     a -inf emission empties the list;
 *   result: the entries L_T-1(j)[r] in the order value descending, ties by (j, r) ascending;
 *     the first K are ranks 0 .. K-1, each followed back through its (i, r) back-pointers.
 * A forced element (opts->forced, as in cv_decode_batch) admits only its state: every other
 * list at that element is empty.  Consequences: rank 0 is cv_decode_batch's f64 VITERBI path
 * and score, bit for bit, for every feasible sequence; every reported score is the f64 fold
 * along its reported path; the first K' ranks of a K-best call are the K'-best call's result.
 * Outputs, with L = offsets[nseq]: path_out is rank-major, plane r (path_out + r * L) a whole
 * path array in cv_decode_batch's layout; score_out[s * k + r]; count_out[s] = min(k, number of
 * finite-score paths of sequence s).  Ranks count_out[s] .. k-1 are unused: score -inf, path -1.
 * status_out: CV_SEQ_OK (count >= 1); CV_SEQ_INFEASIBLE (count 0, every rank unused);
 * CV_SEQ_EMPTY (empty sequence: count 0, scores -inf); CV_SEQ_BADOBS (an observation outside
 * [0, V), checked on the device by both variants: count 0, paths -1, scores NaN).  No sequence
 * disturbs another.  The host variant returns CV_EINFEASIBLE, after writing every output, when
 * a sequence is infeasible.
 * opts: dtype CV_DTYPE_F64 (CV_DTYPE_F32 is CV_EUNSUPPORTED); assoc CV_ASSOC_VITERBI (others
 * CV_EINVAL); kernel CV_KERNEL_AUTO or CV_KERNEL_GENERIC (the same kernels; CV_KERNEL_TRELLIS*
 * is CV_EINVAL); forced, stream and workspace_bytes are honoured.  Limits: 1 <= k <= 16 (else
 * CV_EINVAL); N <= 1,024 and N * KT <= 8,192 (else CV_EUNSUPPORTED), KT = k rounded up to the
 * kernels' list width 2, 4, 8 or 16 (two list rows of N * KT f64 in 128 KiB of LDS).
 * Workspace: u16 back-pointers (i << 4 | r) per (element, state, rank), N * KT * 2 bytes per
 * element, in the handle's workspace, in chunks of whole sequences under opts->workspace_bytes
 * (0 = the generic kernels' default, 8 GiB); a single sequence over the cap is CV_ENOMEM.  The
 * last lists (N * KT * 8 bytes per sequence of a chunk) are kept beside them;
 * cv_hmm_release_workspaces frees both.
 * cv_last_timing: fwd_ms the forward pass, bt_ms select plus walk, launches the chunks, kernel
 * CV_KERNEL_GENERIC, padded_states KT, mfma_tiles the sequences per forward workgroup (1, 2 or
 * 4).  Results are bit-identical between two calls and between the two variants.
 * Host pointers; synchronous. */
CV_API cv_status cv_kbest_batch(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                int32_t k, const cv_opts* opts, int32_t* path_out /*[k][L]*/,
                                double* score_out /*[nseq][k]*/, int32_t* count_out /*[nseq]*/,
                                uint8_t* status_out /*[nseq]*/);
/* The same on device-resident buffers, with cv_posterior_batch_device's contract: enqueued on
 * opts->stream (or the handle's stream), returns after enqueueing (so it reports CV_OK where
 * the host variant reports CV_EINFEASIBLE: read status_dev); offsets_host (nullable) is a host
 * copy of the offsets; opts->forced is a device pointer. */
CV_API cv_status cv_kbest_batch_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                       const int64_t* offsets_dev, const int32_t* obs_dev, int32_t k,
                                       const cv_opts* opts, int32_t* path_dev, double* score_dev,
                                       int32_t* count_dev, uint8_t* status_dev);

/* ---- decode of caller-supplied emission scores ------------------------------------------
 * cv_decode_batch for observations that are not symbols of the handle's alphabet (continuous
 * densities, scores of a tagger, back-off rows): the model (pi, A) is the handle's, its own b
 * is ignored, and the emissions arrive per call as a dense array
 *   emis[e * ld + j] = log10 p(observation of element e | state j),  j < N <= ld,
 * e the element index of the CSR offsets (row e at emis + e * ld; ld is the row stride in
 * doubles, rows need 8-byte alignment only).  Values may be positive (densities) or -inf.
 * The result is, by definition, what cv_decode_batch with dtype CV_DTYPE_F64 gives for the
 * discrete model b[j][e] = emis[e][j] with obs[e] = e: the same recurrence per association,
 * first-index ties, statuses and scores, bit for bit (the same kernels decode staged rows).
 * Per entry: -0.0 reads as +0.0; a sequence with a NaN or +inf in one of its rows gets
 * CV_SEQ_BADOBS with the path and score cv_decode_batch_device reports for a sequence holding
 * an out-of-range observation, and disturbs no other sequence.
 * opts: dtype must be CV_DTYPE_F64 (CV_DTYPE_F32 is CV_EUNSUPPORTED); assoc any; kernel
 * CV_KERNEL_AUTO / GENERIC / TRELLIS_F64 with cv_decode_batch's f64 selection rules
 * (CV_KERNEL_TRELLIS is CV_EUNSUPPORTED); forced wherever cv_decode_batch supports it;
 * workspace_bytes caps the delta rows plus the staged emissions of a chunk (8 P + 4 bytes per
 * element more, P the kernel's table stride: NP for the f64 trellis, N otherwise).
 * ld < N or a null pointer is CV_EINVAL.  cv_last_timing as for cv_decode_batch; fwd_ms and
 * total_ms include the staging kernel.  Host pointers; synchronous. */
CV_API cv_status cv_decode_emissions(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* emis,
                                     int64_t ld, const cv_opts* opts, int32_t* path_out, double* score_out,
                                     uint8_t* status_out);
/* The same on device-resident buffers, with cv_decode_batch_device's contract: enqueued on
 * opts->stream (or the handle's stream), returns after enqueueing; offsets_host (nullable) is a
 * host copy of the offsets; opts->forced is a device pointer.  emis_dev is read in place (no
 * copy besides the staging pass) and must stay valid until the call has run. */
CV_API cv_status cv_decode_emissions_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                            const int64_t* offsets_dev, const double* emis_dev, int64_t ld,
                                            const cv_opts* opts, int32_t* path_dev, double* score_dev,
                                            uint8_t* status_dev);

/* ---- evaluation under caller-supplied emission scores -------------------------------------
 * cv_posterior_batch for the observations of cv_decode_emissions: the handle supplies (pi, A),
 * its own b is ignored, and emis[e * ld + j] = log10 p(observation of element e | state j),
 * j < N <= ld, is read as in cv_decode_emissions (rows 8-byte aligned; the device array is read
 * in place).  loglik_out, path_out (nullable), gamma_out (nullable) and status_out are those of
 * cv_posterior_batch; both NULL is the scoring mode (forward pass only, no stored rows).
 * The result is the exact posterior of the discrete model b[j][e] = emis[e][j], obs[e] = e, read
 * as cv_posterior_batch reads a model, within the bounds below -- not bit-identical to
 * cv_posterior_batch on that model, because the probability-space rows are built differently:
 * row e is staged as p[e][j] = 10^emis[e][j] 2^-k_e with the integer k_e that puts the row's
 * largest entry into [1, 2) (k_e = 0 for a row that is all -inf), and the sequence's sum of k_e
 * joins the forward pass's integer exponent sum before its single log10.  So any finite
 * magnitude works -- scores of -5000 per step over thousands of steps, or a lone density of
 * 10^+40 -- no new rounding enters loglik, and gamma needs nothing (the row scale cancels).
 * Per entry: -inf is 0 exactly; -0.0 reads as +0.0; an entry more than 300 decades below the
 * largest of its own row is outside the accuracy contract (it underflows gradually); a NaN, a
 * +inf or a finite score with |x| >= 2^40 makes its sequence CV_SEQ_BADOBS with the outputs
 * cv_posterior_batch gives for an out-of-range observation (loglik NaN, path -1, gamma rows 0)
 * and disturbs no other sequence.  CV_SEQ_INFEASIBLE and CV_SEQ_EMPTY as in cv_posterior_batch;
 * the host variant returns CV_EINFEASIBLE after writing every output.
 * Numerics: a staged entry is within c u of 10^x 2^-k_e relative, u = 2^-53, with c = 2: the
 * worst case of exp10_scaled (csrc/kernels/exp10_scaled.h), one source for host and device with
 * no math-library call, derived there and pinned against 60-digit arithmetic by the tests
 * (largest error measured: 1.0 u).  The bounds of cv_posterior_batch hold with N + 8 replaced
 * by N + 6 + c, i.e. unchanged:
 *   |loglik - exact| <= 2 T (N + 6 + c) u / ln 10 + 4 T u max(1, S),
 *   |gamma - exact| <= 4 T (N + 6 + c) u gamma + 1e-290, gamma rows sum to 1 within 4 (N + 6 + c) u.
 * Results are bit-identical between two calls, between the two variants and under any chunking.
 * opts as for cv_posterior_batch: dtype CV_DTYPE_F64 (F32: CV_EUNSUPPORTED), assoc
 * CV_ASSOC_VITERBI (others CV_EINVAL), kernel CV_KERNEL_AUTO or CV_KERNEL_GENERIC, forced;
 * N <= 4096 (above: CV_EUNSUPPORTED).  ld < N or a null emis is CV_EINVAL.
 * workspace_bytes caps the forward rows plus the staged emissions and their index of a chunk
 * (8 NP + 4 bytes per element more; they stay until the chunk's backward pass has run), so the
 * scoring mode is chunked too (by the staged bytes alone); a single sequence over the cap is
 * CV_ENOMEM, a sequence of more than INT32_MAX elements CV_ELIMIT.  cv_hmm_release_workspaces
 * frees them.  cv_last_timing as for cv_posterior_batch; fwd_ms includes the staging kernel.
 * Host pointers; synchronous. */
CV_API cv_status cv_posterior_emissions(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* emis,
                                        int64_t ld, const cv_opts* opts, double* loglik_out, int32_t* path_out,
                                        double* gamma_out, uint8_t* status_out);
/* The same on device-resident buffers, with cv_posterior_batch_device's contract: enqueued on
 * opts->stream (or the handle's stream), returns after enqueueing (CV_OK where the host variant
 * reports CV_EINFEASIBLE: read status_dev); offsets_host (nullable) is a host copy of the
 * offsets; opts->forced is a device pointer.  emis_dev is read in place and must stay valid
 * until the call has run. */
CV_API cv_status cv_posterior_emissions_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                               const int64_t* offsets_dev, const double* emis_dev, int64_t ld,
                                               const cv_opts* opts, double* loglik_dev, int32_t* path_dev,
                                               double* gamma_dev, uint8_t* status_dev);

/* ---- expected counts for EM (the E-step's sufficient statistics of pi and A) -------------------
 * The pairwise posterior of cv_posterior_batch's model: the model is read exactly as there
 * (VITERBI association, p = 10^x, -inf = 0, a forced element admits only its state).  For every
 * sequence s with status CV_SEQ_OK, with alpha^, beta^ the scaled forward and backward rows,
 *   u_t+1 = b(o_t+1) o mask_t+1 o beta^_t+1,   rsum_t = sum_i alpha^_t[i] (A u_t+1)[i],
 *   xi_t(i, j) = P(s_t = i, s_t+1 = j | o, tags) = alpha^_t[i] A[i][j] u_t+1[j] / rsum_t,  0 <= t < T - 1,
 *   pi_cnt_out[i]        = sum_s gamma_0(s)[i],
 *   a_cnt_out[i * N + j] = sum_s sum_t xi_t(s)(i, j)      (from-major).
 * Sequences with status EMPTY, BADOBS or INFEASIBLE contribute nothing and disturb no other
 * sequence; a sequence with T = 1 contributes to pi_cnt only.  The outputs are overwritten, not
 * accumulated (nseq = 0 writes zeros): a multi-GPU caller adds the arrays of its shards.
 * loglik_out, gamma_out (nullable) and status_out are those of cv_posterior_batch, bit for bit.
 * How: the backward pass also stores u_t+1 and 1 / rsum_t per element; per chunk one f64
 * matrix-core GEMM forms S = sum_e (alpha^[e] / rsum[e])^T u[e] in parts (fixed row ranges of the
 * chunk, each part's tile stored whole -- no atomic adds), the parts are folded in ascending
 * order into one NP x NP accumulator, chunks in stream order, and a_cnt = A o S is one product
 * per entry: a_cnt is exactly 0 wherever A is 0.  pi_cnt adds the sequences' gamma_0 in one
 * fixed order.  Results are therefore bit-identical between two calls with the same arguments
 * on the same handle state and between the host and device variants; they are NOT bit-identical
 * across chunk plans (workspace_bytes) or part sizes (tuning key xi_part_rows), which regroup
 * the sums -- the bounds hold for all of them.
 * Numerics, with u = 2^-53, T the longest sequence of the call, L its elements, B its sequences:
 *   |a_cnt - exact|  <= (4 T (N + 8) + L + 8) u a_cnt + 1e-290 L,
 *   |pi_cnt - exact| <= (4 T (N + 8) + B) u pi_cnt + 1e-290 B.
 * 4 T (N + 8) u: the row bounds of cv_posterior_batch, 2 T (N + 8) u for each of alpha^ and
 * beta^, cover numerator and normaliser of xi_t as they cover gamma's; + 8: the roundings of one
 * term (the division, alpha^ times it, the emission product in u, the product with A, the
 * matrix core's fused multiply-add); + L (B): a sum of non-negative terms gains at most one
 * rounding per added term in whatever grouping (DESIGN.md "Expected counts").  Under dense
 * emissions N + 8 reads N + 6 + c with c = 2, unchanged (the row scale 2^-k cancels in xi as in
 * gamma).  Entries of A below 10^-290 are outside the contract: S = xi / A can leave the range.
 * opts, limits and errors as for cv_posterior_batch: dtype CV_DTYPE_F64 (F32: CV_EUNSUPPORTED),
 * assoc CV_ASSOC_VITERBI and kernel CV_KERNEL_AUTO or CV_KERNEL_GENERIC (others CV_EINVAL);
 * forced, stream and workspace_bytes are honoured; N <= 4096 (above: CV_EUNSUPPORTED); the host
 * variant returns CV_EINFEASIBLE, after writing every output, when a sequence is infeasible.
 * Workspace: 2 * 8 NP + 8 bytes per element of a chunk (forward row, u row, 1 / rsum), plus
 * 8 NP + 4 with dense emissions, plus the GEMM's partial tiles (8 NP^2 bytes per part; at most
 * 512 MiB and at most half of workspace_bytes, at least one part), all under workspace_bytes
 * (0: the posterior path's default); beside them 8 NP bytes per sequence (gamma_0) and one
 * NP x NP accumulator.  A single sequence over the cap is CV_ENOMEM under dense emissions, as
 * there.  cv_hmm_release_workspaces frees all of it.
 * cv_last_timing: fwd_ms the forward pass (including staging), bt_ms the backward pass plus the
 * count kernels; the rest as for cv_posterior_batch.  Host pointers; synchronous. */
CV_API cv_status cv_expected_counts(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                    const cv_opts* opts, double* loglik_out /*[nseq]*/, double* pi_cnt_out /*[N]*/,
                                    double* a_cnt_out /*[N*N] from-major*/, double* gamma_out /*nullable [L*N]*/,
                                    uint8_t* status_out /*[nseq]*/);
/* The same on device-resident buffers, with cv_posterior_batch_device's contract: enqueued on
 * opts->stream (or the handle's stream), returns after enqueueing (CV_OK where the host variant
 * reports CV_EINFEASIBLE: read status_dev); offsets_host (nullable) is a host copy of the
 * offsets; opts->forced is a device pointer. */
CV_API cv_status cv_expected_counts_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                           const int64_t* offsets_dev, const int32_t* obs_dev, const cv_opts* opts,
                                           double* loglik_dev, double* pi_cnt_dev, double* a_cnt_dev, double* gamma_dev,
                                           uint8_t* status_dev);
/* The same under caller-supplied emission scores, read as cv_posterior_emissions reads them
 * (emis[e * ld + j], j < N <= ld; a NaN, +inf or |x| >= 2^40 makes its sequence CV_SEQ_BADOBS,
 * which counts nothing).  ld < N or a null emis is CV_EINVAL. */
CV_API cv_status cv_expected_counts_emissions(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* emis,
                                              int64_t ld, const cv_opts* opts, double* loglik_out, double* pi_cnt_out,
                                              double* a_cnt_out, double* gamma_out, uint8_t* status_out);
CV_API cv_status cv_expected_counts_emissions_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                                     const int64_t* offsets_dev, const double* emis_dev, int64_t ld,
                                                     const cv_opts* opts, double* loglik_dev, double* pi_cnt_dev,
                                                     double* a_cnt_dev, double* gamma_dev, uint8_t* status_dev);

/* ---- likelihood gradients under emission scores (autograd's backward pass) ---------------------
 * The gradient of  F = sum_s w_s log10 P(o_s | model, tags)  over the sequences with status
 * CV_SEQ_OK, in log10 units on both sides (F in log10, the parameters as the handle and emis hold
 * them, log10):
 *   emis_grad_out[e * ld_grad + j] = dF / d emis[e][j]     = w_s gamma_e[j]            (j < N),
 *   pi_grad_out[i]                 = dF / d log10 pi[i]    = sum_s w_s gamma_0(s)[i],
 *   a_grad_out[i * N + j]          = dF / d log10 A[i][j]  = sum_s w_s sum_t xi_t(s)(i, j).
 * This is cv_expected_counts_emissions with a weight per sequence, and everything that entry
 * promises holds here too: how the model and emis are read, the statuses, opts and their errors,
 * N <= 4096, chunking under workspace_bytes and its sizes, the tuning key xi_part_rows,
 * cv_last_timing, release by cv_hmm_release_workspaces, no atomic adds and the bit-identity of
 * repeated calls and of the host and device variants.  loglik_out and status_out are that
 * entry's bit for bit.  weight null means all 1; with weight null or all 1.0, pi_grad_out,
 * a_grad_out and emis_grad_out (at ld_grad = N) are bit-identical to its pi_cnt_out, a_cnt_out and
 * gamma_out: the weight enters as one product after the division (1 / rsum_t) w_s, gamma w_s.
 * a_grad is exactly 0 wherever A is 0, pi_grad wherever pi is 0, emis_grad wherever the score is
 * -inf or a tag excludes the state.  Outputs are overwritten, not accumulated (nseq = 0 writes
 * zeros to pi_grad and a_grad).
 * emis_grad_out (nullable): N values per element at row stride ld_grad >= N (ld_grad < N with a
 * non-null emis_grad_out is CV_EINVAL); the columns [N, ld_grad) are never written; rows need
 * 8-byte alignment only.  The rows of sequences that are not CV_SEQ_OK are written as zeros, and
 * such sequences contribute nothing to pi_grad and a_grad WHATEVER their weight holds (a select
 * on the status, not a product with 0: NaN and inf weights are harmless there).  An OK sequence
 * with a non-finite weight makes every output it touches non-finite: its emis_grad rows, and the
 * entries of pi_grad and a_grad (possibly all of them).  An OK sequence with weight 0 adds only
 * +-0 terms.  A null pi_grad_out or a_grad_out is CV_EINVAL, as are the null pointers and ld < N
 * that cv_expected_counts_emissions rejects.
 * Numerics, with u = 2^-53, T the longest sequence of the call, L its elements, B its sequences,
 * and X_abs the same statistic computed with |w_s| in place of w_s:
 *   |a_grad - exact|           <= (4 T (N + 8) + L + 9) u a_abs + 1e-290 L,
 *   |pi_grad - exact|          <= (4 T (N + 8) + B + 1) u pi_abs + 1e-290 B,
 *   |emis_grad[e][j] - w_s gamma| <= (4 T (N + 8) + 1) u |w_s| gamma + 1e-290 max(1, |w_s|).
 * These are the bounds of cv_expected_counts* with one more rounding per term (the product with
 * the weight) and, the terms now being signed, each sum of n terms gaining at most (n - 1) u of
 * the sum of their magnitudes (DESIGN.md "Likelihood gradients").  N + 8 reads N + 6 + c, c = 2,
 * as there.  Host pointers; synchronous; CV_EINFEASIBLE after writing every output, as there. */
CV_API cv_status cv_loglik_grad_emissions(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* emis, int64_t ld,
                                          const double* weight /*[nseq], nullable = all 1*/, const cv_opts* opts,
                                          double* loglik_out /*[nseq]*/, double* pi_grad_out /*[N]*/,
                                          double* a_grad_out /*[N*N] from-major*/,
                                          double* emis_grad_out /*nullable, [L][ld_grad]*/, int64_t ld_grad,
                                          uint8_t* status_out /*[nseq]*/);
/* The same on device-resident buffers, with cv_expected_counts_emissions_device's contract:
 * enqueued on opts->stream (or the handle's stream), returns after enqueueing; weight_dev
 * (nullable) and emis_grad_dev (nullable) are device pointers.  This is the backward pass of
 * cviterbi.autograd.sequence_loglik with weight_dev = grad_output. */
CV_API cv_status cv_loglik_grad_emissions_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                                 const int64_t* offsets_dev, const double* emis_dev, int64_t ld,
                                                 const double* weight_dev, const cv_opts* opts, double* loglik_dev,
                                                 double* pi_grad_dev, double* a_grad_dev, double* emis_grad_dev,
                                                 int64_t ld_grad, uint8_t* status_dev);

/* ---- expected counts of the whole discrete model (full EM; the gradient in log10 b) ------------
 * cv_expected_counts with a weight per sequence and the statistics of the emission table b, for
 * the model the handle holds (read exactly as cv_posterior_batch reads it).  Over the sequences s
 * with status CV_SEQ_OK, gamma_e the posterior state marginal of element e:
 *   b_cnt_out[j * V + v] = sum_s w_s sum_{e in s, obs[e] = v} gamma_e[j]      (b's own layout:
 *                          state-major, V = the product of bdims, v the flattened index of
 *                          cv_obs_flatten),
 *   pi_cnt_out[i]        = sum_s w_s gamma_0(s)[i],
 *   a_cnt_out[i * N + j] = sum_s w_s sum_t xi_t(s)(i, j).
 * weight null means all 1: the three arrays are then the expected counts of an E-step, and
 * loglik_out, pi_cnt_out, a_cnt_out, gamma_out and status_out are what cv_expected_counts returns
 * for the same arguments, bit for bit (weight all 1.0 likewise: the weight enters as one product
 * after the division).  With weights the arrays are the gradient of F = sum_s w_s log10 P(o_s) in
 * log10 b, log10 pi and log10 A, in log10 units on both sides, with the weight semantics of
 * cv_loglik_grad_emissions: gamma_out (nullable) holds the rows w_s gamma_e, zeros for a sequence
 * that is not OK; such a sequence contributes nothing WHATEVER its weight holds (a select on the
 * status); an OK sequence with a non-finite weight makes the entries it touches non-finite -- in
 * b_cnt the entries (j, v) of the values v it observes; weight 0 adds only +-0.  The outputs are
 * overwritten, not accumulated (nseq = 0 writes zeros to the three arrays).
 * b_cnt is exactly 0 wherever b[j][v] = -inf, for every v no element of an OK sequence observes
 * (a value only a BADOBS or INFEASIBLE sequence holds counts nothing), and for the states a forced
 * tag excludes at its element.
 * How: the backward pass is the gradient arm's; its rows w_s gamma go to gamma_out's device array
 * or, without one, to a chunk-local workspace.  Per chunk the rows are keyed by observation (rows
 * of sequences that are not OK, and observations outside [0, V), get a discard key and are never
 * read), stable-sorted by key, and the sorted list is cut into fixed parts; a run is a maximal
 * stretch of one key inside one part.  One wave per part and 128 columns adds the rows of each
 * run in sorted order and stores the run's sum whole; the runs of each v are then added in
 * ascending order into a [V][NP] accumulator, chunks in stream order, and a last kernel writes the
 * compact state-major array.  No atomic adds.  Results are therefore bit-identical between two
 * calls with the same arguments on the same handle state and between the host and device
 * variants; they are NOT bit-identical across chunk plans (workspace_bytes), part sizes of the
 * gather (tuning key bcnt_part_rows) or of the count GEMM (xi_part_rows), which regroup the sums
 * -- the bounds hold for all of them.
 * Numerics, with u = 2^-53, T the longest sequence of the call, L its elements, and b_abs the
 * same statistic computed with |w_s| in place of w_s:
 *   |b_cnt - exact| <= (4 T (N + 8) + L + 1) u b_abs + 1e-290 L max(1, max |w|).
 * 4 T (N + 8) u: gamma's bound (cv_posterior_batch); + 1: the product with the weight; + L: a sum
 * of n signed terms gains at most (n - 1) u of the sum of their magnitudes in whatever grouping
 * (runs, then their fold, then the chunks), and no entry has more than L terms; 1e-290 per term
 * for what underflows in gamma (DESIGN.md "Emission counts").  pi_cnt and a_cnt hold the bounds of
 * cv_expected_counts (weight null) and of cv_loglik_grad_emissions' pi_grad and a_grad (weights).
 * opts, limits (N <= 4096), statuses and the CV_EINFEASIBLE-after-writing rule are those of
 * cv_expected_counts.  A null pi_cnt_out, a_cnt_out or b_cnt_out is CV_EINVAL.  Workspace: that of
 * cv_expected_counts, plus 8 NP bytes per element of a chunk without gamma_out, all under
 * workspace_bytes; beside it, on the handle, the [V][NP] accumulator (8 V NP bytes; CV_ENOMEM when
 * it cannot be allocated), 20 bytes per element of a chunk and the sort's scratch, and 8 NP + 4
 * bytes per run (at most parts + min(V + 1, rows) runs per chunk).  A chunk of more than INT32_MAX
 * elements is CV_ELIMIT.  cv_hmm_release_workspaces frees all of it.  cv_last_timing: bt_ms
 * covers the emission-count kernels too.  Host pointers; synchronous. */
CV_API cv_status cv_expected_counts_model(cv_hmm* h, int64_t nseq, const int64_t* offsets, const int32_t* obs,
                                          const double* weight /*[nseq], nullable = all 1*/, const cv_opts* opts,
                                          double* loglik_out /*[nseq]*/, double* pi_cnt_out /*[N]*/,
                                          double* a_cnt_out /*[N*N] from-major*/,
                                          double* b_cnt_out /*[N*V], b's own layout*/,
                                          double* gamma_out /*nullable [L*N]: w_s gamma*/,
                                          uint8_t* status_out /*[nseq]*/);
/* The same on device-resident buffers, with cv_expected_counts_device's contract: enqueued on
 * opts->stream (or the handle's stream), returns after enqueueing; weight_dev (nullable) and
 * gamma_dev (nullable) are device pointers.  This is the backward pass of
 * cviterbi.autograd.discrete_loglik with weight_dev = grad_output. */
CV_API cv_status cv_expected_counts_model_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                                 const int64_t* offsets_dev, const int32_t* obs_dev,
                                                 const double* weight_dev, const cv_opts* opts, double* loglik_dev,
                                                 double* pi_cnt_dev, double* a_cnt_dev, double* b_cnt_dev,
                                                 double* gamma_dev, uint8_t* status_dev);

/* ---- Gaussian emissions: log-densities and the E-step's statistics --------------------------
 * A diagonal-covariance Gaussian HMM on raw observation vectors: the handle supplies (pi, A), its
 * own b is ignored (as in the *_emissions entries), and per state j a mean[j * D + d] and a variance
 * var[j * D + d] (host arrays [N][D], row-major, passed on every call: no handle state).  x holds
 * the observations, element e (the element offsets of the CSR batch) at x + e * ldx, D values, f64,
 * ldx >= D.  The emission score of element e in state j is
 *   E[e][j] = log10 N(x_e; mean_j, var_j) = c_j - kappa q_ej,   q_ej = sum_d (x_ed - mean_jd)^2 w_jd,
 *   w_jd = 1 / var_jd,   c_j = -1/2 sum_d log10(2 pi var_jd),   kappa = 0.5 / ln 10.
 * cv_gauss_emissions writes emis_out[r * ld + j], j < N <= ld, for the rows r < nrows of x; the
 * columns [N, ld) are never written.  The result feeds every *_emissions entry (decode, score,
 * posterior, counts, gradients).
 * How: the host computes w (one division per entry) and c_j (std::log10(2 pi var), summed in
 * ascending d) in f64 and uploads them with the means to a handle-owned buffer
 * (cv_hmm_release_workspaces frees it).  The kernel takes a state per lane: d = x - mean (one
 * rounding), s = d d (one rounding), q = fma(s, w, q) in ascending d, E = c_j - kappa q -- the
 * direct form, not x^2 - 2 x mean + mean^2, which cancels when |mean| >> sigma.  No reduction
 * across lanes: host and device variants and repeated calls are bit-identical.
 * Rows: a row of x that holds a NaN or +-inf is written as N NaNs (every *_emissions entry then
 * flags its sequence CV_SEQ_BADOBS and leaves the others alone); a q that overflows gives -inf, a
 * legal score.
 * Numerics, with u = 2^-53 and c_abs_j = 1/2 sum_d |log10(2 pi var_jd)|:
 *   |E - exact| <= (D + 8) u (kappa q + c_abs_j) + u |E|.
 * D + 8: one rounding in d (two in s, relatively), one in s, one in w, one per fma step over
 * non-negative terms, kappa and its product; for c_j one rounding per log and D - 1 of the plain
 * sum; u |E|: the final subtraction (DESIGN.md "Gaussian emissions").
 * Errors: CV_EINVAL for a null pointer, ldx < D, ld < N, D < 1, a non-finite mean, a variance that
 * is NaN or outside [1e-300, 1e300] (the range keeps w normal); CV_ELIMIT for D > 1024.  They are
 * checked before any device work.  N: whatever the handle holds (up to 65,535).
 * Host pointers; synchronous. */
CV_API cv_status cv_gauss_emissions(cv_hmm* h, int64_t nrows, const double* x, int64_t ldx, int64_t D,
                                    const double* mean /*[N*D]*/, const double* var /*[N*D]*/,
                                    double* emis_out /*[nrows][ld]*/, int64_t ld);
/* The same with x_dev and emis_dev on the device (mean and var stay host pointers): enqueued on
 * opts->stream (or the handle's stream; opts nullable, nothing else of it is read), returns after
 * enqueueing. */
CV_API cv_status cv_gauss_emissions_device(cv_hmm* h, int64_t nrows, const double* x_dev, int64_t ldx, int64_t D,
                                           const double* mean, const double* var, const cv_opts* opts,
                                           double* emis_dev, int64_t ld);
/* The E-step of the Gaussian HMM.  By definition the call is cv_gauss_emissions followed by
 * cv_loglik_grad_emissions on its result: loglik_out and status_out are that pair's, bit for bit,
 * under any chunk plan; gamma_out (nullable, [L][N]: the rows w_s gamma_e, zeros for a sequence that
 * is not OK) is that pair's emis_grad_out at ld_grad = N, bit for bit, under any chunk plan;
 * pi_cnt_out and a_cnt_out are that pair's pi_grad_out and a_grad_out -- bit for bit when both calls
 * run as one chunk, within that entry's bounds otherwise.  weight (nullable = all 1) as there.
 * The three new outputs, over the elements e of the sequences with status CV_SEQ_OK, with
 * g_e = w_s gamma_e and y_ed = x_ed - center_d (center: host [D], nullable = 0, y then exact):
 *   g_cnt_out[j]       = sum_e g_e[j],
 *   m1_out[j * D + d]  = sum_e g_e[j] y_ed,
 *   m2_out[j * D + d]  = sum_e g_e[j] fl(y_ed^2),
 * so that mean_j = center + m1 / g and var_j = m2 / g - (m1 / g)^2 (reestimate_gauss in Python).
 * How: per chunk the density kernel fills a chunk-local [elements][NP] workspace, the staging and
 * the forward pass read it as they read a caller's array, the gradient arm's backward pass puts the
 * rows w_s gamma into gamma_out's device array or a workspace, and one f64 matrix-core GEMM forms
 * M += G^T Phi, Phi = [1 | y | y^2] (2 D + 1 columns, formed on the fly from x, never stored), in
 * parts -- fixed row ranges of the chunk, each part's tile stored whole, the parts folded in
 * ascending order into one accumulator, chunks in stream order, no atomic adds -- and a last kernel
 * writes the compact arrays.  The rows of a sequence that is not OK enter G and Phi as zeros by a
 * select on the status (such a sequence may hold a NaN x or a NaN weight: harmless).  Results are
 * bit-identical between two calls and between the host and device variants; g_cnt, m1 and m2 are
 * NOT bit-identical across chunk plans (workspace_bytes) or part sizes (tuning key gm_part_rows),
 * which regroup the sums -- the bounds hold for all of them.
 * Numerics, with u = 2^-53, T the longest sequence of the call, L its elements, and X_abs the
 * statistic computed from |w_s| and |y| ("exact": exact sums for the scores E as cv_gauss_emissions
 * returns them):
 *   |g_cnt - exact| <= (4 T (N + 8) + L + 1) u g_abs  + 1e-290 L max(1, max |w|) max(1, max |y|^2),
 *   |m1 - exact|    <= (4 T (N + 8) + L + 3) u m1_abs + the same term,
 *   |m2 - exact|    <= (4 T (N + 8) + L + 5) u m2_abs + the same term.
 * The first is b_cnt's bound (gamma's bound, the weight, a signed sum of at most L terms); m1 adds
 * the rounding of y and the product, m2 two more for the square (DESIGN.md "Gaussian emissions").
 * opts, limits (N <= 4096), statuses and errors are those of cv_expected_counts_emissions, plus
 * the argument errors of cv_gauss_emissions; a null pi_cnt_out, a_cnt_out, g_cnt_out, m1_out or
 * m2_out is CV_EINVAL.  forced is honoured; the outputs are overwritten, not accumulated (nseq = 0
 * writes zeros); the host variant returns CV_EINFEASIBLE after writing every output.
 * Workspace: that of cv_loglik_grad_emissions, plus 8 NP bytes per element of a chunk (the
 * densities), plus 8 NP bytes per element without gamma_out, plus the moment GEMM's partial tiles
 * (8 NP W bytes per part, W = 2 D + 1 rounded up to a multiple of 16; at most 256 MiB and at most
 * half of what the count GEMM's tiles leave of workspace_bytes, at least one part), all under
 * workspace_bytes; beside them, on the handle, one NP x W accumulator, 4 bytes per element of a
 * chunk (the row flags) and the tables (8 (N + 2 N D' + D') bytes, D' = D rounded up to 8, 16 or a
 * multiple of 32).  cv_hmm_release_workspaces frees all of it.  cv_last_timing: fwd_ms covers the
 * density kernel, bt_ms the moment kernels.  Host pointers; synchronous. */
CV_API cv_status cv_expected_counts_gauss(cv_hmm* h, int64_t nseq, const int64_t* offsets, const double* x, int64_t ldx,
                                          int64_t D, const double* mean /*[N*D]*/, const double* var /*[N*D]*/,
                                          const double* weight /*[nseq], nullable = all 1*/,
                                          const double* center /*[D], nullable = 0*/, const cv_opts* opts,
                                          double* loglik_out /*[nseq]*/, double* pi_cnt_out /*[N]*/,
                                          double* a_cnt_out /*[N*N] from-major*/, double* g_cnt_out /*[N]*/,
                                          double* m1_out /*[N*D]*/, double* m2_out /*[N*D]*/,
                                          double* gamma_out /*nullable [L*N]: w_s gamma*/,
                                          uint8_t* status_out /*[nseq]*/);
/* The same on device-resident buffers, with cv_expected_counts_emissions_device's contract:
 * enqueued on opts->stream (or the handle's stream), returns after enqueueing; x_dev, weight_dev
 * (nullable), gamma_dev (nullable) and the outputs are device pointers; mean, var and center stay
 * host pointers (read before the call returns). */
CV_API cv_status cv_expected_counts_gauss_device(cv_hmm* h, int64_t nseq, const int64_t* offsets_host,
                                                 const int64_t* offsets_dev, const double* x_dev, int64_t ldx, int64_t D,
                                                 const double* mean, const double* var, const double* weight_dev,
                                                 const double* center, const cv_opts* opts, double* loglik_dev,
                                                 double* pi_cnt_dev, double* a_cnt_dev, double* g_cnt_dev,
                                                 double* m1_dev, double* m2_dev, double* gamma_dev, uint8_t* status_dev);

/* ---- trait Solver (viterbi_solver.rs:11-16) -------------------------------------------
 * kind: "gpu"      f32 trellis kernel, VITERBI association, f64 re-scored objective
 *       "gpu-f64"  f64, VITERBI association (reference numerics, row A0)
 *       "gpu-cp"   CPSolver (cp.rs), what main.rs:120 runs: without constraints the exact
 *                  chained super-sequence decode (cv_decode_superseq_cp, objective and path
 *                  as the reference rounds them)
 *       "gpu-cp-seq" f64, CP association, every sequence decoded on its own (parallel; equal
 *                  to gpu-cp up to the chain's running-total roundings)
 *       "gpu-dp"   f64, DP association = DPSolver (dp.rs), ascending-index ties
 * Unconstrained super-sequences decode per sequence (except "gpu-cp",
 * chained): objective = sum of per-sequence scores (sequence order), solution in element order.  Active
 * constraints go through cv_decode_constrained on the row-A0 association at the kind's
 * precision (f64 for gpu-f64 / gpu-cp / gpu-dp, f32 for gpu); get_explored_nodes then
 * reports the number of (component, state) candidates scored. */
CV_API cv_status cv_solver_create(const char* kind, cv_hmm* h, const cv_superseq_desc* seq, cv_solver** out);
CV_API cv_status cv_solver_solve(cv_solver* s);                                   /* Solver::solve */
CV_API cv_status cv_solver_get_solution(const cv_solver* s, const int32_t** sol, int64_t* len); /* get_solution */
CV_API cv_status cv_solver_get_objective(const cv_solver* s, double* obj);        /* get_objective */
CV_API const char* cv_solver_get_name(const cv_solver* s);                        /* get_name */
CV_API cv_status cv_solver_get_explored_nodes(const cv_solver* s, uint64_t* n);   /* CPSolver::get_explored_nodes cp.rs:128 */
CV_API void cv_solver_destroy(cv_solver* s);
/* write_cfn (viterbi_solver/cfn.rs:82-205): the cost-function network of the solver's
 * super-sequence for toulbar2 -- one variable per active component, unary start/end costs,
 * N x N tables of segment longest paths between consecutive constraint boundaries (rows
 * computed on the GPU in f64, bit-identical to the reference loops), the lower bound, in the
 * reference's text layout and float formatting.  *compile_ms = table time (the value main.rs
 * writes when run_cfn is set, main.rs:116-118).  Cost: (boundaries x N) segment passes of
 * N^2 per element, as in the reference -- meant for the problem sizes toulbar2 takes.
 * At most 10,240 states (two f64 rows in LDS): CV_EUNSUPPORTED above, before any upload. */
CV_API cv_status cv_solver_write_cfn(cv_solver* s, const char* path, uint64_t* compile_ms);

/* ---- HMM fitting (hmm.rs:30-190) ------------------------------------
 * pi[N], a[N*N] (from-major), b[N*V] (state-major, obs row-major over bdims): the CURRENT
 * parameters in PROBABILITY space on entry (the reference starts from HMM::new's random
 * draw, hmm.rs:22-28), the fitted parameters log-mapped on return (the reference's log():
 * 0 -> -inf, else ln(x)/ln(10), hmm.rs:192-205) -- ready for cv_hmm_desc.  f64.
 * tags[sum T]: the state of an element, -1 = unknown (None).  device: HIP device index. */
/* maximum_likelihood_estimation (hmm.rs:30-62): exact integer counts on the GPU, ADDED to
 * the current probabilities with the reference's sequential rounding; every tag >= 0. */
CV_API cv_status cv_hmm_fit_mle(int32_t nstates, int64_t nobs, int64_t nseq, const int64_t* offsets,
                                const int32_t* obs, const int32_t* tags, int32_t device, double* pi, double* a,
                                double* b);
/* train (hmm.rs:69-190): tag-clamped Baum-Welch, E- and M-step on the GPU (N <= 65535: one wave
 * per sequence up to 64 states, 32 sequences per workgroup on the f64 matrix cores up to 256,
 * strided per-sequence kernels above (their vectors in LDS to N = 4096, in global memory
 * beyond); over 64 states the xi sums run as one f64 matrix-core
 * GEMM over stored rows per chunk) with
 * the parameters resident between iterations; the convergence test (sum |new - old| <= tol,
 * checked after the update, hmm.rs:172-177) adds per-block partial sums on the host.
 * *iters_out = iterations run. */
CV_API cv_status cv_hmm_fit_train(int32_t nstates, int64_t nobs, int64_t nseq, const int64_t* offsets,
                                  const int32_t* obs, const int32_t* tags, int32_t max_iter, double tol,
                                  int32_t device, double* pi, double* a, double* b, int32_t* iters_out);
/* How the calling thread's last cv_hmm_fit_train split its corpus (thread-local; all 0 before the
 * first call and after a call that failed before planning).  Length-checked like
 * cv_last_t64_stats: writes min(n, count) words and returns count (5 now), -1 on a bad argument
 * (out may be NULL when n is 0).  Words: 0 chunks of sequences (alpha / beta rows are kept for one
 * chunk at a time); 1 elements of the largest chunk; 2 N <= 64 one-wave kernels: the most pairs
 * of sequences one backward wave walked, ceil(ceil(sequences / 2) / waves) of the chunk with the
 * most sequences (else 0); 3 strided kernels in global scratch: the most launches per chunk (else
 * 0); 4 the E-step kernels that ran: 1 one wave per sequence, 2 one workgroup per sequence
 * (vectors in LDS), 3 matrix cores (32 sequences per workgroup), 4 strided in LDS, 5 strided in
 * global scratch, 0 none (max_iter 0). */
CV_API int32_t cv_hmm_fit_last_stats(int64_t* out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* CVITERBI_H */
