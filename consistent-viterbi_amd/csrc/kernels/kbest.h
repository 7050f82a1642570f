// kbest.h -- argument block and launchers of the K-best (list) Viterbi kernels (kbest.hip).
// Internal to libcviterbi; the public boundary is include/cviterbi.h (cv_kbest_batch*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvkb {

constexpr int kKbestMaxK = 16;         // ranks per call; a back-pointer is u16 (i << 4 | r)
constexpr int kKbestMaxStates = 1024;  // one state per thread
constexpr int kKbestMaxCells = 8192;   // N * KT: two list rows of N * KT f64 in 128 KiB of LDS

// KT: the list width the kernels are instantiated for (k rounded up to 2, 4, 8 or 16)
inline int kbest_width(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

struct KbestArgs {
  const double* pi;  // [N] log10
  const double* a;   // [N][N] from-major, unpadded
  const double* et;  // [V][N] emission column of each observation
  const int64_t* offsets;  // [nseq + 1] element offsets
  const int32_t* obs;      // indexed by element offset
  const int32_t* forced;   // nullable; indexed like obs
  const int32_t* order;    // nullable: slot k of [seq_begin, seq_end) -> sequence (longest first)
  int64_t seq_begin, seq_end;
  int64_t elem_base;  // element offset that maps to row 0 of bp
  int nstates, nobs;
  int k, kt;
  uint16_t* bp;   // [elements][N][KT] back-pointers (i << 4 | r) of the chunk
  double* last;   // [slot - seq_begin][N][KT] the lists of each sequence's last element
  int32_t* end;   // [nseq][k] end point (j << 4 | r) of each rank, -1 unused
  int64_t plane;  // elements per rank plane of path (offsets[nseq])
  int32_t* path;  // [k][plane]
  double* score;  // [nseq][k]
  int32_t* count; // [nseq]
  uint8_t* status;  // [nseq]; zeroed before the forward pass, which flags CVK_SEQ_BADOBS
};

// sequences per workgroup of kbest_fwd (1, 2 or 4): see kbest.hip
int kbest_seqs_per_wg(int n, int kt, int64_t nseq);
// forward pass of the chunk [seq_begin, seq_end): back-pointers, last lists, BADOBS flags
hipError_t launch_kbest_fwd(const KbestArgs& g, int s, hipStream_t stream);
// the k best end points of each sequence of the chunk: scores, counts, statuses, end
hipError_t launch_kbest_select(const KbestArgs& g, hipStream_t stream);
// follows the back-pointers of every (sequence, rank) of the chunk into its plane of path
hipError_t launch_kbest_walk(const KbestArgs& g, hipStream_t stream);

}  // namespace cvkb
