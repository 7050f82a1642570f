// grad.hip -- MI355X (gfx950) kernels of cv_loglik_grad_emissions* (DESIGN.md "Likelihood
// gradients"): the gradient of sum_s w_s log10 P(o_s) in the emission scores, log10 pi and log10 A
// is the expected-counts call under per-sequence weights.
//   post_grad_bwd_mm / post_grad_bwd_gen   the backward pass of counts.hip with the gradient arm of
//                                          post_bwd.h: inv, gamma_0 and the gamma rows times w_s,
//                                          the rows stored at the caller's stride
// The kernels behind them (post_xi_gemm, post_xi_fold, post_cnt_a, post_cnt_pi: counts.hip) run as
// they are, over signed terms.  Every sum keeps its one order, so runs repeat bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mm_core.h"
#include "post_bwd.h"
#include "posterior.h"

namespace cvp {

// EGRAD: the gradient rows of E are stored (g.egrad)
template <int NP, int MT, int WV, bool EGRAD>
__global__ __launch_bounds__(64 * WV, 2) void post_grad_bwd_mm(PostArgs g) {
  bwd_mm_body<NP, MT, WV, EGRAD, true, true>(g);
}
__global__ __launch_bounds__(256) void post_grad_bwd_gen(PostArgs g) { bwd_gen_body<true, true>(g); }

template <int NP>
static void launch_grad_bwd_mm(const PostArgs& g, unsigned grid, hipStream_t stream) {
  if (g.egrad) hipLaunchKernelGGL((post_grad_bwd_mm<NP, 2, 4, true>), dim3(grid), dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((post_grad_bwd_mm<NP, 2, 4, false>), dim3(grid), dim3(256), 0, stream, g);
}

hipError_t launch_post_grad_bwd(const PostArgs& g, bool generic, hipStream_t stream) {
  if (!post_args_ok(g) || !g.rows || !g.urows || !g.inv || !g.g0 || g.gamma) return hipErrorInvalidValue;
  if (g.egrad && g.ld_grad < g.nstates) return hipErrorInvalidValue;
  const int64_t n = g.seq_end - g.seq_begin;
  if (n == 0) return hipSuccess;
  if (generic || g.nstates > kPostMmStates) {
    const size_t lds = gen_lds(reinterpret_cast<const void*>(&post_grad_bwd_gen), g.np);
    hipLaunchKernelGGL(post_grad_bwd_gen, dim3((unsigned)n), dim3(256), lds, stream, g);
    return hipGetLastError();
  }
  const unsigned grid = (unsigned)((n + kPostGroup - 1) / kPostGroup);
  switch (g.np) {
    case 64: launch_grad_bwd_mm<64>(g, grid, stream); break;
    case 128: launch_grad_bwd_mm<128>(g, grid, stream); break;
    case 192: launch_grad_bwd_mm<192>(g, grid, stream); break;
    default: launch_grad_bwd_mm<256>(g, grid, stream); break;
  }
  return hipGetLastError();
}

}  // namespace cvp
