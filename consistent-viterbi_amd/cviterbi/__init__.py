"""cviterbi -- MI355X-native Viterbi decode path behind the consistent-viterbi solver API.

Host mirror of the reference's hmm::HMM and viterbi_solver interfaces over the C ABI
in include/cviterbi.h (libcviterbi.so: hand-written gfx950 HIP kernels).
"""
from ._lib import CVError, EXPORTS, LIB_PATH  # noqa: F401
from .hmm import HMM, tuning_keys  # noqa: F401
from .decode import (constrained_pairs, constrained_partials, constrained_select, decode, decode_batch, decode_batch_device, decode_constrained_device, decode_constrained_exchange,  # noqa: F401
                     decode_constrained, decode_forced_components, decode_superseq_cp, device_memory, f32ru_trace, f32ru_trace_ragged, last_first_pass_kind, last_suffix_traced, last_fixed_first_stats, last_superseq_stats, last_t64_stats, last_timing, timing_begin,
                     timing_end)
from .counts import (expected_counts, expected_counts_device, expected_counts_emissions,  # noqa: F401
                     expected_counts_emissions_device, expected_counts_model, expected_counts_model_device,
                     reestimate, reestimate_model)
from .emissions import decode_emissions, decode_emissions_device  # noqa: F401
from .grad import loglik_grad_emissions, loglik_grad_emissions_device  # noqa: F401
from .gauss import (expected_counts_gauss, expected_counts_gauss_device, fit_gauss, gauss_emissions,  # noqa: F401
                    gauss_emissions_device, gauss_hmm, reestimate_gauss)
from . import autograd  # noqa: F401
from .emissions import posterior_emissions, posterior_emissions_device, score_emissions  # noqa: F401
from .fit import fit_mle, fit_train, last_fit_stats  # noqa: F401
from .kbest import kbest_batch, kbest_batch_device  # noqa: F401
from .posterior import posterior_batch, posterior_batch_device, score_batch  # noqa: F401
from .sample import sample_batch, sample_batch_device, uniform  # noqa: F401
from .solver import (Constraints, GpuSolver, Solver, SuperSequence, load_sequences, load_tags,  # noqa: F401
                     write_output)
