"""MI355X-native particle-filter hot path behind the pf_initialize / pf_update! / pf_resample! /
pf_rejuvenate! API of probcomp/GenParticleFilters.jl.  The directory name contains a
dot, so import it through the repo-root shim:  `import gpf_amd`."""
from . import _lib, models                                        # noqa: F401
from .api import *                                                # noqa: F401,F403
from .api import (DeviceParticleFilterState, DeviceParticleFilterSubState, ParticleFilterState, ParticleFilterSubState, ParticleFilterView, ErrorException, Tempering, mh, move_reweight, locally_optimal, line_fixed, MoveProposal, locally_optimal_move, outlier_propose,
                  pf_initialize, pf_update, pf_step_ess, choiceproduct, pf_resample, pf_multinomial_resample, pf_residual_resample,
                  pf_stratified_resample, pf_resample_blocks, block_resampled, block_ancestor_log_weights, block_stats, block_mean, block_var, block_moments, block_proportionmap, pf_initialize_blocks, pf_update_blocks, pf_run_blocks, BlockRun, pf_rejuvenate_blocks, set_block_params, get_block_params, block_params_rows, pf_resample_across_blocks, block_ancestors, pf_rejuvenate, pf_move_accept, pf_move_reweight,
                  pf_resize, pf_multinomial_resize, pf_residual_resize, pf_optimal_resize, pf_replicate, pf_dereplicate, pf_coalesce, pf_introduce,
                  effective_sample_size, get_ess, log_ml_estimate, get_lml_est, get_log_weights,
                  get_log_norm_weights, get_norm_weights, get_traces, sample_unweighted_traces, block_sample_trajectories, block_backward_trajectories, block_smoothed_moments, block_smoothed_weights, block_smoothed_pair_moments, block_map_trajectories, block_forward_moments, BlockForwardMoments, mean, var, proportionmap)
