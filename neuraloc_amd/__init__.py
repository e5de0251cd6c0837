"""neuraloc_amd -- MI355X-native OCflow rollout (the NeuralOC hot path) behind the reference's
own Python interface.  Importing the package does not load the HIP library; the first call does,
and raises if it is missing."""
from .Phi import Phi, ResNN, antiderivTanh, derivTanh
from .OCflow import OCflow, ocG
from .problem import Cross2D, SwarmTraj, Quadcopter
from .initProb import initProb, resample
from .distributed import OCflow_sharded, shard_rows, reduce_cost_sums
from ._lib import check_errors
from .baseline import baseline_loss, baseline_report, baseline_adam_steps, solve_baseline
from .baseline_quad import quad_baseline_loss, quad_baseline_report, quad_initial_guess, solve_baseline_quad
from .disturb import disturbed_rollout, brownian_disturbances, noise_study
from .train import disturbed_ocflow_train
from .adversary import disturbance_gradient, worst_case_disturbances
from .noise import counter_disturbances, noisy_rollout, noisy_ocflow_train, noise_corr_scales
from .minmax import minmax_ocflow_train, ascend_disturbances, adversarial_step, pgd_ocflow_train
from .ensemble import PhiEnsemble, ensemble_rollout, ensemble_ocflow_train
from .ensemble_noise import ensemble_noisy_rollout, ensemble_noisy_ocflow_train, ensemble_noise_study
from .risk import risk_weights, weighted_ocflow_train, risk_ocflow_train
from .ensemble_risk import ensemble_risk_weights, ensemble_weighted_ocflow_train, ensemble_risk_ocflow_train
from .ensemble_minmax import (ensemble_disturbed_rollout, ensemble_disturbed_ocflow_train, ensemble_minmax_ocflow_train,
                              ensemble_disturbance_gradient, ensemble_ascend_disturbances, ensemble_worst_case_disturbances,
                              ensemble_adversarial_step)
from .hold import held_rollout, hold_study

__all__ = ["Phi", "ResNN", "antiderivTanh", "derivTanh", "OCflow", "ocG", "Cross2D", "SwarmTraj",
           "Quadcopter", "initProb", "resample", "OCflow_sharded", "shard_rows", "reduce_cost_sums", "check_errors",
           "baseline_loss", "baseline_report", "baseline_adam_steps", "solve_baseline",
           "quad_baseline_loss", "quad_baseline_report", "quad_initial_guess", "solve_baseline_quad",
           "disturbed_rollout", "brownian_disturbances", "noise_study", "disturbed_ocflow_train",
           "disturbance_gradient", "worst_case_disturbances",
           "minmax_ocflow_train", "ascend_disturbances", "adversarial_step", "pgd_ocflow_train",
           "PhiEnsemble", "ensemble_rollout", "ensemble_ocflow_train",
           "ensemble_noisy_rollout", "ensemble_noisy_ocflow_train", "ensemble_noise_study",
           "risk_weights", "weighted_ocflow_train", "risk_ocflow_train",
           "ensemble_risk_weights", "ensemble_weighted_ocflow_train", "ensemble_risk_ocflow_train",
           "ensemble_disturbed_rollout", "ensemble_disturbed_ocflow_train", "ensemble_minmax_ocflow_train",
           "ensemble_disturbance_gradient", "ensemble_ascend_disturbances", "ensemble_worst_case_disturbances",
           "ensemble_adversarial_step", "held_rollout", "hold_study"]
