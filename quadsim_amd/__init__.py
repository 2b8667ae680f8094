"""quadsim_amd -- MI355X-native drop-in for QuadSim's env.step() hot path.

Python host code over a C ABI (include/quadsim.h) into hand-written HIP kernels
for gfx950.  No CPU fallback: importing is cheap, but every env needs the built
library and a GPU.
"""
from . import _lib
from ._lib import QuadsimError, build_library
from .drone import Drone, controller, ctrl_batch, drone_step_batch, rel_obs_batch, transform_batch
from .envs import DockingEnv, HoveringEnv, ImitatingDockingEnv, MovingDockingEnv, make, register_gym_ids
from .vec_env import C3_INIT_RANGE, VecDockingEnv, shard_range
from . import distributed
from .policy import EvalResult, MlpPolicy, evaluate_policy, evaluate_policy_episodes, fused_policy_rollout, rollout_with_policy
from .rollout_buffer import EpisodeTracker, compute_gae, gae_and_flatten, swap_and_flatten
from .expert import IncompleteEpisodes, PIDExpert, assemble_expert_dataset, record_expert_dataset
from .mpc import MPPI, ShootingMPC, mppi_plan, plan_splits, shooting_plan
from .dynplan import DynamicsNet, LearnedMPPI, LearnedShootingMPC, check_fit_args, check_mppi_plan_args, learned_mppi_plan, learned_shooting_plan
from .runner import ActorCriticPolicy, Runner, fused_runner_rollout
from .sb2 import load_sb2_model, read_sb2_weights
from .bc import ExpertData, bc_fit, bc_loss, check_bc_args, epoch_schedule, pretrain
from .ppo2 import PPO2, check_ppo2_args, minibatch_schedule, ppo2_update, reset_ppo2_optimizer, torch_ppo2_update
from .gail import GAIL, Discriminator, GailRunner, check_gail_args, discriminator_schedule, torch_discriminator_fit
from .trpo import (TRPO, check_trpo_args, reset_trpo_optimizer, torch_trpo_policy_step, torch_trpo_vf_fit, trpo_policy_step, trpo_vf_fit,
                   vf_schedule)
from .ddpg import DDPG, DDPGPolicy, OUNoise, ReplayBuffer, check_ddpg_args, ddpg_update, replay_schedule, torch_ddpg_update
from .td3 import TD3, NormalActionNoise, TD3Policy, check_td3_args, reset_td3_optimizer, td3_update, torch_td3_update
from .sac import SAC, SACPolicy, check_sac_args, reset_sac_optimizer, sac_update, torch_sac_update

__all__ = ["VecDockingEnv", "DockingEnv", "MovingDockingEnv", "ImitatingDockingEnv", "HoveringEnv", "Drone", "controller", "make", "register_gym_ids",
           "shard_range", "build_library", "QuadsimError", "C3_INIT_RANGE", "drone_step_batch", "ctrl_batch",
           "rel_obs_batch", "transform_batch", "_lib", "distributed", "MlpPolicy", "rollout_with_policy", "fused_policy_rollout", "compute_gae", "swap_and_flatten", "gae_and_flatten", "EpisodeTracker", "PIDExpert", "record_expert_dataset", "assemble_expert_dataset", "IncompleteEpisodes", "ActorCriticPolicy", "Runner", "fused_runner_rollout", "load_sb2_model", "read_sb2_weights",
           "evaluate_policy", "evaluate_policy_episodes", "EvalResult", "ShootingMPC", "shooting_plan", "plan_splits", "MPPI", "mppi_plan",
           "DynamicsNet", "LearnedShootingMPC", "learned_shooting_plan", "LearnedMPPI", "learned_mppi_plan", "check_mppi_plan_args", "check_fit_args",
           "ExpertData", "epoch_schedule", "pretrain", "bc_fit", "bc_loss", "check_bc_args",
           "PPO2", "ppo2_update", "torch_ppo2_update", "minibatch_schedule", "check_ppo2_args", "reset_ppo2_optimizer",
           "GAIL", "Discriminator", "GailRunner", "discriminator_schedule", "torch_discriminator_fit", "check_gail_args",
           "DDPG", "DDPGPolicy", "ReplayBuffer", "OUNoise", "replay_schedule", "ddpg_update", "torch_ddpg_update", "check_ddpg_args",
           "TRPO", "check_trpo_args", "vf_schedule", "trpo_policy_step", "trpo_vf_fit", "reset_trpo_optimizer", "torch_trpo_policy_step",
           "torch_trpo_vf_fit",
           "TD3", "TD3Policy", "NormalActionNoise", "td3_update", "torch_td3_update", "check_td3_args", "reset_td3_optimizer",
           "SAC", "SACPolicy", "sac_update", "torch_sac_update", "check_sac_args", "reset_sac_optimizer"]

register_gym_ids()
