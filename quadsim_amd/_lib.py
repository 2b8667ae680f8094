"""ctypes binding of libquadsim_hip.so (the C ABI declared in include/quadsim.h), and the table (SIDE), build, loader and call
helper of the ten side libraries that dynplan.py, bc.py, ppo2.py, gail.py, trpo.py, ddpg.py, td3.py and sac.py wrap: eleven
libraries with the main one -- which is how the headers count (libquadsim_td3.so is the tenth library, libquadsim_sac.so the
eleventh).

There is deliberately no fallback of any kind: if the HIP library is missing or
no MI355X is visible, loading / qs_create raise.  Nothing here imports oracle/.
"""
import ctypes as C
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("QUADSIM_HIP_LIB") or os.path.join(CSRC, "libquadsim_hip.so")  # override: A/B builds
SOURCES = [os.path.join(CSRC, "quadsim_hip.hip")]
# every fragment of the one translation unit is a rebuild dependency, bar those of the side libraries (SIDE below)
HEADERS = sorted(os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".hpp") and not h.startswith(
    ("dynplan_", "dynmppi_", "dynfit_", "bcfit_", "ppo2_", "gail_", "ddpg_", "trpo_", "td3_", "sac_", "train_", "side_"))) + [os.path.join(HERE, "..", "include", "quadsim.h")]

QS_OK = 0
KIND_V0, KIND_V2, KIND_V1, KIND_HOVER = 0, 1, 2, 3
INTEG_FROZEN, INTEG_RK4 = 0, 1
IO_DEVICE, IO_HOST = 0, 1
RANDOMISE_NONE, RANDOMISE_INIT, RANDOMISE_PARAMS = 0, 1, 2
ORDER_HOST, ORDER_STREAM = 0, 1
SHOOT_REWARD, SHOOT_POSITION = 0, 1
FLAG_DOCKED, FLAG_OVERLIMIT, FLAG_OVERTIME, FLAG_CHASER_LIMITED, FLAG_TARGET_LIMITED = 1, 2, 4, 8, 16


class QsConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("kind", C.c_int32), ("num_envs", C.c_int64), ("device", C.c_int32),
        ("integrator", C.c_int32), ("dt", C.c_float), ("auto_reset", C.c_int32), ("randomise", C.c_int32),
        ("io_space", C.c_int32), ("seed", C.c_uint64), ("env_id_offset", C.c_uint64),
        ("init_range", C.c_float * 4), ("mass_scale", C.c_float * 2), ("inertia_scale", C.c_float * 2),
        ("mass", C.c_float), ("inertia", C.c_float * 3), ("stream", C.c_void_p),
        ("external_stream", C.c_int32), ("reserved", C.c_int32),
    ]


class QsActorCritic(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("squash", C.c_int32),
        ("wt1", C.c_void_p), ("b1", C.c_void_p), ("wt2", C.c_void_p), ("b2", C.c_void_p),
        ("wt3", C.c_void_p), ("b3", C.c_void_p), ("wtv2", C.c_void_p), ("bv2", C.c_void_p),
        ("wtv3", C.c_void_p), ("bv3", C.c_void_p), ("logstd", C.c_float * 4),
    ]


NET_SHARED_TRUNK, NET_TOWERS = 0, 1


class QsActorCriticNet(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("squash", C.c_int32), ("layout", C.c_int32), ("reserved", C.c_int32),
        ("wt1", C.c_void_p), ("b1", C.c_void_p), ("wt2", C.c_void_p), ("b2", C.c_void_p),
        ("wt3", C.c_void_p), ("b3", C.c_void_p), ("wtv1", C.c_void_p), ("bv1", C.c_void_p),
        ("wtv2", C.c_void_p), ("bv2", C.c_void_p), ("wtv3", C.c_void_p), ("bv3", C.c_void_p), ("logstd", C.c_float * 4),
    ]


vp, i64, u64, i32, f32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_float
# argument types of every entry point (all return int), the handle included: load() applies this table, EXPORTS is derived from
# it, and tests/test_call_path_cpu.py compares it with the prototypes of include/quadsim.h
SIGNATURES = {
    "qs_config_default": [C.POINTER(QsConfig)],
    "qs_version": [],
    "qs_create": [C.POINTER(QsConfig), C.POINTER(vp)],
    "qs_destroy": [vp],
    "qs_reset": [vp, vp, vp],
    "qs_step": [vp, vp, vp, vp, vp, vp, vp],
    "qs_rollout": [vp, i64, vp, vp, vp, vp, vp],
    "qs_rollout_stepwise": [vp, i64, vp, vp, vp, vp, vp],
    "qs_rollout_slab": [vp, i64, vp, vp, vp],
    "qs_fill_random_actions": [vp, i64, u64, vp],
    "qs_get_state": [vp] + [vp] * 6,
    "qs_set_state": [vp] + [vp] * 6,
    "qs_set_params": [vp, vp, vp],
    "qs_get_params": [vp, vp, vp],
    "qs_set_init_state": [vp, vp, vp],
    "qs_get_init_state": [vp, vp, vp],
    "qs_obs_dim": [vp, C.POINTER(i32)],
    "qs_get_step_counter": [vp, C.POINTER(u64)],
    "qs_set_step_counter": [vp, u64],
    "qs_set_stream": [vp, vp, i32],
    "qs_sync": [vp],
    "qs_timer_start": [vp],
    "qs_timer_stop": [vp, C.POINTER(f32)],
    "qs_drone_step": [vp, i64, vp, vp, vp, vp, vp],
    "qs_ctrl": [vp, i64, i32, vp, vp, vp, f32, vp],
    "qs_rel_obs": [vp, i64, vp, vp, vp],
    "qs_transform": [vp, i32, i64, vp, vp],
    "qs_gae": [vp, i64, i64, vp, vp, vp, vp, vp, f32, f32, vp, vp],
    "qs_swap_and_flatten": [vp, i64, i64, i64, vp, vp],
    "qs_expert_action": [vp, vp, f32, f32, vp],
    "qs_expert_rollout": [vp, i64, vp, f32, f32] + [vp] * 6,
    "qs_expert_evaluate": [vp, i32, i64, vp, f32, f32] + [vp] * 5,
    "qs_shooting_plan": [vp, i32, i32, i32] + [vp] * 5,
    "qs_mppi_plan": [vp, i32, i32, i32, i32, f32, f32, i32] + [vp] * 8,
    "qs_shooting_plan_split": [vp, i32, i32, i32, i32] + [vp] * 5,
    "qs_shooting_plan_splits": [vp, i32, C.POINTER(i32)],
    "qs_mppi_plan_split": [vp, i32, i32, i32, i32, f32, f32, i32, i32] + [vp] * 8,
    "qs_policy_rollout": [vp, i64] + [vp] * 11,
    "qs_policy_rollout_fast": [vp, i64] + [vp] * 6,
    "qs_policy_rollout_fast_blob_bytes": [],
    "qs_policy_forward": [vp, i64] + [vp] * 8,
    "qs_policy_forward_fast": [vp, i64, vp, vp, vp],
    "qs_policy_evaluate": [vp, i32, i64] + [vp] * 11,
    "qs_policy_evaluate_fast": [vp, i32, i64] + [vp] * 6,
    "qs_runner_rollout": [vp, i64, C.POINTER(QsActorCritic)] + [vp] * 12,
    "qs_runner_rollout_fast": [vp, i64, vp, C.POINTER(C.c_float), i32] + [vp] * 12,
    "qs_runner_rollout_fast_blob_bytes": [],
    "qs_runner_rollout_net": [vp, i64, C.POINTER(QsActorCriticNet)] + [vp] * 12,
    "qs_runner_rollout_net_fast": [vp, i64, i32, vp, C.POINTER(C.c_float), i32] + [vp] * 12,
    "qs_runner_rollout_net_fast_blob_bytes": [i32],
    "qs_step_ex": [vp] * 8,
    "qs_set_groups": [vp, i32, i32],
    "qs_group_count": [vp, C.POINTER(i32)],
    "qs_group_range": [vp, i32, C.POINTER(i64), C.POINTER(i64)],
    "qs_group_stream": [vp, i32, C.POINTER(vp)],
    "qs_group_set_stream": [vp, i32, vp],
    "qs_step_group": [vp, i32] + [vp] * 7,
    "qs_step_groups": [vp] * 8,
    "qs_groups_fork": [vp],
    "qs_groups_join": [vp],
    "qs_swap_and_flatten_u8": [vp, i64, i64, vp, vp],
    "qs_gae_flatten": [vp, i64, i64, vp, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp, vp, vp],
    "qs_episode_stats": [vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp],
    "qs_set_rollout_layout": [vp, i32],
    "qs_set_queue_mode": [vp, i32],
    "qs_get_queue_mode": [vp, C.POINTER(i32)],
    "qs_set_queue_ordering": [vp, i32],
    "qs_get_queue_ordering": [vp, C.POINTER(i32)],
}
EXPORTS = sorted(SIGNATURES) + ["qs_last_error"]


# ---------------------------------------------------------------------------------------------------- the side libraries
class QsdNet(C.Structure):                     # include/quadsim_dyn.h
    _fields_ = [("struct_size", C.c_uint32), ("h1", C.c_int32), ("h2", C.c_int32), ("reserved", C.c_int32)] + [
        (k, C.c_void_p) for k in ("wt1", "b1", "wt2", "b2", "wt3", "b3", "in_mean", "in_rscale", "out_std", "out_mean")]


class QsdfNet(C.Structure):                    # include/quadsim_dyn_fit.h
    _fields_ = [("struct_size", C.c_uint32), ("h1", C.c_int32), ("h2", C.c_int32), ("reserved", C.c_int32),
                ("w", C.c_void_p * 6), ("m", C.c_void_p * 6), ("v", C.c_void_p * 6)] + [
        (k, C.c_void_p) for k in ("in_mean", "in_rscale", "out_mean", "out_rscale")]


class QsbcNet(C.Structure):                    # include/quadsim_bc.h
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("w", C.c_void_p * 6), ("m", C.c_void_p * 6), ("v", C.c_void_p * 6)]


class QspNet(C.Structure):                     # include/quadsim_ppo.h
    _fields_ = [("struct_size", C.c_uint32), ("layout", C.c_int32), ("w", C.c_void_p * 13), ("m", C.c_void_p * 13), ("v", C.c_void_p * 13)]


class QsgNet(C.Structure):                     # include/quadsim_gail.h
    _fields_ = [("struct_size", C.c_uint32), ("hidden", C.c_int32), ("w", C.c_void_p * 6), ("m", C.c_void_p * 6), ("v", C.c_void_p * 6),
                ("mean", C.c_void_p), ("rscale", C.c_void_p)]


class QspBatch(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("n", C.c_int64)] + [
        (k, C.c_void_p) for k in ("obs", "actions", "returns", "values", "neglogp")]


class QspHyper(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32)] + [
        (k, C.c_double) for k in ("lr", "cliprange", "cliprange_vf", "ent_coef", "vf_coef", "max_grad_norm", "beta1", "beta2", "eps")]


class QstNet(C.Structure):                     # include/quadsim_trpo.h
    _fields_ = [("struct_size", C.c_uint32), ("layout", C.c_int32), ("w", C.c_void_p * 13), ("m", C.c_void_p * 13), ("v", C.c_void_p * 13)]


class QstBatch(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("n", C.c_int64)] + [
        (k, C.c_void_p) for k in ("obs", "actions", "returns", "values")]


class QstHyper(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("cg_iters", C.c_int32), ("backtracks", C.c_int32), ("fvp_stride", C.c_int32)] + [
        (k, C.c_double) for k in ("max_kl", "cg_damping", "entcoeff", "residual_tol")]


class QstTrace(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32)] + [
        (k, C.c_void_p) for k in ("fvp_in", "fvp_out", "cg", "x", "fullstep", "ls")]


class QsddNets(C.Structure):                   # include/quadsim_ddpg.h
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("w", C.c_void_p * 24), ("m", C.c_void_p * 12), ("v", C.c_void_p * 12)]


class QsddReplay(C.Structure):                 # the one replay struct of the three off-policy headers (QstdReplay, QssReplay below)
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("n", C.c_int64)] + [
        (k, C.c_void_p) for k in ("obs0", "act", "rew", "obs1", "done")]


QstdReplay = QssReplay = QsddReplay


class QsddHyper(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32)] + [
        (k, C.c_double) for k in ("gamma", "tau", "actor_lr", "critic_lr", "obs_clip", "beta1", "beta2", "eps")]


class QstdNets(C.Structure):                   # include/quadsim_td3.h
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("w", C.c_void_p * 36), ("m", C.c_void_p * 18), ("v", C.c_void_p * 18)]


class QstdHyper(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("policy_delay", C.c_int32)] + [
        (k, C.c_double) for k in ("gamma", "tau", "actor_lr", "critic_lr", "target_policy_noise", "target_noise_clip", "beta1", "beta2", "eps")]


class QssNets(C.Structure):                    # include/quadsim_sac.h
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("w", C.c_void_p * 30), ("m", C.c_void_p * 24), ("v", C.c_void_p * 24),
                ("alpha_state", C.c_void_p)]


class QssHyper(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("auto_alpha", C.c_int32)] + [
        (k, C.c_double) for k in ("gamma", "tau", "lr", "target_entropy", "beta1", "beta2", "eps")]


class QssTrace(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32)] + [
        (k, C.c_void_p) for k in ("logp_out", "vlogp_out", "act_out", "fwd_out")]


f64, psize, psix = C.c_double, C.POINTER(C.c_size_t), C.POINTER(vp * 6)
# The ten libraries beside the main one, each its own translation unit, .so and code object, by short name, in build order.
# They share at the source level only: device fragments (*_kernels.hpp, dynplan_image.hpp, train_pieces.hpp, train_offpolicy.hpp,
# quadsim_device.hpp) and the host fragments side_host.hpp (all ten), dynplan_host.hpp (the two planners) and side_offpolicy.hpp
# (the three off-policy trainers).  An entry: the variable that overrides
# the path (A/B builds) and the file name, the source, the fragments it is rebuilt for, the public header, the prefix that the
# kernel names of its code object start with and no kernel name of another library does, and the signatures of its entry points
# in the header's order -- argument types or, where the result is not int, (argument types, result type).  Everything else is
# derived: the paths, EXPORTS per library, the build, the loader.  tests/test_call_path_cpu.py compares the signatures with the
# headers, tests/side_cases.py holds the rest of an entry against the built library.
SIDE = {
    # random-shooting MPC over the learned net (bound in dynplan.py).  kernels: the other two kernels of this library, k_dyn_finish
    # and k_dyn_pack, come in with dynplan_kernels.hpp and so are in "dynmppi" as well, and k_dyn_ begins the kernel of "dynfit" too:
    # k_dyn_plan is the longest prefix that separates this library from both
    "dyn": dict(env="QUADSIM_DYN_LIB", file="libquadsim_dyn.so", source="dynplan.hip", header="quadsim_dyn.h", prefix="qsd_", kernels=b"k_dyn_plan",
                fragments=("dynplan_host.hpp", "dynplan_image.hpp", "dynplan_kernels.hpp", "quadsim_device.hpp", "side_host.hpp"),
                signatures={
                    "qsd_version": [],
                    "qsd_last_error": ([], C.c_char_p),
                    "qsd_net_image_bytes": [i32, i32, psize],
                    "qsd_net_pack": [C.POINTER(QsdNet), vp, vp],
                    "qsd_plan_workspace_bytes": [i64, i32, psize],
                    "qsd_shooting_plan": [vp, i64, vp, u64, u64, u64, i32, i32] + [vp] * 8}),
    # MPPI over the learned net (dynplan.py): the device code of "dyn" (the model step, the image layout), no host state of it
    "dynmppi": dict(env="QUADSIM_DYNMPPI_LIB", file="libquadsim_dynmppi.so", source="dynmppi.hip", header="quadsim_dyn_mppi.h", prefix="qsdm_", kernels=b"k_dynm_",
                    fragments=("dynmppi_kernels.hpp", "dynplan_host.hpp", "dynplan_image.hpp", "dynplan_kernels.hpp", "quadsim_device.hpp",
                               "side_host.hpp"),
                    signatures={
                        "qsdm_version": [],
                        "qsdm_last_error": ([], C.c_char_p),
                        "qsdm_workspace_bytes": [i64, i32, i32, psize],
                        "qsdm_mppi_plan": [vp, i32, i32, i64, vp, u64, u64, u64, i32, i32, i32, f32, f32, i32] + [vp] * 11}),
    # the Adam fit of the learned net (dynplan.py): takes the net's own tensors, not the image; the chunk primitives of
    # train_pieces.hpp, the Philox generator of the main library
    "dynfit": dict(env="QUADSIM_DYNFIT_LIB", file="libquadsim_dynfit.so", source="dynfit.hip", header="quadsim_dyn_fit.h", prefix="qsdf_", kernels=b"k_dyn_fit",
                   fragments=("dynfit_kernels.hpp", "quadsim_device.hpp", "side_host.hpp", "train_pieces.hpp"),
                   signatures={
                       "qsdf_version": [],
                       "qsdf_last_error": ([], C.c_char_p),
                       "qsdf_fit": [C.POINTER(QsdfNet), vp, vp, i64, i64, i32, i32, f64, f64, f64, f64, i64, u64, u64, vp, vp, vp, psix, vp]}),
    # behaviour cloning of the actor (bc.py): takes the policy's own tensors; the tower pieces of train_pieces.hpp
    "bc": dict(env="QUADSIM_BC_LIB", file="libquadsim_bc.so", source="bcfit.hip", header="quadsim_bc.h", prefix="qsbc_", kernels=b"k_bc_",
               fragments=("bcfit_kernels.hpp", "quadsim_device.hpp", "side_host.hpp", "train_pieces.hpp"),
               signatures={
                   "qsbc_version": [],
                   "qsbc_last_error": ([], C.c_char_p),
                   "qsbc_fit": [C.POINTER(QsbcNet), vp, vp, i64, vp, vp, i32, i32, f64, f64, f64, f64, i64, vp, psix, vp],
                   "qsbc_loss_blocks": ([i64], i64),
                   "qsbc_loss": [psix, vp, vp, i64, vp, i64, vp, vp, i32, vp]}),
    # the PPO2 update (ppo2.py): takes the policy's own tensors; the tower pieces of train_pieces.hpp
    "ppo": dict(env="QUADSIM_PPO_LIB", file="libquadsim_ppo.so", source="ppo2.hip", header="quadsim_ppo.h", prefix="qsp_", kernels=b"k_ppo_",
                fragments=("ppo2_kernels.hpp", "quadsim_device.hpp", "side_host.hpp", "train_pieces.hpp"),
                signatures={
                    "qsp_version": [],
                    "qsp_last_error": ([], C.c_char_p),
                    "qsp_auto_slices": [i64],
                    "qsp_workspace_bytes": [i64, i32, psize],
                    "qsp_update": [C.POINTER(QspNet), C.POINTER(QspBatch), vp, i32, i64, i32, C.POINTER(QspHyper), i64, vp, u64, vp,
                                   C.POINTER(vp * 13), vp]}),
    # GAIL's discriminator (gail.py): its own tensors; the Adam step and the chunk geometry of train_pieces.hpp, q_tanh of the main library
    "gail": dict(env="QUADSIM_GAIL_LIB", file="libquadsim_gail.so", source="gail.hip", header="quadsim_gail.h", prefix="qsg_", kernels=b"k_gail_",
                 fragments=("gail_kernels.hpp", "quadsim_device.hpp", "side_host.hpp", "train_pieces.hpp"),
                 signatures={
                     "qsg_version": [],
                     "qsg_last_error": ([], C.c_char_p),
                     "qsg_fit": [C.POINTER(QsgNet), vp, vp, i64, vp, vp, i64, vp, vp, vp, i32, i32, f64, f64, f64, f64, f64, i64, vp, psix, vp],
                     "qsg_reward": [C.POINTER(QsgNet), vp, vp, i64, i64, i64, vp, vp, i32, vp],
                     "qsg_math": [i32, vp, vp, i64, vp]}),
    # the TRPO update (trpo.py): the policy's own tensors; the tower pieces of train_pieces.hpp
    "trpo": dict(env="QUADSIM_TRPO_LIB", file="libquadsim_trpo.so", source="trpo.hip", header="quadsim_trpo.h", prefix="qst_", kernels=b"k_trpo_",
                 fragments=("trpo_kernels.hpp", "quadsim_device.hpp", "side_host.hpp", "train_pieces.hpp"),
                 signatures={
                     "qst_version": [],
                     "qst_last_error": ([], C.c_char_p),
                     "qst_auto_slices": [i64],
                     "qst_workspace_bytes": [i64, i32, psize],
                     "qst_policy_step": [C.POINTER(QstNet), C.POINTER(QstBatch), i32, C.POINTER(QstHyper), vp, u64, vp, vp,
                                         C.POINTER(QstTrace), vp],
                     "qst_vf_fit": [C.POINTER(QstNet), vp, vp, i64, vp, i32, i32, f64, f64, f64, f64, i64, vp, psix, vp]}),
    # the DDPG update (ddpg.py): the four nets' own tensors; the tower pieces of train_pieces.hpp, the off-policy pieces of
    # train_offpolicy.hpp and side_offpolicy.hpp, q_tanh of the main library
    "ddpg": dict(env="QUADSIM_DDPG_LIB", file="libquadsim_ddpg.so", source="ddpg.hip", header="quadsim_ddpg.h", prefix="qsdd_", kernels=b"k_ddpg_",
                 fragments=("ddpg_kernels.hpp", "quadsim_device.hpp", "side_host.hpp", "side_offpolicy.hpp", "train_offpolicy.hpp", "train_pieces.hpp"),
                 signatures={
                     "qsdd_version": [],
                     "qsdd_last_error": ([], C.c_char_p),
                     "qsdd_workspace_bytes": [psize],
                     "qsdd_update": [C.POINTER(QsddNets), C.POINTER(QsddReplay), vp, vp, i32, i32, C.POINTER(QsddHyper), i64, vp, u64, vp,
                                     C.POINTER(vp * 12), vp]}),
    # the TD3 update (td3.py): the six nets' own tensors; the tower pieces and the streamed nets of train_pieces.hpp, the off-policy
    # pieces, q_tanh, the Philox counter and the normals of the main library
    "td3": dict(env="QUADSIM_TD3_LIB", file="libquadsim_td3.so", source="td3.hip", header="quadsim_td3.h", prefix="qstd_", kernels=b"k_td3_",
                fragments=("td3_kernels.hpp", "quadsim_device.hpp", "side_host.hpp", "side_offpolicy.hpp", "train_offpolicy.hpp", "train_pieces.hpp"),
                signatures={
                    "qstd_version": [],
                    "qstd_last_error": ([], C.c_char_p),
                    "qstd_workspace_bytes": [psize],
                    "qstd_update": [C.POINTER(QstdNets), C.POINTER(QstdReplay), vp, vp, i32, i32, C.POINTER(QstdHyper), i64, i64, vp, u64, vp,
                                    vp, u64, vp, C.POINTER(vp * 18), vp]}),
    # the SAC update (sac.py): the five nets' own tensors and the temperature; the tower pieces and the streamed nets of
    # train_pieces.hpp, the off-policy pieces, q_tanh, q_ln, the Philox counter and the normals of the main library
    "sac": dict(env="QUADSIM_SAC_LIB", file="libquadsim_sac.so", source="sac.hip", header="quadsim_sac.h", prefix="qss_", kernels=b"k_sac_",
                fragments=("sac_kernels.hpp", "quadsim_device.hpp", "side_host.hpp", "side_offpolicy.hpp", "train_offpolicy.hpp", "train_pieces.hpp"),
                signatures={
                    "qss_version": [],
                    "qss_last_error": ([], C.c_char_p),
                    "qss_workspace_bytes": [psize],
                    "qss_update": [C.POINTER(QssNets), C.POINTER(QssReplay), vp, vp, i32, i32, C.POINTER(QssHyper), i64, vp, u64, vp, vp, u64,
                                   vp, C.POINTER(QssTrace), C.POINTER(vp * 24), vp],
                    "qss_math": [i32, vp, vp, i64, vp]}),
}
for _e in SIDE.values():
    _e["path"] = os.environ.get(_e["env"]) or os.path.join(CSRC, _e["file"])
    _e["sources"] = [os.path.join(CSRC, _e["source"])]
    _e["headers"] = [os.path.join(CSRC, h) for h in _e["fragments"]] + [os.path.join(HERE, "..", "include", _e["header"])]
    _e["exports"] = list(_e["signatures"])
# the positions of every entry point's pointer parameters: side_call sends those through as_arg and leaves the scalars to the
# argtypes (as_arg on a scalar costs 0.3 us, and a plan has a dozen of them)
SIDE_POINTERS = {name: tuple(i for i, t in enumerate(sig[0] if isinstance(sig, tuple) else sig) if t is vp or issubclass(t, C._Pointer))
                 for _e in SIDE.values() for name, sig in _e["signatures"].items()}


class QuadsimError(RuntimeError):
    pass


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise QuadsimError("hipcc not found: cannot build libquadsim_hip.so")


def _up_to_date(lib, deps):
    return os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(d) for d in deps)


# -ffp-contract=on: a*b+c fuses only where one expression says so, so every kernel that inlines the same device
# function computes the same bits (the serial and the role-split step kernel, the policy kernels' env step);
# hipcc's default (fast) fuses across statements depending on the surrounding code.  Same instruction count.
# -fno-slp-vectorize: SLP packs the scalar f32 chains into v_pk_* pairs at the price of ~300 extra
# v_mov and +56 VGPRs; measured 5 % slower on the step kernel (profiles/r01/ab_slp.txt)
HIPCC_FLAGS = ["-std=c++20", "-O3", "-fno-slp-vectorize", "-ffp-contract=on", "--offload-arch=gfx950", "-fPIC", "-shared", "-Wno-unused-result"]


def build_one_library(sources, deps, out, link=(), force=False, verbose=False):
    """hipcc HIPCC_FLAGS sources link -o out, unless `out` is newer than the sources and `deps` -> out"""
    if force or not _up_to_date(out, sources + deps):
        cmd = [hipcc_path(), *HIPCC_FLAGS, *sources, *link, "-o", out]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return out


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -shared: cross-compiles without a GPU.  Builds all eleven libraries (the ten side libraries, then the
    main one), returns the main one's path."""
    for e in SIDE.values():
        build_one_library(e["sources"], e["headers"], e["path"], (), force, verbose)
    return build_one_library(SOURCES, HEADERS, LIB_PATH, ["-lhsa-runtime64"], force, verbose)

_lib = None


def load():
    """dlopen the library; raises QuadsimError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QuadsimError(
            "%s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). quadsim_amd has no CPU fallback." % LIB_PATH)
    # torch (the owner of device memory and streams in this package) bundles its own HIP runtime;
    # it must be the one already resident when libquadsim_hip.so resolves libamdhip64, otherwise two
    # runtimes end up in one process and device pointers / streams cannot be shared.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.qs_last_error.argtypes = []
    lib.qs_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != QS_OK:
        msg = load().qs_last_error().decode("utf-8", "replace")
        raise QuadsimError("%s failed (%d): %s" % (what or "quadsim call", rc, msg))


def as_arg(a):
    """what an entry point receives for `a`: a torch tensor as its device pointer, a numpy array as its data pointer, None as
    NULL; anything else (scalars, ctypes values, byref) as it is.  Pointers go as plain ints, which the argtypes of SIGNATURES
    turn into void * (building a c_void_p for each costs 0.1 us, seven times per step); the caller keeps the array alive"""
    if a is None:
        return None
    data_ptr = getattr(a, "data_ptr", None)
    if data_ptr is not None:
        return data_ptr()
    ct = getattr(a, "ctypes", None)
    return a if ct is None else ct.data


def call(h, name, *args):
    """the entry point `name` on the handle `h`, arguments through as_arg; QuadsimError unless it returns QS_OK.  Nothing is
    ordered against any stream here: handles with a stream protocol call through VecDockingEnv._call"""
    check(getattr(_lib or load(), name)(h, *map(as_arg, args)), name)


def create(cfg):
    """qs_create -> the new handle"""
    h = C.c_void_p()
    check(load().qs_create(C.byref(cfg), C.byref(h)), "qs_create")
    return h


def fast_blob_bytes(entry, *args):
    """the size the library expects of the packed weight image of the split-bf16 entry point `entry` (a size, not a status)"""
    return getattr(load(), entry + "_blob_bytes")(*args)


def default_config():
    cfg = QsConfig()
    check(load().qs_config_default(C.byref(cfg)), "qs_config_default")
    return cfg


# ---------------------------------------------------------------------------------------------------- the side libraries' call path
_side = {}


def side_load(key):
    """dlopen the side library `key` of SIDE, once; raises QuadsimError if it has not been built (there is no fallback)"""
    lib = _side.get(key)
    if lib is None:
        e = SIDE[key]
        if not os.path.exists(e["path"]):
            raise QuadsimError("%s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'`." % e["path"])
        import torch  # noqa: F401  (its HIP runtime must be the resident one: see load)
        lib = C.CDLL(e["path"])
        for name, sig in e["signatures"].items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
        _side[key] = lib
    return lib


def side_check(key, rc, what):
    if rc != 0:
        msg = getattr(side_load(key), SIDE[key]["prefix"] + "last_error")().decode("utf-8", "replace")
        raise QuadsimError("%s failed (%d): %s" % (what, rc, msg))


def side_call(key, lib, name, *args, device=None):
    """the entry point `name` of `lib`, the loaded side library `key` (from the wrapper's own loader, which tests replace),
    its pointer arguments (tensors, arrays, None) through as_arg, its scalars as they are.  With `device`: that device selected and torch's current stream on it as the last argument.
    QuadsimError unless it returns 0; an entry point whose result is no status (qsbc_loss_blocks) -> the result"""
    fn = getattr(lib, name)
    args, pointers = list(args), SIDE_POINTERS[name]
    for i in (pointers if device is None else pointers[:-1]):      # the last pointer of a launching entry point is its stream
        args[i] = as_arg(args[i])
    if device is None:
        rc = fn(*args)
    else:
        import torch
        with torch.cuda.device(device):
            rc = fn(*args, torch.cuda.current_stream(device).cuda_stream)
    if fn.restype is not C.c_int:
        return rc
    side_check(key, rc, name)


def six(tensors):
    """void *[6] of six tensors' device pointers (the w / m / v / grads arrays of both fits)"""
    return (C.c_void_p * 6)(*map(as_arg, tensors))


def pointers(tensors):
    """void *[len] of the tensors' device pointers, NULL for None (the w / m / v / grads arrays of QspNet)"""
    return (C.c_void_p * len(tensors))(*map(as_arg, tensors))


def new_tensor(device, shape, dtype):
    """an uninitialised output of the call, from torch's caching allocator: no device allocation in steady state"""
    import torch
    return torch.empty(shape, dtype=getattr(torch, dtype), device=device)


def check_tensor(name, t, dtype, shape, device):
    """ValueError unless `t` is a contiguous torch tensor of `dtype` (its torch name) and `shape` on `device`; a str in `shape`
    names a free dimension, shape None is any shape"""
    import torch
    ok = isinstance(t, torch.Tensor) and t.dtype == getattr(torch, dtype) and t.device == device and t.is_contiguous() and (
        shape is None or t.dim() == len(shape))
    if ok and shape is not None:
        for s, d in zip(shape, t.shape):
            ok = ok and (s == d or isinstance(s, str))
    if not ok:
        of = "" if shape is None else " of shape [%s]" % ", ".join(map(str, shape))
        raise ValueError("%s must be a contiguous %s tensor%s on %s" % (name, dtype, of, device))


def check_adam_args(lr, beta1, beta2, eps, t0, steps, word):
    """-> (lr, beta1, beta2, eps) as floats; ValueError for what both fits refuse of Adam's arguments (`word`: what the fit
    calls its steps)"""
    import math
    lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
    if not (t0 >= 0 and t0 + steps < 1 << 31):
        raise ValueError("t0 must be >= 0 with t0 + %s below 2^31, got %d" % (word, t0))
    for name, val in (("lr", lr), ("eps", eps)):
        if not math.isfinite(val):
            raise ValueError("%s must be finite, got %r" % (name, val))
    for name, val in (("beta1", beta1), ("beta2", beta2)):
        if not 0.0 <= val < 1.0:
            raise ValueError("%s must be in [0, 1), got %r" % (name, val))
    return lr, beta1, beta2, eps
