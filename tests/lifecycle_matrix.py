"""One row per instantiation of the lifecycle kernels at the end of csrc/step_kernels.hpp: the resets (k_reset, k_hover_reset),
the construction-time fills (k_ctor_init, k_fill_init_nominal, k_fill_ctr, k_nominal_obs, k_fill_par), the action stream
(k_fill_actions) and the AoS <-> AoSoA conversions behind get / set (k_state_io<TO_USER>, k_par_io<TO_USER>): 8 + 2 + 2 = 12.
Every other matrix builds its cases and reads its results through these kernels.

Imported by tests/test_lifecycle_cpu.py, which checks that the rows are exactly the instantiations in the built code object,
and by tests/test_gpu_lifecycle.py, which runs every row.  Plain Python: no torch here.

A row holds the C ABI entry point that launches the kernel in production, the handle configuration (env id, randomise,
set_init_state) that reaches it, and the id of one GPU test case that holds it to its reference on every element between
sentinel bytes.  The kernels are plain or <bool> kernels of the anonymous namespace: kernel_notes.anon_instantiations() sees
them.
"""
KERNELS = ("k_reset", "k_hover_reset", "k_ctor_init", "k_fill_init_nominal", "k_fill_ctr", "k_nominal_obs", "k_fill_par",
           "k_fill_actions", "k_state_io", "k_par_io")

_F = "tests/test_gpu_lifecycle.py::"


def _row(key, entry, env_id, test, randomise=0, set_init=False):
    return dict(id="-".join(str(x) for x in key), kernel=key[0], key=key, entry=entry, env_id=env_id, randomise=randomise,
                set_init=set_init, test=_F + test)


ROWS = [
    _row(("k_reset",), "qs_reset", "docking-v0", "test_reset[rocrand2-1000]", randomise=2),
    _row(("k_hover_reset",), "qs_reset", "hovering-v0", "test_reset[hover-257]"),
    _row(("k_ctor_init",), "qs_create", "docking-v1", "test_ctor_jitter[docking-v1-1000]"),
    _row(("k_fill_init_nominal",), "qs_set_init_state", "docking-v0", "test_reset[stored_nominal_target-257]", randomise=2, set_init=True),
    _row(("k_fill_ctr",), "qs_set_step_counter", "docking-v0", "test_step_counter_reaches_every_tile", randomise=1),
    _row(("k_nominal_obs",), "qs_create", "docking-v0", "test_nominal_obs_is_the_nominal_reset_observation[257]"),
    _row(("k_fill_par",), "qs_create", "docking-v2", "test_fresh_handle[docking-v2-2-1000]", randomise=2),
    _row(("k_fill_actions",), "qs_fill_random_actions", "docking-v0", "test_fill_random_actions[3-1000]"),
    _row(("k_state_io", 0), "qs_set_state", "docking-v0", "test_state_io[docking-v0-257]"),
    _row(("k_state_io", 1), "qs_get_state", "hovering-v0", "test_state_io[hovering-v0-257]"),
    _row(("k_par_io", 0), "qs_set_params", "docking-v0", "test_par_io[257]"),
    _row(("k_par_io", 1), "qs_get_params", "docking-v0", "test_par_io[1000]"),
]

# Census: every kernel base name of the built gfx950 code object -> the matrix module (its ROWS carry the test ids) or one test id
# that pins it.  tests/test_lifecycle_cpu.py fails for a kernel the table does not name and for a name no kernel has.
CENSUS = {
    # env step and evaluation: tests/step_matrix.py
    "k_env": "step_matrix", "k_env_split": "step_matrix", "k_env_resident": "step_matrix", "k_hover": "step_matrix",
    "k_policy_evaluate": "step_matrix", "k_policy_evaluate_fast": "step_matrix",
    # Runner and policy roll-outs: tests/rollout_matrix.py
    "k_runner_rollout": "rollout_matrix", "k_runner_split": "rollout_matrix", "k_policy_rollout": "rollout_matrix",
    "k_policy_rollout_fast": "rollout_matrix",
    # GAE, flatten, episode accounting: tests/postproc_matrix.py
    "k_gae_reduce": "postproc_matrix", "k_gae_apply": "postproc_matrix", "k_gae_serial": "postproc_matrix",
    "k_gae_flatten": "postproc_matrix", "k_swap_flatten": "postproc_matrix", "k_swap_flatten_v4": "postproc_matrix",
    "k_episode_stats": "postproc_matrix",
    # PID expert: tests/expert_matrix.py
    "k_expert_action": "expert_matrix", "k_expert_rollout": "expert_matrix", "k_expert_evaluate": "expert_matrix",
    # the actor alone: the actor numerics
    "k_policy_forward": "tests/test_gpu_actor_numerics.py::test_predict_hip_within_bound",
    "k_policy_forward_fast": "tests/test_gpu_actor_numerics.py::test_predict_hip_within_bound",
    # layer 1 and layer 0: tests/layer1_matrix.py
    "k_drone_step": "layer1_matrix", "k_ctrl": "layer1_matrix", "k_rel_obs": "layer1_matrix", "k_transform": "layer1_matrix",
    # the planners on the exact simulator: tests/plan_matrix.py
    "k_shooting_plan": "plan_matrix", "k_wide_candidates": "plan_matrix", "k_wide_finish": "plan_matrix", "k_mppi": "plan_matrix",
    "k_pathint_part_roll": "plan_matrix", "k_pathint_part_sums": "plan_matrix", "k_pathint_part_finish": "plan_matrix",
}
CENSUS.update({k: "lifecycle_matrix" for k in KERNELS})
