"""The table of the training-loop tests (tests/test_gpu_loops.py runs every row on the device, tests/test_loops_cpu.py holds the table
itself and runs what has a host path).  A helper module, not a test.

Each row names the loop, its constructor arguments, the seams between kernels the row is about and the mutants of the loop's Python
(MUTANTS; profiles/loops/README.md has the table of which test fails for which) it must catch.  The shapes are the smallest at which
every seam shows: 6 envs x 10 steps gives minibatches of 15 rows (the tail of the update's 16-row chunk) and T % 4 != 0 (the scalar
path of k_gae_flatten), 6 x 16 the vector path with one full group; `total` is never a multiple of the batch.

`ends`: the step of the run, counted from 1, at which the first episode of env 0, 1, 2 .. times out (the envs named are placed
600 - end steps into their episode after the first reset; the others run on): one inside the first roll-out or cycle, one ON its
last step (the flag that is carried over the boundary), one inside the second; the rest are in mid-episode at every boundary.  The
tests assert all of that on the record.
"""
import numpy as np

MUTANTS = {
    1: "frac computed with update instead of update - 1",
    2: "the schedule generator re-seeded every update",
    3: "swap_and_flatten skipped for one array: time-major rows",
    4: "the Runner keeps the first policy's cached image",
    5: "self.dones zeroed between roll-outs",
    6: "GAIL: tuple element 8 set to the paid reward",
    7: "discriminator_schedule drawn before minibatch_schedule",
    8: "collect_and_train stores obs1 as obs0",
    9: "action_noise.reset dropped",
    10: "replay_schedule drawn over capacity instead of size",
    11: "TD3's actor_t0 restarted at 0 on each learn call",
    12: "pretrain drops the partial minibatch",
    13: "pretrain reuses one shuffle",
}
TIME_LIMIT = 600               # the docking envs' episode length in steps


# the schedules of the rates: affine in frac, so that a frac that is off by one update gives another rate at EVERY update
def lr_of(frac):
    return 5.0e-4 + 5.0e-4 * frac


def clip_of(frac):
    return 0.1 + 0.1 * frac


def clipvf_of(frac):
    return 0.2 + 0.2 * frac


def frac_of(update, n_updates):
    """the remaining progress at update `update` (from 1) of `n_updates`, as the reference loop has it"""
    return 1.0 - (update - 1.0) / n_updates


def start_times(n_envs, ends):
    """t [n_envs] float32 for set_state: env i is 600 - ends[i] steps into its episode, the rest at 0"""
    t = np.zeros(n_envs, np.float32)
    t[:len(ends)] = TIME_LIMIT - np.asarray(ends, np.float32)
    return t


_PPO2 = dict(nminibatches=4, noptepochs=2, learning_rate=lr_of, cliprange=clip_of, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, gamma=0.99,
             lam=0.95)
_SEAMS_ON = ("rates at frac", "one carried schedule generator", "env-major rows under a minibatch index", "the next roll-out runs the updated policy",
             "dones carried over the roll-out boundary", "logs are the float64 means of the steps")


def _ppo2(layout, n_steps, vclip, seed):
    return dict(id="ppo2-%s-t%d-%s" % (layout, n_steps, "vclip" if vclip else "novclip"), loop="ppo2", layout=layout, env_id="docking-v0", n_envs=6,
                n_steps=n_steps, seed=seed, env_seed=seed + 10, ends=(4, n_steps, n_steps + 3),
                kwargs=dict(_PPO2, cliprange_vf=clipvf_of if vclip else None), seams=_SEAMS_ON, mutants=(1, 2, 3, 4, 5))


_GAIL = dict(d_steps=2, d_batch=16, d_learning_rate=1.0e-3, n_steps=10, **dict(_PPO2, cliprange_vf=None))
_OFF_SEAMS = ("the c-th draw of the carried generator over the ring's size", "the ring's rows under the schedule", "obs carried over the learn boundary",
              "the behaviour action: updated actor, OU noise reset where done", "reward_mean")
_DDPG = dict(nb_rollout_steps=20, nb_train_steps=2, batch_size=10, buffer_size=512, actor_lr=1.0e-3, critic_lr=2.0e-3, tau=0.05, gamma=0.99,
             obs_clip=5.0)
_TD3 = dict(learning_starts=0, train_freq=20, gradient_steps=3, batch_size=10, buffer_size=512, policy_delay=2, learning_rate=1.0e-3, tau=0.05,
            gamma=0.99, target_policy_noise=0.2, target_noise_clip=0.5)
_TRPO = dict(n_steps=8, max_kl=0.01, cg_iters=10, cg_damping=1.0e-2, entcoeff=0.0, gamma=0.99, lam=0.98, vf_stepsize=1.0e-3, vf_iters=2, vf_batch=32,
             fvp_stride=5, backtracks=10)

ROWS = [
    _ppo2("shared", 10, False, 11), _ppo2("towers", 10, True, 12), _ppo2("shared", 16, True, 23), _ppo2("towers", 16, False, 14),
    dict(id="gail-v1-stepwise", loop="gail", layout="towers", env_id="docking-v1", fused=None, n_envs=6, n_steps=10, seed=15, env_seed=25,
         ends=(4, 10, 13), expert=dict(n=50, train_fraction=0.8, seed=3), disc_seed=4, kwargs=_GAIL,
         seams=_SEAMS_ON + ("minibatch_schedule, then discriminator_schedule, on one generator", "the expert cursor reshuffles inside update 2",
                            "tuple element 8 is the env's reward, the returns are GAE over the paid one", "one merge of the running statistics per fit"),
         mutants=(1, 2, 3, 5, 6, 7)),
    dict(id="gail-v0-fused", loop="gail", layout="towers", env_id="docking-v0", fused=True, n_envs=6, n_steps=10, seed=16, env_seed=26,
         ends=(4, 10, 13), expert=dict(n=50, train_fraction=0.8, seed=3), disc_seed=4, kwargs=_GAIL,
         seams=_SEAMS_ON + ("minibatch_schedule, then discriminator_schedule, on one generator", "the expert cursor reshuffles inside update 2",
                            "tuple element 8 is the env's reward, the returns are GAE over the paid one", "one merge of the running statistics per fit"),
         mutants=(1, 2, 4, 5, 6, 7)),
    dict(id="trpo-plain", loop="trpo", env_id="docking-v0", n_envs=8, seed=17, env_seed=27, updates=2, expert=None, kwargs=_TRPO,
         seams=("policy step, then the value fit on the carried generator", "vf_loss is the mean of the value steps", "_trpo_steps continues"),
         mutants=(2,)),
    dict(id="trpo-expert", loop="trpo", env_id="docking-v0", n_envs=8, seed=18, env_seed=28, updates=2, expert=dict(n=50, train_fraction=0.8, seed=3),
         disc_seed=4, kwargs=dict(_TRPO, g_step=2, d_step=1, d_batch=32, d_stepsize=1.0e-3),
         seams=("two generator steps per update, both roll-outs recorded", "the discriminator fit on the LAST roll-out's rows, the cursor carried",
                "_trpo_steps continues"), mutants=(2,)),
    dict(id="ddpg", loop="ddpg", n_envs=16, cycles=3, seed=5, policy_seed=2, noise_seed=3, env_seed=7, ends=(7, 20, 27, 45),
         kwargs=dict(_DDPG, random_exploration=0.0), seams=_OFF_SEAMS, mutants=(2, 8, 9, 10)),
    dict(id="ddpg-explore", loop="ddpg", n_envs=16, cycles=1, seed=5, policy_seed=2, noise_seed=3, env_seed=7, ends=(7, 20),
         kwargs=dict(_DDPG, random_exploration=1.0), seams=("uniform actions in [-1, 1) replace the policy's",), mutants=()),
    dict(id="td3-keyed", loop="td3", noise="keyed", n_envs=16, cycles=3, seed=5, policy_seed=2, noise_seed=3, env_seed=7, ends=(7, 20, 27, 45),
         kwargs=_TD3, seams=_OFF_SEAMS + ("the delay phase straddles the learn calls", "the keyed normals of cycle c start at t0 = 3 (c - 1)"),
         mutants=(2, 8, 9, 10, 11)),
    dict(id="td3-caller", loop="td3", noise="caller", n_envs=16, cycles=3, seed=6, policy_seed=8, noise_seed=9, env_seed=10, ends=(7, 20, 27, 45),
         kwargs=_TD3, seams=_OFF_SEAMS + ("the delay phase straddles the learn calls", "the keyed normals of cycle c start at t0 = 3 (c - 1)"),
         mutants=(2, 8, 9, 10, 11)),
    dict(id="pretrain", loop="pretrain", n=150, train_fraction=0.7, batch_size=64, data_seed=61, split_seed=2,
         calls=(dict(n_epochs=3, val_interval=2, learning_rate=1.0e-3, adam_epsilon=1.0e-8, seed=4),
                dict(n_epochs=1, val_interval=1, learning_rate=1.0e-3, adam_epsilon=1.0e-8, seed=6)),
         seams=("every epoch a fresh shuffle from one generator", "the partial last minibatch of 41 rows", "train_loss and val_loss",
                "the second call continues the moments and the step count"), mutants=(12, 13)),
]
BY_ID = {r["id"]: r for r in ROWS}


def rows_of(loop):
    return [r for r in ROWS if r["loop"] == loop]


def ids_of(loop):
    return [r["id"] for r in rows_of(loop)]


def pretrain_data(row):
    """obs [n,12] docking observations and actions [n,4]: a fixed linear map of the observation through tanh, so that there is something
    to fit"""
    import dynplan_ref as dr
    rng = np.random.default_rng(row["data_seed"])
    obs = dr.sample_obs(row["n"], seed=row["data_seed"] + 1)
    act = np.tanh(obs.astype(np.float64) @ (rng.standard_normal((12, 4)) / 4.0)).astype(np.float32)
    return obs, act


def expert_data(spec):
    """a synthetic expert: obs [n,12] docking observations, actions [n,4] in [-1, 1]"""
    import dynplan_ref as dr
    rng = np.random.default_rng(spec["seed"] + 100)
    return {"obs": dr.sample_obs(spec["n"], seed=spec["seed"] + 101), "actions": rng.uniform(-1.0, 1.0, (spec["n"], 4)).astype(np.float32)}


# ---------------------------------------------------------------------------------------------------- explained_variance
# The one quantity of a log without a bound of its own.  Its reference is the float64 formula on the recorded values and returns.
# EV_MEASURED: the largest |float32 torch formula - float64| over ev_fixture at both recorded shapes (60 and 96 rows) and the seeds
# 0 .. 31, measured on the CPU by tests/test_loops_cpu.py, which asserts the figure; the device's reduction order is another, so its
# tolerance is 8 times that.  tests/test_gpu_loops.py asserts that the tolerance is below a tenth of the distance from the reference
# to the formula with its arguments swapped, on every recorded roll-out.
EV_MEASURED = 5.0e-8
EV_TOL = 8.0 * EV_MEASURED
EV_SHAPES, EV_SEEDS = (60, 96), range(32)


def ev_fixture(n, seed):
    """values and returns [n] float32 of the size a fresh policy's roll-out has: returns of a few tenths around an offset, values that
    explain a part of them"""
    rng = np.random.default_rng(1000 * n + seed)
    returns = (-0.5 + 0.3 * rng.standard_normal(n)).astype(np.float32)
    values = (0.5 * returns + 0.1 * rng.standard_normal(n) - 0.2).astype(np.float32)
    return values, returns
