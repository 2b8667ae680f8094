"""-m gpu: the one call path (VecDockingEnv._call) on a real device.  A handle on a stream of its own (use_torch_stream=False)
returns what a handle that follows torch's stream returns, bit for bit, from every wrapper and with nothing but the wrapper
itself ordering its kernels against torch's; and a wrapper called first under ``torch.cuda.stream(side)`` launches on `side`."""
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_best_model_v0.npz")
N = 65                                      # two tiles of 64 envs, the second holding one


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def nets(qa):
    return qa.MlpPolicy.from_npz(GOLDEN), qa.ActorCriticPolicy.from_npz(GOLDEN)


def _bits(torch, t):
    """a tensor as integers of its element width: equality of these is equality of bits (NaN slots included)"""
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()]) if t.is_floating_point() else t


def _drive(qa, torch, nets, **handle):
    """one handle through every wrapper; every input is produced by torch right before the call that reads it and every result
    is read (cloned on torch's stream) right after the call returns, with no synchronisation of the test's own
    -> [(label, tensor)]"""
    pol, ac = nets
    env = qa.VecDockingEnv("docking-v0", num_envs=N, randomise=1, auto_reset=True, seed=9, init_range=qa.C3_INIT_RANGE, **handle)
    dev = env.device
    g = torch.Generator(device=dev).manual_seed(3)
    got = []

    def fresh(*shape):
        return torch.rand(shape, generator=g, device=dev) * 2.0 - 1.0

    def keep(label, *tensors):
        got.extend(("%s[%d]" % (label, i), t.clone()) for i, t in enumerate(tensors) if t is not None)

    obs = env.reset()
    keep("reset", obs)
    for k in range(3):
        obs, rew, done, _ = env.step(fresh(N, 4))
        keep("step%d" % k, obs, rew, done, env.last_flags)
    obs, rew, done, a = env.step_policy(pol)
    keep("step_policy", obs, rew, done, a, env.last_flags)
    a = pol.predict_hip(env, obs * 1.0)
    keep("predict_hip", a)
    keep("predict_hip+step", *env.step(a)[:3])
    keep("rollout", *env.rollout(fresh(3, N, 4)))
    keep("rollout_slab", env.rollout_slab(fresh(3, N, 4)))
    keep("random_actions", env.random_actions(3))
    st = env.get_state(as_numpy=False)
    keep("get_state", *st.values())
    env.set_state(**{k: v * 1.0 for k, v in st.items()})
    keep("set_state", *env.get_state(as_numpy=False).values())
    keep("fused_policy_rollout", *qa.fused_policy_rollout(env, pol, 3))
    keep("evaluate", *qa.evaluate_policy_episodes(pol, env, 1, max_steps=4).tensors())
    ro = qa.fused_runner_rollout(env, ac, 3, noise=torch.randn((3, N, 4), generator=g, device=dev),
                                 dones_in=torch.zeros(N, dtype=torch.uint8, device=dev))
    keep("runner", *ro.values())
    gf = qa.gae_and_flatten(env, ro["rewards"], ro["values"], ro["neglogp"], ro["dones"], ro["last_values"], ro["last_dones"])
    keep("gae_and_flatten", *gf.values())
    ex = qa.PIDExpert(env)
    a = ex.act()
    keep("expert.act", a)
    keep("expert.act+step", *env.step(a)[:3])
    keep("expert.rollout", *ex.rollout(3).values())
    keep("shooting_plan", *env.shooting_plan(horizon=2, paths=8).values())
    keep("mppi_plan", *env.mppi_plan(horizon=2, paths=8, iterations=1).values())
    torch.cuda.synchronize()
    env.close()
    return got


def test_owned_stream_handle_equals_following_handle(qa, torch, nets):
    followed = _drive(qa, torch, nets)
    owned = _drive(qa, torch, nets, use_torch_stream=False)
    assert [k for k, _ in owned] == [k for k, _ in followed] and len(followed) > 60
    for (label, a), (_, b) in zip(followed, owned):
        assert a.dtype == b.dtype and a.shape == b.shape, label
        assert torch.equal(_bits(torch, a), _bits(torch, b)), label


def test_first_call_under_another_stream_follows_it(qa, torch, nets):
    """PIDExpert.act and predict_hip, each the first wrapper call inside ``with torch.cuda.stream(side)``: the handle moves
    to `side`, and the results are those of the same calls on the default stream (both are read-only on the env)"""
    pol, _ = nets
    env = qa.VecDockingEnv("docking-v0", num_envs=N, randomise=1, seed=9, init_range=qa.C3_INIT_RANGE)
    obs = env.reset()
    ex = qa.PIDExpert(env)
    a0, p0 = ex.act().clone(), pol.predict_hip(env, obs)
    default = env._stream
    for first in ("act", "predict_hip"):
        side = torch.cuda.Stream(device=env.device)
        assert side.cuda_stream != env._stream
        side.wait_stream(torch.cuda.current_stream(env.device))
        with torch.cuda.stream(side):
            got = ex.act().clone() if first == "act" else pol.predict_hip(env, obs)
            assert env._stream == side.cuda_stream, first
        side.synchronize()
        assert torch.equal(got, a0 if first == "act" else p0), first
    env.reset()                                                    # back on the default stream
    assert env._stream == default
    env.close()
