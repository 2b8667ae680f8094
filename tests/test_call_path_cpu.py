"""-m "not gpu": the one way from the Python wrappers to the C ABI -- the signature table against include/quadsim.h, the shipped
VecDockingEnv._call against a recording fake library, every wrapper that takes an env against a stub env that records what it
is asked to call, and a source scan for call sites that go round it."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "policy_best_model_v0.npz")
SCALARS = {"int32_t": "int32", "int64_t": "int64", "uint64_t": "uint64", "float": "float", "double": "double",
           "int": "int32"}   # LP64: int is 32 bits


def _header_prototypes(header="quadsim.h", prefix="qs_"):
    """{entry point: (kind of the result, [kind of every parameter])} of the prototypes `prefix`* in include/`header`, kinds
    "ptr" / "int32" / "int64" / "uint64" / "float" / "double" """
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def kind(decl):
        return "ptr" if "*" in decl else SCALARS[decl.replace("const", "").split()[0]]
    protos = {}
    for result, name, params in re.findall(r"\b((?:const\s+)?\w+[\s*]+)(%s[a-z_0-9]+)\s*\(([^()]*)\)\s*;" % prefix, text):
        assert name not in protos, name
        protos[name] = (kind(result), [kind(p) for p in (q.strip() for q in params.split(",")) if p != "void"])
    return protos


def _ctype_kind(t):
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    return {C.c_int32: "int32", C.c_int64: "int64", C.c_uint64: "uint64", C.c_float: "float", C.c_double: "double"}[t]


def test_signature_table_matches_the_header():
    """the count and the kind (pointer, int32, int64, uint64, float) of every parameter of every entry point"""
    from quadsim_amd import _lib
    protos = _header_prototypes()
    assert protos.pop("qs_last_error") == ("ptr", [])
    assert sorted(protos) == sorted(_lib.SIGNATURES) and len(protos) == 68
    for name, (result, kinds) in protos.items():
        assert result == "int32" and [_ctype_kind(t) for t in _lib.SIGNATURES[name]] == kinds, name
    assert sorted(_lib.EXPORTS) == sorted(list(_lib.SIGNATURES) + ["qs_last_error"])


def test_side_signature_tables_match_their_headers():
    """the same for the ten side libraries: the prototypes of each header are exactly the table's entries, with the count and
    kind (pointer, int32, int64, uint64, float, double) of every parameter and the kind of the result, and SIDE_POINTERS holds
    the positions of the pointers"""
    from quadsim_amd import _lib
    assert list(_lib.SIDE) == ["dyn", "dynmppi", "dynfit", "bc", "ppo", "gail", "trpo", "ddpg", "td3", "sac"]
    counts = {}
    for key, e in _lib.SIDE.items():
        protos = _header_prototypes(e["header"], e["prefix"])
        assert sorted(protos) == sorted(e["signatures"]) == sorted(e["exports"]), key
        for name, sig in e["signatures"].items():
            args, result = sig if isinstance(sig, tuple) else (sig, C.c_int)
            assert (_ctype_kind(result), [_ctype_kind(t) for t in args]) == protos[name], name
            assert _lib.SIDE_POINTERS[name] == tuple(i for i, k in enumerate(protos[name][1]) if k == "ptr"), name
        assert protos[e["prefix"] + "last_error"] == ("ptr", []) and protos[e["prefix"] + "version"] == ("int32", [])
        counts[key] = len(protos)
    assert counts == {"dyn": 6, "dynmppi": 4, "dynfit": 3, "bc": 5, "ppo": 5, "gail": 5, "trpo": 6, "ddpg": 4, "td3": 4, "sac": 5}
    assert _header_prototypes("quadsim_bc.h", "qsbc_")["qsbc_loss_blocks"] == ("int64", ["int64"])


def test_each_side_library_keeps_its_own_error_text():
    """a refused call (refused before the device is touched: nothing is launched) writes the error text of its own library and
    leaves the other nine as they were"""
    from quadsim_amd import _lib
    _lib.build_library()
    libs = {key: _lib.side_load(key) for key in _lib.SIDE}
    nbytes, six = C.c_size_t(0), (C.c_void_p * 6)()
    x = C.addressof(six)                                       # a non-NULL pointer that no refused call dereferences
    net = _lib.QsdfNet(12345)                                  # a struct_size no other test uses
    nets, replay, hyper = _lib.QsddNets(12345), _lib.QsddReplay(), _lib.QsddHyper()
    tnets, thyper, snets, shyper = _lib.QstdNets(12345), _lib.QstdHyper(), _lib.QssNets(12345), _lib.QssHyper()
    refusals = {
        "dyn": (lambda lib: lib.qsd_plan_workspace_bytes(-12345, 200, C.byref(nbytes)), b"n must be >= 1, got -12345"),
        "dynmppi": (lambda lib: lib.qsdm_workspace_bytes(1, -12345, 200, C.byref(nbytes)), b"horizon must be in [1, 1024], got -12345"),
        "dynfit": (lambda lib: lib.qsdf_fit(C.byref(net), x, x, 1, 1, 1, 1, 1e-4, 0.9, 0.999, 1e-8, 0, 0, 0, None, x, None, None, None),
                   b"QsdfNet.struct_size is 12345, expected %d" % C.sizeof(_lib.QsdfNet)),
        "bc": (lambda lib: lib.qsbc_loss(six, x, x, -12345, None, 1, x, x, 0, None), b"n must be in [1, 2^31), got -12345"),
        "ppo": (lambda lib: lib.qsp_workspace_bytes(-12345, 1, C.byref(nbytes)), b"batch must be in [1, 2^31), got -12345"),
        "gail": (lambda lib: lib.qsg_math(-12345, x, x, 10, None), b"kind must be in [0, 4], got -12345"),
        "trpo": (lambda lib: lib.qst_workspace_bytes(-54321, 7, C.byref(nbytes)), b"n must be in [1, 2^31), got -54321"),
        "ddpg": (lambda lib: lib.qsdd_update(C.byref(nets), C.byref(replay), x, None, 100, 10, C.byref(hyper), 0, x, 0, x, None, None),
                 b"QsddNets.struct_size is 12345, expected %d" % C.sizeof(_lib.QsddNets)),
        "td3": (lambda lib: lib.qstd_update(C.byref(tnets), C.byref(replay), x, None, 100, 10, C.byref(thyper), 0, 0, None, 0, None, x, 0, x,
                                            None, None),
                b"QstdNets.struct_size is 12345, expected %d" % C.sizeof(_lib.QstdNets)),
        "sac": (lambda lib: lib.qss_update(C.byref(snets), C.byref(replay), x, None, 100, 10, C.byref(shyper), 0, None, 0, None, x, 0, x,
                                           None, None, None),
                b"QssNets.struct_size is 12345, expected %d" % C.sizeof(_lib.QssNets)),
    }

    def texts():
        return {key: getattr(lib, _lib.SIDE[key]["prefix"] + "last_error")() for key, lib in libs.items()}
    for key, (refuse, text) in refusals.items():
        before = texts()
        assert before[key] != text
        assert refuse(libs[key]) == 1                          # Q??_ERR_INVALID
        after = texts()
        assert after.pop(key) == text
        del before[key]
        assert after == before, key
    assert len(set(texts().values())) == 10


# ---------------------------------------------------------------- the shipped _call on a fake library
class FakeLib:
    """every qs_* entry point logs (name, args after the handle) and returns `rc`"""

    def __init__(self, log):
        self.log, self.rc = log, 0

    def qs_last_error(self):
        return b"said the fake"

    def __getattr__(self, name):
        def fn(h, *args):
            assert h == "handle"
            self.log.append((name, args))
            return self.rc
        return fn


@pytest.fixture
def fake_env(monkeypatch):
    """a VecDockingEnv that was never constructed (no device): its own _call / _launch, the three stream hooks logging, and
    the module's library replaced by a FakeLib"""
    from quadsim_amd import _lib, vec_env
    log = []
    lib = FakeLib(log)
    monkeypatch.setattr(_lib, "_lib", lib)                     # what _lib.load() returns
    env = vec_env.VecDockingEnv.__new__(vec_env.VecDockingEnv)
    env._h, env._lib, env._follow_torch_stream, env._queue_host_ordered = "handle", lib, True, False
    env._use_current_stream = lambda: log.append("follow")
    env._inputs_ready = lambda queued=False: log.append(("inputs", queued))
    env._outputs_ready = lambda queued=False: log.append(("outputs", queued))
    yield env, lib, log
    env._h = None                                              # nothing for __del__ to destroy


def test_call_orders_follow_inputs_call_outputs(fake_env):
    env, lib, log = fake_env
    env._call("qs_reset", None, 7)
    assert log == ["follow", ("inputs", False), ("qs_reset", (None, 7)), ("outputs", False)]
    del log[:]
    env._launch("qs_step_ex", 1, 2.5, queued=True)             # the form step_async uses: step_wait orders the outputs
    assert log == ["follow", ("inputs", True), ("qs_step_ex", (1, 2.5))]
    del log[:]
    env._call("qs_rollout", 3, queued=True)
    assert log == ["follow", ("inputs", True), ("qs_rollout", (3,)), ("outputs", True)]


def test_call_converts_tensors_arrays_and_none(fake_env):
    torch = pytest.importorskip("torch")
    env, lib, log = fake_env
    t, a = torch.zeros(5), np.zeros(3, np.float32)
    k = C.c_uint64(0)
    ref = C.byref(k)
    env._call("qs_x", t, a, None, 4, 0.5, ref)
    (name, args), = [e for e in log if e[0] == "qs_x"]
    assert args[0] == t.data_ptr() and args[1] == a.ctypes.data and type(args[0]) is type(args[1]) is int
    assert args[2] is None and args[3] == 4 and type(args[3]) is int and args[4] == 0.5 and args[5] is ref


def test_call_raises_on_a_status_and_names_the_entry_point(fake_env):
    from quadsim_amd import QuadsimError
    env, lib, log = fake_env
    lib.rc = 2
    with pytest.raises(QuadsimError, match=r"qs_get_params failed \(2\): said the fake"):
        env._call("qs_get_params", None, None)
    assert log[-1][0] == "qs_get_params"                       # the outputs were not declared ready


def test_host_ordered_queue_is_drained_only_for_step_entry_points(fake_env):
    """the shipped _outputs_ready: on a handle that follows torch's stream it drains (qs_sync) exactly when the entry point
    launches steps and the private queue is host-ordered"""
    from quadsim_amd import vec_env
    env, lib, log = fake_env
    del env._outputs_ready                                     # the class's own
    assert type(env)._outputs_ready is vec_env.VecDockingEnv._outputs_ready
    env._outputs_ready()
    env._outputs_ready(queued=True)
    env._queue_host_ordered = True
    env._outputs_ready()
    assert log == []
    env._outputs_ready(queued=True)
    assert log == [("qs_sync", ())]
    env._queue_host_ordered, env._follow_torch_stream = False, False
    env._outputs_ready()
    assert log == [("qs_sync", ())] * 2


# ---------------------------------------------------------------- every wrapper that takes an env, on a stub env
class StubEnv:
    """what the wrappers may use of an env: a device, num_envs and _call (recorded).  No _lib, no _h, no stream hooks: a
    wrapper that reaches for them goes round _call and fails here"""

    def __init__(self, torch):
        self.device, self.num_envs, self.calls, self._nstep = torch.device("cpu"), 65, [], 0

    def _call(self, name, *args):
        self.calls.append((name, args))

    def get_init_state(self):                                  # PIDExpert.__init__: docking-v0 stores no initial states
        from quadsim_amd import QuadsimError
        raise QuadsimError("no stored initial states")

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _assert_calls(env, *names):
    """exactly these entry points, each with the arguments SIGNATURES gives it after the handle: tensors, arrays, None or
    ctypes references where the header has a pointer, Python ints and floats where it has a scalar"""
    import torch
    from quadsim_amd import _lib
    calls = env.take()
    assert [c[0] for c in calls] == list(names)
    for name, args in calls:
        kinds = [_ctype_kind(t) for t in _lib.SIGNATURES[name][1:]]
        assert len(args) == len(kinds), (name, len(args), len(kinds))
        for i, (a, kind) in enumerate(zip(args, kinds)):
            if kind == "ptr":
                assert a is None or isinstance(a, (torch.Tensor, np.ndarray, C.Array)) or type(a).__name__ == "CArgObject", (name, i, a)
            elif kind == "float":
                assert type(a) is float, (name, i, a)
            else:
                assert type(a) is int, (name, i, a)


@pytest.fixture
def stub():
    torch = pytest.importorskip("torch")
    return torch, StubEnv(torch)


def test_policy_wrappers_call_through_the_env(stub):
    import quadsim_amd as qa
    from quadsim_amd.policy import evaluate_policy_episodes, fused_policy_rollout
    torch, env = stub
    pol = qa.MlpPolicy.from_npz(GOLDEN, device="cpu")
    acts = pol.predict_hip(env, torch.zeros((65, 12)))
    assert acts.shape == (65, 4)
    _assert_calls(env, "qs_policy_forward")
    out = fused_policy_rollout(env, pol, 3)
    assert [tuple(t.shape) for t in out] == [(3, 65, 12), (3, 65), (3, 65), (3, 65), (3, 65, 4)]
    _assert_calls(env, "qs_policy_rollout")
    res = evaluate_policy_episodes(pol, env, 2, max_steps=4)
    assert res.returns.shape == (2, 65) and bool(torch.isnan(res.returns).all()) and not res.lengths.any()
    _assert_calls(env, "qs_policy_evaluate")
    # an ActorCriticPolicy is evaluated through its actor, whose weight list is built once
    ac = qa.ActorCriticPolicy.from_npz(GOLDEN, device="cpu")
    evaluate_policy_episodes(ac, env, 1)
    (_, first), = env.take()
    evaluate_policy_episodes(ac, env, 1)
    (_, second), = env.take()
    assert all(a is b for a, b in zip(first[2:8], second[2:8])) and first[2].shape == (128, 12)


def test_runner_wrapper_calls_through_the_env_in_both_layouts(stub):
    import quadsim_amd as qa
    from quadsim_amd import _lib
    torch, env = stub
    with np.load(GOLDEN, allow_pickle=False) as z:
        W = {k: z[k] for k in z.files}
    towers = dict(W, wv0=W["w0"][:, ::-1].copy(), bv0=W["b0"][::-1].copy())
    for weights, entry, struct in ((W, "qs_runner_rollout", _lib.QsActorCritic), (towers, "qs_runner_rollout_net", _lib.QsActorCriticNet)):
        ac = qa.ActorCriticPolicy(weights, device="cpu")
        s = ac.c_struct()
        assert type(s) is struct and s.struct_size == C.sizeof(struct) and s.wt1 == ac._wt[0].data_ptr() and s.bv3 == ac._wt[-1].data_ptr()
        assert all(getattr(s, f) for f, t in struct._fields_ if t is C.c_void_p)
        out = qa.fused_runner_rollout(env, ac, 3, noise=torch.zeros((3, 65, 4)), dones_in=torch.zeros(65))
        assert out["obs"].shape == (3, 65, 12) and out["flags"] is None
        _assert_calls(env, "qs_set_rollout_layout", entry)
    assert s.layout == _lib.NET_TOWERS and s.wtv1 == ac._wt[6].data_ptr()


def test_rollout_buffer_wrappers_call_through_the_env(stub):
    from quadsim_amd.rollout_buffer import EpisodeTracker, compute_gae, gae_and_flatten, swap_and_flatten
    torch, env = stub
    T, n = 3, 65
    f, u = torch.zeros((T, n)), torch.zeros((T, n), dtype=torch.uint8)
    advs, rets = compute_gae(env, f, f, u, f[0], u[0])
    assert advs.shape == rets.shape == (T, n)
    _assert_calls(env, "qs_gae")
    assert swap_and_flatten(env, torch.zeros((T, n, 12))).shape == (n * T, 12)
    _assert_calls(env, "qs_swap_and_flatten")
    assert swap_and_flatten(env, u).dtype == torch.uint8
    _assert_calls(env, "qs_swap_and_flatten_u8")
    out = gae_and_flatten(env, f, f, f, u, f[0], u[0])
    assert out["masks"].dtype == torch.bool and out["advs"] is None
    _assert_calls(env, "qs_gae_flatten")
    EpisodeTracker(env).update(f, u, u[0])
    _assert_calls(env, "qs_episode_stats")


def test_expert_wrappers_call_through_the_env(stub):
    import quadsim_amd as qa
    torch, env = stub
    ex = qa.PIDExpert(env)
    assert ex.act().shape == (65, 4)
    _assert_calls(env, "qs_expert_action")
    out = ex.rollout(3)
    assert out["dones"].dtype == torch.bool and env._nstep == 3
    _assert_calls(env, "qs_set_rollout_layout", "qs_expert_rollout")
    res = ex.evaluate(1, max_steps=4)
    assert res.finished.shape == (65,)
    _assert_calls(env, "qs_expert_evaluate")


def test_planner_wrappers_call_through_the_env(stub):
    from quadsim_amd import mpc
    torch, env = stub
    mpc.shooting_plan(env, 2, 8)
    _assert_calls(env, "qs_shooting_plan")
    mpc.shooting_plan(env, 2, 8, splits=2, return_scores=True, return_sequence=True)
    _assert_calls(env, "qs_shooting_plan_split")
    mpc.mppi_plan(env, 2, 8, 1)
    _assert_calls(env, "qs_mppi_plan")
    mpc.mppi_plan(env, 2, 8, 1, splits="auto", nominal=torch.zeros((65, 2, 4)), shift=True, return_trace=True)
    _assert_calls(env, "qs_mppi_plan_split")
    # the single-env shims have the same _call (without a stream protocol), so the host planners are the same code
    env.num_envs = 1
    mpc.shooting_plan_host(env, 2, 8)
    mpc.mppi_plan_host(env, 2, 8, 1, nominal=np.zeros((2, 4)))
    _assert_calls(env, "qs_shooting_plan_split", "qs_mppi_plan_split")


# ---------------------------------------------------------------- nothing goes round it
def test_no_call_site_goes_round_the_call_path():
    """in quadsim_amd/*.py outside _lib.py: no entry point is called on a library object (qs_destroy excepted: a handle that is
    going away follows no stream), raw _lib.call is used only by the host-I/O handles and, in vec_env.py, by the call path
    itself and the commented group-stream launches, and tensors become pointers in _lib.py alone.  The side libraries' entry
    points are attributes of nothing anywhere, _lib.py included: they are named as strings to _lib.side_call, which looks them
    up, and dynplan.py and bc.py reach their libraries through it alone"""
    raw_ok = {"qs_set_stream", "qs_sync", "name", "qs_step_group", "qs_step_groups"}
    for path in sorted(glob.glob(os.path.join(ROOT, "quadsim_amd", "*.py"))):
        f = os.path.basename(path)
        src = open(path).read()
        assert not re.findall(r"\.(qs(?:d|dm|df|bc)_[a-z_0-9]+)", src), f
        if f == "_lib.py":
            assert len(re.findall(r"getattr\(lib, name\)", src)) == 3          # the two loaders and side_call
            continue
        direct = re.findall(r"(?:\blib|\b_lib|load\w*\(\))\.(qs[a-z]*_[a-z_0-9]+)", src)
        assert set(direct) <= {"qs_destroy"}, (f, direct)
        for needle in ("data_ptr()", "data_as", "C.c_void_p(", "CDLL", "argtypes", "cuda_stream"):
            assert needle not in src or (needle == "cuda_stream" and f == "vec_env.py"), (f, needle)
        if f in ("dynplan.py", "bc.py"):
            assert "getattr(lib" not in src and src.count("_lib.side_call(") >= 3, f
        raw = re.findall(r"_lib\.call\(\s*([^,]+),\s*\"?([a-z_0-9]+)\"?", src)
        if f == "vec_env.py":
            assert sorted(n for _, n in raw) == sorted(raw_ok), raw
            for name in ("qs_step_group", "qs_step_groups"):
                before = src[:src.index('_lib.call(self._h, "%s"' % name)].rstrip().splitlines()[-1]
                assert before.lstrip().startswith("# not _call:"), (name, before)
        else:
            assert f in ("envs.py", "drone.py") or not raw, (f, raw)

