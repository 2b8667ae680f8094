"""-m gpu: the layer-0 / layer-1 batch kernels of csrc/layer1_kernels.hpp (k_drone_step, k_ctrl, k_transform, k_rel_obs) and the
hand-rolled device math beneath them, against the float64 references and the derived bounds of tests/layer1_ref.py: every row of
tests/layer1_matrix.py at every env count of layer1_ref.N_ENVS, the seven subsets of simultaneous limiter violations, the ladder of
states around each limiter threshold, and the sweeps of q_asin, q_atan2 and q_sincos that qs_transform hands out bit for bit.
Every call goes through the raw C entry point on a device-I/O handle (one per integrator, which is part of a handle's
configuration), with each buffer a view into a larger device tensor, 256 sentinel bytes on each side (the Guards of
test_gpu_postproc.py): a store outside a buffer shows as a changed sentinel byte, never as a fault, and an output the kernel skips
keeps its sentinel payload.  Every input is a finite float inside the domain include/quadsim.h states -- but for the two
measurements of that domain, whose rows run over every binade of float32 and whose non-finite results are counted, not asserted.

Every test prints `layer1 ratio <kernel or function> <x>`: the worst error as a fraction of its bound."""
import ctypes as C
import functools

import numpy as np
import pytest

import layer1_matrix as M
import layer1_ref as L
from test_gpu_postproc import Guards

pytestmark = pytest.mark.gpu

f32 = np.float32
INTEG = {"frozen": 0, "rk4": 1}


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _report(what, worst):
    print("layer1 ratio %s %s" % (what, " ".join("%s=%.4f" % kv for kv in sorted(worst.items())) if isinstance(worst, dict) else "%.4f" % worst))


class Ctx:
    """a device-I/O handle as the context of the layer-1 calls; its nominal parameters are NOT the defaults (layer1_ref.PAR_NOM), so a
    kernel that ignores the configuration shows; each call is ordered against torch by a device-wide synchronisation before and a
    qs_sync after, and every buffer of every call sits between sentinel bands that are checked when the call has returned"""

    def __init__(self, qa, torch, integ):
        self.qa, self.torch, self.lib = qa, torch, qa._lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device())
        cfg = qa._lib.default_config()
        cfg.num_envs, cfg.device, cfg.integrator, cfg.dt = 1, torch.cuda.current_device(), integ, L.DT
        cfg.io_space = qa._lib.IO_DEVICE
        cfg.mass = L.PAR_NOM[0]
        cfg.inertia = (C.c_float * 3)(*L.PAR_NOM[1:4])
        self.h = C.c_void_p()
        qa._lib.check(self.lib.qs_create(C.byref(cfg), C.byref(self.h)), "qs_create")

    def close(self):
        if self.h:
            self.lib.qs_destroy(self.h)
            self.h = None

    def call(self, name, *args):
        self.torch.cuda.synchronize()
        rc = getattr(self.lib, name)(self.h, *args)
        assert rc == 0, "%s returned %d: %s" % (name, rc, self.lib.qs_last_error().decode("utf-8", "replace"))
        assert self.lib.qs_sync(self.h) == 0
        self.torch.cuda.synchronize()

    def _inout(self, G, a):
        """an in/out buffer: allocated as an output (its bands are checked, its payload may change), then filled"""
        t = G.out(a.shape, a.dtype)
        t.copy_(self.torch.as_tensor(np.ascontiguousarray(a)).to(self.device))
        return t

    def drone_step(self, x, limited_given=True):
        """-> the `after` of layer1_ref.check_drone_step; state and u_prev are in/out, as the header allows"""
        n = x["state"].shape[0]
        G = Guards(self.torch, self.device)
        state, u_prev = self._inout(G, x["state"]), self._inout(G, x["u_prev"])
        u = G.put(x["u"])
        par = G.put(x["par"]) if x["par"] is not None else None
        lim = G.out((n,), np.uint8)
        self.call("qs_drone_step", C.c_int64(n), _p(state), _p(u_prev), _p(u), _p(par), _p(lim) if limited_given else None)
        G.check()
        return dict(state=state.cpu().numpy(), u_prev=u_prev.cpu().numpy(), limited=lim.cpu().numpy(), u=u.cpu().numpy(),
                    par=par.cpu().numpy() if par is not None else None)

    def ctrl(self, x, mode, pass_last):
        n = x["state"].shape[0]
        G = Guards(self.torch, self.device)
        sd = self._inout(G, x["state_des"])
        s, sl = G.put(x["state"]), G.put(x["state_last"])
        u = G.out((n, 4))
        self.call("qs_ctrl", C.c_int64(n), C.c_int32(mode), _p(sd), _p(s), _p(sl) if pass_last else None, C.c_float(L.MASS), _p(u))
        G.check()
        return dict(state_des=sd.cpu().numpy(), u=u.cpu().numpy(), state=s.cpu().numpy(), state_last=sl.cpu().numpy())

    def transform(self, op, x):
        G = Guards(self.torch, self.device)
        xin = G.put(np.ascontiguousarray(x, f32))
        out = G.out((x.shape[0], L.WIDTH[op][1]))
        self.call("qs_transform", C.c_int32(op), C.c_int64(x.shape[0]), _p(xin), _p(out))
        G.check()
        return out.cpu().numpy()

    def rel_obs(self, x):
        n = x["chaser"].shape[0]
        G = Guards(self.torch, self.device)
        c, t = G.put(x["chaser"]), G.put(x["target"])
        obs = G.out((n, 12))
        self.call("qs_rel_obs", C.c_int64(n), _p(c), _p(t), _p(obs))
        G.check()
        return dict(obs=obs.cpu().numpy(), chaser=c.cpu().numpy(), target=t.cpu().numpy())


@pytest.fixture(scope="module")
def ctx(qa, torch):
    made = {name: Ctx(qa, torch, code) for name, code in INTEG.items()}
    yield made
    for c in made.values():
        c.close()


# the references are computed once per input and shared by the cases that need them
@functools.lru_cache(maxsize=None)
def _drone_case(n, integ, par_given):
    x = L.drone_inputs(n, integ, par_given)
    return x, L.drone_ref(x, integ)


@functools.lru_cache(maxsize=None)
def _ctrl_case(n):
    x = L.ctrl_inputs(n)
    return x, {mode: L.ctrl_ref(x, mode) for mode in (0, 1)}


def _before(x):
    return dict(x, limited=np.full(x["state"].shape[0], 0xA5, np.uint8))


# ---------------------------------------------------------------------------------------------------- the matrix
_DRONE = [(i, p, l, n) for i in M.INTEG for p in M.PAR for l in M.LIMITED for n in L.N_ENVS]


@pytest.mark.parametrize("integ,par,limited,n", _DRONE, ids=["%s-%s-%s-%d" % c for c in _DRONE])
def test_drone_step(ctx, integ, par, limited, n):
    x, ref = _drone_case(n, INTEG[integ], par == "par_given")
    after = ctx[integ].drone_step(x, limited == "limited_given")
    _report("k_drone_step", L.check_drone_step(_before(x), after, ref, limited == "limited_given"))


_CTRL = [(c, n) for c in M.CTRL for n in L.N_ENVS]


@pytest.mark.parametrize("case,n", _CTRL, ids=["%s-%d" % c for c in _CTRL])
def test_ctrl(ctx, case, n):
    x, refs = _ctrl_case(n)
    mode = 1 if case == "mode1" else 0
    after = ctx["frozen"].ctrl(x, mode, case != "mode0_last_null")
    _report("k_ctrl", L.check_ctrl(x, after, refs[mode], mode))


_TRANSFORM = [(name, n) for name in M.OPS for n in L.N_ENVS]


@pytest.mark.parametrize("name,n", _TRANSFORM, ids=["%s-%d" % c for c in _TRANSFORM])
def test_transform(ctx, name, n):
    op = M.OPS.index(name)
    x = L.transform_inputs(op, n)
    out = ctx["frozen"].transform(op, x)
    _report("k_transform-" + name, L.check_transform(op, x, dict(out=out), L.transform_ref(op, x)))


@pytest.mark.parametrize("n", L.N_ENVS)
def test_rel_obs(ctx, n):
    x = L.rel_obs_inputs(n)
    _report("k_rel_obs", L.check_rel_obs(x, ctx["rk4"].rel_obs(x), L.rel_obs_ref(x)))


# ---------------------------------------------------------------------------------------------------- the limiter
@pytest.mark.parametrize("integ", M.INTEG)
def test_limiter_subsets(ctx, integ):
    """every non-empty subset of {roll, pitch, yaw} violated at once, both signs, both saturated branches, r12 == -1.0f: the rewritten
    quaternion, the zeroed rates and the flag against float64"""
    x, which = L.limiter_inputs(INTEG[integ])
    ref = L.drone_ref(x, INTEG[integ])
    assert ref["limited"].all()
    _report("k_drone_step-limiter-subsets", L.check_drone_step(_before(x), ctx[integ].drone_step(x), ref))


@pytest.mark.parametrize("integ", M.INTEG)
def test_limiter_band(ctx, integ):
    """no decision differs from float64's at DELTA0 or more from a threshold; inside the band the flips are counted"""
    x, axis, want, actual = L.band_inputs(INTEG[integ])
    ref = L.drone_ref(x, INTEG[integ])
    after = ctx[integ].drone_step(x)
    out = L.outside_band(axis, actual)
    flips = after["limited"] != ref["limited"]
    for a, name in enumerate(L.AXES):
        m = axis == a
        print("layer1 band %s %s: delta_0 %.2e, flips inside %d of %d rows, outside %d of %d" % (
            integ, name, L.DELTA0[name], (flips & ~out & m).sum(), (~out & m).sum(), (flips & out & m).sum(), (out & m).sum()))
    assert not (flips & out).any(), "decisions differ at |delta| %s" % np.abs(actual[flips & out])[:8].tolist()
    sel = lambda d: {k: (None if v is None else v[out]) for k, v in d.items()}            # noqa: E731
    _report("k_drone_step-limiter-band", L.check_drone_step(sel(_before(x)), sel(after), sel(ref)))


# ---------------------------------------------------------------------------------------------------- the device math
def test_math_asin(ctx):
    R, _ = L.asin_sweep()
    worst = L.check_asin_sweep(R, ctx["frozen"].transform(3, R))
    _report("q_asin", worst)
    assert worst <= 1.0


def test_math_atan2(ctx):
    R = L.atan2_sweep()
    worst = L.check_atan2_sweep(R, ctx["frozen"].transform(3, R))
    _report("q_atan2", worst)
    assert worst <= 1.0


def test_math_sincos(ctx):
    x, a = L.sincos_sweep()
    out = ctx["frozen"].transform(1, x)
    sn, cs = L.check_sincos_sweep(a, out)
    for rng in L.SINCOS_RANGES:                                  # the worst of each range, for the record
        m = np.abs(a) <= f32(rng)
        print("layer1 sincos |x| <= %g: sin %.4f cos %.4f" % ((rng,) + L.check_sincos_sweep(a[m], out[m])))
    _report("q_sincos-sin", sn)
    _report("q_sincos-cos", cs)
    assert sn <= 1.0 and cs <= 1.0


def test_atan2_domain(ctx):
    """the domain include/quadsim.h states is the measured one, less a binade on each side"""
    R, es = L.domain_sweep()
    lo, hi = L.clean_binades(R, es, ctx["frozen"].transform(3, R))
    print("layer1 domain q_atan2: every binade of max(|y|, |x|) from 2^%d to 2^%d is clean; stated 2^%d .. 2^%d" % (lo, hi, L.ATAN2_LO, L.ATAN2_HI))
    assert lo <= L.ATAN2_LO - 1 and hi >= L.ATAN2_HI + 1


def test_quaternion_domain(ctx):
    q, es = L.quat_domain_sweep()
    lo, hi = L.clean_quat_binades(q, es, ctx["frozen"].transform(0, q), ctx["frozen"].transform(2, q))
    print("layer1 domain quat2euler, quat2rot: every binade of |q| from 2^%d to 2^%d is clean; stated 2^%d .. 2^%d" % (lo, hi, L.QUAT_LO, L.QUAT_HI))
    assert lo <= L.QUAT_LO - 1 and hi >= L.QUAT_HI + 1


# ---------------------------------------------------------------------------------------------------- the host-I/O wrappers
def test_host_wrappers_give_the_bits_of_the_device_path(qa, ctx):
    """one case per kernel through quadsim_amd/drone.py (a host-I/O handle of its own)"""
    n = 257
    x, _ = _drone_case(n, 1, True)
    dev = ctx["rk4"].drone_step(x)
    s, up, lim = qa.drone_step_batch(x["state"], x["u_prev"], x["u"], par=x["par"], dt=L.DT, integrator="rk4")
    assert L.same_bits(s, dev["state"]) and L.same_bits(up, dev["u_prev"]) and np.array_equal(lim, dev["limited"] != 0)
    x, _ = _ctrl_case(n)
    dev = ctx["frozen"].ctrl(x, 1, True)
    u, sd = qa.ctrl_batch(1, x["state_des"], x["state"], x["state_last"], mass=L.MASS)
    assert L.same_bits(u, dev["u"]) and L.same_bits(sd, dev["state_des"])
    for op, name in enumerate(M.OPS):
        xi = L.transform_inputs(op, n)
        assert L.same_bits(qa.transform_batch(name, xi).reshape(n, -1), ctx["frozen"].transform(op, xi))
    x = L.rel_obs_inputs(n)
    assert L.same_bits(qa.rel_obs_batch(x["chaser"], x["target"]), ctx["frozen"].rel_obs(x)["obs"])
