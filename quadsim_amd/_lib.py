"""ctypes binding of libquadsim_hip.so (the C ABI declared in include/quadsim.h).

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
# every fragment of the one translation unit is a rebuild dependency (dynplan_*.hpp belong to the second library,
# dynmppi_*.hpp to the third, dynfit_*.hpp to the fourth, bcfit_*.hpp to the fifth)
HEADERS = sorted(os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".hpp") and not h.startswith(("dynplan_", "dynmppi_", "dynfit_", "bcfit_"))) + [os.path.join(HERE, "..", "include", "quadsim.h")]
# the second library, libquadsim_dyn.so (include/quadsim_dyn.h; bound in dynplan.py): its own translation unit and code object
DYN_LIB_PATH = os.environ.get("QUADSIM_DYN_LIB") or os.path.join(CSRC, "libquadsim_dyn.so")
DYN_SOURCES = [os.path.join(CSRC, "dynplan.hip")]
DYN_HEADERS = [os.path.join(CSRC, h) for h in ("dynplan_image.hpp", "dynplan_kernels.hpp", "quadsim_device.hpp")] + [os.path.join(HERE, "..", "include", "quadsim_dyn.h")]
# the third library, libquadsim_dynmppi.so (include/quadsim_dyn_mppi.h; bound in dynplan.py): MPPI over the learned net.  It shares
# the second library's device code (the model step and the image layout) and none of its host code
DYNMPPI_LIB_PATH = os.environ.get("QUADSIM_DYNMPPI_LIB") or os.path.join(CSRC, "libquadsim_dynmppi.so")
DYNMPPI_SOURCES = [os.path.join(CSRC, "dynmppi.hip")]
DYNMPPI_HEADERS = [os.path.join(CSRC, h) for h in ("dynmppi_kernels.hpp", "dynplan_image.hpp", "dynplan_kernels.hpp", "quadsim_device.hpp")] + [
    os.path.join(HERE, "..", "include", "quadsim_dyn_mppi.h")]
# the fourth library, libquadsim_dynfit.so (include/quadsim_dyn_fit.h; bound in dynplan.py): the Adam fit of the learned net.  It
# takes the net's own tensors, not the image, and shares only the Philox generator of quadsim_device.hpp
DYNFIT_LIB_PATH = os.environ.get("QUADSIM_DYNFIT_LIB") or os.path.join(CSRC, "libquadsim_dynfit.so")
DYNFIT_SOURCES = [os.path.join(CSRC, "dynfit.hip")]
DYNFIT_HEADERS = [os.path.join(CSRC, h) for h in ("dynfit_kernels.hpp", "quadsim_device.hpp")] + [
    os.path.join(HERE, "..", "include", "quadsim_dyn_fit.h")]
# the fifth library, libquadsim_bc.so (include/quadsim_bc.h; bound in bc.py): behaviour cloning of the actor.  It takes the policy's
# own tensors and shares the forward chain and the Adam step of the fourth library's fragment at the source level
BC_LIB_PATH = os.environ.get("QUADSIM_BC_LIB") or os.path.join(CSRC, "libquadsim_bc.so")
BC_SOURCES = [os.path.join(CSRC, "bcfit.hip")]
BC_HEADERS = [os.path.join(CSRC, h) for h in ("bcfit_kernels.hpp", "dynfit_kernels.hpp", "quadsim_device.hpp")] + [
    os.path.join(HERE, "..", "include", "quadsim_bc.h")]

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


class QuadsimError(RuntimeError):
    pass


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise QuadsimError("hipcc not found: cannot build libquadsim_hip.so")


def _up_to_date(lib, deps):
    return os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(d) for d in deps)


def build_dyn_library(force=False, verbose=False):
    """libquadsim_dyn.so with the flags of the main library -> its path"""
    if not force and _up_to_date(DYN_LIB_PATH, DYN_SOURCES + DYN_HEADERS):
        return DYN_LIB_PATH
    cmd = [hipcc_path(), "-std=c++20", "-O3", "-fno-slp-vectorize", "-ffp-contract=on", "--offload-arch=gfx950", "-fPIC", "-shared",
           "-Wno-unused-result", *DYN_SOURCES, "-o", DYN_LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return DYN_LIB_PATH


def build_dynmppi_library(force=False, verbose=False):
    """libquadsim_dynmppi.so with the flags of the main library -> its path"""
    if not force and _up_to_date(DYNMPPI_LIB_PATH, DYNMPPI_SOURCES + DYNMPPI_HEADERS):
        return DYNMPPI_LIB_PATH
    cmd = [hipcc_path(), "-std=c++20", "-O3", "-fno-slp-vectorize", "-ffp-contract=on", "--offload-arch=gfx950", "-fPIC", "-shared",
           "-Wno-unused-result", *DYNMPPI_SOURCES, "-o", DYNMPPI_LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return DYNMPPI_LIB_PATH


def build_dynfit_library(force=False, verbose=False):
    """libquadsim_dynfit.so with the flags of the main library -> its path"""
    if not force and _up_to_date(DYNFIT_LIB_PATH, DYNFIT_SOURCES + DYNFIT_HEADERS):
        return DYNFIT_LIB_PATH
    cmd = [hipcc_path(), "-std=c++20", "-O3", "-fno-slp-vectorize", "-ffp-contract=on", "--offload-arch=gfx950", "-fPIC", "-shared",
           "-Wno-unused-result", *DYNFIT_SOURCES, "-o", DYNFIT_LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return DYNFIT_LIB_PATH


def build_bc_library(force=False, verbose=False):
    """libquadsim_bc.so with the flags of the main library -> its path"""
    if not force and _up_to_date(BC_LIB_PATH, BC_SOURCES + BC_HEADERS):
        return BC_LIB_PATH
    cmd = [hipcc_path(), "-std=c++20", "-O3", "-fno-slp-vectorize", "-ffp-contract=on", "--offload-arch=gfx950", "-fPIC", "-shared",
           "-Wno-unused-result", *BC_SOURCES, "-o", BC_LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return BC_LIB_PATH


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -shared: cross-compiles without a GPU.  Builds all five libraries, returns the main one's
    path."""
    build_dyn_library(force, verbose)
    build_dynmppi_library(force, verbose)
    build_dynfit_library(force, verbose)
    build_bc_library(force, verbose)
    deps = SOURCES + HEADERS
    if not force and _up_to_date(LIB_PATH, deps):
        return LIB_PATH
    # -ffp-contract=on: a*b+c fuses only where one expression says so, so every kernel that inlines the same device
    # function computes the same bits (the serial and the role-split step kernel, the policy kernels' env step);
    # hipcc's default (fast) fuses across statements depending on the surrounding code.  Same instruction count.
    # -fno-slp-vectorize: SLP packs the scalar f32 chains into v_pk_* pairs at the price of ~300 extra
    # v_mov and +56 VGPRs; measured 5 % slower on the step kernel (profiles/r01/ab_slp.txt)
    cmd = [hipcc_path(), "-std=c++20", "-O3", "-fno-slp-vectorize", "-ffp-contract=on", "--offload-arch=gfx950", "-fPIC", "-shared",
           "-Wno-unused-result", *SOURCES, "-lhsa-runtime64", "-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


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
