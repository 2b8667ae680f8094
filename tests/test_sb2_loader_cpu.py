"""-m "not gpu": the stable-baselines archive loader (quadsim_amd.sb2) on the committed re-packed archives, the tower
layout's torch heads and weight images, the C ABI of the layout-aware Runner entry points, and the ISA of the tower Runner
kernels in the built library."""
import io
import json
import os
import re
import shutil
import subprocess
import zipfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOWERS_ZIP = os.path.join(GOLDEN, "sb2_ppo2_docking_621_h_30M.zip")
SHARED_ZIP = os.path.join(GOLDEN, "sb2_best_model_v0.zip")
REF = os.environ.get("QUADSIM_REFERENCE", "/root/reference")
LLVM = "/opt/rocm/llvm/bin"


def tower_forward64(W, obs):
    """float64 restatement of the tower MlpPolicy (rl_baselines/common/policies.py:35-92 mlp_extractor with
    net_arch [dict(pi=[128, 128], vf=[128, 128])], ReLU; :583-588 heads) -> (mean [N,4], value [N])"""
    f = lambda k: np.asarray(W[k], np.float64)                    # noqa: E731
    x = np.asarray(obs, np.float64)
    hp = np.maximum(np.maximum(x @ f("w0") + f("b0"), 0.0) @ f("w1") + f("b1"), 0.0)
    hv = np.maximum(np.maximum(x @ f("wv0") + f("bv0"), 0.0) @ f("wv1") + f("bv1"), 0.0)
    return hp @ f("w2") + f("b2"), (hv @ f("wv2") + f("bv2"))[:, 0]


def _rewrite(src, dst, data=None, params=None):
    """copy of an archive with `data` and / or the parameter arrays replaced (parameter_list follows the arrays)"""
    with zipfile.ZipFile(src) as z:
        d = json.loads(z.read("data")) if data is None else data
        p = np.load(io.BytesIO(z.read("parameters")), allow_pickle=False)
        arrays = {k: p[k] for k in p.files} if params is None else params
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    with zipfile.ZipFile(dst, "w") as z:
        z.writestr("data", json.dumps(d))
        z.writestr("parameters", buf.getvalue())
        z.writestr("parameter_list", json.dumps(list(arrays)))
    return dst


def _params(path):
    with zipfile.ZipFile(path) as z:
        p = np.load(io.BytesIO(z.read("parameters")), allow_pickle=False)
        return {k: p[k] for k in p.files}


# ---------------------------------------------------------------- loader
def test_repacked_archives_have_no_serialized_fields():
    for path in (TOWERS_ZIP, SHARED_ZIP):
        with zipfile.ZipFile(path) as z:
            assert sorted(z.namelist()) == ["data", "parameter_list", "parameters"]
            assert ":serialized:" not in z.read("data").decode("utf-8")


def test_shared_archive_equals_the_policy_fixture_bit_for_bit():
    from quadsim_amd.sb2 import read_sb2_weights
    layout, W = read_sb2_weights(SHARED_ZIP)
    assert layout == "shared" and "wv0" not in W
    with np.load(os.path.join(GOLDEN, "policy_best_model_v0.npz"), allow_pickle=False) as z:
        assert sorted(z.files) == sorted(W)
        for k in z.files:
            assert W[k].dtype == np.float32 and np.array_equal(W[k], z[k]), k


def test_tower_archive_maps_onto_tower_keys():
    from quadsim_amd.sb2 import read_sb2_weights
    layout, W = read_sb2_weights(TOWERS_ZIP)
    P = _params(TOWERS_ZIP)
    assert layout == "towers"
    want = {"w0": "pi_fc0/w", "b0": "pi_fc0/b", "w1": "pi_fc1/w", "b1": "pi_fc1/b", "w2": "pi/w", "b2": "pi/b",
            "wv0": "vf_fc0/w", "bv0": "vf_fc0/b", "wv1": "vf_fc1/w", "bv1": "vf_fc1/b", "wv2": "vf/w", "bv2": "vf/b"}
    assert sorted(W) == sorted(list(want) + ["logstd"])
    for k, name in want.items():
        assert np.array_equal(W[k], P["model/%s:0" % name]), k
    assert W["w0"].shape == (12, 128) and W["wv0"].shape == (12, 128) and W["w1"].shape == (128, 128)
    assert np.array_equal(W["logstd"], P["model/pi/logstd:0"].reshape(-1))


def test_loader_never_unpickles(monkeypatch):
    import pickle
    from quadsim_amd.sb2 import read_sb2_weights

    def boom(*a, **k):
        raise AssertionError("unpickling attempted")
    monkeypatch.setattr(pickle, "loads", boom)
    monkeypatch.setattr(pickle, "load", boom)
    monkeypatch.setattr(pickle, "Unpickler", boom)
    assert read_sb2_weights(TOWERS_ZIP)[0] == "towers"
    assert read_sb2_weights(SHARED_ZIP)[0] == "shared"


@pytest.mark.parametrize("case", ["tanh_default", "sigmoid", "width64", "obs13", "act3", "deeper_shared", "deeper_towers"])
def test_loader_rejects_what_the_kernels_do_not_run(tmp_path, case):
    from quadsim_amd.sb2 import read_sb2_weights
    with zipfile.ZipFile(TOWERS_ZIP) as z:
        data = json.loads(z.read("data"))
    P = _params(TOWERS_ZIP)
    rs = np.random.RandomState(0)
    if case == "tanh_default":
        data["policy_kwargs"] = {}
        match = "activation 'tanh'"
    elif case == "sigmoid":
        data["policy_kwargs"]["act_fun"] = "<function sigmoid at 0x0>"
        match = "activation 'sigmoid'"
    elif case == "width64":
        P = {k: (v[..., :64] if v.ndim and v.shape[-1] == 128 else v) for k, v in P.items()}
        P = {k: (v[:64] if v.ndim == 2 and v.shape[0] == 128 else v) for k, v in P.items()}
        match = "hidden width"
    elif case == "obs13":
        P["model/pi_fc0/w:0"] = rs.randn(13, 128).astype(np.float32)
        match = "observation size"
    elif case == "act3":
        P["model/pi/w:0"] = P["model/pi/w:0"][:, :3]; P["model/pi/b:0"] = P["model/pi/b:0"][:3]
        match = "action size"
    elif case == "deeper_shared":
        P = _params(SHARED_ZIP)
        P["model/shared_fc1/w:0"] = rs.randn(128, 128).astype(np.float32)
        P["model/shared_fc1/b:0"] = np.zeros(128, np.float32)
        match = "layout unsupported"
    else:
        P["model/pi_fc2/w:0"] = rs.randn(128, 128).astype(np.float32)
        P["model/pi_fc2/b:0"] = np.zeros(128, np.float32)
        match = "layout unsupported"
    path = _rewrite(TOWERS_ZIP, str(tmp_path / "m.zip"), data=data, params=P)
    with pytest.raises(ValueError, match=match):
        read_sb2_weights(path)


def test_reference_archives_when_present():
    """every PPO2 archive the reference ships: the seven ppo2_docking*.zip load as towers, best_model_v0 as the shared trunk
    (arrays equal to the committed re-pack), ppo2_hover.zip (12 -> 64 -> 64, tanh) is refused"""
    if not os.path.isdir(REF):
        pytest.skip("reference tree not on this machine")
    from quadsim_amd.sb2 import read_sb2_weights
    docking = sorted(f for f in os.listdir(REF) if re.fullmatch(r"ppo2_docking.*\.zip", f))
    assert len(docking) == 7
    for f in docking:
        layout, W = read_sb2_weights(os.path.join(REF, f))
        assert layout == "towers" and W["wv0"].shape == (12, 128), f
    layout, W = read_sb2_weights(os.path.join(REF, "trained_model", "best_model_v0.zip"))
    _, W2 = read_sb2_weights(SHARED_ZIP)
    assert layout == "shared" and all(np.array_equal(W[k], W2[k]) for k in W)
    _, W3 = read_sb2_weights(os.path.join(REF, "ppo2_docking_621_h_30M.zip"))
    _, W4 = read_sb2_weights(TOWERS_ZIP)
    assert all(np.array_equal(W3[k], W4[k]) for k in W3)
    with pytest.raises(ValueError, match="tanh"):
        read_sb2_weights(os.path.join(REF, "ppo2_hover.zip"))


# ---------------------------------------------------------------- tower heads on torch (CPU) and the weight images
def test_tower_policy_torch_heads_and_actor_match_float64():
    import torch
    import quadsim_amd as qa
    from quadsim_amd.sb2 import read_sb2_weights
    _, W = read_sb2_weights(TOWERS_ZIP)
    pol = qa.load_sb2_model(TOWERS_ZIP, device="cpu")
    act = qa.MlpPolicy.from_sb2_zip(TOWERS_ZIP, device="cpu")
    assert pol.towers
    g = np.load(os.path.join(GOLDEN, "g13_towers_episode.npz"), allow_pickle=False)
    obs = np.concatenate([g["obs_in"], np.random.RandomState(1).randn(500, 12) * 2]).astype(np.float32)
    mean, value = pol._heads(torch.as_tensor(obs))
    m64, v64 = tower_forward64(W, obs)
    np.testing.assert_allclose(mean.numpy(), m64, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(value.numpy(), v64, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(act.predict(torch.as_tensor(obs)).numpy(), np.clip(m64, -1, 1), atol=1e-5)
    # the fixture's value column is the same float64 network
    np.testing.assert_allclose(tower_forward64(W, g["obs_in"])[1], g["values"], rtol=1e-12, atol=1e-12)
    # the fixture's actions are the deterministic actor's
    np.testing.assert_allclose(np.clip(tower_forward64(W, g["obs_in"])[0], -1, 1), g["actions"], atol=1e-5)
    assert len(g["actions"]) == 323 and g["done"][-1] and not g["done"][:-1].any() and g["flags"][-1] & 2


def test_tower_fast_image_extends_the_shared_layout():
    """pack_fast_actor_critic of a tower policy: the shared-trunk image built from pi_fc0 / pi_fc1 / pi / vf_fc1 / vf, then
    vf_fc0^T as float32 [128][13] and its bias; sizes as the library reports per layout"""
    import quadsim_amd as qa
    from quadsim_amd import _lib
    from quadsim_amd.runner import pack_fast_actor_critic
    pol = qa.load_sb2_model(TOWERS_ZIP, device="cpu")
    blob = pack_fast_actor_critic(pol)
    _, W = qa.read_sb2_weights(TOWERS_ZIP)
    as_shared = dict(W); del as_shared["wv0"], as_shared["bv0"]
    head = pack_fast_actor_critic(qa.ActorCriticPolicy(as_shared, device="cpu"))
    assert head.size == 141888 and blob.size == 141888 + 128 * 13 * 4 + 128 * 4
    assert np.array_equal(blob[:head.size], head)
    tail = blob[head.size:].view(np.float32)
    w = tail[:128 * 13].reshape(128, 13)
    assert np.array_equal(w[:, :12], W["wv0"].T) and not w[:, 12].any() and np.array_equal(tail[128 * 13:], W["bv0"])
    _lib.build_library()
    lib = _lib.load()
    assert lib.qs_runner_rollout_net_fast_blob_bytes(_lib.NET_TOWERS) == blob.size
    assert lib.qs_runner_rollout_net_fast_blob_bytes(_lib.NET_SHARED_TRUNK) == head.size == lib.qs_runner_rollout_fast_blob_bytes()
    assert lib.qs_runner_rollout_net_fast_blob_bytes(7) < 0


# ---------------------------------------------------------------- C ABI
C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "quadsim.h"
int main(void) {
    static float w[128 * 128];
    QsActorCriticNet net;
    memset(&net, 0, sizeof net);
    net.struct_size = sizeof(QsActorCriticNet);
    net.layout = QS_NET_TOWERS;
    net.wt1 = w; net.b1 = w; net.wt2 = w; net.b2 = w; net.wt3 = w; net.b3 = w;
    net.wtv1 = w; net.bv1 = w; net.wtv2 = w; net.bv2 = w; net.wtv3 = w; net.bv3 = w;
    if (0) {
        qs_runner_rollout_net(NULL, 1, &net, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
        qs_runner_rollout_net_fast(NULL, 1, QS_NET_TOWERS, w, net.logstd, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL,
                                   NULL, NULL, NULL);
    }
    printf("%d %d\n", qs_runner_rollout_net_fast_blob_bytes(QS_NET_TOWERS), qs_runner_rollout_net_fast_blob_bytes(QS_NET_SHARED_TRUNK));
    return 0;
}
"""


def test_net_abi_symbols_and_plain_c(tmp_path):
    """the layout-aware Runner entry points are exported and include/quadsim.h's QsActorCriticNet compiles and links from
    plain C99 (no torch in that process)"""
    from quadsim_amd import _lib
    _lib.build_library()
    lib = _lib.load()
    for name in ("qs_runner_rollout_net", "qs_runner_rollout_net_fast", "qs_runner_rollout_net_fast_blob_bytes"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.qs_version() == 131
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "net.c"
    src.write_text(C_PROGRAM)
    exe = str(tmp_path / "net")
    libdir = os.path.join(ROOT, "quadsim_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir,
                           "-lquadsim_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["149056", "141888"]
    import ctypes
    assert ctypes.sizeof(_lib.QsActorCriticNet) == 16 + 12 * 8 + 16


# ---------------------------------------------------------------- ISA of the tower Runner kernels
@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    from quadsim_amd import _lib
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip("ROCm LLVM tools not installed")
    so = _lib.build_library()
    d = tmp_path_factory.mktemp("isa")
    fat, co = str(d / "fat.bin"), str(d / "dev.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so, str(d / "so.copy")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return co


def _kernel_notes(co):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count", notes):
        m = re.search(r"\.name:\s+(\S+)", block)
        if m:
            field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", block).group(1))   # noqa: E731
            out[m.group(1)] = {k: field(k) for k in ("group_segment_fixed_size", "private_segment_fixed_size",
                                                     "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return out


def test_tower_runner_kernels_isa(code_object):
    """every tower instantiation (NET = 1) of k_runner_rollout / k_runner_split: no scratch, LDS within the CU's 160 KiB,
    the split kernel at <= 256 VGPRs (two waves per SIMD, as the shared-trunk one), f32 MFMA in the exact kernels and bf16
    MFMA in the split-bf16 ones"""
    notes = _kernel_notes(code_object)
    tow = {k: v for k, v in notes.items() if re.search(r"k_runner_(rollout|split)ILi\dELi\dELb[01]ELb[01]ELi1E", k)}
    assert len(tow) == 40, sorted(tow)
    for name, n in tow.items():
        # (SGPR spills land in VGPR lanes, as in the shared-trunk kernels: no memory)
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, name
        assert n["group_segment_fixed_size"] <= 163840, (name, n)
        if "k_runner_split" in name:
            assert n["vgpr_count"] <= 256, (name, n)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(tow),
                          code_object], capture_output=True, text=True, check=True).stdout
    bodies = dict(zip(*[iter(re.split(r"^(?:[0-9a-f]+ )?<(\S+)>:\n", dis, flags=re.M)[1:])] * 2))
    assert sorted(bodies) == sorted(tow)
    for name, body in bodies.items():
        assert "scratch_" not in body and "buffer_store" not in body, name
        fast = bool(re.search(r"ELb1ELi1E", name))
        assert "v_mfma_f32_16x16x4_f32" in body, name           # layer 1 runs on the f32 MFMA in both flavours
        assert ("v_mfma_f32_16x16x32_bf16" in body) == fast, name
