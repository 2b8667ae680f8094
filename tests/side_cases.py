"""What the tests of the ten side libraries (quadsim_amd._lib.SIDE) have in common.  For the CPU tests, tests/test_*_cpu.py: each
generic check of a library's ABI as a function of its table key and of the data the caller states -- the header's names against the
exports, the entry's files against every other entry's, the kernel-name prefixes against the bytes of all eleven libraries, the C99
caller, the census of the code object against the rows of a tests/*_matrix.py.  For the trainers' GPU tests: the guard buffer.
A helper module, not a conftest: imported where it is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np

import kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what the name of a file says when it belongs to that library alone: the fragments and the source, the public header
NAMES = {"dyn": ("dynplan", "quadsim_dyn.h"), "dynmppi": ("dynmppi", "dyn_mppi"), "dynfit": ("dynfit", "dyn_fit"), "bc": ("bc",),
         "ppo": ("ppo",), "gail": ("gail",), "trpo": ("trpo",), "ddpg": ("ddpg",), "td3": ("td3",), "sac": ("sac",)}
# the one pair that shares files of such a name on purpose: MPPI over the learned net is built from the shooting planner's fragments
SHARED = {("dyn", "dynmppi"): ("dynplan_host.hpp", "dynplan_image.hpp", "dynplan_kernels.hpp")}


def _side(key):
    from quadsim_amd import _lib
    return _lib, _lib.SIDE[key]


def declared(key):
    """the sorted `prefix`* names that the library's header calls, comments stripped"""
    _, e = _side(key)
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", e["header"])).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % e["prefix"], text)))


def check_exports(key, lib, expected_names):
    """the header's names are the table's exports, are `expected_names`, are what the built library defines; `lib`, the loaded
    library, has them all and is version 1"""
    _, e = _side(key)
    names = declared(key)
    assert names == sorted(e["exports"]) == sorted(expected_names), key
    out = subprocess.run(["nm", "-D", "--defined-only", e["path"]], capture_output=True, text=True, check=True).stdout
    assert sorted(w for w in out.split() if w.startswith(e["prefix"])) == names, key
    assert not [n for n in names if not hasattr(lib, n)]
    assert getattr(lib, e["prefix"] + "version")() == 1


def check_entry(key, fragments, source):
    """the entry's files are `fragments` (base names, the public header among them) and `source`, and exist; its signatures are
    in SIDE_POINTERS; no file of the main library or of another entry carries this library's name; QUADSIM_<KEY>_LIB moves it"""
    _lib, e = _side(key)
    assert os.path.basename(e["path"]) == e["file"] == "libquadsim_%s.so" % key
    assert sorted(os.path.basename(h) for h in e["headers"]) == sorted(fragments) and e["header"] in fragments, key
    assert [os.path.basename(s) for s in e["sources"]] == [source] and all(os.path.exists(h) for h in e["headers"] + e["sources"]), key
    assert all(name in _lib.SIDE_POINTERS for name in e["signatures"])
    others = {k: o for k, o in _lib.SIDE.items() if k != key}
    assert len(others) == 9
    theirs = [(k, os.path.basename(h)) for k, o in others.items() for h in o["headers"] + o["sources"]]
    theirs = [f for k, f in theirs if f not in SHARED.get((key, k), ())] + [os.path.basename(h) for h in _lib.HEADERS + _lib.SOURCES]
    assert not [f for f in theirs if any(word in f for word in NAMES[key])], key
    assert e["env"] == "QUADSIM_%s_LIB" % key.upper()
    env = dict(os.environ, **{e["env"]: "/somewhere/else.so"})
    got = subprocess.run([sys.executable, "-c", "from quadsim_amd import _lib; print(_lib.SIDE[%r]['path'])" % key], cwd=ROOT, env=env,
                         capture_output=True, text=True, check=True).stdout.strip()
    assert got == "/somewhere/else.so"


def check_no_foreign_kernels(key):
    """the library's kernel-name prefix is in its own bytes and in those of no other library, the main one included, and no other
    side library's prefix is in this one"""
    _lib, e = _side(key)
    _lib.build_library()
    blob = open(e["path"], "rb").read()
    assert e["kernels"] in blob, key
    for k, o in _lib.SIDE.items():
        if k != key:
            assert e["kernels"] not in open(o["path"], "rb").read(), (key, k)
            assert o["kernels"] not in blob, (k, key)
    assert e["kernels"] not in open(_lib.LIB_PATH, "rb").read(), key


def run_c_caller(key, text, tmp_path):
    """`text`, a plain C program, compiled -std=c99 -Wall -Werror against the library's header and linked against that library
    alone, refuses every call it makes and counts as many entry points as the header declares"""
    _, e = _side(key)
    assert shutil.which("gcc") is not None
    src = tmp_path / (key + "_caller.c")
    src.write_text(text)
    exe = str(tmp_path / (key + "_caller"))
    libdir = os.path.join(ROOT, "quadsim_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir,
                           "-l" + e["file"][len("lib"):-len(".so")], "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ALL-REFUSED", str(len(declared(key)))]


def code_object_notes(key, tmp_path_factory):
    """{mangled kernel name: resource fields} of the library's gfx950 code object"""
    _lib, e = _side(key)
    _lib.build_library()
    co = kernel_notes.code_object(tmp_path_factory.mktemp("isa_" + key), so=e["path"])
    return kernel_notes.kernel_notes(co, kernel_notes.FIELDS + ("sgpr_spill_count",))


def check_census(notes, matrix, instantiations, what, sgpr_spills=()):
    """the rows of `matrix` are exactly the kernels of the code object, `instantiations(notes)` their keys; no kernel uses scratch
    or spills, each fits the compute unit's LDS and is compiled for its row's block -> {key: resource fields}.  The kernels named
    in `sgpr_spills` may spill scalar registers (into lanes of a vector register: that costs no scratch), as the fit kernels that
    keep Adam's state in registers do"""
    keys = [r["key"] for r in matrix.ROWS]
    assert len(keys) == len(set(keys)) == len(notes), "duplicate rows, or not one row per kernel"
    got = instantiations(notes)
    assert got == set(keys), "rows without a kernel: %s; kernels without a row: %s" % (
        sorted(set(keys) - got, key=str), sorted(got - set(keys), key=str))
    assert kernel_notes.base_names(notes) == set(matrix.KERNELS)
    by_key = {}
    for sym, fl in notes.items():
        (k,) = instantiations({sym: fl})
        by_key[k] = fl
    for r in matrix.ROWS:
        fl = by_key[r["key"]]
        assert fl["private_segment_fixed_size"] == 0 and fl["vgpr_spill_count"] == 0, (r["id"], fl)
        assert fl["sgpr_spill_count"] == 0 or r["kernel"] in sgpr_spills, (r["id"], fl)
        assert fl["group_segment_fixed_size"] <= 160 * 1024 and fl["max_flat_workgroup_size"] == r["block"], (r["id"], fl)
        print("%s notes %s %s" % (what, r["id"], fl))
    return by_key


def check_rows_name_gpu_tests(matrix):
    """every row's `test` is an id that pytest collects"""
    files = sorted({r["test"].split("::")[0] for r in matrix.ROWS})
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    ids = set(out.stdout.split())
    missing = [r["test"] for r in matrix.ROWS if r["test"] not in ids]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------- the trainers' GPU tests
GUARD = 256


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Guarded:
    """a device array between sentinel bytes: a copy of `a`, or `nbytes` zero bytes"""

    def __init__(self, torch, a=None, nbytes=None):
        if a is None:
            a = np.zeros(nbytes, np.uint8)
        a = np.ascontiguousarray(a)
        self.raw = torch.full((a.nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.n, self.shape, self.dtype = a.nbytes, a.shape, a.dtype
        self.raw[GUARD:GUARD + self.n].copy_(torch.as_tensor(a.view(np.uint8).reshape(-1)))
        self.ptr = self.raw.data_ptr() + GUARD

    def get(self, name):
        h = self.raw.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + self.n:] == 0xA5).all(), "sentinel bytes around %s were overwritten" % name
        return h[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape).copy()


def six(gs):
    """void *[6] of six guarded arrays"""
    return (C.c_void_p * 6)(*[g.ptr for g in gs])
