"""What the CPU tests of the four planner entry points share (test_shooting_cpu.py, test_mppi_cpu.py, test_shooting_split_cpu.py,
test_mppi_split_cpu.py): the header's declarations, the kernels of the built library's code object, a stub library that records
calls, and the recipe "compile a C99 caller, link it against the library, run it".  A helper module, not a conftest: a test
module imports the two fixtures by name."""
import os
import re
import shutil
import subprocess

import pytest

import kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_COMBOS = {(i, p) for i in (0, 1) for p in (0, 1)}       # INTEG x PARAMS


def declarations(header):
    """the header without comments, white space normalised"""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    return re.sub(r" ([,)])", r"\1", text)


def library_and_header():
    """-> (the built library, loaded; the text of include/quadsim.h)"""
    from quadsim_amd import _lib
    _lib.build_library()
    return _lib.load(), open(os.path.join(ROOT, "include", "quadsim.h")).read()


def run_c_caller(tmp_path, program, name):
    """`program` as NAME.c, compiled as C99 with -Wall -Werror against include/quadsim.h, linked against the built library and
    run without a device -> the words it printed"""
    assert shutil.which("gcc") is not None
    src = tmp_path / (name + ".c")
    src.write_text(program)
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "quadsim_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir,
                           "-lquadsim_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.split()


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    """the gfx950 code object of the built library, unbundled once per test module"""
    return kernel_notes.code_object(tmp_path_factory.mktemp("isa_plan"))


@pytest.fixture(scope="module")
def notes(code_object):
    return kernel_notes.kernel_notes(code_object)


def combos(notes, pattern):
    """{(INTEG, PARAMS): symbol} of the kernels whose mangled name matches `pattern` (two groups)"""
    return {(int(m.group(1)), int(m.group(2))): sym for sym in notes for m in [re.search(pattern, sym)] if m}


class StubLib:
    """records the name and the scalar arguments (of the types `scalars`) of every entry point called on it and reports success"""

    def __init__(self, scalars=(int,)):
        self.calls, self.scalars = [], scalars

    def __getattr__(self, name):
        def fn(handle, *args):
            self.calls.append((name, tuple(a for a in args if isinstance(a, self.scalars))))
            return 0
        return fn


def stub_env(torch, lib, num_envs=3):
    """an env of `num_envs` on the CPU whose _call goes straight to `lib` (VecDockingEnv._call itself is covered by
    test_call_path_cpu.py)"""
    import types
    return types.SimpleNamespace(num_envs=num_envs, device=torch.device("cpu"),
                                 _call=lambda name, *args: getattr(lib, name)(None, *args))
