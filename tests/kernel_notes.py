"""The gfx950 code object of the built library and the kernel metadata in its notes (llvm-readelf --notes), for the CPU tests
that check the instantiations and resources of the kernels.  A helper module, not a conftest: imported where it is needed."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/llvm/bin"


FIELDS = ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "max_flat_workgroup_size")


def code_object(directory, so=None):
    """unbundle the gfx950 code object of the built library (or of the library `so`) into `directory` -> its path (skips
    without the ROCm LLVM tools)"""
    from quadsim_amd import _lib
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip("ROCm LLVM tools not installed")
    so = so or _lib.build_library()
    d = str(directory)
    fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so, os.path.join(d, "so.copy")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return co


def kernel_notes(co, fields=FIELDS):
    """{mangled kernel name: resource fields} of every kernel in the code object"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n(?=\s+- \.agpr_count)", notes):
        m = re.search(r"\.name:\s+(\S+)", block)
        if m:
            field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", block).group(1))   # noqa: E731
            out[m.group(1)] = {k: field(k) for k in fields}
    return out


def instantiations(notes, kernels):
    """{(kernel, template arguments...)} of the kernels named in `kernels` (integer and bool template arguments, in declaration
    order) among the symbols of the code object's notes"""
    # longest name first: k_env must not match inside k_env_split, k_policy_rollout not inside k_policy_rollout_fast
    sym_re = re.compile(r"_GLOBAL__N_1\d+(%s)I((?:L[ib]\d+E)+)E" % "|".join(sorted(kernels, key=len, reverse=True)))
    got = set()
    for sym in notes:
        m = sym_re.search(sym)
        if m:
            got.add((m.group(1),) + tuple(int(a) for a in re.findall(r"L[ib](\d+)E", m.group(2))))
    return got


def anon_instantiations(notes, kernels):
    """{(kernel, bool template arguments...)} of the kernels named in `kernels` that live in the anonymous namespace and are
    plain kernels -- (kernel,) -- or templated on bools alone -- k_state_io<true> -> ("k_state_io", 1).  instantiations() above
    sees only templated kernels, instantiations_with_types() only a named namespace."""
    # the length prefix of the Itanium mangling keeps k_reset from matching inside k_reset_all; a plain kernel's name is followed
    # by the E that closes the nested name, a templated one's by I <arguments> E E
    sym_re = re.compile(r"^_ZN12_GLOBAL__N_1(?:%s)(?:I(?P<args>(?:Lb[01]E)+)E)?E" % "|".join(
        "%d(?P<k%d>%s)" % (len(k), j, re.escape(k)) for j, k in enumerate(kernels)))
    got = set()
    for sym in notes:
        m = sym_re.match(sym)
        if m:
            name = next(v for k, v in m.groupdict().items() if v and k != "args")
            got.add((name,) + tuple(int(a) for a in re.findall(r"Lb([01])E", m.group("args") or "")))
    return got


def base_names(notes):
    """{kernel base name} of every kernel symbol: the last component of the (nested) name, without template arguments --
    _ZN12_GLOBAL__N_15k_envILi0ELb1EEEvPf and _ZN2qs5k_envE... both give k_env.  A symbol that is not an Itanium-mangled function
    name is returned as it is, so that a census cannot lose it."""
    got = set()
    for sym in notes:
        m = re.match(r"^_Z(N?)", sym)
        if not m:
            got.add(sym)
            continue
        pos, name = m.end(), None
        while True:
            d = re.match(r"\d+", sym[pos:])
            if not d:
                break
            ln = int(d.group(0))
            name = sym[pos + d.end():pos + d.end() + ln]
            pos += d.end() + ln
            if not m.group(1):
                break
        got.add(name if name else sym)
    return got


_ITANIUM_TYPES = {"f": "float", "d": "double", "h": "uint8_t", "a": "int8_t", "i": "int", "j": "unsigned", "l": "long", "m": "unsigned long"}


def instantiations_with_types(notes, kernels, namespace="qs"):
    """{(kernel, template arguments...)} of the kernels named in `kernels`, which live in the named namespace `namespace`:
    plain kernels give (kernel,), integer / bool template arguments give ints and builtin type arguments their C names
    (k_swap_flatten<13, float> -> ("k_swap_flatten", 13, "float")).  instantiations() above sees none of the first and
    third kind."""
    arg = r"L[ib]\d+E|[%s]" % "".join(_ITANIUM_TYPES)
    # the length prefix of the Itanium mangling keeps k_swap_flatten from matching inside k_swap_flatten_v4
    sym_re = re.compile(r"^_ZN%d%s(?:%s)(?:I((?:%s)+)E)?E" % (len(namespace), namespace, "|".join(
        "%d(?P<k%d>%s)" % (len(k), j, re.escape(k)) for j, k in enumerate(kernels)), arg))
    got = set()
    for sym in notes:
        m = sym_re.match(sym)
        if m:
            name = next(v for k, v in m.groupdict().items() if v)
            args = re.findall(arg, m.group(len(kernels) + 1) or "")
            got.add((name,) + tuple(int(a[2:-1]) if a[0] == "L" else _ITANIUM_TYPES[a] for a in args))
    return got
