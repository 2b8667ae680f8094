"""Compare the gfx950 code objects of two builds of libquadsim_hip.so kernel by kernel: the set of kernel names, the resource
fields of the notes, and the disassembly (addresses, encodings and branch-target annotations stripped).

    python tools/isa_diff.py PARENT.so BRANCH.so > profiles/<topic>/isa_diff.txt

One line per kernel: `same`, or the fields that moved and the instruction counts.  Exit status 1 if the name sets differ."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests.kernel_notes import LLVM, code_object, kernel_notes  # noqa: E402

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")


def disassembly(co):
    """{symbol: [instruction text]} of the code object"""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-leading-addr", "--no-show-raw-insn", co],
                          capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":      # "...": zero padding behind a kernel, no instruction
            cur.append(re.sub(r"\s*(//|<).*$", "", line).strip())
    return out


def load(so):
    with tempfile.TemporaryDirectory() as d:
        co = code_object(d, so)
        return kernel_notes(co, FIELDS), disassembly(co)


def main(parent, branch):
    (na, da), (nb, db) = load(parent), load(branch)
    print("kernels: parent %d, branch %d, only in parent %s, only in branch %s"
          % (len(na), len(nb), sorted(set(na) - set(nb)), sorted(set(nb) - set(na))))
    same = 0
    for k in sorted(set(na) & set(nb)):
        moved = ["%s %d -> %d" % (f, na[k][f], nb[k][f]) for f in FIELDS if na[k][f] != nb[k][f]]
        if da[k] != db[k]:
            moved.append("instructions %d -> %d" % (len(da[k]), len(db[k])) if len(da[k]) != len(db[k])
                         else "instructions %d, %d lines differ" % (len(da[k]), sum(x != y for x, y in zip(da[k], db[k]))))
        same += not moved
        print("%s: %s" % (k, "; ".join(moved) or "same"))
    print("identical in fields and disassembly: %d of %d" % (same, len(set(na) & set(nb))))
    return 0 if set(na) == set(nb) else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
