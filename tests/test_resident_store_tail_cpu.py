"""CPU: the chaser loop of every k_env_resident instantiation, read from the built code object.  gfx950 counts loads, returning
atomics and stores in one in-order vmcnt, so any `s_waitcnt vmcnt` behind a step's output stores is a wait for their acknowledge
with nothing to issue.  The loop must therefore

  * hold no wait that names vmcnt between the step's last output store and the branch back to the loop header,
  * not open with one either (the state loads are waited for in front of the loop): none before the step's first memory request,
  * write its outputs with global_store_*: a flat_store_* counts in lgkmcnt too, and every LDS wait would wait for it.

The chaser loop is found from its stores: done and flags are the kernel's only non-temporal BYTE stores, and the loop's back-edge
is the innermost backward branch of the straight-line code behind the last of them.  That it is the step loop is checked by what
it must contain: both workgroup barriers of a step and the system-scope request of the next descriptor."""
import os
import re
import subprocess

import pytest

import kernel_notes
from kernel_notes import LLVM


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """{symbol: [(address, instruction text, branch target address or None)]} of the k_env_resident instantiations"""
    co = kernel_notes.code_object(tmp_path_factory.mktemp("isa_store_tail"))
    syms = sorted(s for s in kernel_notes.kernel_notes(co) if re.search(r"_GLOBAL__N_1\d+k_env_residentI", s))
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(syms), co],
                         capture_output=True, text=True, check=True).stdout
    bodies = dict(zip(*[iter(re.split(r"^(?:[0-9a-f]+ )?<(\S+)>:\n", dis, flags=re.M)[1:])] * 2))
    assert sorted(bodies) == syms
    out = {}
    for sym, body in bodies.items():
        ins = []
        for line in body.splitlines():
            m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line)
            if not m:
                continue
            t = re.search(r"<%s\+0x([0-9a-fA-F]+)>" % re.escape(sym), m.group(3))
            ins.append([int(m.group(2), 16), m.group(1), int(t.group(1), 16) if t and m.group(1).startswith(("s_branch", "s_cbranch")) else None])
        base = ins[0][0]
        out[sym] = [(a, text, None if t is None else base + t) for a, text, t in ins]
    return out


def _chaser_loop(sym, ins):
    """(index of the loop header, index of the last non-temporal byte store, index of the branch back to the header)"""
    stores = [i for i, (_, text, _) in enumerate(ins) if re.match(r"(global|flat)_store_byte\b.*\bnt\b", text)]
    assert stores, "%s: no non-temporal byte store (a QS_PLAIN_STORES build?)" % sym
    last = stores[-1]
    # the straight-line code behind the store ends at the first unconditional branch; of its branches to an address in front of
    # the store the innermost is the loop's (the loop exit may be laid out in front of the header, and blocks of the loop behind
    # its back-edge)
    end = next(i for i in range(last + 1, len(ins)) if ins[i][1].startswith(("s_branch", "s_endpgm")))
    around = [(t, i) for i, (_, _, t) in enumerate(ins[:end + 1]) if t is not None and i > last and t <= ins[last][0]]
    assert around, "%s: no backward branch around the output stores" % sym
    target, back = max(around)
    head = next(i for i, (a, _, _) in enumerate(ins) if a == target)
    texts = [text for _, text, _ in ins[head:back + 1]]
    assert sum(t.startswith("s_barrier") for t in texts) == 2, (sym, "the loop found is not the step loop")
    assert any(re.match(r"global_load_dwordx2\b.*\bsc0 sc1", t) for t in texts), (sym, "no descriptor request in the loop found")
    assert all(head <= i <= back for i in stores), (sym, "byte stores outside the loop found")
    return head, last, back


def test_all_twenty_instantiations_are_read(listings):
    assert len(listings) == 20, sorted(listings)


def test_no_counter_wait_behind_the_output_stores(listings):
    for sym, ins in listings.items():
        _, last, back = _chaser_loop(sym, ins)
        waits = [text for _, text, _ in ins[last + 1:back + 1] if text.startswith("s_waitcnt") and "vmcnt" in text]
        assert not waits, (sym, waits)


def test_loop_header_carries_no_counter_wait(listings):
    for sym, ins in listings.items():
        head, _, back = _chaser_loop(sym, ins)
        first_mem = next(i for i in range(head, back) if re.match(r"(global|flat|buffer|scratch)_", ins[i][1]))
        waits = [text for _, text, _ in ins[head:first_mem] if text.startswith("s_waitcnt") and "vmcnt" in text]
        assert not waits, (sym, waits)
        # ... and the wait for the state loads stands in front of the loop
        before = [text for _, text, _ in ins[:head] if text.startswith("s_waitcnt")]
        assert any(re.search(r"vmcnt\(0\)", t) for t in before), sym


def test_output_stores_are_global(listings):
    for sym, ins in listings.items():
        head, _, back = _chaser_loop(sym, ins)
        stores = [text for _, text, _ in ins[head:back + 1] if re.match(r"(global|flat|buffer|scratch)_store", text)]
        assert len([t for t in stores if re.search(r"\bnt\b", t)]) >= 5, (sym, stores)   # obs (3 x 16 B), reward, done [, flags]
        assert all(t.startswith("global_store_") for t in stores), (sym, [t for t in stores if not t.startswith("global_store_")])
