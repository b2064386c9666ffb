"""The queue-order shade's record loads (no GPU needed), read from the built
library's code objects as test_kernel_resources.py does.

All six queue-order wf_shade_slots (256 / 512 / 1024 threads x material table in
LDS or not) load a hit's triangle record and vertex normals as one group behind
the queue's words (wavefront.hip, above the include of wf_shade_item.hpp).  Two
things are held here:

* registers: each of the six at <= 80 VGPRs + AGPRs without scratch -- the
  512-thread ones run two waves per SIMD beside the LDS extend, and the group
  was made to fit that budget in all of them;
* structure, not instruction counts: in the kernel's main loop (the loop that
  holds the non-temporal loads of the queue's words), in program order, every
  global load before the records belongs to the queue (the three non-temporal
  16-B words, and 4-B hit ids), then come the six record loads with neither a
  wait nor a branch between them, and no global load follows them before the
  loop's back edge (the last on the three kernels with the material table in
  LDS; in the other three the table's fields are global loads).  Before the change the loop held three dependent groups
  (the geometry index, tri_hit_params' records, scatter's normals), each behind
  a branch that the group before decided.
"""
import importlib.util
import os
import re

import pytest

from test_kernel_resources import LLVM, ROOT, _code_objects, _disasm, _kernels

QUEUE_ORDER = re.compile(r"wf_shade_slotsILi(256|512|1024)ELb[01]ELb0EE")


@pytest.fixture(scope="module")
def shades(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("ROCm llvm tools not available")
    spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "montecarlopathtracer_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = b.build()                                 # no-op when libmcpt.so is up to date
    res = {}
    for co in _code_objects(lib, tmp_path_factory.mktemp("co")):
        res.update(_kernels(co))
    text = _disasm(lib, tmp_path_factory.mktemp("dis"))
    names = sorted(n for n in res if QUEUE_ORDER.search(n))
    assert len(names) == 6, names
    return {n: (res[n], text[n]) for n in names}


def test_six_queue_order_shades_fit_80_registers_without_scratch(shades):
    for name, (r, _) in shades.items():
        assert r["vgpr"] + r["agpr"] <= 80 and r["scratch"] == 0, (name, r)


def _parse(lines):
    """-> [(address, mnemonic, operands, branch target or None)] of a kernel's instruction lines"""
    out = []
    for ln in lines:
        if ln == "...":                             # (objdump's mark for a run of zero padding)
            continue
        m = re.match(r"^(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", ln)
        assert m, ln
        out.append([int(m.group(3), 16), m.group(1), m.group(2), m.group(4)])
    start = out[0][0]
    for ins in out:
        t = re.search(r"<[^>]*\+0x([0-9a-f]+)>", ins[3]) if ins[1].startswith(("s_cbranch", "s_branch")) else None
        ins[3] = start + int(t.group(1), 16) if t else None
    return out


def main_loop(lines):
    """the instructions of the loop that holds the queue's non-temporal loads, header to last back edge"""
    ins = _parse(lines)
    nt = [a for a, op, args, _ in ins if op.startswith("global_load") and re.search(r"\bnt\b", args)]
    assert nt, "no non-temporal load: the queue's words"
    back = [(t, a) for a, op, _, t in ins if t is not None and t <= a and t <= nt[0] <= a]
    assert back, "no loop around the queue's loads"
    lo, hi = min(t for t, _ in back), max(a for _, a in back)
    assert all(lo <= a <= hi for a in nt)
    return [i for i in ins if lo <= i[0] <= hi]


def test_record_loads_are_one_group_behind_the_queue_words(shades):
    for name, (_, lines) in shades.items():
        loop = main_loop(lines)
        at = [k for k, i in enumerate(loop) if i[1].startswith("global_load")]
        geo_lds = "ELb1ELb0EE" in name                  # template <BLOCK, GEO_LDS, SORTB = false>
        is_queue = lambda i: bool(re.search(r"\bnt\b", i[2])) or i[1] == "global_load_dword"  # noqa: E731
        first_rec = next(k for k in at if not is_queue(loop[k]))
        queue = [k for k in at if k < first_rec]
        # the record group: the run of global loads from the first record load on that no wait and
        # no branch interrupts
        rec = []
        for k in range(first_rec, len(loop)):
            if loop[k][1].startswith(("s_waitcnt", "s_cbranch", "s_branch")):
                break
            if loop[k][1].startswith("global_load"):
                rec.append(k)
        later = [k for k in at if k > rec[-1]]
        print(name, len(loop), "instructions in the loop; queue loads", len(queue), "record loads", len(rec),
              "later loads", len(later))
        # group 1: the queue's words -- the three non-temporal 16-B streams and the hit id
        assert sum(1 for k in queue if re.search(r"\bnt\b", loop[k][2])) == 3, name
        assert any(loop[k][1] == "global_load_dword" for k in queue), name
        # group 2: three triangle records and three normals, nothing of the queue among them,
        # issued back to back
        assert len(rec) == 6 and not any(is_queue(loop[k]) for k in rec), (name, [loop[k][1:3] for k in rec])
        # no global load follows the second group before the back edge.  Where the material table
        # is in global memory (GEO_LDS false: it did not fit beside the extend) its fields are
        # global loads behind a geometry index by definition, so that half is asserted on the
        # LDS twins: the same source but for the table's place, where those reads are LDS reads
        # and no global load is left
        if geo_lds:
            assert not later, (name, [loop[k][1:3] for k in later])
        # the loop stores the next queue's words, so it is the shading loop, not a setup loop
        assert any(i[1].startswith("global_store") for i in loop), name
