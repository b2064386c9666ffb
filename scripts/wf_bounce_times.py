#!/usr/bin/env python3
"""Per-bounce extend / shade times from a rocprofv3 kernel trace of wavefront
renders on ONE stream (kernels serialized): dispatches are grouped per batch
(wf_generate, or a generate-free bounce-0 extend -- wf_extend_primary,
wf_primary_lists, which resolves the tiles' candidate lists, or wf_primary_shade,
which also shades bounce 0 and is reported as bounce 0's extend with a shade of
0, so that the two together compare with earlier rows -- starts one) and
indexed by bounce; wf_cull_terminal (the terminal cull in front of the last
extend; wf_sphere_clip, the secondary extend that also clips walks to
spheres, counts as its bounce's extend) and wf_tile_candidates (the primary lists' candidate pass, once per
render) are summed on their own.  usage: wf_bounce_times.py DIR"""
import csv
import glob
import sys
from collections import defaultdict


def main(d):
    rows = []
    for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    ext, sh = defaultdict(list), defaultdict(list)
    cull, cand = [], []
    b_ext = b_sh = -1
    batches = 0
    for t0, t1, name in rows:
        if ("wf_generate" in name or "wf_extend_primary" in name or "wf_primary_lists" in name
                or "wf_primary_shade" in name):
            b_ext = b_sh = -1
            batches += 1
        if "wf_primary_shade" in name:
            # bounce 0's extend + shade in one kernel: reported as bounce 0's extend, its shade 0,
            # so that the row's sum compares with earlier rows' extend + shade of bounce 0
            b_ext += 1
            b_sh += 1
            ext[b_ext].append((t1 - t0) / 1e6)
            sh[b_sh].append(0.0)
        elif "wf_cull_terminal" in name:
            cull.append((t1 - t0) / 1e6)
        elif "wf_tile_candidates" in name:
            cand.append((t1 - t0) / 1e6)
        elif "wf_extend" in name or "wf_primary_lists" in name or "wf_sphere_clip" in name:
            b_ext += 1
            ext[b_ext].append((t1 - t0) / 1e6)
        elif "wf_shade" in name:
            b_sh += 1
            sh[b_sh].append((t1 - t0) / 1e6)
    print(f"batches {batches}")
    for b in sorted(ext):
        e, s = ext[b], sh.get(b, [0])
        print(f"bounce {b}: extend {sum(e) / batches:8.2f} ms/frame-batch-avg x{len(e)}  "
              f"(per dispatch {sum(e) / len(e):.3f})  shade {sum(s) / max(len(s), 1):.3f}")
    print("extend total per batch", sum(sum(v) for v in ext.values()) / batches)
    print("shade total per batch", sum(sum(v) for v in sh.values()) / batches)
    if cull:
        print(f"terminal cull per batch {sum(cull) / batches:.3f} x{len(cull)}")
    if cand:
        print(f"candidate pass per render {sum(cand) / len(cand):.4f} x{len(cand)}")


if __name__ == "__main__":
    main(sys.argv[1])
