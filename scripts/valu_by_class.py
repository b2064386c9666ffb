#!/usr/bin/env python3
"""SQ_INSTS_VALU (or another counter) of a rocprofv3 --pmc pass over wavefront
renders, summed per kernel class: extend0 (bounce 0: wf_extend_primary /
wf_primary_lists), extend0+shade0 (wf_primary_shade: compare it with extend0 plus
bounce 0's share of shade in earlier rows), extend, shade, cull_terminal, other.
usage: valu_by_class.py DIR [COUNTER]"""
import csv
import glob
import sys
from collections import defaultdict


def kernel_class(name):
    if "wf_primary_shade" in name:         # bounce 0's extend and shade in one kernel
        return "extend0+shade0"
    if "wf_extend_primary" in name or "wf_primary_lists" in name:
        return "extend0"
    if "wf_extend" in name or "wf_sphere_clip" in name:   # (the secondary extend that clips walks to spheres)
        return "extend"
    if "wf_shade" in name:
        return "shade"
    if "wf_cull_terminal" in name:
        return "cull_terminal"
    return "other"


def main(d, counter="SQ_INSTS_VALU"):
    tot, disp = defaultdict(float), defaultdict(set)
    for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if r["Counter_Name"] != counter:
                    continue
                c = kernel_class(r["Kernel_Name"])
                tot[c] += float(r["Counter_Value"])
                disp[c].add(r["Dispatch_Id"])
    for c in sorted(tot):
        print(f"  {counter} {c:14s} {tot[c]:.4e} over {len(disp[c])} dispatches")
    print(f"  {counter} {'total':14s} {sum(tot.values()):.4e}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
