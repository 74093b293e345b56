#!/usr/bin/env python3
"""Grouped calls (k_leaf_group_lazy): how a wave streams a run of plain ports — LEAF_GROUP_PIPE (k_leaf.hip.h) 0 and 1 at
(G, U) = (2, 8), and stage 1 at U = 4 and U = 16.  (profiles/leaf_pipe_sweep.jsonl also holds stage 2, a rolling window of U ports inside a
run: it lost to stage 1 and its code was deleted, so it is no variant here any more.)

  build   one library per (G, U, PIPE) beside the product's, as compile-time values (the Makefile's OBJDIR / OUT / EXTRA); no GPU needed
  sweep   the interleaved protocol of leaf_group_sweep.py: ONE process, in each of --rounds rounds every variant gets a fresh context with
          the switch on and one with it off on the headline shape, timed alternately

Prints JSON lines; --out also writes them to a file."""
import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import leaf_group_sweep as lgs  # noqa: E402

VARIANTS = [(2, 8, 0), (2, 8, 1), (2, 4, 1), (2, 16, 1)]


def lib_path(g, u, p):
    return os.path.join(lgs.CSRC, "libfwgpu_g%du%dp%d.so" % (g, u, p))


def build(jobs):
    for g, u, p in VARIANTS:
        subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", lgs.CSRC, "OBJDIR=_obj_g%du%dp%d" % (g, u, p), "OUT=" + os.path.basename(lib_path(g, u, p)),
                               "EXTRA=-DLEAF_GROUP_G=%d -DLEAF_GROUP_U=%d -DLEAF_GROUP_PIPE=%d" % (g, u, p)])
        print("built", lib_path(g, u, p))


def sweep(rounds, steps, fh):
    V, B, K, F, _ = __import__("bench").DEFAULTS["cfg2"]
    b = lgs.Bench(B, F, V)
    libs = {v: lgs.load(lib_path(*v)) for v in VARIANTS}
    rows = {v: [] for v in VARIANTS}
    for r in range(rounds):
        for v in VARIANTS:
            on, off, grouped, same = b.pair(libs[v], K, steps)
            rows[v].append((on, off))
            lgs.emit({"round": r, "G": v[0], "U": v[1], "pipe": v[2], "ms_on": round(on, 4), "ms_off": round(off, 4), "grouped_batches": grouped,
                      "same_bits": same}, fh)
    for v in VARIANTS:
        ons, offs = [x[0] for x in rows[v]], [x[1] for x in rows[v]]
        lgs.emit({"summary": "G=%d U=%d pipe=%d" % v, "median_on": round(statistics.median(ons), 4), "min_on": round(min(ons), 4),
                  "max_on": round(max(ons), 4), "spread_on": round(max(ons) - min(ons), 4), "median_off": round(statistics.median(offs), 4),
                  "min_off": round(min(offs), 4), "max_off": round(max(offs), 4)}, fh)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["build", "sweep"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "build":
        return build(a.jobs)
    sweep(a.rounds, a.steps, open(a.out, "w") if a.out else None)


if __name__ == "__main__":
    main()
