#!/usr/bin/env python3
"""Grouped calls (k_leaf_group_lazy): which geometry ships, and from which size on.

  build   compile one library per (G, U) — waves per (block, piece), ports in flight per wave — beside the product's, as compile-time
          values (the Makefile's OBJDIR / OUT / EXTRA); no GPU needed
  sweep   ONE process, variants interleaved (profiles/PLACEMENT.md: a context's buffers land in one of two placement states, so a variant
          is only ever compared inside a process and across fresh contexts): in each of --rounds rounds every variant gets a fresh
          context with the switch on and one with it off on the headline shape (bench.py's cfg2), and the two are timed alternately,
          --steps steps each in chunks of 5
  sizes   the size rule: bench.py's k_sweep shapes (K = 16, 64, 768 at block 256) and block 1024 x K = 64, both switch settings, fresh
          contexts, the shipped geometry

Prints JSON lines; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "firewheel_amd", "csrc")
sys.path.insert(0, ROOT)
VARIANTS = [(1, 16), (2, 8), (2, 16), (4, 8), (4, 16)]


def lib_path(g, u):
    return os.path.join(CSRC, "libfwgpu_g%du%d.so" % (g, u))


def build(jobs):
    for g, u in VARIANTS:
        subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", CSRC, "OBJDIR=_obj_g%du%d" % (g, u), "OUT=" + os.path.basename(lib_path(g, u)),
                               "EXTRA=-DLEAF_GROUP_G=%d -DLEAF_GROUP_U=%d" % (g, u)])
        print("built", lib_path(g, u))


def load(path):
    import firewheel_amd._lib as flib

    lib = C.CDLL(path)
    for name, (res, args) in flib.SIGNATURES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


class Bench(object):
    def __init__(self, B, F, V=1024):
        import torch

        import bench
        import firewheel_amd as fa
        import firewheel_amd._lib as flib

        self.torch, self.bench, self.fa, self.flib = torch, bench, fa, flib
        self.V, self.B, self.F = V, B, F
        self.src = torch.empty((V, 2, F), dtype=torch.float32, device="cuda")
        self.src.uniform_(-1.0, 1.0)
        self.args = types.SimpleNamespace(force_generic=False, taps=0, master=False, voice_fx=False)
        self.stream = torch.cuda.current_stream().cuda_stream

    def context(self, lib, on, K):
        """a fresh context of the headline graph on library `lib`, created with the switch `on`, warmed into its steady (lazy) calls"""
        saved = {k: os.environ.get(k) for k in ("FWGPU_LEAF_GROUP", "FWGPU_LEAF_GROUP_MIN")}
        os.environ["FWGPU_LEAF_GROUP"] = "1" if on else "0"
        os.environ["FWGPU_LEAF_GROUP_MIN"] = "1"
        keep = self.flib._lib
        self.flib._lib = lib
        try:
            cx, _, _, _ = self.bench.make_gpu(self.fa, "cfg2", self.V, self.B, K, 32, self.src, self.F, "f32", 0, self.args, self.stream, 0)
        finally:
            self.flib._lib = keep
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        out = self.torch.empty(K * self.B * 2, dtype=self.torch.float32, device="cuda")
        for _ in range(5):
            cx.process_blocks_device(K, out.data_ptr(), 2)
        cx.synchronize()
        return cx, out

    def time_steps(self, cx, out, K, n):
        t = self.torch
        s = t.cuda.ExternalStream(cx.hip_stream())  # the stream the context launches on (its own when it was given none)
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(n):
            cx.process_blocks_device(K, out.data_ptr(), 2)
        e1.record(s)
        e1.synchronize()
        cx.synchronize()
        return e0.elapsed_time(e1) / n

    def pair(self, lib, K, steps):
        """(ms per step switch on, switch off, grouped batches of the on context) — fresh contexts, timed alternately in chunks of 5"""
        on, out_on = self.context(lib, True, K)
        off, out_off = self.context(lib, False, K)
        g0 = on.group_stats()
        t_on, t_off = [], []
        for _ in range(max(1, steps // 5)):
            t_on.append(self.time_steps(on, out_on, K, 5))
            t_off.append(self.time_steps(off, out_off, K, 5))
        grouped = on.group_stats() - g0
        assert off.group_stats() == 0
        same = bool(self.torch.equal(out_on.view(self.torch.int32), out_off.view(self.torch.int32)))
        del on, off
        return statistics.mean(t_on), statistics.mean(t_off), grouped, same


def emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def sweep(rounds, steps, fh):
    V, B, K, F, _ = __import__("bench").DEFAULTS["cfg2"]
    b = Bench(B, F, V)
    libs = {v: load(lib_path(*v)) for v in VARIANTS}
    rows = {v: [] for v in VARIANTS}
    for r in range(rounds):
        for v in VARIANTS:
            on, off, grouped, same = b.pair(libs[v], K, steps)
            rows[v].append((on, off))
            emit({"round": r, "G": v[0], "U": v[1], "ms_on": round(on, 4), "ms_off": round(off, 4), "grouped_batches": grouped, "same_bits": same}, fh)
    for v in VARIANTS:
        ons, offs = [x[0] for x in rows[v]], [x[1] for x in rows[v]]
        emit({"summary": "G=%d U=%d" % v, "median_on": round(statistics.median(ons), 4), "min_on": round(min(ons), 4), "max_on": round(max(ons), 4),
              "median_off": round(statistics.median(offs), 4), "min_off": round(min(offs), 4), "max_off": round(max(offs), 4)}, fh)


def sizes(rounds, fh, lib_file):
    import torch

    torch.cuda.init()  # (the device runtime is torch's: up before the library is opened, as in bench.py)
    lib = load(lib_file)
    for B, K, F in ((256, 16, 262144), (256, 64, 262144), (256, 768, 262144), (1024, 64, 262144)):
        b = Bench(B, F)
        steps = max(20, min(400, 3072 // K))
        got = [b.pair(lib, K, steps) for _ in range(rounds)]
        pieces = (B + 255) // 256
        emit({"block": B, "K": K, "items": K * pieces, "ms_on": [round(x[0], 4) for x in got], "ms_off": [round(x[1], 4) for x in got],
              "median_on": round(statistics.median(x[0] for x in got), 4), "median_off": round(statistics.median(x[1] for x in got), 4),
              "grouped": [x[2] for x in got], "same_bits": all(x[3] for x in got)}, fh)
        del b
        __import__("torch").cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["build", "sweep", "sizes"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--lib", default=os.path.join(CSRC, "libfwgpu.so"), help="sizes: the library to measure")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "build":
        return build(a.jobs)
    fh = open(a.out, "w") if a.out else None
    if a.what == "sweep":
        sweep(a.rounds, a.steps, fh)
    else:
        sizes(a.rounds, fh, a.lib)


if __name__ == "__main__":
    main()
