"""What a master level meter (FWGPU_METER) costs on config 2's graph: 1024 voices (sampler -> gain -> pan), block
256, K = 768 blocks per step, built twice in one process on one device — as bench.py builds it, and with a 2 -> 2 meter between the root
SumNode and graph_out — and the same number of K-block steps timed for both, in alternating rounds, after the clocks have settled the way
bench.py's `other_configs` entries settle them.  Prints one JSON line: both ms_per_step (median round) and their difference.

usage: python scripts/meter_cost.py [--steps 40] [--rounds 5] [--only plain|metered]     (--only: one graph, for a profiler run)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (config 2's graph, sources and warm-up rule are bench.py's own)

K_METER = 16


def make(fa, torch, shard, metered, V, B, K, F, src, stream):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    samplers, _, root = bench.graph_bank(g, V, 32, 0, False, (), None, connect_out=not metered)
    meter = None
    if metered:
        meter = g.add(K_METER, 2, 2, [1024.0])
        g.connect_stereo(root, meter)
        g.connect_stereo(meter, g.out_node())
        g.update()
    for v, s in enumerate(samplers):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    assert cx.plan_kind() == 1, cx.plan_kind()
    return cx, meter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["plain", "metered"], default=None)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    V, B, K, F, _ = bench.DEFAULTS["cfg2"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    names = [args.only] if args.only else ["plain", "metered"]
    ctx = {n: make(fa, torch, shard, n == "metered", V, B, K, F, src, stream) for n in names}

    def run(cx, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            cx.process_blocks_device(K, out.data_ptr(), 2)
        cx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for n in names:  # untimed steps until the clocks have settled (bench.py OTHER_WARM_MS)
        t0 = time.perf_counter()
        run(ctx[n][0], 5)
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            run(ctx[n][0], 2)
    rounds = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            rounds[n].append(run(ctx[n][0], args.steps))
    med = {n: sorted(r)[len(r) // 2] for n, r in rounds.items()}
    line = {"workload": "cfg2", "voices": V, "block": B, "blocks_per_step": K, "steps": args.steps, "rounds": args.rounds,
            "ms_per_step": {n: round(med[n], 4) for n in names}, "rounds_ms": {n: [round(x, 4) for x in r] for n, r in rounds.items()}}
    if len(names) == 2:
        line["meter_ms_per_step"] = round(med["metered"] - med["plain"], 4)
    if "metered" in ctx:
        cx, meter = ctx["metered"]
        rd, done = cx.meter_read(meter, max(0, cx.meter_read(meter, 0, 0)[1] - 2), 2)
        line["blocks_done"] = int(done)
        line["last_reading"] = {"peak": [float(x) for x in rd["peak"][-1]], "over": [int(x) for x in rd["over"][-1]]}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
