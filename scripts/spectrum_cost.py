"""What a master spectrum meter (a FWGPU_METER with fft_size and bands) costs on config 2's graph: 1024 voices
(sampler -> gain -> pan), block 256, K = 768 blocks per step, built three times in one process on one device — with a plain 2 -> 2 meter
between the root SumNode and graph_out, and with a spectrum meter of N = 1024 / 32 bands and of N = 4096 / every bin in its place — and
the same number of K-block steps timed for each, in alternating rounds, after the clocks have settled the way bench.py's
`other_configs` entries settle them.  Prints one JSON line: the three ms_per_step (median round) and the differences to the plain meter.

usage: python scripts/spectrum_cost.py [--steps 40] [--rounds 5] [--only plain|n1024_b32|n4096_b0]     (--only: one graph, for a profiler run)
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
GRAPHS = {"plain": [1024.0], "n1024_b32": [1024.0, 1024.0, 32.0], "n4096_b0": [1024.0, 4096.0, 0.0]}


def make(fa, params, V, B, K, F, src, stream):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    samplers, _, root = bench.graph_bank(g, V, 32, 0, False, (), None, connect_out=False)
    meter = g.add(K_METER, 2, 2, params)
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
    ap.add_argument("--only", choices=sorted(GRAPHS), default=None)
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
    names = [args.only] if args.only else ["plain", "n1024_b32", "n4096_b0"]
    ctx = {n: make(fa, GRAPHS[n], V, B, K, F, src, stream) for n in names}

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
    if "plain" in med:
        line["spectrum_ms_per_step"] = {n: round(med[n] - med["plain"], 4) for n in names if n != "plain"}
    for n in names:
        if n == "plain":
            continue
        cx, meter = ctx[n]
        rd, done = cx.spectrum_read(meter, cx.spectrum_read(meter, 0, 0)[1] - 1, 1)
        line["blocks_done"] = int(done)
        line.setdefault("last_record_peak_db", {})[n] = [round(float(x), 2) for x in fa.MeterNode.power_db(rd[-1].max(axis=1))]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
