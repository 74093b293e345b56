"""What a master look-ahead limiter (FWGPU_LIMITER) costs on the headline graphs: config 2 (1024 voices, sampler ->
gain -> pan, block 256, K = 768 blocks per step: the voice-bank plan) and config 3 (4096 voices, sampler -> biquad -> delay -> gain, block
512, K = 64: the chain plan), each built twice in one process on one device — as bench.py builds it, and with a 2 -> 2 limiter between the
root SumNode and graph_out — and the same number of K-block steps timed for both, in alternating rounds, after the clocks have settled the
way bench.py's `other_configs` entries settle them.  The graph without the node is what the library did before the node existed.  Prints
one JSON line per config: both ms_per_step (median round), their difference, and that difference per block.

usage: python scripts/limiter_cost.py [--steps 40] [--rounds 5] [--hold 128] [--ceiling 1.0] [--workload cfg2|cfg3|both]
                                      [--only plain|limited]     (--only: one graph, for a profiler run)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (the graphs, sources and warm-up rule are bench.py's own)

K_LIMITER = 17


def make(fa, wl, limited, V, B, K, F, src, stream, ceiling, hold):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    if wl == "cfg2":
        samplers, _, root = bench.graph_bank(g, V, 32, 0, False, (), None, connect_out=not limited)
    else:
        samplers, _, root = bench.graph_chain(g, V, 32, 0, False, connect_out=not limited)
    if limited:
        lim = g.add(K_LIMITER, 2, 2, [ceiling, float(hold)])
        g.connect_stereo(root, lim)
        g.connect_stereo(lim, g.out_node())
        g.update()
    for v, s in enumerate(samplers):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    want = bench.want_plan(wl, False)
    assert cx.plan_kind() == want, (cx.plan_kind(), want)
    return cx


def measure(fa, torch, shard, wl, args):
    V, B, K, F, _ = bench.DEFAULTS[wl]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    names = [args.only] if args.only else ["plain", "limited"]
    ctx = {n: make(fa, wl, n == "limited", V, B, K, F, src, stream, args.ceiling, args.hold) for n in names}

    def run(cx, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            cx.process_blocks_device(K, out.data_ptr(), 2)
        cx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for n in names:  # untimed steps until the clocks have settled (bench.py OTHER_WARM_MS)
        t0 = time.perf_counter()
        run(ctx[n], 5)
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            run(ctx[n], 2)
    rounds = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            rounds[n].append(run(ctx[n], args.steps))
    med = {n: sorted(r)[len(r) // 2] for n, r in rounds.items()}
    line = {"workload": wl, "voices": V, "block": B, "blocks_per_step": K, "steps": args.steps, "rounds": args.rounds, "hold_frames": args.hold,
            "ceiling": args.ceiling, "parallel_path": B >= args.hold + 126,
            "ms_per_step": {n: round(med[n], 4) for n in names}, "rounds_ms": {n: [round(x, 4) for x in r] for n, r in rounds.items()}}
    if len(names) == 2:
        line["limiter_ms_per_step"] = round(med["limited"] - med["plain"], 4)
        line["limiter_us_per_block"] = round((med["limited"] - med["plain"]) * 1e3 / K, 4)
    if "limited" in ctx:  # what came out stays under the ceiling
        peak = float(out.abs().max().item())
        line["last_step_peak"] = peak
        assert peak <= args.ceiling * (1.0 + 66.0 * 2.0 ** -24), peak
    for cx in ctx.values():
        cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hold", type=int, default=128)
    ap.add_argument("--ceiling", type=float, default=1.0)
    ap.add_argument("--workload", choices=["cfg2", "cfg3", "both"], default="both")
    ap.add_argument("--only", choices=["plain", "limited"], default=None)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    for wl in (("cfg2", "cfg3") if args.workload == "both" else (args.workload,)):
        measure(fa, torch, shard, wl, args)


if __name__ == "__main__":
    main()
