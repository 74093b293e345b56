"""What latency compensation (FWGPU_DELAY_COMP) costs on a desk of config 2's size: its 1024 voices (sampler -> gain ->
pan, block 256, K = 768 blocks per step) split into two halves, each under a sub-mix of its own (a radix-32 SumNode tree), the first
through a look-ahead limiter, the two summed into graph_out.  The graph is built three times in one process on one device — the second
sub-mix straight into the last SumNode ("plain": misaligned by 63 frames), through DelayCompNode(63) ("comp"), and through FWGPU_DELAY
of 63 frames with feedback 0 and mix 1 ("delay": what a user has without the node; on a bus it walks the K blocks in sequence) — and the
same number of K-block steps timed for each, in alternating rounds, after the clocks have settled the way bench.py's `other_configs`
entries settle them.  Prints one JSON line: the three ms_per_step (median round), the differences to "plain", and what the level
launches of a step take in each graph between HIP events (comp - plain is k_delay_comp + k_delay_comp_hist: one launch of each per
step).  Read "comp" against "delay" of the same run, and against 8 bytes per frame and channel over the HBM peak.

usage: python scripts/delay_comp_cost.py [--steps 40] [--rounds 5] [--frames 63] [--only plain|comp|delay]   (--only: for a profiler run)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (the voices, sources and warm-up rule are bench.py's own)

K_DELAY = 11
K_LIMITER = 17
K_DELAY_COMP = 19
NAMES = ["plain", "comp", "delay"]


def make(fa, how, V, B, K, F, src, stream, args):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    s_a, _, bus_a = bench.graph_bank(g, V // 2, 32, 0, False, (), None, connect_out=False)
    s_b, _, bus_b = bench.graph_bank(g, V - V // 2, 32, 1, False, (), None, connect_out=False)
    top = g.add(bench.K_SUM, 4, 2)
    lim = g.add(K_LIMITER, 2, 2, [1.0, 0.0])
    g.connect_stereo(bus_a, lim)
    g.connect_stereo(lim, top)
    if how == "plain":
        g.connect_stereo(bus_b, top, 2)
    else:
        mid = g.add(K_DELAY_COMP, 2, 2, [float(args.frames)]) if how == "comp" else g.add(K_DELAY, 2, 2, [args.frames / 48000.0, 0.0, 1.0])
        g.connect_stereo(bus_b, mid)
        g.connect_stereo(mid, top, 2)
    g.connect_stereo(top, g.out_node())
    g.update()
    for v, s in enumerate(s_a + s_b):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    return cx


def measure(fa, torch, shard, args):
    V, B, K, F, _ = bench.DEFAULTS["cfg2"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    names = [args.only] if args.only else NAMES
    ctx = {n: make(fa, n, V, B, K, F, src, stream, args) for n in names}
    if len(names) > 1:  # neither node changes a planner decision
        assert len({ctx[n].plan_kind() for n in names}) == 1 and len({ctx[n].plan_fused_voices() for n in names}) == 1
        assert ctx["plain"].latency_report() and not ctx["comp"].latency_report()

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
    levels = {}
    for n in names:  # a separate pass: HIP events around the level launches of every step
        ctx[n].timing_reset()
        ctx[n].timing_enable(True)
        run(ctx[n], 5)
        ctx[n].timing_enable(False)
        ms, cnt = ctx[n].timing_read(3)
        levels[n] = round(ms / 5, 4)
    line = {"workload": "cfg2 as two sub-mixes, one limited", "voices": V, "block": B, "blocks_per_step": K, "steps": args.steps,
            "rounds": args.rounds, "frames": args.frames, "plan_kind": ctx[names[0]].plan_kind(),
            "fused_voices": ctx[names[0]].plan_fused_voices(),
            "ms_per_step": {n: round(med[n], 4) for n in names}, "rounds_ms": {n: [round(x, 4) for x in r] for n, r in rounds.items()},
            "level_launches_ms_per_step": levels,
            # what the copy must move at the least: 4 bytes in and 4 bytes out per frame and channel
            "comp_bytes_per_step": 8 * 2 * B * K}
    if len(names) > 1:
        for n in ("comp", "delay"):
            line[n + "_ms_per_step"] = round(med[n] - med["plain"], 4)
            line[n + "_us_per_block"] = round((med[n] - med["plain"]) * 1e3 / K, 4)
        line["k_delay_comp_mean_ms"] = round(levels["comp"] - levels["plain"], 4)   # one k_delay_comp + one k_delay_comp_hist launch per step
        line["bus_delay_mean_ms"] = round(levels["delay"] - levels["plain"], 4)
        if line["k_delay_comp_mean_ms"] > 0:
            line["k_delay_comp_gb_per_s"] = round(line["comp_bytes_per_step"] / (line["k_delay_comp_mean_ms"] * 1e-3) / 1e9, 1)
    for cx in ctx.values():
        cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=63)
    ap.add_argument("--only", choices=NAMES, default=None)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    measure(fa, torch, shard, args)


if __name__ == "__main__":
    main()
