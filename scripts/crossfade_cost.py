"""What the crossfader (FWGPU_CROSSFADE) costs on a desk of config 2's size: its 1024 voices (sampler -> gain -> pan,
block 256, K = 768 blocks per step) split into two halves, each under a sub-mix of its own (a radix-32 SumNode tree), the two joined
into graph_out 0,1; beside the join a VolumeNode that nothing feeds goes to graph_out 2,3, so that all three graphs are the hybrid plan (a
tree of SumNodes over voices and nothing else would be the voice-bank plan as a whole, and the difference to it would hold the plan's
overhead, not the node's).  The graph is built three times in one process on one device — joined by a 4 -> 2 SumNode ("sum": the twin), by the
crossfader at rest at 0.5 ("rest": the gains once per wave), and by the crossfader inside a Bezier segment of 2^24 frames ("fade":
position and gains per frame; the segment is started again in an untimed step in front of every timed round, so no message lands in a
timed step and every block of it renders on the frozen path) — and the same number of K-block steps timed for each, in alternating
rounds, after the clocks have settled the way bench.py's `other_configs` entries settle them.  Prints one JSON line: the three ms_per_step (median round), the differences to "sum", and what the level launches of a step take
in each graph between HIP events (the same levels in all three, the join's level holding a SumNode or the crossfader: rest - sum and
fade - sum are what the crossfader takes more than a 4 -> 2 SumNode, inside k_level<0> — it has no launch of its own).  Read against 12 bytes per frame and channel (two loads, one store) over the HBM peak.

usage: python scripts/crossfade_cost.py [--steps 40] [--rounds 5] [--only sum|rest|fade]   (--only: for a profiler run)
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

K_CROSSFADE = 20
NAMES = ["sum", "rest", "fade"]
FADE_FRAMES = 1 << 24  # (the longest segment: 85 steps of 768 blocks of 256 frames — more than one round, fewer than the whole run)


def make(fa, how, V, B, K, F, src, stream):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 4, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    s_a, _, bus_a = bench.graph_bank(g, V // 2, 32, 0, False, (), None, connect_out=False)
    s_b, _, bus_b = bench.graph_bank(g, V - V // 2, 32, 1, False, (), None, connect_out=False)
    join = g.add(bench.K_SUM, 4, 2) if how == "sum" else g.add(K_CROSSFADE, 4, 2, [0.5 if how == "rest" else 0.0, 1.0])
    g.connect_stereo(bus_a, join)
    g.connect_stereo(bus_b, join, 2)
    g.connect_stereo(join, g.out_node())
    g.connect_stereo(g.add(bench.K_VOLUME, 2, 2, [100.0]), g.out_node(), 2)
    g.update()
    for v, s in enumerate(s_a + s_b):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    return cx, join


def arm(name, cx, join, run):
    """"fade": back to 0 and into a new segment, applied by one untimed step (the one batch that is walked in order)"""
    if name != "fade":
        return
    cx._check(cx.L.fwgpu_crossfade_to(cx.c, join, 0.0, 0, 0, 0.0, 0.0, 1.0, 1.0, 0))
    cx._check(cx.L.fwgpu_crossfade_to(cx.c, join, 1.0, FADE_FRAMES, 1, 0.42, 0.0, 0.58, 1.0, 0))
    run(cx, 1)


def measure(fa, torch, shard, args):
    V, B, K, F, _ = bench.DEFAULTS["cfg2"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K * B * 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    names = [args.only] if args.only else NAMES
    made = {n: make(fa, n, V, B, K, F, src, stream) for n in names}
    ctx = {n: made[n][0] for n in names}
    joins = {n: made[n][1] for n in names}
    if len(names) > 1:  # the node changes no planner decision
        assert len({ctx[n].plan_kind() for n in names}) == 1 and len({ctx[n].plan_fused_voices() for n in names}) == 1

    def run(cx, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            cx.process_blocks_device(K, out.data_ptr(), 4)
        cx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for n in names:  # untimed steps until the clocks have settled (bench.py OTHER_WARM_MS)
        t0 = time.perf_counter()
        run(ctx[n], 5)
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            run(ctx[n], 2)
    assert (args.steps + 1) * K * B < FADE_FRAMES, "a round must end inside the segment"
    rounds = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            arm(n, ctx[n], joins[n], run)
            rounds[n].append(run(ctx[n], args.steps))
    med = {n: sorted(r)[len(r) // 2] for n, r in rounds.items()}
    levels = {}
    for n in names:  # a separate pass: HIP events around the level launches of every step
        arm(n, ctx[n], joins[n], run)
        ctx[n].timing_reset()
        ctx[n].timing_enable(True)
        run(ctx[n], 5)
        ctx[n].timing_enable(False)
        ms, _ = ctx[n].timing_read(3)
        levels[n] = round(ms / 5, 4)
    line = {"workload": "cfg2 as two sub-mixes, joined", "voices": V, "block": B, "blocks_per_step": K, "steps": args.steps,
            "rounds": args.rounds, "plan_kind": ctx[names[0]].plan_kind(), "fused_voices": ctx[names[0]].plan_fused_voices(),
            "ms_per_step": {n: round(med[n], 4) for n in names}, "rounds_ms": {n: [round(x, 4) for x in r] for n, r in rounds.items()},
            "level_launches_ms_per_step": levels,
            # what the blend must move at the least: two 4-byte loads and one 4-byte store per frame and output channel
            "crossfade_bytes_per_step": 12 * 2 * B * K}
    if len(names) > 1:
        for n in ("rest", "fade"):
            line[n + "_ms_per_step"] = round(med[n] - med["sum"], 4)          # per-step difference to the SumNode twin
            line[n + "_us_per_block"] = round((med[n] - med["sum"]) * 1e3 / K, 4)
            line[n + "_level_share_ms"] = round(levels[n] - levels["sum"], 4)  # the same levels, the join's holding the crossfader in place of a SumNode
    for cx in ctx.values():
        cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=NAMES, default=None)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    measure(fa, torch, shard, args)


if __name__ == "__main__":
    main()
