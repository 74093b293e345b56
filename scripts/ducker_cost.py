"""What a sidechain ducker (FWGPU_DUCKER) costs on a desk of config 2's size: its 1024 voices (sampler -> gain -> pan,
block 256, K = 768 blocks per step) split into a music half and a dialogue half, each under a sub-mix of its own (a radix-32 SumNode
tree), the two sub-mixes summed into graph_out.  The graph is built twice in one process on one device — music straight into the last
SumNode, and music through a ducker keyed by the dialogue sub-mix — and the same number of K-block steps timed for both, in alternating
rounds, after the clocks have settled the way bench.py's `other_configs` entries settle them.  Prints one JSON line: both ms_per_step
(median round), their difference, that difference per block, and what the level launches of a step take in either graph between HIP
events (their difference is k_ducker + k_ducker_hist: the ducker's level holds nothing else).

usage: python scripts/ducker_cost.py [--steps 40] [--rounds 5] [--threshold 0.5] [--depth 0.25] [--attack 480] [--release 12000]
                                     [--hold 4800] [--only plain|ducked]     (--only: one graph, for a profiler run)
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

K_DUCKER = 18


def make(fa, ducked, V, B, K, F, src, stream, args):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    s_music, _, music = bench.graph_bank(g, V // 2, 32, 0, False, (), None, connect_out=False)
    s_dialogue, _, dialogue = bench.graph_bank(g, V - V // 2, 32, 1, False, (), None, connect_out=False)
    top = g.add(bench.K_SUM, 4, 2)
    if ducked:
        duck = g.add(K_DUCKER, 4, 2, [args.threshold, args.depth, float(args.attack), float(args.release), float(args.hold)])
        g.connect_stereo(music, duck)
        g.connect_stereo(dialogue, duck, 2)
        g.connect_stereo(duck, top)
    else:
        g.connect_stereo(music, top)
    g.connect_stereo(dialogue, top, 2)
    g.connect_stereo(top, g.out_node())
    g.update()
    for v, s in enumerate(s_music + s_dialogue):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    return cx


def measure(fa, torch, shard, args):
    V, B, K, F, _ = bench.DEFAULTS["cfg2"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    names = [args.only] if args.only else ["plain", "ducked"]
    ctx = {n: make(fa, n == "ducked", V, B, K, F, src, stream, args) for n in names}
    if len(names) == 2:  # the ducker changes no planner decision
        assert ctx["plain"].plan_kind() == ctx["ducked"].plan_kind(), (ctx["plain"].plan_kind(), ctx["ducked"].plan_kind())
        assert ctx["plain"].plan_fused_voices() == ctx["ducked"].plan_fused_voices()

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
    line = {"workload": "cfg2 as two sub-mixes", "voices": V, "block": B, "blocks_per_step": K, "steps": args.steps, "rounds": args.rounds,
            "plan_kind": ctx[names[0]].plan_kind(), "fused_voices": ctx[names[0]].plan_fused_voices(),
            "ducker": {"threshold": args.threshold, "depth": args.depth, "attack_frames": args.attack, "release_frames": args.release,
                       "hold_frames": args.hold},
            "ms_per_step": {n: round(med[n], 4) for n in names}, "rounds_ms": {n: [round(x, 4) for x in r] for n, r in rounds.items()},
            "level_launches_ms_per_step": levels}
    if len(names) == 2:
        line["ducker_ms_per_step"] = round(med["ducked"] - med["plain"], 4)
        line["ducker_us_per_block"] = round((med["ducked"] - med["plain"]) * 1e3 / K, 4)
        line["k_ducker_mean_ms"] = round(levels["ducked"] - levels["plain"], 4)   # one k_ducker + one k_ducker_hist launch per step
    for cx in ctx.values():
        cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--depth", type=float, default=0.25)
    ap.add_argument("--attack", type=int, default=480)
    ap.add_argument("--release", type=int, default=12000)
    ap.add_argument("--hold", type=int, default=4800)
    ap.add_argument("--only", choices=["plain", "ducked"], default=None)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    measure(fa, torch, shard, args)


if __name__ == "__main__":
    main()
