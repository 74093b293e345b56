"""What a bus compressor (FWGPU_COMPRESSOR) costs on a desk of config 2's size, next to its yardstick, the sidechain
ducker: the desk of scripts/ducker_cost.py — config 2's 1024 voices (sampler -> gain -> pan, block 256, K = 768 blocks per step) as a
music half and a dialogue half under a sub-mix each, the two summed into graph_out.  Four graphs in one process on one device, the music
sub-mix going through: a 2 -> 2 volume (the twin), a compressor at (A, R, H) = (240, 12000, 0), a compressor at the caps (32768, 32768,
2048), and a ducker of the first windows keyed by the dialogue sub-mix.  The same number of K-block steps is timed for all four in
alternating rounds, after the clocks have settled the way bench.py's `other_configs` entries settle them.  Prints one JSON line: every
ms_per_step (median round), what each node adds over the volume twin, and the compressor's added cost over the ducker's.

usage: python scripts/compressor_cost.py [--steps 40] [--rounds 5] [--only volume|comp|comp_caps|duck]   (--only: one graph, for a profiler run)
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

K_DUCKER, K_COMPRESSOR, K_VOLUME = 18, 21, 2
WINDOWS = {"comp": (240, 12000, 0), "comp_caps": (32768, 32768, 2048), "duck": (240, 12000, 0)}
NAMES = ["volume", "comp", "comp_caps", "duck"]


def make(fa, how, V, B, K, F, src, stream, args):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    s_music, _, music = bench.graph_bank(g, V // 2, 32, 0, False, (), None, connect_out=False)
    s_dialogue, _, dialogue = bench.graph_bank(g, V - V // 2, 32, 1, False, (), None, connect_out=False)
    top = g.add(bench.K_SUM, 4, 2)
    if how == "volume":
        mid = g.add(K_VOLUME, 2, 2, [100.0])
    elif how == "duck":
        a, r, h = WINDOWS[how]
        mid = g.add(K_DUCKER, 4, 2, [args.threshold, 0.25, float(a), float(r), float(h)])
        g.connect_stereo(dialogue, mid, 2)
    else:
        a, r, h = WINDOWS[how]
        mid = g.add(K_COMPRESSOR, 2, 2, [args.threshold, 4.0, 6.0, float(a), float(r), float(h), 1.0])
    g.connect_stereo(music, mid)
    g.connect_stereo(mid, top)
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
    names = [args.only] if args.only else NAMES
    ctx = {n: make(fa, n, V, B, K, F, src, stream, args) for n in names}
    for n in names[1:]:  # no node changes a planner decision
        assert ctx[n].plan_kind() == ctx[names[0]].plan_kind() and ctx[n].plan_fused_voices() == ctx[names[0]].plan_fused_voices(), n

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
            "plan_kind": ctx[names[0]].plan_kind(), "fused_voices": ctx[names[0]].plan_fused_voices(), "windows": WINDOWS,
            "ms_per_step": {n: round(med[n], 4) for n in names}, "rounds_ms": {n: [round(x, 4) for x in r] for n, r in rounds.items()},
            "level_launches_ms_per_step": levels}
    if len(names) == len(NAMES):
        line["added_ms_per_step"] = {n: round(med[n] - med["volume"], 4) for n in names[1:]}
        line["added_level_launches_ms"] = {n: round(levels[n] - levels["volume"], 4) for n in names[1:]}
        duck = med["duck"] - med["volume"]
        line["compressor_over_ducker"] = {n: round((med[n] - med["volume"]) / duck, 2) if duck > 0 else None for n in ("comp", "comp_caps")}
    for cx in ctx.values():
        cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--only", choices=NAMES, default=None)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    measure(fa, torch, shard, args)


if __name__ == "__main__":
    main()
