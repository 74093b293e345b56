"""What a FIR reverb morph (SPEC FIR morph) costs on config 4's shape: 256 voices, sampler -> 65 536-tap stereo FIR ->
radix-32 sum tree, block 256, K = 16 blocks per step.  The graph is built three times in one process on one device — with plain
one-parameter FIR nodes ("plain": the twin, bench.py's cfg4 graph), with morph-capable nodes at rest at slot A ("rest": slot B's GEMM
workgroups return before their first load; the control step and the morph reduce run), and with every node inside a fade of 2^24
frames ("fade": both slots' GEMMs; the fade is started again in an untimed step in front of every timed round, so no message lands in
a timed step) — and the same number of K-block steps timed for each, in alternating rounds, after the clocks have settled the way
bench.py's `other_configs` entries settle them.  Prints one JSON line: the three ms_per_step (median round), the two ratios to
"plain", the GEMM launches' own time between HIP events, and the morph groups' workgroup counters per step.  Expect about two GEMMs for
"fade" and the plain step plus the idle workgroups' exit and the control step for "rest".

usage: python scripts/fir_morph_cost.py [--steps 6] [--rounds 5] [--only plain|rest|fade] [--voices 256] [--taps 65536]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (the voices, sources, impulse response and warm-up rule are bench.py's own)

NAMES = ["plain", "rest", "fade"]
FADE_FRAMES = 1 << 24  # (the longest segment: 4096 steps of 16 blocks of 256 frames)


def make(fa, how, V, B, K, F, taps, src, stream):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    ir = cx.new_sample(bench.PLANAR_F32, 2, bench.reverb_ir(taps))
    ir_b = cx.new_sample(bench.PLANAR_F32, 2, bench.reverb_ir(taps)[:, ::-1].copy())
    ends, samplers = [], []
    for v in range(V):
        s = g.add(bench.K_SAMPLER, 0, 2, [100.0])
        f = g.add(bench.K_FIR, 2, 2, [float(ir)] if how == "plain" else [float(ir), float(ir_b), 0.0, 0.0, 1.0])
        g.connect_stereo(s, f)
        samplers.append(s)
        ends.append(f)
    bench.sum_tree(g, ends, 32, False, True)
    g.update()
    for v, s in enumerate(samplers):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    return cx, ends


def arm(name, cx, nodes, run):
    """"fade": back to 0 and into a new segment, applied by one untimed step"""
    if name != "fade":
        return
    for f in nodes:
        cx._check(cx.L.fwgpu_fir_morph(cx.c, f, 0.0, 0, 0, 0.0, 0.0, 1.0, 1.0, 0))
        cx._check(cx.L.fwgpu_fir_morph(cx.c, f, 1.0, FADE_FRAMES, 1, 0.42, 0.0, 0.58, 1.0, 0))
    run(cx, 1)


def measure(fa, torch, shard, args):
    V, B, K, F, _ = bench.DEFAULTS["cfg4"]
    V = args.voices or V
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    names = [args.only] if args.only else NAMES
    made = {n: make(fa, n, V, B, K, F, args.taps, src, stream) for n in names}
    ctx = {n: made[n][0] for n in names}
    nodes = {n: made[n][1] for n in names}

    def run(cx, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            cx.process_blocks_device(K, out.data_ptr(), 2)
        cx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for n in names:  # untimed steps until the clocks have settled (bench.py OTHER_WARM_MS)
        t0 = time.perf_counter()
        run(ctx[n], 2)
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            run(ctx[n], 1)
    assert (args.steps + 1) * K * B < FADE_FRAMES, "a round must end inside the segment"
    rounds = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            arm(n, ctx[n], nodes[n], run)
            rounds[n].append(run(ctx[n], args.steps))
    med = {n: sorted(r)[len(r) // 2] for n, r in rounds.items()}
    gemm, tiles = {}, {}
    for n in names:  # a separate pass: HIP events around the GEMM launch of every step, and the morph groups' counters
        arm(n, ctx[n], nodes[n], run)
        r0 = ctx[n].fir_morph_stats()
        ctx[n].timing_reset()
        ctx[n].timing_enable(True)
        run(ctx[n], 3)
        ctx[n].timing_enable(False)
        ms, _ = ctx[n].timing_read(4)
        r1 = ctx[n].fir_morph_stats()
        gemm[n] = round(ms / 3, 4)
        tiles[n] = {"run": (r1[0] - r0[0]) // 3, "skipped": (r1[1] - r0[1]) // 3}
    line = {"workload": "cfg4", "voices": V, "taps": args.taps, "block": B, "blocks_per_step": K, "steps": args.steps, "rounds": args.rounds,
            "plan_kind": {n: ctx[n].plan_kind() for n in names}, "ms_per_step": {n: round(med[n], 4) for n in names},
            "rounds_ms": {n: [round(x, 4) for x in r] for n, r in rounds.items()}, "gemm_ms_per_step": gemm, "gemm_workgroups_per_step": tiles}
    if len(names) > 1:
        for n in ("rest", "fade"):
            line[n + "_over_plain"] = round(med[n] / med["plain"], 4)
    for cx in ctx.values():
        cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=NAMES, default=None)
    ap.add_argument("--voices", type=int, default=None)
    ap.add_argument("--taps", type=int, default=65536)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    measure(fa, torch, shard, args)


if __name__ == "__main__":
    main()
