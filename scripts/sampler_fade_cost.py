"""What a fading voice costs on config 2's bank (1024 voices sampler -> gain -> pan under a radix-32 SumNode tree, block 256, planar
f32 sources looping): one process on one device, after the clocks have settled the way bench.py's `other_configs` entries settle
them, in three configurations:

  rest    no message: every voice's envelope rests at 1.0, every call after the first is lazy (no control kernel).  The figure to hold
          against the parent commit's (the same script there, --only rest_k768: the parent has no fwgpu_sampler_fade to call)
  fade    every voice inside ONE long fade (fwgpu_sampler_fade, 2^24 frames, 1.0 -> 0.5) for the whole timed region — the fade is
          started again in an untimed step in front of every timed round, so no message lands in a timed step
  stairs  the status quo for a gain that moves: one set_percent_volume per voice per block, at the largest K the message ring allows
          (32 768 messages between two calls: K = 31 blocks per step for 1024 voices)

"rest" and "fade" are timed at K = 768 blocks per step (bench.py's cfg2) AND at the K of "stairs", so that the three can be read
against one another per block.  Prints one JSON line: ms per step and us per block (median round) and the lazy / control launch
batches per step (fwgpu_lazy_stats) of each.

usage: python scripts/sampler_fade_cost.py [--steps 10] [--rounds 3] [--only NAME]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402  (the voices, sources and warm-up rule are bench.py's own)

RING = 1 << 15             # fwgpu_ctx::RING_CAP: messages in flight between two process calls
FADE_FRAMES = 1 << 24      # the longest fade: 85 steps of 768 blocks of 256 frames


def make(fa, V, B, K, F, src, stream):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    voices, _, _ = bench.graph_bank(g, V, 32, 0, False, ())
    for v, s in enumerate(voices):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    return cx, voices


def measure(fa, torch, shard, args):
    import numpy as np

    V, B, K_BIG, F, _ = bench.DEFAULTS["cfg2"]
    K_MSG = RING // V - 1          # one message per voice per block, and room for the ring's one empty slot
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K_BIG * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    configs = [("rest_k768", "rest", K_BIG), ("fade_k768", "fade", K_BIG), ("rest_k%d" % K_MSG, "rest", K_MSG),
               ("fade_k%d" % K_MSG, "fade", K_MSG), ("stairs_k%d" % K_MSG, "stairs", K_MSG)]
    if args.only:
        configs = [c for c in configs if c[0] == args.only]
    line = {"workload": "cfg2, sampler sources", "voices": V, "block": B, "steps": args.steps, "rounds": args.rounds, "configs": {}}
    for name, how, K in configs:
        cx, voices = make(fa, V, B, K, F, src, stream)
        L = cx.L

        # the game's side of a fade today: a new volume for every voice at every block of the call, sent as ONE list
        # (fwgpu_node_set_params), so that the timed region holds the queueing but no per-message call overhead
        m_nodes = np.repeat(np.asarray(voices, dtype=np.int64), K)
        m_params = np.zeros(V * K, dtype=np.int32)
        m_at = np.tile(np.arange(K, dtype=np.uint32), V)
        as_ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))

        def step(n, msgs=False):
            t0 = time.perf_counter()
            for i in range(n):
                if msgs:
                    vals = (100.0 - 0.5 * ((i * K + m_at) % 64)).astype(np.float32)
                    cx._check(L.fwgpu_node_set_params(cx.c, V * K, as_ptr(m_nodes, C.c_int64), as_ptr(m_params, C.c_int), as_ptr(vals, C.c_float),
                                                      as_ptr(m_at, C.c_uint32)))
                cx.process_blocks_device(K, out.data_ptr(), 2)
            cx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        def arm():
            if how != "fade":
                return
            for node in voices:      # back to 1.0, then into a fade that outlasts the round
                cx._check(L.fwgpu_sampler_fade(cx.c, node, 1.0, 0, 0, 0))
                cx._check(L.fwgpu_sampler_fade(cx.c, node, 0.5, FADE_FRAMES, 0, 0))
            step(1)

        assert (args.steps + 1) * K * B < FADE_FRAMES, "a round must end inside the fade"
        t0 = time.perf_counter()
        arm()
        step(2)
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            step(1)
        rounds, lazy, ctl = [], 0, 0
        for _ in range(args.rounds):
            arm()
            a = cx.lazy_stats()
            rounds.append(step(args.steps, msgs=how == "stairs"))
            b = cx.lazy_stats()
            lazy, ctl = lazy + b[0] - a[0], ctl + b[1] - a[1]
        med = sorted(rounds)[len(rounds) // 2]
        n = args.steps * args.rounds
        line["configs"][name] = {"blocks_per_step": K, "ms_per_step": round(med, 4), "us_per_block": round(med * 1e3 / K, 3),
                                 "rounds_ms": [round(x, 4) for x in rounds], "lazy_batches_per_step": round(lazy / n, 3),
                                 "control_batches_per_step": round(ctl / n, 3), "plan_kind": cx.plan_kind(),
                                 "includes_the_message_list_call": how == "stairs"}
        cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    measure(fa, torch, shard, args)


if __name__ == "__main__":
    main()
