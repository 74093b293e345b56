"""What a moving filter costs on config 3's bank (4096 voices sampler -> biquad LPF -> delay -> gain under a radix-32 SumNode tree,
block 512; bench.py's graph_chain): one process on one device, after the clocks have settled the way bench.py's `other_configs`
entries settle them, in three configurations:

  steady  no message: every call after the first is lazy (no control kernel), k_chain's steady instantiation
  sweep   every voice inside ONE coefficient sweep (fwgpu_biquad_sweep, 2^24 frames) for the whole timed region — the sweep is started
          again in an untimed step in front of every timed round, so no message lands in a timed step; the control kernel runs in
          every call and k_chain's sweep instantiation renders it
  steps   the status quo for a moving cutoff: one set_cutoff_hz per voice per block, at the largest K the message ring admits
          (32 768 messages between two calls: K = 7 blocks per step for 4096 voices)

"steady" and "sweep" are timed at K = 64 blocks per step (bench.py's cfg3) AND at the K of "steps", so that the three can be read
against one another per block.  Prints one JSON line: ms per step and us per block (median round) and the lazy / control launch
batches per step (fwgpu_lazy_stats) of each.

usage: python scripts/bq_sweep_cost.py [--steps 10] [--rounds 3] [--only NAME]
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
SWEEP_FRAMES = 1 << 24     # the longest sweep: 512 steps of 64 blocks of 512 frames


class Side(bench.GpuSide):
    """bench.GpuSide that remembers the biquads it adds, in voice order"""

    def __init__(self, cx):
        bench.GpuSide.__init__(self, cx)
        self.biquads = []

    def add(self, kind, n_in, n_out, params=()):
        n = bench.GpuSide.add(self, kind, n_in, n_out, params)
        if kind == bench.K_BIQUAD:
            self.biquads.append((n, float(params[1])))
        return n


def make(fa, V, B, K, F, src, stream):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = Side(cx)
    samplers, _, _ = bench.graph_chain(g, V, 32)
    for v, s in enumerate(samplers):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    return cx, g.biquads


def measure(fa, torch, shard, args):
    import numpy as np

    V, B, K_BIG, F, _ = bench.DEFAULTS["cfg3"]
    K_MSG = RING // V - 1          # one message per voice per block, and room for the ring's one empty slot
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K_BIG * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    configs = [("steady_k%d" % K_BIG, "steady", K_BIG), ("sweep_k%d" % K_BIG, "sweep", K_BIG), ("steady_k%d" % K_MSG, "steady", K_MSG),
               ("sweep_k%d" % K_MSG, "sweep", K_MSG), ("steps_k%d" % K_MSG, "steps", K_MSG)]
    if args.only:
        configs = [c for c in configs if c[0] == args.only]
    line = {"workload": "cfg3, biquad + delay voices", "voices": V, "block": B, "steps": args.steps, "rounds": args.rounds, "configs": {}}
    for name, how, K in configs:
        cx, biquads = make(fa, V, B, K, F, src, stream)
        L = cx.L
        nodes = np.asarray([b[0] for b in biquads], dtype=np.int64)
        cut0 = np.asarray([b[1] for b in biquads], dtype=np.float64)

        # the game's side of a moving cutoff today: a new cutoff for every voice at every block of the call, sent as ONE list
        # (fwgpu_node_set_params), so that the timed region holds the queueing but no per-message call overhead
        m_nodes = np.repeat(nodes, K)
        m_params = np.ones(V * K, dtype=np.int32)
        m_at = np.tile(np.arange(K, dtype=np.uint32), V)
        as_ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))

        def step(n, msgs=False):
            t0 = time.perf_counter()
            for i in range(n):
                if msgs:
                    vals = (np.repeat(cut0, K) * (1.0 + 1e-3 * ((i * K + m_at) % 64))).astype(np.float32)
                    cx._check(L.fwgpu_node_set_params(cx.c, V * K, as_ptr(m_nodes, C.c_int64), as_ptr(m_params, C.c_int), as_ptr(vals, C.c_float),
                                                      as_ptr(m_at, C.c_uint32)))
                cx.process_blocks_device(K, out.data_ptr(), 2)
            cx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        def arm():
            if how != "sweep":
                return
            for v in range(V):      # back to the voice's own cutoff, then into a sweep that outlasts the round
                cx._check(L.fwgpu_biquad_sweep(cx.c, int(nodes[v]), float(cut0[v]), 0.707, 0, 0))
                cx._check(L.fwgpu_biquad_sweep(cx.c, int(nodes[v]), float(cut0[v] * 0.25), 0.707, SWEEP_FRAMES, 0))
            step(1)

        assert (args.steps + 1) * K * B < SWEEP_FRAMES, "a round must end inside the sweep"
        t0 = time.perf_counter()
        arm()
        step(2)
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            step(1)
        rounds, lazy, ctl = [], 0, 0
        for _ in range(args.rounds):
            arm()
            a = cx.lazy_stats()
            rounds.append(step(args.steps, msgs=how == "steps"))
            b = cx.lazy_stats()
            lazy, ctl = lazy + b[0] - a[0], ctl + b[1] - a[1]
        med = sorted(rounds)[len(rounds) // 2]
        n = args.steps * args.rounds
        line["configs"][name] = {"blocks_per_step": K, "ms_per_step": round(med, 4), "us_per_block": round(med * 1e3 / K, 3),
                                 "rounds_ms": [round(x, 4) for x in rounds], "lazy_batches_per_step": round(lazy / n, 3),
                                 "control_batches_per_step": round(ctl / n, 3), "plan_kind": cx.plan_kind(),
                                 "includes_the_message_list_call": how == "steps"}
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
