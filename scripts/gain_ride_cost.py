"""What a gain ride costs on config 2's bank (bench.py cfg2: 1024 voices sampler -> gain -> pan under a radix-32 SumNode tree, block 256,
looping): one process on one device, after the clocks have settled the way bench.py's `other_configs` entries settle them, in four
configurations, timed in this order on ONE context:

  steady        no message: every call lazy (the kernels a graph without rides runs)
  ride          every voice's volume inside ONE ride (fwgpu_gain_ride, 2^24 frames, an ease) for the whole timed region — the ride is
                started again in an untimed step in front of every timed round, so no message lands in a timed step
                (k_voice_control_ride writes the per-frame gain rows, the leaf kernel reads them as it reads a ramp)
  glide         every voice inside the existing one-pole glide: one set_param per voice in front of every timed step (the 10 ms
                smoother covers 480 frames, not quite two of a step's 768 blocks; the queueing call is inside the timed region)
  steady_again  the steady bank behind the ride: a step that ends the ride (frames == 0), untimed steps, then the timed rounds — the
                lazy calls must be back (control_batches_per_step 0)

Prints one JSON line: ms per step and us per block (median round), the rounds, and the control launch batches per step
(fwgpu_lazy_stats).  Run it several times in fresh processes (contexts) and take the median, as the measuring guide says.

usage: python scripts/gain_ride_cost.py [--steps 10] [--rounds 3] [--blocks 768]
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

RIDE_FRAMES = 1 << 24      # the longest ride: 85 steps of 768 blocks of 256 frames
EASE = (0.42, 0.0, 0.58, 1.0)


def measure(fa, torch, shard, args):
    import numpy as np

    V, B, K, F, _ = bench.DEFAULTS["cfg2"]
    K = args.blocks or K
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = bench.GpuSide(cx)
    samplers, volumes, _ = bench.build_graph(g, "cfg2", V, 32, 0, False)
    for v, s in enumerate(samplers):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    assert cx.plan_kind() == 1 and len(volumes) == V
    L = cx.L
    nodes = np.asarray(volumes, dtype=np.int64)
    params = np.zeros(V, dtype=np.int32)
    at = np.zeros(V, dtype=np.uint32)
    as_ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))

    def step(n, glide=False):
        t0 = time.perf_counter()
        for i in range(n):
            if glide:
                vals = np.full(V, 40.0 + 30.0 * (i % 2), dtype=np.float32)
                cx._check(L.fwgpu_node_set_params(cx.c, V, as_ptr(nodes, C.c_int64), as_ptr(params, C.c_int), as_ptr(vals, C.c_float), as_ptr(at, C.c_uint32)))
            cx.process_blocks_device(K, out.data_ptr(), 2)
        cx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def ride(value, frames):
        for node in volumes:
            cx._check(L.fwgpu_gain_ride(cx.c, node, value, frames, 1, EASE[0], EASE[1], EASE[2], EASE[3], 0))

    def arm(how):
        if how == "ride":           # back to full volume, then into a ride that outlasts the round
            ride(100.0, 0)
            ride(30.0, RIDE_FRAMES)
            step(1)
        elif how == "steady_again":
            pass

    assert (args.steps + 1) * K * B < RIDE_FRAMES, "a round must end inside the ride"
    line = {"workload": "cfg2", "voices": V, "block": B, "blocks_per_step": K, "steps": args.steps, "rounds": args.rounds, "configs": {}}
    for how in ("steady", "ride", "glide", "steady_again"):
        if how == "steady_again":   # end the ride, let the control calls behind it pass
            ride(100.0, 0)
            step(3)
        t0 = time.perf_counter()
        arm(how)
        step(2, glide=how == "glide")
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            step(1, glide=how == "glide")
        rounds, ctl = [], 0
        for _ in range(args.rounds):
            arm(how)
            a = cx.lazy_stats()
            rounds.append(step(args.steps, glide=how == "glide"))
            ctl += cx.lazy_stats()[1] - a[1]
        if how == "glide":          # let the last glide settle before the next configuration
            step(3)
        med = sorted(rounds)[len(rounds) // 2]
        line["configs"][how] = {"ms_per_step": round(med, 4), "us_per_block": round(med * 1e3 / K, 3), "rounds_ms": [round(x, 4) for x in rounds],
                                "control_batches_per_step": round(ctl / (args.steps * args.rounds), 3),
                                "includes_the_message_list_call": how == "glide"}
    cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=0)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    measure(fa, torch, shard, args)


if __name__ == "__main__":
    main()
