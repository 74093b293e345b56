"""What streaming voices cost on config 2's bank (1024 voices sampler -> gain -> pan under a radix-32 SumNode tree, block 256, planar
f32 sources): one process on one device, after the clocks have settled the way bench.py's `other_configs` entries settle them, with
0, 1 and 64 of the voices playing a stream (fwgpu_sample_create_stream) and the others looping a plain sample.

A step is K = 16 blocks (4096 frames): the writer appends 4096 frames to every stream from device memory (fwgpu_sample_stream_write_device)
in front of each step, untimed, so no stream is ever starved; the timed part is the process call alone.  With no stream every call
after the first is lazy (no control kernel); with a stream bound every call runs the control kernel and ends with the one launch that
publishes the streaming samplers' counts — the difference between the rows is the price of leaving the lazy path plus that launch.
The control-side time of one 4096-frame write (host memory and device memory) is reported next to them.

Prints one JSON line: ms per step (median round), the lazy / control launch batches per step (fwgpu_lazy_stats), starved blocks (0 is
expected) and us per write.

usage: python scripts/stream_cost.py [--steps 50] [--rounds 3]
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

K = 16


def measure(fa, torch, shard, args):
    import numpy as np

    V, B, _, F, _ = bench.DEFAULTS["cfg2"]
    W = K * B                       # frames per write and per step
    R = 4 * W                       # a ring that holds a whole call and more
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K * B * 2, dtype=torch.float32, device=dev)
    chunk = torch.empty(2 * W, dtype=torch.float32, device=dev).uniform_(-1.0, 1.0)
    chunk_host = np.ascontiguousarray(chunk.cpu().numpy())
    torch.cuda.synchronize()
    line = {"workload": "cfg2, sampler sources", "voices": V, "block": B, "blocks_per_step": K, "ring_frames": R, "steps": args.steps,
            "rounds": args.rounds, "configs": {}}
    for n_streams in (0, 1, 64):
        cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
        cx.set_max_batch(K)
        g = bench.GpuSide(cx)
        voices, _, _ = bench.graph_bank(g, V, 32, 0, False, ())
        streams = []
        for v, s in enumerate(voices):
            if v < n_streams:
                st = cx.new_stream(bench.PLANAR_F32, 2, R)
                cx._check(cx.L.fwgpu_sampler_set_sample(cx.c, s, st.id, 0, 0))
                cx._check(cx.L.fwgpu_sampler_play(cx.c, s, 0))
                streams.append(st)
            else:
                g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))

        def step(n):
            t = 0.0
            for _ in range(n):
                for st in streams:
                    st.write(chunk)
                t0 = time.perf_counter()
                cx.process_blocks_device(K, out.data_ptr(), 2)
                cx.synchronize()
                t += time.perf_counter() - t0
            return t * 1e3 / n

        t0 = time.perf_counter()
        step(2)
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            step(1)
        rounds, lazy, ctl = [], 0, 0
        for _ in range(args.rounds):
            a = cx.lazy_stats()
            rounds.append(step(args.steps))
            b = cx.lazy_stats()
            lazy, ctl = lazy + b[0] - a[0], ctl + b[1] - a[1]
        med = sorted(rounds)[len(rounds) // 2]
        n = args.steps * args.rounds
        row = {"ms_per_step": round(med, 4), "rounds_ms": [round(x, 4) for x in rounds], "lazy_batches_per_step": round(lazy / n, 3),
               "control_batches_per_step": round(ctl / n, 3), "plan_kind": cx.plan_kind(), "starved_blocks": sum(st.status()[2] for st in streams)}
        if n_streams == 1:  # the control-side time of one 4096-frame write, a process call in between to make room
            for name, data in (("write_device_us", chunk), ("write_host_us", chunk_host)):
                ts = []
                for _ in range(20):
                    cx.process_blocks_device(K, out.data_ptr(), 2)
                    cx.synchronize()
                    t1 = time.perf_counter()
                    got = streams[0].write(data)
                    ts.append((time.perf_counter() - t1) * 1e6)
                    assert got == W, got
                row[name] = round(sorted(ts)[len(ts) // 2], 2)
        line["configs"]["streams_%d" % n_streams] = row
        cx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    import firewheel_amd as fa
    from firewheel_amd import shard

    measure(fa, torch, shard, args)


if __name__ == "__main__":
    main()
