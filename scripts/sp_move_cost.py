"""What a moving source costs on config 2's spatialiser bank (bench.py cfg2_spatial: 1024 voices sampler -> gain -> pan -> 3D spatialiser
under a radix-32 SumNode tree, block 256, looping): one process on one device, after the clocks have settled the way bench.py's
`other_configs` entries settle them, in three configurations:

  rest    no message: every voice at rest (the kernels a graph without moves runs: k_voice_control, k_leaf_sum_sp)
  move    every voice inside ONE move (fwgpu_spatial_move, 2^24 frames) for the whole timed region — the move is started again in an
          untimed step in front of every timed round, so no message lands in a timed step (k_voice_control_spm writes the per-frame
          rows, k_leaf_sum_sp_spm's port-by-port path reads them)
  steps   the status quo for a moving source: one set_position (three set_param calls: nine messages) per voice per block, at the
          largest K the message ring allows

"rest" and "move" are timed at K = 768 blocks per step (bench.py's cfg2) AND at the K of "steps", so that the three can be read
against one another per block.  Prints one JSON line: ms per step and us per block (median round), the rounds, the control launch
batches per step (fwgpu_lazy_stats), how many voices the message ring lets through per call of K blocks when every voice is given a
set_position per block, and the moving leaf kernel's share of its HBM roofline from the bytes a move block touches.  Run it several
times in fresh processes (contexts) and take the median, as the measuring guide says.

usage: python scripts/sp_move_cost.py [--steps 10] [--rounds 3] [--only NAME]
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
MSGS_PER_POSITION = 9      # set_position = params 0, 1, 2, each CMD_SET_P0 + CMD_SET_P1 + CMD_SP_ITD
MOVE_FRAMES = 1 << 24      # the longest move: 85 steps of 768 blocks of 256 frames
HBM_BYTES_PER_S = 8.0e12   # MI355X peak


class Side(bench.GpuSide):
    """bench.GpuSide that remembers the spatialisers it adds"""

    def __init__(self, cx):
        bench.GpuSide.__init__(self, cx)
        self.spatial = []

    def add(self, kind, n_in, n_out, params=()):
        n = bench.GpuSide.add(self, kind, n_in, n_out, params)
        if kind == bench.K_SPATIAL:
            self.spatial.append(n)
        return n


def make(fa, V, B, K, F, src, stream):
    cx = fa.FirewheelGpuCtx(48000, B, 0, 2, device=0, stream=stream)
    cx.set_max_batch(K)
    g = Side(cx)
    samplers, _, _ = bench.build_graph(g, "cfg2", V, 32, 0, False, None, "spatial")
    for v, s in enumerate(samplers):
        g.start(s, cx.new_sample_device(bench.PLANAR_F32, 2, F, src[v].data_ptr()))
    assert cx.plan_kind() == 1 and len(g.spatial) == V
    return cx, g.spatial


def measure(fa, torch, shard, args):
    import numpy as np

    V, B, K_BIG, F, _ = bench.DEFAULTS["cfg2"]
    K_MSG = max(1, RING // (V * MSGS_PER_POSITION) - 1)      # nine messages per voice per block, and room for the ring's one empty slot
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = bench.shard_sources(torch, shard, 0, V, F, dev)
    out = torch.empty(K_BIG * B * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    configs = [("rest_k768", "rest", K_BIG), ("move_k768", "move", K_BIG), ("rest_k%d" % K_MSG, "rest", K_MSG),
               ("move_k%d" % K_MSG, "move", K_MSG), ("steps_k%d" % K_MSG, "steps", K_MSG)]
    if args.only:
        configs = [c for c in configs if c[0] == args.only]
    line = {"workload": "cfg2_spatial", "voices": V, "block": B, "steps": args.steps, "rounds": args.rounds,
            "voices_the_ring_lets_through_per_call": {"k%d" % K_BIG: RING // (K_BIG * MSGS_PER_POSITION), "k%d" % K_MSG: min(V, RING // (K_MSG * MSGS_PER_POSITION)),
                                                      "k1": min(V, (RING - 1) // MSGS_PER_POSITION)},
            "configs": {}}
    for name, how, K in configs:
        cx, spatial = make(fa, V, B, K, F, src, stream)
        L = cx.L
        # the game's side of a moving source today: a new position for every voice at every block of the call, sent as ONE list
        # (fwgpu_node_set_params), so that the timed region holds the queueing but no per-message call overhead
        m_nodes = np.repeat(np.repeat(np.asarray(spatial, dtype=np.int64), K), 3)
        m_params = np.tile(np.arange(3, dtype=np.int32), V * K)
        m_at = np.repeat(np.tile(np.arange(K, dtype=np.uint32), V), 3)
        as_ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))

        def step(n, msgs=False):
            t0 = time.perf_counter()
            for i in range(n):
                if msgs:
                    x = (2.0 + 1e-3 * ((i * K + m_at) % 64)).astype(np.float32)
                    vals = np.where(m_params == 0, x, np.where(m_params == 1, np.float32(0.5), np.float32(-3.0))).astype(np.float32)
                    cx._check(L.fwgpu_node_set_params(cx.c, 3 * V * K, as_ptr(m_nodes, C.c_int64), as_ptr(m_params, C.c_int), as_ptr(vals, C.c_float),
                                                      as_ptr(m_at, C.c_uint32)))
                cx.process_blocks_device(K, out.data_ptr(), 2)
            cx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        def arm():
            if how != "move":
                return
            for node in spatial:      # back to the voice's own position, then into a move that outlasts the round
                cx._check(L.fwgpu_spatial_move(cx.c, node, 2.0, 0.5, -3.0, 0, 0))
                cx._check(L.fwgpu_spatial_move(cx.c, node, -2.0, 0.5, -3.0, MOVE_FRAMES, 0))
            step(1)

        assert (args.steps + 1) * K * B < MOVE_FRAMES, "a round must end inside the move"
        t0 = time.perf_counter()
        arm()
        step(2)
        while (time.perf_counter() - t0) * 1e3 < bench.OTHER_WARM_MS:
            step(1)
        rounds, ctl = [], 0
        for _ in range(args.rounds):
            arm()
            a = cx.lazy_stats()
            rounds.append(step(args.steps, msgs=how == "steps"))
            ctl += cx.lazy_stats()[1] - a[1]
        med = sorted(rounds)[len(rounds) // 2]
        n = args.steps * args.rounds
        rec = {"blocks_per_step": K, "ms_per_step": round(med, 4), "us_per_block": round(med * 1e3 / K, 3),
               "rounds_ms": [round(x, 4) for x in rounds], "control_batches_per_step": round(ctl / n, 3), "plan_kind": cx.plan_kind(),
               "includes_the_message_list_call": how == "steps"}
        if how == "move":
            # bytes of a move block per voice: the source (2 channels), the piece's 64 frames of history read again, the four per-frame
            # rows (two gains, two delays) written by the control kernel and read by the leaf kernel; the step holds both kernels
            per_block = V * (2 * B * 4 + 2 * 64 * 4 + 2 * 4 * B * 4)
            rec["hbm_bytes_per_block"] = per_block
            rec["share_of_hbm_roofline_whole_step"] = round(per_block * K / (med * 1e-3) / HBM_BYTES_PER_S, 4)
        line["configs"][name] = rec
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
