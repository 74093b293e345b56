"""GPU tier (-m gpu): what `bench.py --dump-outputs` writes is what the timed path computed in its last step — bit for bit against
the oracle, on a single rank and on two ranks (the default exchange, two processes on one device: --share-device), where it must be
the REDUCED bus of the whole graph, not rank 0's own shard."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import fwapi

ROOT = fwapi.ROOT
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

# a small config-2 shape: 64 voices per rank, blocks of 64 frames, 4 blocks per step, 1152 frames of looping source per voice (the
# last timed step reads frames 1024..1151 and 0..127: an offset no other step of the run starts at, across the loop's end)
V, B, K, F, STEPS, WARMUP = 64, 64, 4, 1152, 3, 2
ARGS = types.SimpleNamespace(master=False, voice_fx=False)


def run_dump(tmp_path, extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FWGPU_BENCH_HOSTONLY"):
        env.pop(k, None)
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--voices", str(V), "--block", str(B),
                        "--blocks-per-step", str(K), "--src-frames", str(F), "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--dump-outputs", out] + extra, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    got = np.load(os.path.join(out, "mix_bus.npy"))
    assert got.dtype == np.float32 and got.shape == (K * B, 2)
    return got


def last_step_sources(rank):
    """rank's sources as the oracle must see them: the K x B frames the last timed step read.  Every voice loops over its F
    frames and has played WARMUP + STEPS - 1 steps of K blocks before that step."""
    import torch

    from firewheel_amd import shard

    src = bench.shard_sources(torch, shard, rank, V, F, "cuda")
    p0 = (WARMUP + STEPS - 1) * K * B % F
    idx = torch.arange(p0, p0 + K * B, device="cuda") % F
    return src[:, :, idx].cpu().numpy()


def test_dump_is_the_last_timed_steps_mix_bus(tmp_path):
    got = run_dump(tmp_path, [])
    o, _, _ = bench.make_oracle("cfg2", V, B, 32, 0, ARGS, last_step_sources(0))
    ref = np.asarray(o.e.process_blocks(K), dtype=np.float32).reshape(-1)
    assert np.any(ref)
    assert np.array_equal(got.reshape(-1).view(np.uint32), ref.view(np.uint32))


def test_two_rank_dump_is_the_reduced_bus_of_the_whole_graph(tmp_path):
    got = run_dump(tmp_path, ["--gpus", "2", "--share-device"])
    o = bench.make_oracle_whole("cfg2", 2, V, B, 32, ARGS, [last_step_sources(r) for r in range(2)])
    ref = np.asarray(o.e.process_blocks(K), dtype=np.float32).reshape(-1)
    own, _, _ = bench.make_oracle("cfg2", V, B, 32, 0, ARGS, last_step_sources(0))
    assert not np.array_equal(ref, np.asarray(own.e.process_blocks(K), dtype=np.float32).reshape(-1))  # the test can tell them apart
    assert np.array_equal(got.reshape(-1).view(np.uint32), ref.view(np.uint32))  # the exchange is rank-ordered: bit-exact
