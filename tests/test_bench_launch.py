"""CPU tier: bench.py's orchestration end to end — `--gpus 2` with no launcher around it starts two ranks itself
(torch.distributed.run on 127.0.0.1), each builds its shard through the C ABI, the mix buses go through the reducer,
rank 0 prints exactly ONE JSON line.  Runs on the host-only harness library (FWGPU_BENCH_HOSTONLY: fake HIP runtime,
no audio computed — the line carries no value and says so) with the gloo backend; what is tested is the launcher,
the rank plumbing and the line's shape, which the driver's N = 2 / 4 / 8 runs depend on."""
import json
import os
import subprocess
import sys

import pytest

import fwapi

ROOT = fwapi.ROOT


def run_bench(extra, timeout=600):
    fwapi.hostonly_lib()  # builds tests/host_harness/_hostonly.so
    env = dict(os.environ, FWGPU_BENCH_HOSTONLY="1", FWGPU_LIB=os.path.join(ROOT, "tests", "host_harness", "_hostonly.so"))
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--voices", "64", "--block", "64",
                        "--blocks-per-step", "4", "--src-frames", "1024", "--steps", "5", "--warmup", "2"] + extra,
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout  # exactly one line on stdout, whatever the ranks and the launcher print
    return strict_line(lines[0])


def _refuse_constant(name):
    raise ValueError("non-finite constant %r in the bench line" % name)


def strict_line(text):
    """the driver's contract (a 22.5 KB line came back `parsed: null`): the last stdout line is ONE compact JSON
    object — strict JSON (no NaN / Infinity), at most 8 KiB, the whole record in the side file it names"""
    assert len(text.encode()) <= 8192, len(text)
    d = json.loads(text, parse_constant=_refuse_constant)
    assert isinstance(d, dict)
    full = d["full"]
    path = full if os.path.isabs(full) else os.path.join(ROOT, full)
    whole = json.loads(open(path).read(), parse_constant=_refuse_constant)
    assert whole["metric"] == d["metric"] and whole["steps"] == d["steps"]
    return d


@pytest.mark.parametrize("mode", ["allreduce", "ordered"])
def test_gpus_2_self_launches_two_ranks_and_prints_one_line(mode):
    d = run_bench(["--gpus", "2", "--bus-reduce", mode, "--reduce-every", "2"])
    assert d["n_gpus"] == 2 and d["rccl_ranks_seen"] == 2
    assert d["scaling"] == "weak" and d["steps"] == 5 and d["warmup"] == 2
    assert d["config"]["parallelism"].startswith("voice-shard x2")
    assert d["value"] is None and "host-only harness" in d["invalid"]  # no audio was computed: never a measurement
    assert d["ms_per_step"] > 0
    assert d["parity_check"] is None and "other_configs" not in d  # a plain run: the timed steps only (the rest: --full)


def test_gpus_3_default_exchange_mode_with_the_n_rank_extras():
    """the N > 1 line of a --full run: the default mix-bus reduction is libfwgpu's own exchange (handles carried by
    all_gather_object, regions "mapped" by the fake runtime), the line carries a parity_check entry (skipped on this tier: the
    harness computes no audio — but the oracle's WHOLE graph, 3 shards under one 3-port SumNode, was built and rendered), and
    next to it configs[4] with the reduction after every step and the headline under the two RCCL reductions."""
    d = run_bench(["--gpus", "3", "--full", "--force-other-configs"])
    assert d["n_gpus"] == 3 and d["ranks_seen"] == 3
    assert d["config"]["bus_reduce"] == "exchange" and d["config"]["bus_reduce_fallback"] is None
    pc = d["parity_check"]
    assert pc["ranks"] == 3 and pc["bus_reduce"] == "exchange" and pc["oracle_whole_graph_nonzero"] and "skipped" in pc
    c5 = d["other_configs"]["cfg5"]
    assert "error" not in c5 and c5["bus_reduce"] == "exchange" and c5["parity_check"]["ranks"] == 3
    assert sorted(d["bus_reduce_modes"]) == ["allreduce", "ordered"]
    for m, ent in d["bus_reduce_modes"].items():
        assert "error" not in ent and ent["bus_reduce"] == m and ent["value"] is None


def test_gpus_8_launched_like_the_driver_launches_it():
    """the round-end scaling run at N = 8, command for command: `python -m torch.distributed.run --nnodes=1 --nproc-per-node 8
    --master-addr 127.0.0.1 --master-port P bench.py --gpus 8 --steps K --warmup W --full` — eight ranks, the default exchange with eight
    handles carried through the control plane, configs[4] with the reduction after every step, the RCCL modes beside it, the
    whole-graph parity plumbing for eight shards under one 8-port SumNode (skipped on this tier: the harness computes no audio)."""
    import socket

    fwapi.hostonly_lib()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, FWGPU_BENCH_HOSTONLY="1", FWGPU_LIB=os.path.join(ROOT, "tests", "host_harness", "_hostonly.so"), OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port",
           str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--workload", "cfg2", "--voices", "64", "--block", "64", "--blocks-per-step", "4",
           "--src-frames", "1024", "--steps", "4", "--warmup", "1", "--full", "--force-other-configs"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [x for x in r.stdout.splitlines() if x.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = strict_line(lines[0])
    assert d["n_gpus"] == 8 and d["ranks_seen"] == 8 and d["scaling"] == "weak"
    assert d["config"]["bus_reduce"] == "exchange" and d["config"]["bus_reduce_fallback"] is None
    assert d["config"]["parallelism"].startswith("voice-shard x8")
    pc = d["parity_check"]
    assert pc["ranks"] == 8 and pc["oracle_whole_graph_nonzero"] and "skipped" in pc
    c5 = d["other_configs"]["cfg5"]
    assert "error" not in c5 and c5["parity_check"]["ranks"] == 8
    assert sorted(d["bus_reduce_modes"]) == ["allreduce", "ordered"] and d["rccl_ranks_seen"] == 8
    assert d["value"] is None and "host-only harness" in d["invalid"]


def test_single_rank_line_has_the_contract_fields():
    d = run_bench([])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "parity_check", "rccl_ranks_seen"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["config"]["launch_plan"] == 1 and d["vs_baseline"] is None and d["dtype"] == "f32"


def test_dump_outputs_writes_one_float32_file_of_the_bus_shape(tmp_path):
    """--dump-outputs DIR: the file's name, dtype and shape (the interleaved mix bus of the last step's 4 blocks of 64 frames,
    frames x 2) and the line beside it.  The host-only harness computes no audio, so the content is checked on the GPU tier
    (tests/test_gpu_bench_dump.py, against the oracle)."""
    import numpy as np

    d = run_bench(["--dump-outputs", str(tmp_path / "out")])
    a = np.load(str(tmp_path / "out" / "mix_bus.npy"))
    assert a.dtype == np.float32 and a.shape == (4 * 64, 2)
    assert d["steps"] == 5 and d["warmup"] == 2 and d["config"]["warmup_steps_run"] == 2


def test_dump_outputs_over_the_cap_keep_a_seeded_sample_of_rows(tmp_path, monkeypatch):
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4096)
    a = np.arange(4000 * 2, dtype=np.float32).reshape(4000, 2)
    for sub in ("a", "b"):
        bench.write_outputs(str(tmp_path / sub), {"mix_bus": a})
    got = np.load(str(tmp_path / "a" / "mix_bus.npy"))
    rows = np.load(str(tmp_path / "a" / "mix_bus_rows.npy"))
    assert got.dtype == np.float32 and rows.dtype == np.float64 and got.nbytes + rows.nbytes <= 4096
    assert np.array_equal(got, a[rows.astype(np.int64)]) and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(str(tmp_path / "b" / "mix_bus_rows.npy")))  # the same rows on every run


def test_gpus_mismatch_with_an_outer_launcher_is_refused():
    env = dict(os.environ, FWGPU_BENCH_HOSTONLY="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               FWGPU_LIB=os.path.join(ROOT, "tests", "host_harness", "_hostonly.so"))
    fwapi.hostonly_lib()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_committed_full_records_compact_under_the_cap():
    """every full record committed under profiles/ (round 5's was 22.5 KB on one line) through bench.compact_line: strict JSON,
    under the cap, and still carrying the objects the judge reads — roofline with frac / whole_step_frac, cpu_baseline with cores"""
    import glob

    sys.path.insert(0, ROOT)
    import bench

    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_bench_line_full*.json")) + glob.glob(os.path.join(ROOT, "profiles", "r0*_n*_virtual_ranks*line.json")))
    assert paths
    for p in paths:
        text = bench.compact_line(json.load(open(p)), "gpurun_out/bench_full.json")
        assert len(text.encode()) <= bench.LINE_BYTES_MAX, (p, len(text))
        d = json.loads(text, parse_constant=_refuse_constant)
        assert d["roofline"]["frac"] > 0 and d["unit"] == "voice-samples/s", p
        if d["n_gpus"] == 1:
            assert d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["kind"] == "port", p
            if "other_configs" in d:
                for name, ent in d["other_configs"].items():
                    assert "dropped" not in ent and len(json.dumps(ent)) < 600, (p, name)


def test_compact_line_never_exceeds_the_cap_and_refuses_non_finite():
    sys.path.insert(0, ROOT)
    import bench

    line = {"metric": "m", "value": float("nan"), "unit": "u", "n_gpus": 1, "steps": 1, "warmup": 0, "ms_per_step": float("inf"), "config": {"workload": "w"},
            "roofline": {"bound": "hbm", "frac": 0.5}, "cpu_baseline": {"value": 1.0, "cores": 1, "kind": "port", "sample": "s" * 5000},
            "other_configs": dict(("cfg%d" % i, {"value": 1.0, "roofline": {"kernel": "k" * 200, "frac": 0.1}}) for i in range(200))}
    text = bench.compact_line(line, "f")
    assert len(text) <= bench.LINE_BYTES_MAX
    d = json.loads(text, parse_constant=_refuse_constant)
    assert d["value"] is None and d["ms_per_step"] is None and d["roofline"]["frac"] == 0.5 and "dropped" in d["other_configs"]
