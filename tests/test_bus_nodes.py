"""The host harness and the bus nodes with a kernel of their own (limiter, ducker, latency-compensation delay): what its launch stubs
hold the plan build to — launch bits that are the OR over each level's nodes, states their kernels render (fwgpu_types.h X_state_ok)
and ext slices of exactly the length the kernels index (X_ext_len), inside the pool.  CPU tier only."""
import numpy as np
import pytest

import fwapi
from busnodes import DELAY_COMP, DUCKER, LIMITER, METER
from fwapi import HostOnlyEngine


def test_the_harness_checks_catch_each_mistake_and_pass_each_kind():
    L = fwapi.hostonly_lib()
    before = L.fwh_violation()
    assert L.fwh_selftest_bus_checks() == 0
    assert L.fwh_violation() == before     # (the self-test puts the string back)
    L.fwh_launch_reset()


KINDS = ["volume", "biquad", "meter", "limiter", "ducker", "dcomp"]
BUS = KINDS[3:]


def _random_node(e, rng, n, kinds=KINDS):
    """-> (node, key channels, kind): n main channels in and out (a ducker: k key channels more in), valid random parameters, the caps
    among them"""
    kind = str(rng.choice(kinds))
    pick = lambda *values: float(rng.choice(values))
    if kind == "volume":
        return e.volume(float(rng.uniform(10, 100)), ch=n), 0, kind
    if kind == "biquad":
        return e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 8000)), ch=n), 0, kind
    if kind == "meter":
        return e.add_node(METER, n, n, [pick(1, 7, 1024, 65536)]), 0, kind
    if kind == "limiter":
        return e.add_node(LIMITER, n, n, [pick(0.001, 0.5, 1000.0), pick(0, 1, 128, 1919, 1920)]), 0, kind
    if kind == "dcomp":
        return e.add_node(DELAY_COMP, n, n, [pick(0, 1, 63, 64, 200, 8191, 8192)]), 0, kind
    k = int(rng.choice([1, 2, 8]))
    windows = (1, 7, 64, 333, 32767, 32768)
    return e.add_node(DUCKER, n + k, n, [pick(1e-6, 0.05, 1000.0), pick(0.0, 0.25, 1.0), pick(*windows), pick(*windows), pick(0, *windows)]), k, kind


@pytest.mark.parametrize("seed", range(40))
def test_bus_nodes_random_graphs_leave_no_violation(seed):
    """graph_in -> 2..6 nodes in series -> graph_out (a ducker's key channels come from the graph inputs behind the main ones), calls
    of ragged length, and mid-way a bus node taken out of the chain or put into it"""
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.choice([1, 2, 3, 8]))
    mbf = int(rng.choice([64, 96, 256]))
    e = HostOnlyEngine(max_block_frames=mbf, num_graph_inputs=n + 8, num_graph_outputs=n, max_batch=int(rng.choice([1, 3, 64])))
    chain = [_random_node(e, rng, n) for _ in range(int(rng.integers(2, 7)))]

    def wire(edge):
        """e.connect or e.disconnect: graph_in -> chain -> graph_out"""
        cur = e.graph_in_node
        for node, k, _ in chain + [(e.graph_out_node, 0, "")]:
            for c in range(n):
                edge(cur, c, node, c)
            for c in range(k):
                edge(e.graph_in_node, n + c, node, n + c)
            cur = node

    def calls(count):
        for _ in range(count):
            frames = int(rng.choice([1, 17, mbf - 1, mbf, 2 * mbf + 5, 3 * mbf, 5 * mbf, 7 * mbf + 37]))
            e.process_interleaved(frames, n_out_ch=n, inp=np.zeros(frames * (n + 8), dtype=np.float32), n_in_ch=n + 8)
            assert e.violation() == "", (seed, frames)

    try:
        wire(e.connect)
        e.update()
        calls(4)
        wire(e.disconnect)
        bus = [i for i, (_, _, kind) in enumerate(chain) if kind in BUS]
        if bus and rng.uniform() < 0.5:
            e.remove_node(chain.pop(int(rng.choice(bus)))[0])
        else:
            chain.insert(int(rng.integers(0, len(chain) + 1)), _random_node(e, rng, n, BUS))
        wire(e.connect)
        e.update()
        calls(4)
    finally:   # (the harness' report and counts are the process's: nothing of this test may reach the tests behind it)
        fwapi.hostonly_lib().fwh_violation_reset()
        e.reset_launches()
