"""Latency compensation: the delay node (FWGPU_DELAY_COMP = 19; SPEC) and the graph latency queries.

The reference for sample values and silence flags is `model(x, flags, D, block_lengths)` below: a shift by D frames plus the SPEC's
counter rule, applied to the whole stream since the node's activation and sliced per call.  What the model takes as input is obtained
without the node: the stream input itself, or the OracleEngine's output of the same graph built without the node (the oracle does not
know the kind).  Every comparison on the GPU tier is `fwapi.bits` equality.

CPU tier: the model against a per-frame brute force; shapes and the creation parameter on the host-only harness; the latency queries
and compensate_latency; the planner on the harness; the typed Python mirror, the header and the generated ffi.rs.

GPU tier: G1 stream graphs on the level executor, G2 silence flags, G3 a limited bus and its compensated dry copy, G4 a delayed
sub-mix beside fused voice banks, G5 graph edits, G6 fwgpu_node_process, G7 a level shared with a limiter, a biquad and a volume (and,
in a case of its own, a ducker).
"""
import os
import re

import numpy as np
import pytest

import fwapi
import scenarios
from busnodes import CHAIN, DELAY_COMP, DRY, DUCKER, LB_DELAY_COMP, LB_LEVEL, LIMITER, _host, _start, _voice, assert_bits, bank, harness_run, planar
from fwapi import LOOP_FULL, GpuEngine, HostOnlyEngine, OracleEngine

INVALID = -20
COMPILE_CYCLE = -10
DMAX = 8192
F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ------------------------------------------------------------------------------------------------ the SPEC in numpy
def model(x, flags, D, block_lengths):
    """x: [channels][frames] since the node's activation; flags: [channels][blocks], True where the input channel is flagged silent
    for the block; block_lengths: frames per block -> (y of x's shape, out_flags of flags' shape)"""
    x = np.asarray(x, dtype=F32)
    n, N = x.shape
    flags = np.zeros((n, len(block_lengths)), dtype=bool) if flags is None else np.asarray(flags, dtype=bool)
    starts = np.concatenate([[0], np.cumsum(block_lengths)]).astype(np.int64)
    assert starts[-1] == N and flags.shape == (n, len(block_lengths))
    seen = x.copy()
    out_flags = np.zeros_like(flags)
    for c in range(n):
        loud = 0
        for k, F in enumerate(block_lengths):
            if flags[c, k]:
                seen[c, starts[k]:starts[k + 1]] = F32(0.0)      # counts as +0.0
                out_flags[c, k] = loud == 0
                loud = max(0, loud - int(F))
            else:
                loud = D
    y = np.concatenate([np.zeros((n, D), dtype=F32), seen], axis=1)[:, :N]     # x[n - D], +0.0 in front
    return y, out_flags


def brute(x, flags, D, block_lengths):
    """the same, one frame and one block at a time, as the SPEC's sentences read"""
    n, N = x.shape
    starts = np.concatenate([[0], np.cumsum(block_lengths)]).astype(np.int64)
    block_of = np.repeat(np.arange(len(block_lengths)), block_lengths)
    y = np.zeros((n, N), dtype=F32)
    out_flags = np.zeros((n, len(block_lengths)), dtype=bool)
    for c in range(n):
        for f in range(N):
            s = f - D
            if s >= 0 and not flags[c, block_of[s]]:
                y[c, f] = x[c, s]
        for k in range(len(block_lengths)):
            # flagged exactly when the block itself and every block that holds one of the D frames in front of it were flagged
            window = range(max(0, int(starts[k]) - D), int(starts[k]))
            out_flags[c, k] = flags[c, k] and all(flags[c, block_of[s]] for s in window)
    return y, out_flags


def special_noise(rng, n, N):
    """noise with -0.0, both infinities, subnormals and a NaN with a payload sprinkled in: a copy keeps every bit"""
    x = rng.uniform(-1.0, 1.0, size=(n, N)).astype(F32)
    u = fwapi.bits(x).copy()
    where = rng.integers(0, N, size=(n, max(8, N // 10)))
    words = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7FC01234, 0x00000000], dtype=np.uint32)
    for c in range(n):
        u[c, where[c]] = words[np.arange(where.shape[1]) % len(words)]
    return u.view(F32).reshape(n, N)


# ================================================================================================ CPU tier: the model
RAGGED = [64, 64, 17, 1, 64, 64, 64, 5, 64, 64, 64, 64, 30, 64, 64, 64]


def _random_flags(rng, n, blocks):
    """runs of flagged blocks of every length, and channels that start flagged"""
    fl = np.zeros((n, blocks), dtype=bool)
    for c in range(n):
        k = 0 if c % 2 else int(rng.integers(0, 3))
        while k < blocks:
            run = int(rng.integers(1, 6))
            if rng.uniform() < 0.5:
                fl[c, k:k + run] = True
            k += run
    return fl


@pytest.mark.parametrize("D", [0, 1, 63, 64, 100, 200])
def test_model_equals_the_brute_force_evaluation(D):
    rng = np.random.default_rng(3 + D)
    x = special_noise(rng, 3, sum(RAGGED))
    fl = _random_flags(rng, 3, len(RAGGED))
    y, of = model(x, fl, D, RAGGED)
    by, bf = brute(x, fl, D, RAGGED)
    assert_bits(y, by, "D %d" % D)
    assert np.array_equal(of, bf), (D, of, bf)
    assert fl.any() and not fl.all() and (of.any() or D > 150)


def test_model_with_a_delay_of_zero_is_the_identity():
    rng = np.random.default_rng(4)
    x = special_noise(rng, 2, sum(RAGGED))
    y, of = model(x, None, 0, RAGGED)
    assert_bits(y, x, "D 0")
    assert not of.any()
    fl = _random_flags(rng, 2, len(RAGGED))
    y, of = model(x, fl, 0, RAGGED)
    assert np.array_equal(of, fl)      # nothing lingers: flagged in, flagged out


@pytest.mark.parametrize("D", [1, 63, 200, 1000])
def test_model_never_flags_a_block_that_holds_a_nonzero_sample(D):
    rng = np.random.default_rng(5 + D)
    x = rng.uniform(0.5, 1.0, size=(4, sum(RAGGED))).astype(F32)     # no zero anywhere
    fl = _random_flags(rng, 4, len(RAGGED))
    y, of = model(x, fl, D, RAGGED)
    starts = np.concatenate([[0], np.cumsum(RAGGED)])
    for c in range(4):
        for k in range(len(RAGGED)):
            blk = y[c, starts[k]:starts[k + 1]]
            if of[c, k]:
                assert not fwapi.bits(blk).any(), (c, k)
            elif fl[c, k] and not blk.any():
                # conservative only where a block that was heard overlaps the D frames in front of this one
                lo = max(0, starts[k] - D)
                assert any(not fl[c, j] and starts[j + 1] > lo for j in range(k)), (c, k)


# ================================================================================================ CPU tier: shapes and the parameter
@pytest.mark.parametrize("n_in,n_out", [(0, 0), (9, 9), (2, 1), (1, 2)])
def test_shapes_refused_at_add_node(n_in, n_out):
    e, _ = _host()
    with pytest.raises(e.fa.FwgpuError) as ei:
        e.add_node(DELAY_COMP, n_in, n_out, [63.0])
    assert ei.value.code == INVALID and "DelayCompNode" in str(ei.value)
    e.update()  # nothing was added


@pytest.mark.parametrize("params", [[float("nan")], [0.5], [-1.0], [8193.0], [float("inf")]])
def test_frames_refused_at_update(params):
    e, v = _host()
    m = e.add_node(DELAY_COMP, 2, 2, params)
    for _ in range(2):  # (still there, still refused)
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.update()
        assert ei.value.code == INVALID and "DelayCompNode" in str(ei.value)
    e.remove_node(m)
    good = e.add_node(DELAY_COMP, 2, 2, [63.0])
    e.connect_stereo(v, good)
    e.update()  # the graph is usable


@pytest.mark.parametrize("params,D", [([], 63), ([0.0], 0), ([1.0], 1), ([63.0], 63), ([8192.0], 8192)])
@pytest.mark.parametrize("n", [1, 8])
def test_frames_and_shapes_accepted_and_set_param_refused(params, D, n):
    e, _ = _host()
    m = e.add_node(DELAY_COMP, n, n, params)
    assert e.cx.node_latency(m) == D
    e.update()
    assert e.cx.plan_node_level(m) >= 0
    with pytest.raises(e.fa.FwgpuError) as ei:
        e.set_param(m, 0, 5.0)
    assert ei.value.code == INVALID and "DelayCompNode" in str(ei.value)


# ================================================================================================ CPU tier: the latency queries
def test_node_latency_of_every_kind():
    e, v = _host()
    smp = e.new_sample(fwapi.PLANAR_F32, 2, scenarios.voice_source(3, 256, 2))
    assert e.cx.node_latency(e.add_node(LIMITER, 2, 2, [1.0, 0.0])) == 63
    assert e.cx.node_latency(e.add_node(LIMITER, 1, 1, [0.5, 1920.0])) == 63
    for D in (0, 1, 63, 8192):
        assert e.cx.node_latency(e.add_node(DELAY_COMP, 2, 2, [float(D)])) == D
    others = {0: (2, 2, []), 1: (0, 2, []), 2: (2, 2, []), 3: (4, 2, []), 4: (0, 2, []), 5: (2, 2, []), 6: (1, 2, []), 7: (2, 1, []), 8: (2, 2, []),
              9: (2, 2, []), 10: (2, 2, []), 11: (2, 2, [63.0 / 48000.0, 0.0, 1.0]), 12: (2, 2, [float(smp)]), 13: (0, 2, [float(smp)]),
              14: (1, 2, []), 15: (2, 2, []), 16: (2, 2, []), DUCKER: (4, 2, [])}
    assert sorted(others) == [k for k in range(20) if k not in (LIMITER, DELAY_COMP)]
    for kind, (n_in, n_out, params) in others.items():
        assert e.cx.node_latency(e.add_node(kind, n_in, n_out, params)) == 0, kind    # FWGPU_DELAY (11) is an effect, not latency
    assert e.cx.node_latency(e.graph_out_node) == 0 and e.cx.node_latency(v) == 0
    gone = e.add_node(DELAY_COMP, 2, 2, [5.0])
    e.remove_node(gone)
    for bad in (gone, 12345 << 32, -1):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.cx.node_latency(bad)
        assert ei.value.code == INVALID


def _stream(n_in=2, n_out=2, mbf=64):
    return HostOnlyEngine(max_block_frames=mbf, num_graph_inputs=n_in, num_graph_outputs=n_out)


def _limiter(e, src, ch=2, sport0=0):
    lim = e.add_node(LIMITER, ch, ch, [1.0, 0.0])
    for c in range(ch):
        e.connect(src, sport0 + c, lim, c)
    return lim


def test_report_a_limited_bus_summed_with_its_dry_copy():
    e = _stream()
    lim = _limiter(e, e.graph_in_node)
    s = e.sum(2)
    e.connect_stereo(lim, s, 0)
    e.connect_stereo(e.graph_in_node, s, 2)
    e.connect_stereo(s, e.graph_out_node)
    # no update() yet: the queries read the edge set
    assert e.cx.latency_report() == [(s, 2, 63), (s, 3, 63)]
    assert e.cx.output_latency() == 63
    e.update()
    assert e.cx.latency_report() == [(s, 2, 63), (s, 3, 63)]


def test_report_b_two_limiters_in_series_against_dry():
    e = _stream()
    l2 = _limiter(e, _limiter(e, e.graph_in_node))
    s = e.sum(2)
    e.connect_stereo(l2, s, 0)
    e.connect_stereo(e.graph_in_node, s, 2)
    e.connect_stereo(s, e.graph_out_node)
    assert e.cx.latency_report() == [(s, 2, 126), (s, 3, 126)]
    assert e.cx.output_latency() == 126


def test_report_c_a_diamond_of_equal_latencies_is_empty():
    e = _stream()
    a, b = _limiter(e, e.graph_in_node), e.add_node(DELAY_COMP, 2, 2, [63.0])
    e.connect_stereo(e.graph_in_node, b)
    s = e.sum(2)
    e.connect_stereo(a, s, 0)
    e.connect_stereo(b, s, 2)
    e.connect_stereo(s, e.graph_out_node)
    assert e.cx.latency_report() == []
    assert e.cx.output_latency() == 63


def test_report_d_a_ducker_whose_key_passes_a_limiter():
    e = _stream(n_in=4)
    lim = _limiter(e, e.graph_in_node, sport0=2)
    d = e.add_node(DUCKER, 4, 2, [])
    e.connect_stereo(e.graph_in_node, d, 0)
    e.connect_stereo(lim, d, 2)
    e.connect_stereo(d, e.graph_out_node)
    assert e.cx.latency_report() == [(d, 0, 63), (d, 1, 63)]     # the main ports wait for the key
    assert e.cx.output_latency() == 63


def test_report_e_a_cap_smaller_than_the_count():
    import ctypes as C

    from firewheel_amd import _lib as flib

    e = _stream(n_in=8, n_out=2)
    lim = _limiter(e, e.graph_in_node)
    s = e.sum(4)
    e.connect_stereo(lim, s, 0)
    for p in range(1, 4):
        e.connect_stereo(e.graph_in_node, s, 2 * p, 2 * p)
    e.connect_stereo(s, e.graph_out_node)
    full = e.cx.latency_report()
    assert full == [(s, p, 63) for p in range(2, 8)]
    L = e.cx.L
    buf = (flib.LatencySkew * 8)()
    for i in range(8):
        buf[i].node, buf[i].port, buf[i].lead_frames = -7, 77, 777
    assert L.fwgpu_graph_latency_report(e.cx.c, buf, 4) == 6
    assert [(buf[i].node, buf[i].port, buf[i].lead_frames) for i in range(4)] == full[:4]
    assert [(buf[i].node, buf[i].port, buf[i].lead_frames) for i in range(4, 8)] == [(-7, 77, 777)] * 4     # nothing past the cap
    assert L.fwgpu_graph_latency_report(e.cx.c, None, 0) == 6
    assert L.fwgpu_graph_latency_report(e.cx.c, None, 3) == INVALID


def test_report_f_unconnected_ports_are_ignored():
    e = _stream()
    lim = _limiter(e, e.graph_in_node)
    s = e.sum(3)                      # ports 4, 5 stay open
    e.connect_stereo(lim, s, 0)
    e.connect(e.graph_in_node, 0, s, 2)      # and so does port 3
    e.connect_stereo(s, e.graph_out_node)
    lone = e.add_node(LIMITER, 2, 2, [])     # a limiter nothing feeds and nothing reads
    assert e.cx.latency_report() == [(s, 2, 63)]
    assert e.cx.output_latency() == 63 and e.cx.node_latency(lone) == 63


def test_report_g_compensate_latency_empties_the_report_once():
    e = _stream(n_in=4, n_out=4)
    gi, go = e.graph_in_node, e.graph_out_node
    l1 = _limiter(e, gi)
    l2 = _limiter(e, l1)
    s = e.sum(3)
    e.connect_stereo(l2, s, 0)      # 126 late
    e.connect_stereo(l1, s, 2)      # 63 late
    e.connect_stereo(gi, s, 4)      # on time
    e.connect_stereo(s, go, 0)
    e.connect_stereo(gi, go, 2, 2)  # graph_out's own ports are skewed too
    assert e.cx.latency_report() == [(go, 2, 126), (go, 3, 126), (s, 2, 63), (s, 3, 63), (s, 4, 126), (s, 5, 126)]
    before = e.cx.output_latency()
    assert before == 126
    added = e.cx.compensate_latency()
    assert len(added) == 3          # one stereo node per (source, destination, lead)
    assert sorted(e.cx.node_latency(a) for a in added) == [63, 126, 126]
    assert all(isinstance(e.cx.node(a), e.fa.DelayCompNode) and e.cx.node(a).channels == 2 for a in added)
    assert e.cx.latency_report() == [] and e.cx.output_latency() == before
    assert e.cx.compensate_latency() == []
    e.update()
    assert all(e.cx.plan_node_level(a) >= 0 for a in added)


def test_report_g_wide_and_long_leads_are_split():
    """nine mono edges that share source, destination and lead take two nodes (8 + 1 channels); a lead beyond 8192 takes nodes in series"""
    import firewheel_amd as fa

    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=10, num_graph_outputs=1)
    gi, go = cx.graph_in_node(), cx.graph_out_node()
    cur = gi
    for _ in range(131):            # 131 x 63 = 8253 frames
        lim = cx.add_node(1, 1, fa.LimiterNode(1.0, 0, channels=1))
        cx.connect(cur, 0, lim, 0)
        cur = lim
    s = cx.add_node(10, 1, fa.SumNode())
    cx.connect(cur, 0, s, 0)
    for p in range(1, 10):
        cx.connect(gi, p, s, p)
    cx.connect(s, 0, go, 0)
    assert cx.latency_report() == [(s, p, 8253) for p in range(1, 10)]
    added = cx.compensate_latency()
    assert sorted((cx.node(a).channels, cx.node_latency(a)) for a in added) == [(1, 61), (1, 8192), (8, 61), (8, 8192)]
    assert cx.latency_report() == [] and cx.output_latency() == 8253 and cx.compensate_latency() == []
    cx.update()
    cx.close()


def test_report_h_a_cycle_returns_the_compile_error():
    e = _stream()
    a, b = e.volume(50.0), e.volume(50.0)
    e.connect(e.graph_in_node, 0, a, 0)
    e.connect(a, 0, b, 0, check_for_cycles=False)
    e.connect(b, 0, a, 1, check_for_cycles=False)       # a -> b -> a
    e.connect_stereo(b, e.graph_out_node)
    with pytest.raises(fwapi.CompileGraphError) as ei:
        e.update()
    assert ei.value.code == COMPILE_CYCLE
    for call in (e.cx.latency_report, e.cx.output_latency, e.cx.compensate_latency):
        with pytest.raises(e.fa.CompileGraphError) as ei:
            call()
        assert ei.value.code == COMPILE_CYCLE
    assert e.cx.L.fwgpu_graph_latency_report(e.cx.c, None, 0) == COMPILE_CYCLE
    assert e.cx.node_latency(a) == 0                     # a node's own latency needs no order


# ================================================================================================ the desk: a delayed sub-mix beside voice banks
# the banks of plans 1 / 2 / 3 (busnodes.PLANS) and one whose master chain no fused plan takes.  detect_fused is unchanged
# and covers whole graphs only, so with a sub-mix beside the bank — through a delay-comp or through the twin's volume — every one of
# them is the hybrid plan (3): what stays is the banks' fused kernels, voice-bank (DRY) and chain (CHAIN)
DESKS = {1: dict(shapes=DRY), 2: dict(shapes=CHAIN), 3: dict(shapes=DRY, send=True), "hybrid": dict(shapes=DRY, spatial=True)}
SUBMIX_D = 63


def desk(e, shapes, middle, **kw):
    """busnodes.bank with a master volume and a sub-mix S beside it.  middle: "dcomp" (DelayCompNode(63), the bank's `middle` node),
    "volume" (the twin) or None (the oracle's graph: S itself)"""
    return bank(e, shapes, [("v", 90.0)], submix=True, middle=("dcomp", SUBMIX_D) if middle == "dcomp" else middle, rng_base=5200, salt=71, **kw)


# ================================================================================================ CPU tier: the planner
def _harness_desk(which, middle, max_batch):
    e = HostOnlyEngine(max_block_frames=256, num_graph_outputs=4, max_batch=max_batch)
    desk(e, middle=middle, **DESKS[which])
    return (e,) + harness_run(e, n_out_ch=4)


@pytest.mark.parametrize("which", [1, 2, 3, "hybrid"])
@pytest.mark.parametrize("max_batch", [64, 3])
def test_a_delay_comp_on_a_sub_mix_changes_no_planner_decision(which, max_batch):
    """the twin graph, a 2 -> 2 volume in the node's place: the same plan kind, fused voices, launches and lazy calls; the level that
    holds the node is launched with bit 6"""
    e0, la0, seen0 = _harness_desk(which, "volume", max_batch)
    e, la, seen = _harness_desk(which, "dcomp", max_batch)
    assert seen & LB_DELAY_COMP and not seen & ~(LB_DELAY_COMP | LB_LEVEL) and not seen0 & ~LB_LEVEL, (seen, seen0)
    assert e.cx.plan_kind() == e0.cx.plan_kind() == 3 and e.cx.plan_fused_voices() == e0.cx.plan_fused_voices()
    assert e.cx.plan_fused_voices() == len(DESKS[which]["shapes"]) + 2    # the banks' voices and the sub-mix's stay with the fused kernels
    assert la == la0, (la, la0)
    assert e.cx.lazy_stats() == e0.cx.lazy_stats(), (e.cx.lazy_stats(), e0.cx.lazy_stats())


def test_one_launch_level_with_bit_6_per_batch():
    e = HostOnlyEngine(max_block_frames=64, num_graph_inputs=2, max_batch=4)
    m = e.add_node(DELAY_COMP, 2, 2, [63.0])
    e.connect_stereo(e.graph_in_node, m)
    e.connect_stereo(m, e.graph_out_node)
    e.update()
    assert e.cx.plan_kind() == 0
    e.reset_launches()
    e.process_blocks(4)
    assert e.violation() == ""
    assert e.launches()["level"] == 1
    # the graph's other nodes are graph_in and graph_out: I/O edges with kernels of their own, in no level list, so they add no bit
    assert e.level_kinds_seen() == LB_DELAY_COMP


# ================================================================================================ CPU tier: mirror, header, ffi.rs
def test_typed_mirror_header_and_generated_ffi():
    import firewheel_amd as fa
    from firewheel_amd import _lib as flib

    node = fa.DelayCompNode()
    assert (node.KIND, node.frames, node.latency_frames, node.channels, node.params()) == (DELAY_COMP, 63, 63, 2, [63.0])
    assert fa.DelayCompNode(200, channels=3).params() == [200.0] and fa.DelayCompNode(200).latency_frames == 200
    assert fa.DelayCompNode.MAX_FRAMES == DMAX and fa.LimiterNode.latency_frames == fa.DelayCompNode().frames
    for name in ("fwgpu_node_latency", "fwgpu_graph_latency_report", "fwgpu_graph_output_latency"):
        assert name in flib.SIGNATURES
    # the node the raw call builds: same kind, same parameter list, accepted by the same checks
    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=0, num_graph_outputs=2)
    v = cx.add_node(2, 2, fa.VolumeNode(50.0))
    m = cx.add_node(node.channels, node.channels, node)
    for c in range(2):
        cx.connect(v, c, m, c)
        cx.connect(m, c, cx.graph_out_node(), c)
    cx.update()
    assert cx.node_latency(m) == 63 and cx.output_latency() == 63 and cx.latency_report() == []
    with pytest.raises(fa.FwgpuError):
        cx.add_node(2, 3, fa.DelayCompNode())
    bad = cx.add_node(2, 2, fa.DelayCompNode(frames=8193))
    with pytest.raises(fa.FwgpuError):
        cx.update()
    cx.remove_node(bad)
    cx.update()
    cx.close()
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    assert re.search(r"FWGPU_DELAY_COMP = 19\b", hdr) and re.search(r"#define FWGPU_DELAY_COMP_MAX 8192\b", hdr)
    assert re.search(r"typedef struct fwgpu_latency_skew \{\s*int64_t node;[^}]*uint32_t port;[^}]*uint32_t lead_frames;[^}]*\} fwgpu_latency_skew;", hdr)
    assert [f[0] for f in flib.LatencySkew._fields_] == ["node", "port", "lead_frames"]
    import ctypes as C
    assert C.sizeof(flib.LatencySkew) == 16
    for decl in ("int fwgpu_node_latency(fwgpu_ctx* ctx, int64_t node, uint32_t* frames);",
                 "int64_t fwgpu_graph_latency_report(fwgpu_ctx* ctx, fwgpu_latency_skew* out, uint32_t cap);",
                 "int fwgpu_graph_output_latency(fwgpu_ctx* ctx, uint32_t* frames);"):
        assert decl in hdr, decl
    types = open(os.path.join(ROOT, "firewheel_amd", "csrc", "fwgpu_types.h")).read()
    assert re.search(r"K_DELAY_COMP = 19\b", types) and re.search(r"#define DCOMP_MAX 8192u", types) and re.search(r"#define DCOMP_CH_MAX 8\b", types)
    ffi = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "ffi.rs")).read()
    assert "pub const FWGPU_DELAY_COMP: c_int = 19;" in ffi and "pub const FWGPU_DELAY_COMP_MAX: u32 = 8192;" in ffi
    assert "pub struct fwgpu_latency_skew {\n    pub node: i64,\n    pub port: u32,\n    pub lead_frames: u32,\n}" in ffi
    assert "pub fn fwgpu_graph_latency_report(ctx: *mut fwgpu_ctx, out: *mut fwgpu_latency_skew, cap: u32) -> i64;" in ffi
    assert "pub fn fwgpu_node_latency(ctx: *mut fwgpu_ctx, node: i64, frames: *mut u32) -> c_int;" in ffi
    assert "pub fn fwgpu_graph_output_latency(ctx: *mut fwgpu_ctx, frames: *mut u32) -> c_int;" in ffi
    nodes = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "nodes.rs")).read()
    assert "pub struct GpuDelayCompNode" in nodes and "ffi::FWGPU_DELAY_COMP" in nodes


# ================================================================================================ GPU tier
# ---- G1: graph_in(n) -> delay-comp -> graph_out(n) on the level executor
G1_CASES = [(64, 0), (64, 1), (64, 63), (64, 64), (64, 200), (256, 63), (256, 254), (256, 255), (256, 256), (256, 257), (512, 8192)]
_g1_cache = {}


def g1_calls(mbf, D):
    """1 block, 5 blocks, 3 blocks + 17 frames, 1 frame, 5 blocks: every border between the stored history, earlier blocks of the batch
    and the wave's own block is crossed; repeated until the stream is long enough for the delay to come out and be shifted again"""
    pattern = [mbf, 5 * mbf, 3 * mbf + 17, 1, 5 * mbf]
    return pattern * (1 + (D + 2 * mbf) // sum(pattern))


def _g1_reference(n, mbf, D):
    if (n, mbf) not in _g1_cache:
        _g1_cache[(n, mbf)] = special_noise(np.random.default_rng(100 * n + mbf), n, sum(g1_calls(mbf, DMAX if mbf == 512 else 257)))
    calls = g1_calls(mbf, D)
    x = _g1_cache[(n, mbf)][:, :sum(calls)]
    return calls, x, np.concatenate([np.zeros((n, D), dtype=F32), x], axis=1)[:, :x.shape[1]]   # (graph inputs are never flagged)


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,D", G1_CASES)
@pytest.mark.parametrize("n", [1, 2, 8])
def test_g1_stream_graphs(n, mbf, D):
    calls, x, want = _g1_reference(n, mbf, D)
    assert sum(calls) > D + mbf
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=n, num_graph_outputs=n, max_batch=8)
    m = g.add_node(DELAY_COMP, n, n, [float(D)])
    for c in range(n):
        g.connect(g.graph_in_node, c, m, c)
        g.connect(m, c, g.graph_out_node, c)
    g.update()
    assert g.cx.plan_kind() == 0
    a = 0
    for k, f in enumerate(calls):
        inp = np.ascontiguousarray(x[:, a:a + f].T).ravel()
        y = planar(g.process_interleaved(f, n_out_ch=n, inp=inp, n_in_ch=n), n)
        assert_bits(y, want[:, a:a + f], "n %d mbf %d D %d call %d (%d frames at %d)" % (n, mbf, D, k, f, a))
        a += f
    u = fwapi.bits(want)
    assert (u == 0x80000000).any() and (u == 0x7F800000).any() and (u == 0x00000001).any() and (u == 0x7FC01234).any()


# ---- G2: silence
@pytest.mark.gpu
@pytest.mark.parametrize("mbf,D", [(64, 63), (64, 200), (256, 63), (256, 256)])
@pytest.mark.parametrize("pattern", ["live quiet quiet live", "quiet from the start"])
def test_g2_a_sampler_that_stops_and_starts(mbf, D, pattern):
    """sampler -> delay-comp -> graph_out: the sampler's output is flagged silent while it is stopped.  The graph output's silence mask
    and the values against the model, whose input — values and flags — is the same graph without the node"""
    calls = [3, 4, 2, 5, 1, 4, 3, 2]     # blocks; max_batch 4
    quiet = (2, 3, 4, 5) if pattern == "live quiet quiet live" else (0, 1, 2, 6)    # (calls during which the sampler is stopped)

    def run(e, with_node):
        s = e.sampler(100.0)
        cur = s
        if with_node:
            cur = e.add_node(DELAY_COMP, 2, 2, [float(D)])
            e.connect_stereo(s, cur)
        e.connect_stereo(cur, e.graph_out_node)
        e.update()
        e.sampler_set_sample(s, e.new_sample(fwapi.PLANAR_F32, 2, scenarios.voice_source(91, 5 * mbf + 13, 2)))
        e.sampler_set_loop_range(s, LOOP_FULL)
        outs = []
        for i, k in enumerate(calls):
            (e.sampler_stop if i in quiet else e.sampler_play)(s)
            outs.append(e.process_blocks_flags(k))
        return planar(np.concatenate([np.asarray(o[0], F32) for o in outs])), np.concatenate([o[1] for o in outs]).T.astype(bool)

    xo, fo = run(OracleEngine(max_block_frames=mbf), False)
    xt, ft = run(GpuEngine(max_block_frames=mbf, max_batch=4), False)
    assert_bits(xt, xo, "the graph without the node")
    assert np.array_equal(ft, fo)
    blocks = sum(calls)
    want, want_flags = model(xo, fo, D, [mbf] * blocks)
    assert fo.any() and not fo.all() and want_flags.any() and (want_flags != fo).any()    # the tail of D frames is heard after the stop
    yg, fg = run(GpuEngine(max_block_frames=mbf, max_batch=4), True)
    assert_bits(yg, want, "%s, mbf %d D %d" % (pattern, mbf, D))
    assert np.array_equal(fg, want_flags), (fg.astype(int), want_flags.astype(int))


# ---- G3: the purpose
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["by hand", "compensate_latency"])
def test_g3_a_limited_bus_and_its_compensated_dry_copy_are_equal(how):
    import firewheel_amd as fa

    mbf = 256
    calls = [mbf, 4 * mbf, 3 * mbf + 17, 1, 4 * mbf]
    rng = np.random.default_rng(33)
    x = rng.uniform(-0.9, 0.9, size=(2, sum(calls))).astype(F32)      # below the ceiling: the limiter is a delay of 63 frames
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=2, num_graph_outputs=4, max_batch=4)
    lim = g.cx.add_node(2, 2, fa.LimiterNode(1.0, 0))
    g.connect_stereo(g.graph_in_node, lim)
    g.connect_stereo(lim, g.graph_out_node, 0)
    if how == "by hand":
        dc = g.cx.add_node(2, 2, fa.DelayCompNode(fa.LimiterNode.latency_frames))
        g.connect_stereo(g.graph_in_node, dc)
        g.connect_stereo(dc, g.graph_out_node, 2)
    else:
        g.connect_stereo(g.graph_in_node, g.graph_out_node, 2)
        assert g.cx.latency_report() == [(g.graph_out_node, 2, 63), (g.graph_out_node, 3, 63)]
        added = g.cx.compensate_latency()
        assert len(added) == 1 and g.cx.node_latency(added[0]) == 63
    assert g.cx.latency_report() == [] and g.cx.output_latency() == 63
    g.update()
    a, outs = 0, []
    for f in calls:
        outs.append(np.asarray(g.process_interleaved(f, n_out_ch=4, inp=np.ascontiguousarray(x[:, a:a + f].T).ravel(), n_in_ch=2)))
        a += f
    y = planar(np.concatenate(outs), 4)
    assert_bits(y[2:4], y[0:2], "the delayed dry copy against the limited bus")
    assert_bits(y[2:4, 63:], x[:, :-63], "... which is the input 63 frames late")
    assert not fwapi.bits(y[:, :63]).any()


# ---- G4: beside the fused plans
G4_MBF = 256
G4_CALLS = [3, 4, 2, 4, 3, 4, 2]     # blocks; max_batch 4


@pytest.mark.gpu
@pytest.mark.parametrize("which", [1, 2, 3, "hybrid"])
def test_g4_a_delayed_sub_mix_beside_the_fused_voice_banks(which):
    calls = [k * G4_MBF for k in G4_CALLS] + [100]

    def run(e, middle):
        desk(e, middle=middle, **DESKS[which])
        return planar(np.concatenate([np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in calls]), 4)

    ro = run(scenarios.TaggedOracle(OracleEngine(max_block_frames=G4_MBF, num_graph_outputs=4, short_blocks=True)), None)
    t = GpuEngine(max_block_frames=G4_MBF, num_graph_outputs=4, max_batch=4)
    rt = run(t, "volume")
    assert_bits(rt, ro, "the twin")
    g = GpuEngine(max_block_frames=G4_MBF, num_graph_outputs=4, max_batch=4)
    rg = run(g, "dcomp")
    assert g.cx.plan_kind() == t.cx.plan_kind() == 3 and g.cx.plan_fused_voices() == t.cx.plan_fused_voices()
    assert g.cx.plan_fused_voices() == len(DESKS[which]["shapes"]) + 2
    assert_bits(rg[0:2], ro[0:2], "the banks' mix")
    want, _ = model(ro[2:4], None, SUBMIX_D, [G4_MBF] * sum(G4_CALLS) + [100])
    assert_bits(rg[2:4], want, "the sub-mix, %d frames late" % SUBMIX_D)
    assert np.abs(want).max() > 0.01


# ---- G5: edits
@pytest.mark.gpu
@pytest.mark.parametrize("D", [63, 300])
def test_g5_an_edit_elsewhere_keeps_the_history_and_a_new_node_starts_from_zeros(D):
    mbf = 256
    phases = [[3 * mbf, 2 * mbf], [4 * mbf, 100], [2 * mbf, 4 * mbf], [3 * mbf, 2 * mbf]]

    def run(e, gpu):
        d = desk(e, shapes=DRY, middle=None)
        outs = [np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in phases[0]]

        def insert():
            d.middle = e.add_node(DELAY_COMP, 2, 2, [float(D)])
            e.connect_stereo(d.S, d.middle)
            e.connect_stereo(d.middle, e.graph_out_node, 2)
            e.update()

        if gpu:  # the node goes in between S and graph_out
            for c in range(2):
                e.disconnect(d.S, c, e.graph_out_node, 2 + c)
            insert()
        outs += [np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in phases[1]]
        rng = np.random.default_rng(98)   # an edit elsewhere: one more voice on the last leaf's free ports
        end = _voice(e, d, "v", len(d.samplers), rng)
        e.connect_stereo(end, d.spare[0], d.spare[1])
        e.update()
        _start(e, d.samplers[-1], d.seed, len(d.samplers) - 1, d.salt)
        outs += [np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in phases[2]]
        if gpu:  # removed and added again in one update: a new node, a history of zeros
            e.remove_node(d.middle)
            insert()
        outs += [np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in phases[3]]
        return planar(np.concatenate(outs), 4)

    ro = run(scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf, num_graph_outputs=4, short_blocks=True)), False)
    rg = run(GpuEngine(max_block_frames=mbf, num_graph_outputs=4, max_batch=4), True)
    n1 = sum(phases[0])
    n3 = n1 + sum(phases[1]) + sum(phases[2])
    assert_bits(rg[0:2], ro[0:2], "the banks' mix")
    assert_bits(rg[2:4, :n1], ro[2:4, :n1], "before the node")
    shift = lambda x: np.concatenate([np.zeros((2, D), dtype=F32), x], axis=1)[:, :x.shape[1]]
    assert_bits(rg[2:4, n1:n3], shift(ro[2:4, n1:n3]), "from the activation on, across the voice edit")
    assert_bits(rg[2:4, n3:], shift(ro[2:4, n3:]), "from the second activation on: zeros in front")
    assert np.abs(ro[2:4, n3 - D:n3]).max() > 0.01     # (the old node's history was not silence)


# ---- G6: fwgpu_node_process
@pytest.mark.gpu
@pytest.mark.parametrize("D,f", [(63, 100), (250, 100), (5, 256)])
def test_g6_node_process_renders_block_by_block_through_the_stored_history(D, f):
    g = GpuEngine(max_block_frames=256)
    m = g.add_node(DELAY_COMP, 2, 2, [float(D)])
    g.connect_stereo(m, g.graph_out_node)
    g.update()
    blocks = 9
    x = special_noise(np.random.default_rng(8 + D), 2, blocks * f)
    flags = np.zeros((2, blocks), dtype=bool)
    flags[1, 1] = True                   # channel 1 flagged in the second call: it counts as +0.0 and is not read
    flags[0, 3:8] = True                 # channel 0 flagged for five calls: its output follows once D frames have passed
    flags[1, 4:6] = True
    want, want_flags = model(x, flags, D, [f] * blocks)
    assert want_flags.any() and (want_flags != flags).any()
    for k in range(blocks):
        sl = slice(k * f, (k + 1) * f)
        ins = [np.full(f, 77.0, dtype=F32) if flags[c, k] else x[c, sl] for c in range(2)]
        mask = sum(1 << c for c in range(2) if flags[c, k])
        y, om = g.node_process(m, f, ins, 2, in_mask=mask)
        assert om == sum(1 << c for c in range(2) if want_flags[c, k]), (k, om)
        assert_bits(y, want[:, sl], "B1 call %d" % k)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["live quiet quiet live", "quiet from the start"])
def test_g6_node_process_silence_patterns(pattern):
    D, f = 150, 64
    g = GpuEngine(max_block_frames=64)
    m = g.add_node(DELAY_COMP, 1, 1, [float(D)])
    g.connect(m, 0, g.graph_out_node, 0)
    g.update()
    quiet = [0, 1, 1, 1, 1, 1, 0, 1, 0] if pattern == "live quiet quiet live" else [1, 1, 1, 0, 1, 1, 1, 1, 0]
    flags = np.array([quiet], dtype=bool)
    x = np.random.default_rng(9).uniform(0.5, 1.0, size=(1, len(quiet) * f)).astype(F32)
    want, want_flags = model(x, flags, D, [f] * len(quiet))
    for k in range(len(quiet)):
        sl = slice(k * f, (k + 1) * f)
        y, om = g.node_process(m, f, [x[0, sl]], 1, in_mask=int(quiet[k]))
        assert om == int(want_flags[0, k]), (k, om)
        assert_bits(y, want[:, sl], "call %d" % k)
    assert want_flags.sum() >= 2 and (want_flags != flags).sum() >= 3


# ---- G7: a level that holds a delay-comp, a limiter, a biquad and a volume; in a case of its own, a ducker too
def _g7(with_ducker):
    from test_limiter import model as limiter_model

    mbf, D = 256, 200
    calls = [2 * mbf, 4 * mbf, mbf, 3 * mbf + 37, 1, 4 * mbf]
    N = sum(calls)
    rng = np.random.default_rng(12)
    inp = rng.uniform(-0.5, 0.5, size=(9, N)).astype(F32)
    inp[6:8, 1000:1040] *= F32(5.0)                                  # the limiter's bus passes its ceiling
    inp[8] *= (rng.uniform(size=N) < 0.02) * F32(1.0) + F32(0.1)     # the ducker's key: sparse spikes above 0.1
    n_out = 10 if with_ducker else 8

    def build(e, full):
        gi, go = e.graph_in_node, e.graph_out_node
        v = e.volume(70.0)
        b = e.biquad(0, 1200.0, 0.707)
        for c in range(2):
            e.connect(gi, c, v, c)
            e.connect(gi, 2 + c, b, c)
            e.connect(v, c, go, c)
            e.connect(b, c, go, 2 + c)
        if full:
            dc = e.add_node(DELAY_COMP, 2, 2, [float(D)])
            lim = e.add_node(LIMITER, 2, 2, [1.0, 0.0])
            for c in range(2):
                e.connect(gi, 4 + c, dc, c)
                e.connect(dc, c, go, 4 + c)
                e.connect(gi, 6 + c, lim, c)
                e.connect(lim, c, go, 6 + c)
            if with_ducker:
                dk = e.add_node(DUCKER, 3, 2, [0.1, 0.25, 16.0, 400.0, 30.0])
                for c, src in enumerate((4, 5, 8)):
                    e.connect(gi, src, dk, c)
                for c in range(2):
                    e.connect(dk, c, go, 8 + c)
        e.update()

    def run(e, n_out):
        a, outs = 0, []
        for f in calls:
            outs.append(np.asarray(e.process_interleaved(f, n_out_ch=n_out, inp=np.ascontiguousarray(inp[:, a:a + f].T).ravel(), n_in_ch=9)))
            a += f
        return planar(np.concatenate(outs), n_out)

    o = OracleEngine(max_block_frames=mbf, num_graph_inputs=9, num_graph_outputs=4, short_blocks=True)
    build(o, False)
    ro = run(o, 4)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=9, num_graph_outputs=n_out, max_batch=4)
    build(g, True)
    rg = run(g, n_out)
    want = np.concatenate([np.zeros((2, D), dtype=F32), inp[4:6]], axis=1)[:, :N]
    # the delay-comp first: a failure of a neighbour must not be mistaken for one of this kernel
    assert_bits(rg[4:6], want, "the delay-comp")
    assert_bits(rg[0:4], ro, "the volume and the biquad beside it")
    assert_bits(rg[6:8], limiter_model(inp[6:8], 1.0, 0), "the limiter")
    return rg, inp


@pytest.mark.gpu
def test_g7_a_level_shared_with_a_limiter_a_biquad_and_a_volume():
    _g7(False)


@pytest.mark.gpu
def test_g7_the_same_level_with_a_ducker_too():
    """k_ducker's own GPU tier is tests/test_ducker.py: the delay-comp, the limiter, the biquad and the volume are compared first, so a
    failure of the last assertion alone is the ducker's"""
    from test_ducker import model as ducker_model

    rg, inp = _g7(True)
    assert_bits(rg[8:10], ducker_model(inp[4:6], inp[8:9], 0.1, 0.25, 16, 400, 30), "the ducker")
