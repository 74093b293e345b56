"""The look-ahead limiter node (FWGPU_LIMITER = 17; SPEC).

The reference for sample values is `model(x, C, H)` below: the SPEC's text in numpy — a vectorised minimum over 64 + H shifts of the
target gain, then 63 vectorised f32 adds in the SPEC's order — applied to the whole stream since the node's activation and sliced per
call.  What the model takes as input is obtained without the limiter: the stream input itself, or the OracleEngine's output of the same
graph built without the node (the oracle does not know the kind).  Every comparison on the GPU tier is `fwapi.bits` equality.

CPU tier: the model against a brute-force per-frame evaluation, its overshoot bound and its identity below the ceiling; shapes and
creation parameters on the host-only harness; the planner on the harness; the typed Python mirror, the header and the generated ffi.rs.

GPU tier: G1 stream graphs on the level executor, G2 a master limiter on the three fused plans, G3 its neighbours in a master chain,
G4 graph edits, G5 fwgpu_node_process.  By construction (`frames >= H + 126` and K > 1 blocks in the batch) the parallel path renders the
multi-block calls of (max_block_frames, H) = (256, 0), (256, 130), (512, 130) in G1 and the H = 0 runs of G2, G3 and G4; the serial path
renders (64, 0), (256, 131), (512, 1920), every one-block call, every short tail block, the H = 1920 runs of G2 and G5.
"""
import os
import re

import numpy as np
import pytest

import fwapi
import scenarios
from busnodes import LB_LEVEL, LB_LIMITER, LIMITER, PLANS, _host, _start, _voice, assert_bits, bank, harness_batches, harness_run, planar, ragged_calls
from fwapi import GpuEngine, HostOnlyEngine, OracleEngine

INVALID = -20
LOOK = 64
LATENCY = 63
F32 = np.float32
BOUND = 1.0 + 66.0 * 2.0 ** -24   # 63 adds, a division and a product, each rounded to nearest
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ------------------------------------------------------------------------------------------------ the SPEC in numpy
def target_gain(x, C):
    x = np.asarray(x, dtype=F32)
    key = np.zeros(x.shape[1], dtype=F32)
    for c in range(x.shape[0]):
        key = np.fmax(key, np.abs(x[c]))          # fmaxf: a NaN sample is ignored
    C = F32(C)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(key > C, C / key, F32(1.0)).astype(F32)


def model(x, C=1.0, H=128):
    """x: [channels][frames] since the node's activation -> y of the same shape"""
    x = np.asarray(x, dtype=F32)
    n, N = x.shape
    L = LOOK + H
    tp = np.concatenate([np.ones(L - 1, dtype=F32), target_gain(x, C)])        # t[k < 0] = 1
    m = tp[L - 1:L - 1 + N].copy()
    for k in range(1, L):
        m = np.minimum(m, tp[L - 1 - k:L - 1 - k + N])
    mp = np.concatenate([np.ones(LOOK - 1, dtype=F32), m])                      # m[n < 0] = 1
    s = mp[0:N].copy()                                                          # m[n - 63]
    for k in range(1, LOOK):
        s = (s + mp[k:k + N]).astype(F32)                                       # ... + m[n - 63 + k], ascending
    g = (s * F32(0.015625)).astype(F32)
    xd = np.concatenate([np.zeros((n, LOOK - 1), dtype=F32), x], axis=1)[:, :N]  # x[n - 63], +0.0 in front
    return (xd * g).astype(F32)


def brute_frame(x, t, C, H, n):
    """frame n of every channel, evaluated as the SPEC's text reads: one window at a time, one add at a time"""
    def m_at(j):
        lo = j - (LOOK - 1) - H
        w = t[max(lo, 0):j + 1] if j >= 0 else t[0:0]
        v = F32(1.0) if (lo < 0 or w.size == 0) else w[0]   # (t[k < 0] = 1.0)
        return F32(min(v, w.min())) if w.size else v

    s = m_at(n - (LOOK - 1))
    for j in range(n - (LOOK - 2), n + 1):
        s = F32(s + m_at(j))
    g = F32(s * F32(0.015625))
    return np.array([F32((x[c, n - LATENCY] if n >= LATENCY else F32(0.0)) * g) for c in range(x.shape[0])], dtype=F32)


# ------------------------------------------------------------------------------------------------ the probe signal and its calls
def probe(n, calls, mbf, C, seed):
    """noise at about 0.3 (below every ceiling used here) with bursts of 6x .. 30x: one inside the last 63 frames of a call, one
    straddling a block boundary inside a call, one over the short tail block, the 1-frame call and the start of the next call, a
    single-sample spike, a stretch where only channel 1 is loud, 400 frames left alone, samples of exactly +C and -C, a run of -0.0"""
    N = sum(calls)
    ends = np.cumsum(calls)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.3, 0.3, size=(n, N)).astype(F32)

    def burst(a, b, chans=None):
        f = F32(rng.uniform(6.0, 30.0))
        for c in (range(n) if chans is None else chans):
            x[c, a:b] = x[c, a:b] * f

    burst(ends[1] - 40, ends[1] - 20)                      # the look-ahead crosses the call boundary
    burst(ends[0] + mbf - 10, ends[0] + mbf + 10)          # call 1 has five blocks: across its first block boundary
    burst(ends[3] - 30, ends[4] + 12)                      # the 37-frame tail block, the 1-frame call, the next call
    x[:, ends[1] + mbf // 2 + 3] = F32(7.0)                # one sample
    q = ends[4] + 3 * mbf // 2
    if n >= 2:
        burst(q, q + 30, chans=[1])                        # the link: channel 0 is turned down with it
    quiet = ends[4] + 3 * mbf                              # [quiet, quiet + 400): noise only
    x[0, quiet + 100] = F32(C)
    x[n - 1, quiet + 150] = -F32(C)
    x[:, quiet + 410:quiet + 460] = F32(-0.0)
    for _ in range(5):
        a = int(rng.integers(quiet + 500, N - 100))
        burst(a, a + int(rng.integers(5, 80)))
    assert quiet + 500 < N - 100 and np.abs(x[:, quiet:quiet + 400]).max() <= F32(C)
    return x


# ================================================================================================ CPU tier: the model
MODEL_CASES = [(1.0, 0), (0.891, 128), (0.5, 1920)]


@pytest.fixture(scope="module")
def probe2():
    calls = ragged_calls(256)
    return calls, probe(2, calls, 256, 0.5, seed=11)


@pytest.mark.parametrize("C,H", MODEL_CASES)
def test_model_equals_the_brute_force_evaluation(probe2, C, H):
    calls, x = probe2
    y = model(x, C, H)
    t = target_gain(x, C)
    over = np.nonzero(t < 1.0)[0]
    assert over.size > 50
    # the first frames, the frames around the end of the hold behind the first burst and behind the spike, and some anywhere
    first_end = over[np.nonzero(np.diff(over) > 1)[0][0]]
    frames = list(range(0, 70)) + [LATENCY + H + first_end + d for d in range(-3, 70, 6)] + [int(v) for v in np.linspace(200, x.shape[1] - 1, 25)]
    for n in frames:
        assert_bits(y[:, n], brute_frame(x, t, C, H, n), "C %g H %d frame %d" % (C, H, n))
    assert np.any(y != 0)


@pytest.mark.parametrize("C,H", MODEL_CASES)
def test_model_never_passes_the_ceiling_by_more_than_66_roundings(probe2, C, H):
    _, x = probe2
    y = model(x, C, H)
    assert np.abs(x).max() > 6 * C
    assert float(np.abs(y).max()) <= float(F32(C)) * BOUND, float(np.abs(y).max()) / float(F32(C)) - 1.0


@pytest.mark.parametrize("C,H", MODEL_CASES)
def test_model_below_the_ceiling_is_a_delay_of_63_frames_bit_for_bit(C, H):
    rng = np.random.default_rng(5)
    x = rng.uniform(-C, C, size=(3, 3000)).astype(F32)
    x = np.clip(x, -F32(C), F32(C))
    x[0, 100], x[1, 200], x[2, 300:340] = F32(C), -F32(C), F32(-0.0)
    y = model(x, C, H)
    assert_bits(y[:, LATENCY:], x[:, :-LATENCY], "delayed input")
    assert not fwapi.bits(y[:, :LATENCY]).any()


# ================================================================================================ CPU tier: shapes and parameters
@pytest.mark.parametrize("n_in,n_out", [(2, 1), (1, 2), (2, 0), (0, 0), (9, 9)])
def test_shapes_refused_at_add_node(n_in, n_out):
    e, _ = _host()
    with pytest.raises(e.fa.FwgpuError) as ei:
        e.add_node(LIMITER, n_in, n_out, [1.0, 128.0])
    assert ei.value.code == INVALID and "LimiterNode" in str(ei.value)
    e.update()  # nothing was added


@pytest.mark.parametrize("params", [[float("nan")], [float("inf")], [0.0], [-1.0], [1001.0], [1.0, 0.5], [1.0, -1.0], [1.0, 1921.0],
                                    [1.0, float("nan")]])
def test_parameters_refused_at_update(params):
    e, v = _host()
    m = e.add_node(LIMITER, 2, 2, params)
    for _ in range(2):  # (still there, still refused)
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.update()
        assert ei.value.code == INVALID and "LimiterNode" in str(ei.value)
    e.remove_node(m)
    good = e.add_node(LIMITER, 2, 2, [1.0, 128.0])
    e.connect_stereo(v, good)
    e.update()  # the graph is usable


@pytest.mark.parametrize("params", [[], [1.0], [0.001, 0.0], [1000.0, 1920.0], [0.891, 128.0]])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_parameters_and_shapes_accepted(params, n):
    e, _ = _host()
    m = e.add_node(LIMITER, n, n, params)
    e.update()
    assert e.cx.plan_node_level(m) >= 0
    with pytest.raises(e.fa.FwgpuError) as ei:
        e.set_param(m, 0, 0.5)
    assert ei.value.code == INVALID
    with pytest.raises(e.fa.FwgpuError):
        e.set_param(m, 1, 64.0)


# ================================================================================================ banks with a master chain (busnodes.bank)
def run_calls(e, calls):
    return [np.asarray(e.process_interleaved(n)) for n in calls]


def oracle(mbf, short_blocks=False):
    return scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf, short_blocks=short_blocks))


# ================================================================================================ CPU tier: the planner
def _harness_bank(plan, master, max_batch):
    e = HostOnlyEngine(max_block_frames=256, max_batch=max_batch)
    bank(e, master=master, **PLANS[plan])
    return (e,) + harness_run(e)


@pytest.mark.parametrize("plan", [1, 2, 3])
@pytest.mark.parametrize("max_batch", [64, 3])
def test_a_master_limiter_leaves_the_plan_its_launches_and_its_lazy_calls_alone(plan, max_batch):
    """the same graph without the node: the same plan kind and fused voices, the same launches plus one launch_level per batch — with
    the limiter's bit — and the same lazy calls"""
    e0, la0, seen0 = _harness_bank(plan, [("v", 90.0)], max_batch)
    assert e0.cx.plan_kind() == plan and not seen0 & ~LB_LEVEL
    for master in ([("v", 90.0), ("L", 1.0, 128.0)], [("L", 0.5, 0.0), ("v", 90.0)]):
        e, la, seen = _harness_bank(plan, master, max_batch)
        assert seen & LB_LIMITER and not seen & ~(LB_LIMITER | LB_LEVEL), seen
        assert e.cx.plan_kind() == plan and e.cx.plan_fused_voices() == e0.cx.plan_fused_voices()
        assert la == dict(la0, level=la0["level"] + harness_batches(max_batch)), (la, la0)
        assert e.cx.lazy_stats() == e0.cx.lazy_stats(), (e.cx.lazy_stats(), e0.cx.lazy_stats())
        if plan != 3:
            assert e.cx.lazy_stats()[0] > 0


def test_a_limiter_of_another_width_goes_to_the_level_executor():
    e = HostOnlyEngine(max_block_frames=256, num_graph_inputs=3, num_graph_outputs=3)
    m = e.add_node(LIMITER, 3, 3, [])
    for c in range(3):
        e.connect(e.graph_in_node, c, m, c)
        e.connect(m, c, e.graph_out_node, c)
    e.update()
    assert e.cx.plan_kind() == 0


# ================================================================================================ CPU tier: mirror, header, ffi.rs
def test_typed_mirror_header_and_generated_ffi():
    import firewheel_amd as fa
    from firewheel_amd import graph as G

    node = fa.LimiterNode()
    assert (node.KIND, node.latency_frames, node.channels, node.params()) == (LIMITER, LATENCY, 2, [1.0, 128.0])
    assert fa.LimiterNode(0.5, 77, channels=3).params() == [0.5, 77.0]
    # ceiling_db goes through the function MeterNode.peak_db inverts
    r = np.zeros(1, dtype=G.METER_DTYPE)
    for db in (-6.0, -0.1, 0.0, 3.0):
        ln = fa.LimiterNode(ceiling_db=db, hold_frames=0)
        assert fwapi.bits(F32(ln.ceiling)) == fwapi.bits(G.MeterNode.db_to_gain(db))
        r["peak"] = ln.ceiling
        assert abs(float(G.MeterNode.peak_db(r)[0]) - db) <= 2e-6 * max(1.0, abs(db)) and abs(ln.ceiling_db - db) <= 2e-6 * max(1.0, abs(db))
    assert fwapi.bits(G.MeterNode.db_to_gain(0.0)) == fwapi.bits(F32(1.0))
    # the node the raw call builds: same kind, same parameter list, accepted by the same checks
    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=0, num_graph_outputs=2)
    v = cx.add_node(2, 2, G.VolumeNode(50.0))
    m = cx.add_node(node.channels, node.channels, node)
    for c in range(2):
        cx.connect(v, c, m, c)
        cx.connect(m, c, cx.graph_out_node(), c)
    cx.update()
    with pytest.raises(fa.FwgpuError):
        cx.add_node(2, 3, fa.LimiterNode())
    bad = cx.add_node(2, 2, fa.LimiterNode(ceiling=0.0))
    with pytest.raises(fa.FwgpuError):
        cx.update()
    cx.remove_node(bad)
    cx.update()
    cx.close()
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    assert re.search(r"FWGPU_LIMITER = 17\b", hdr) and re.search(r"#define FWGPU_LIMITER_LATENCY 63\b", hdr)
    ffi = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "ffi.rs")).read()
    assert "pub const FWGPU_LIMITER: c_int = 17;" in ffi and "pub const FWGPU_LIMITER_LATENCY: u32 = 63;" in ffi


# ================================================================================================ GPU tier
# ---- G1: graph_in(n) -> limiter -> graph_out(n) on the level executor
G1_CEILING = {1: 1.0, 2: 0.891, 3: 0.5, 8: 1.0}
_g1_cache = {}


def _g1_reference(n, mbf, H):
    """the probe and the model's output for it: computed once per (n, mbf, H); the probe once per (n, mbf)"""
    C = G1_CEILING[n]
    if (n, mbf) not in _g1_cache:
        calls = ragged_calls(mbf)
        _g1_cache[(n, mbf)] = (calls, probe(n, calls, mbf, C, seed=100 * n + mbf))
    calls, x = _g1_cache[(n, mbf)]
    if (n, mbf, H) not in _g1_cache:
        _g1_cache[(n, mbf, H)] = model(x, C, H)
    return C, calls, x, _g1_cache[(n, mbf, H)]


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,H", [(64, 0), (256, 0), (256, 130), (256, 131), (512, 130), (512, 1920)])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_g1_stream_graphs(n, mbf, H):
    C, calls, x, want = _g1_reference(n, mbf, H)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=n, num_graph_outputs=n, max_batch=8)
    m = g.add_node(LIMITER, n, n, [C, float(H)])
    for c in range(n):
        g.connect(g.graph_in_node, c, m, c)
        g.connect(m, c, g.graph_out_node, c)
    g.update()
    assert g.cx.plan_kind() == 0
    a = 0
    for k, f in enumerate(calls):
        inp = np.ascontiguousarray(x[:, a:a + f].T).ravel()
        y = planar(g.process_interleaved(f, n_out_ch=n, inp=inp, n_in_ch=n), n)
        assert_bits(y, want[:, a:a + f], "n %d mbf %d H %d call %d (%d frames at %d)" % (n, mbf, H, k, f, a))
        a += f
    assert float(np.abs(want).max()) <= float(F32(C)) * BOUND and np.abs(want).max() > 0.9 * C


# ---- G2: a master limiter on the fused plans
G2_CALLS = [3, 4, 2, 4, 3, 4, 2]   # blocks; max_batch 4: every batch has K >= 2
G2_MBF = 256
_g2_cache = {}


def _g2_plain(plan, tail):
    """the graph without the limiter: the oracle's output per call, and the product's plan kind and lazy calls"""
    if (plan, tail) not in _g2_cache:
        calls = [k * G2_MBF for k in G2_CALLS] + ([tail] if tail else [])
        master = [("v", 120.0), ("L", 0.0, 0.0)]
        o = oracle(G2_MBF, short_blocks=bool(tail))
        bank(o, master=master, leave_out="L", **PLANS[plan])
        ro = run_calls(o, calls)
        g = GpuEngine(max_block_frames=G2_MBF, max_batch=4)
        bank(g, master=master, leave_out="L", **PLANS[plan])
        rg = run_calls(g, calls)
        for k, (a, b) in enumerate(zip(ro, rg)):
            assert_bits(b, a, "plan %d without the limiter, call %d" % (plan, k))
        _g2_cache[(plan, tail)] = (calls, ro, g.cx.plan_kind(), g.cx.lazy_stats())
    return _g2_cache[(plan, tail)]


@pytest.mark.gpu
@pytest.mark.parametrize("plan,H,tail", [(1, 0, 100), (1, 1920, 0), (2, 0, 0), (2, 1920, 0), (3, 0, 0), (3, 1920, 100)])
def test_g2_master_limiter_on_fused_plans(plan, H, tail):
    C = 1.0
    calls, ro, kind0, lazy0 = _g2_plain(plan, tail)
    assert kind0 == plan
    x = planar(np.concatenate(ro))
    assert np.abs(x).max() > 1.5 * C and np.mean(np.abs(x).max(axis=0) > C) < 0.9   # the sum passes C, and not all the time
    want = model(x, C, H)
    g = GpuEngine(max_block_frames=G2_MBF, max_batch=4)
    bank(g, master=[("v", 120.0), ("L", C, float(H))], **PLANS[plan])
    rg = run_calls(g, calls)
    assert g.cx.plan_kind() == plan
    assert g.cx.lazy_stats() == lazy0, (g.cx.lazy_stats(), lazy0)
    if plan != 3:
        assert lazy0[0] > 0
    a = 0
    for k, y in enumerate(rg):
        f = y.size // 2
        assert_bits(planar(y), want[:, a:a + f], "plan %d H %d call %d" % (plan, H, k))
        a += f
    assert float(np.abs(want).max()) <= C * BOUND


# ---- G3: neighbours in the master chain
@pytest.mark.gpu
@pytest.mark.parametrize("H", [0, 1920])
def test_g3_volume_limiter_meter(H):
    mbf, C = G2_MBF, 1.0
    calls, ro, _, _ = _g2_plain(1, 0)
    want = model(planar(np.concatenate(ro)), C, H)
    g = GpuEngine(max_block_frames=mbf, max_batch=4)
    b = bank(g, master=[("v", 120.0), ("L", C, float(H)), ("M", 64.0)], **PLANS[1])
    rg = run_calls(g, calls)
    assert g.cx.plan_kind() == 1
    assert_bits(planar(np.concatenate(rg)), want, "volume -> limiter -> meter, H %d" % H)
    blocks = sum(G2_CALLS)
    rd, done = g.cx.meter_read(b.node["M"], 0, blocks)
    assert done == blocks and rd.shape == (blocks, 2)
    per_block = np.abs(want).reshape(2, blocks, mbf)
    assert_bits(rd["peak"], per_block.max(axis=2).T, "peak per block")
    assert float(rd["peak"].max()) <= C * BOUND
    overs = (per_block > F32(1.0)).sum(axis=2).T
    assert np.array_equal(rd["over"], overs)
    if not overs.any():
        assert not rd["over"].any()


@pytest.mark.gpu
def test_g3_limiter_hard_clip():
    """the limiter leaves up to 2.0, the clip behind it takes that to 1.0: what the clip does is asked of the reference itself, fed
    with the model's output"""
    mbf, C, H = G2_MBF, 2.0, 0
    calls, ro, _, _ = _g2_plain(1, 0)
    lim = model(planar(np.concatenate(ro)), C, H)
    assert np.abs(lim).max() > 1.5
    o = OracleEngine(max_block_frames=mbf, num_graph_inputs=2)
    c = o.hard_clip(0.0)
    o.connect_stereo(o.graph_in_node, c)
    o.connect_stereo(c, o.graph_out_node)
    o.update()
    want = np.asarray(o.process_interleaved(lim.shape[1], inp=np.ascontiguousarray(lim.T).ravel(), n_in_ch=2))
    g = GpuEngine(max_block_frames=mbf, max_batch=4)
    bank(g, master=[("v", 120.0), ("L", C, float(H)), ("C", 0.0)], **PLANS[1])
    rg = np.concatenate(run_calls(g, calls))
    assert g.cx.plan_kind() == 1
    assert_bits(rg, want, "limiter -> hard clip")
    assert np.abs(rg).max() == 1.0


# ---- G4: edits
@pytest.mark.gpu
@pytest.mark.parametrize("H", [0, 1920])
def test_g4_a_limiter_added_to_a_running_graph_and_a_later_edit(H):
    import firewheel_amd as fa

    mbf, C = 256, 1.0
    before, between, after = [3 * mbf, 2 * mbf], [4 * mbf, 2 * mbf, 3 * mbf], [2 * mbf, 4 * mbf, 3 * mbf]

    def run(e, gpu):
        b = bank(e, master=[("v", 120.0)], **PLANS[1])
        outs = run_calls(e, before)
        if gpu:  # the limiter goes in behind the master volume, through the typed mirror
            lim = e.cx.add_node(2, 2, fa.LimiterNode(ceiling=C, hold_frames=H))
            for c in range(2):
                e.disconnect(b.last, c, e.graph_out_node, c)
            e.connect_stereo(b.last, lim)
            e.connect_stereo(lim, e.graph_out_node)
            e.update()
        outs += run_calls(e, between)
        rng = np.random.default_rng(99)   # one more voice on the last leaf's free ports
        end = _voice(e, b, "v", len(b.samplers), rng)
        e.connect_stereo(end, b.spare[0], b.spare[1])
        e.update()
        _start(e, b.samplers[-1], b.seed, len(b.samplers) - 1, b.salt)
        outs += run_calls(e, after)
        return np.concatenate(outs)

    ro = planar(run(oracle(mbf), False))
    g = GpuEngine(max_block_frames=mbf, max_batch=4)
    rg = planar(run(g, True))
    assert g.cx.plan_kind() == 1
    n0 = sum(before)
    assert_bits(rg[:, :n0], ro[:, :n0], "before the limiter")
    assert_bits(rg[:, n0:], model(ro[:, n0:], C, H), "from the limiter's activation on, H %d" % H)   # a zero history at n0


# ---- G5: fwgpu_node_process
@pytest.mark.gpu
def test_g5_node_process_keeps_the_history_between_calls():
    mbf, C, H, f = 256, 1.0, 128, 100
    g = GpuEngine(max_block_frames=mbf)
    m = g.add_node(LIMITER, 2, 2, [C, float(H)])
    g.connect_stereo(m, g.graph_out_node)
    g.update()
    rng = np.random.default_rng(8)
    x = rng.uniform(-0.4, 0.4, size=(2, 3 * f)).astype(F32)
    x[:, 70:95] *= F32(9.0)      # held into the second call
    x[0, 130:140] *= F32(20.0)
    x[:, 250:260] *= F32(5.0)
    seen = x.copy()
    seen[1, f:2 * f] = 0.0       # channel 1 is flagged silent in the second call: it counts as +0.0 and is not read
    want = model(seen, C, H)
    for k in range(3):
        ins = [x[0, k * f:(k + 1) * f], x[1, k * f:(k + 1) * f] if k != 1 else np.full(f, 77.0, dtype=F32)]
        y, om = g.node_process(m, f, ins, 2, in_mask=0b10 if k == 1 else 0)
        assert om == 0
        assert_bits(y, want[:, k * f:(k + 1) * f], "B1 call %d" % k)
    assert np.abs(want).max() > 0.9 and float(np.abs(want).max()) <= C * BOUND
