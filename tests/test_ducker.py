"""The sidechain ducker node (FWGPU_DUCKER = 18; SPEC).

The reference for sample values is `model(x, key, T, D, A, R, H)` below: the SPEC's text in numpy — `np.maximum.accumulate` for the hold,
`cumsum` for the two window counts, `astype(float32)` after every f32 operation — applied to the whole stream since the node's
activation and sliced per call.  What the model takes as input is what the node sees, obtained without the node: the stream input
itself, or the OracleEngine's output of the same graph built without the ducker, its main and key buses on four graph outputs (the
oracle does not know the kind).  Every comparison on the GPU tier is `fwapi.bits` equality.

CPU tier: the model against a brute-force per-frame evaluation that reads like the SPEC, the SPEC's properties, shapes and creation
parameters on the host-only harness, the planner on the harness, the typed Python mirror, the header and the generated ffi.rs.

GPU tier: G1 stream graphs on the level executor, G2 a two-sub-mix desk, G3 graph edits, G4 fwgpu_node_process, G5 a level with two
duckers, a limiter, a biquad and a volume side by side.

One case of the issue's list of refused shapes, (n_in, n_out) = (9, 1), is n = 1 main and k = 8 key channels, which the same issue's
SPEC (n and k in 1..8) accepts; the SPEC is what the node implements, so (9, 1) is asserted to be accepted, and (10, 1) and (1, 9)
stand in the list of refused shapes for the two mistakes it may have meant.
"""
import os
import re

import numpy as np
import pytest

import fwapi
import scenarios
from busnodes import DUCKER, LB_DUCKER, LB_LEVEL, LIMITER, _host, _start, _voice, assert_bits, harness_run, planar, ragged_calls
from fwapi import GpuEngine, HostOnlyEngine, OracleEngine

INVALID = -20
F32 = np.float32
CAP = 32768
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SPEC_SETS = [(1, 1, 0), (7, 100, 3), (64, 333, 129), (300, 50, 0)]   # (A, R, H)


# ------------------------------------------------------------------------------------------------ the SPEC in numpy
def gate(key, T):
    """key: [k][frames] -> on[frames]"""
    key = np.asarray(key, dtype=F32)
    m = np.zeros(key.shape[1], dtype=F32)
    for j in range(key.shape[0]):
        m = np.fmax(m, np.abs(key[j]))            # fmaxf from +0.0: a NaN sample is ignored
    return m > F32(T)


def amount(on, A, R, H):
    """u[frames] for the gate bits since the node's activation"""
    N = on.size
    idx = np.arange(N)
    last = np.maximum.accumulate(np.where(on, idx, -(1 << 40)))     # the last frame at or before n with the gate on
    opened = (idx - last) <= H
    cs = np.concatenate([[0], np.cumsum(opened)])                   # cs[i] = number of open frames in [0, i)

    def count(L):
        return cs[idx + 1] - cs[np.maximum(idx + 1 - L, 0)]         # open frames in (n - L, n]

    a = (count(A).astype(F32) / F32(A)).astype(F32)
    r = (count(R).astype(F32) / F32(R)).astype(F32)
    return np.fmax(a, r).astype(F32)


def gain(u, D):
    dd = F32(F32(1.0) - F32(D))
    return (F32(1.0) - (dd * u).astype(F32)).astype(F32)


def model(x, key, T, D, A, R, H):
    """x: [n][frames] main, key: [k][frames], both since the node's activation -> y [n][frames]"""
    x = np.asarray(x, dtype=F32)
    return (x * gain(amount(gate(key, T), A, R, H), D)).astype(F32)


def brute_u(on, A, R, H, n):
    """u at frame n as the SPEC's text reads: one window at a time"""
    def is_open(m):
        return m >= 0 and any(on[k] for k in range(max(m - H, 0), m + 1))

    ca = sum(1 for k in range(n - A + 1, n + 1) if is_open(k))
    cr = sum(1 for k in range(n - R + 1, n + 1) if is_open(k))
    a = F32(F32(ca) / F32(A))
    r = F32(F32(cr) / F32(R))
    return np.fmax(a, r)


# ------------------------------------------------------------------------------------------------ the probe signal and its calls
def probe(n, k, mbf, T, A, R, H, seed, total=None):
    """-> (calls, main [n][N], key [k][N], marks).  The key is noise below T with, above T: a burst inside the last frames of a call (the
    hold crosses into the next), one straddling a block boundary inside a call, one over the 37-frame tail block, the 1-frame call and
    the start of the next call, a single-sample spike, a stretch where only the LAST key channel is loud; samples of exactly +T and -T;
    one quiet stretch longer than max(A, R) + H with a run of -0.0 in the main bus at its idle end; one open stretch longer than
    max(A, R); random bursts; a last-but-one call whose key is all zeros and a last call whose main bus is.  `total`: the stream's
    length is given (the caps: there is no room for a quiet stretch of 65 536 frames, and the idle stretch is the stream's start,
    where the history is the zeros of activation)."""
    W, M = max(A, R) + H, max(A, R)
    compact = total is not None
    head = 12 * mbf + 38 + 3 * mbf // 2 + 200          # calls 0..4 and the last-channel burst
    need = total if compact else head + (W + 150) + (M + 100) + 700 + 8 * mbf
    calls = ragged_calls(mbf, need)
    N = sum(calls)
    ends = np.cumsum(calls)
    rng = np.random.default_rng(seed)
    T32 = F32(T)
    x = rng.uniform(-0.5, 0.5, size=(n, N)).astype(F32)
    key = (rng.uniform(-0.8, 0.8, size=(k, N)) * float(T32)).astype(F32)
    assert np.abs(key).max() < T32

    def burst(a, b, chans=None):
        for j in (range(k) if chans is None else chans):
            key[j, a:b] = (rng.uniform(1.5, 6.0, size=b - a) * float(T32) * rng.choice([-1.0, 1.0], size=b - a)).astype(F32)

    w = max(2, min(H, 20))
    burst(ends[1] - w, ends[1] - w // 2)                   # inside the last H frames of call 1
    burst(ends[0] + mbf - 10, ends[0] + mbf + 10)          # call 1 has five blocks: across its first block boundary
    burst(ends[3] - 30, ends[4] + 12)                      # the 37-frame tail block, the 1-frame call, the next call
    key[0, ends[1] + mbf // 2 + 3] = F32(4.0) * T32        # one sample
    q = ends[4] + 3 * mbf // 2
    burst(q, q + 30, chans=[k - 1])                        # only the last key channel
    marks = {}
    if compact:
        idle = 5                                           # nothing has opened the gate yet
        exact = 60
        opn = q + 100
    else:
        quiet = q + 60                                     # [quiet, quiet + W + 150): noise below T only
        idle = quiet + W + 40
        exact = quiet + 7
        opn = quiet + W + 150
        marks["quiet"] = (quiet + 30, quiet + W + 150)
    key[0, exact] = T32                                    # exactly +T and -T: the gate stays closed
    key[k - 1, exact + 5] = -T32
    x[:, idle:idle + 50] = F32(-0.0)
    marks["idle"] = (idle, idle + 50)
    burst(opn, opn + M + 100)                              # open for longer than max(A, R)
    marks["open"] = (opn, opn + M + 100)
    lo, hi = opn + M + 300, N - calls[-1] - calls[-2] - 100
    assert lo + 200 < hi, (lo, hi)
    for _ in range(6):
        a = int(rng.integers(lo, hi))
        burst(a, min(a + int(rng.integers(3, 90)), hi))
    key[:, N - calls[-1] - calls[-2]:N - calls[-1]] = F32(0.0)   # graph inputs of zeros arrive flagged silent
    x[:, N - calls[-1]:] = F32(0.0)
    return calls, x, key, marks


# ================================================================================================ CPU tier: the model
@pytest.fixture(scope="module")
def small_probe():
    out = {}
    for A, R, H in SPEC_SETS:
        out[(A, R, H)] = probe(2, 2, 64, 0.05, A, R, H, seed=7 + A)
    return out


@pytest.mark.parametrize("A,R,H", SPEC_SETS)
def test_model_equals_the_brute_force_evaluation(small_probe, A, R, H):
    calls, x, key, marks = small_probe[(A, R, H)]
    on = gate(key, 0.05)
    u = amount(on, A, R, H)
    ends = np.cumsum(calls)
    # the first frames, the frames around three bursts and their holds and releases, the start of the open stretch, and some anywhere
    frames = set(range(0, 40))
    for c in (ends[0] + 64 - 10, ends[3] - 30, marks["open"][0] - 5):
        frames.update(range(c, c + 60))
        frames.update(range(c + H + min(A, R) - 20, c + H + min(A, R) + 40))
    frames.update(int(v) for v in np.linspace(100, x.shape[1] - 1, 60))
    frames = sorted(f for f in frames if 0 <= f < x.shape[1])
    assert len(frames) >= 300
    for n in frames:
        assert fwapi.bits(u[n]) == fwapi.bits(brute_u(on, A, R, H, n)), (A, R, H, n, u[n], brute_u(on, A, R, H, n))
    assert on[ends[1] + 64 // 2 + 3] and not on[marks["quiet"][0] - 30 + 7] and not on[marks["quiet"][0] - 30 + 12]   # the spike; +T, -T


@pytest.mark.parametrize("A,R,H", SPEC_SETS)
@pytest.mark.parametrize("D", [0.25, 0.0])
def test_model_properties(small_probe, A, R, H, D):
    calls, x, key, marks = small_probe[(A, R, H)]
    u = amount(gate(key, 0.05), A, R, H)
    y = model(x, key, 0.05, D, A, R, H)
    W, M = max(A, R) + H, max(A, R)
    # idle: closed for max(A, R) + H frames -> u == 0, g == 1.0f, the output is the input bit for bit, -0.0 included
    qa, qb = marks["quiet"]
    assert not gate(key, 0.05)[qa:qb].any() and qb - qa > W
    assert not fwapi.bits(u[qa + W:qb]).any()
    assert fwapi.bits(gain(u[qa + W:qb], D)).tolist() == [fwapi.bits(F32(1.0))] * (qb - qa - W)
    assert_bits(y[:, qa + W:qb], x[:, qa + W:qb], "idle")
    ia, ib = marks["idle"]
    assert qa + W <= ia and ib <= qb and (fwapi.bits(y[:, ia:ib]) == 0x80000000).all()
    # fully ducked: after max(A, R) open frames u == 1 exactly and g == 1.0f - (1.0f - D)
    oa, ob = marks["open"]
    assert gate(key, 0.05)[oa:ob].all() and (u[oa + M - 1:ob] == F32(1.0)).all()
    full = F32(F32(1.0) - F32(F32(1.0) - F32(D)))
    assert (fwapi.bits(gain(u[oa + M - 1:ob], D)) == fwapi.bits(full)).all()
    # bounded step: |u[n] - u[n-1]| <= 1 / min(A, R), up to the rounding of the two quotients
    step = np.abs(np.diff(u.astype(np.float64)))
    assert step.max() <= 1.0 / min(A, R) + 2.0 ** -23, (step.max(), 1.0 / min(A, R))
    assert (u >= 0).all() and (u <= 1).all()


def test_model_attack_is_the_short_window_and_release_the_long_one():
    """A <= R: u rises with the A-window and falls with the R-window; a burst shorter than R plateaus at len / R"""
    A, R, H = 10, 100, 0
    on = np.zeros(1000, dtype=bool)
    on[100:400] = True      # longer than R
    on[600:630] = True      # shorter than R
    u = amount(on, A, R, H)
    assert u[100 + A - 1] == 1.0 and u[100 + A - 2] < 1.0                      # full depth after A frames
    assert u[399] == 1.0 and u[400 + R - 1] == 0.0 and u[400 + R - 2] > 0.0    # back after R frames, linearly
    assert np.allclose(np.diff(u[400:400 + R - 1].astype(np.float64)), -1.0 / R, atol=1e-7)
    assert u[600 + A - 1] == 1.0 and u[629] == 1.0
    assert fwapi.bits(u[630 + A - 1]) == fwapi.bits(F32(F32(30) / F32(R)))      # the plateau len / R, reached over A frames
    assert (u[630 + A - 1:600 + R] == u[630 + A - 1]).all() and u[630 + R - 1] == 0.0


# ================================================================================================ CPU tier: shapes and parameters
GOOD = [0.05, 0.25, 480.0, 12000.0, 4800.0]


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (4, 0), (2, 3), (17, 8), (10, 1), (1, 9), (0, 0)])
def test_shapes_refused_at_add_node(n_in, n_out):
    e, _ = _host()
    with pytest.raises(e.fa.FwgpuError) as ei:
        e.add_node(DUCKER, n_in, n_out, GOOD)
    assert ei.value.code == INVALID and "DuckerNode" in str(ei.value)
    e.update()  # nothing was added


def _with(slot, value):
    p = list(GOOD)
    p[slot] = value
    return p


BAD_PARAMS = ([_with(s, float("nan")) for s in range(5)] + [_with(s, float("inf")) for s in range(5)] + [_with(s, float("-inf")) for s in range(5)] +
              [_with(0, 0.0), _with(0, 1001.0), _with(1, -0.1), _with(1, 1.5), _with(2, 0.0), _with(2, 32769.0), _with(3, 0.0), _with(3, 32769.0),
               _with(4, -1.0), _with(4, 32769.0), _with(2, 1.5), _with(3, 100.25), _with(4, 0.5), [float("nan")], [0.05, 2.0]])


@pytest.mark.parametrize("params", BAD_PARAMS)
def test_parameters_refused_at_update(params):
    e, v = _host()
    m = e.add_node(DUCKER, 4, 2, params)
    for _ in range(2):  # (still there, still refused)
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.update()
        assert ei.value.code == INVALID and "DuckerNode" in str(ei.value)
    e.remove_node(m)
    good = e.add_node(DUCKER, 4, 2, GOOD)
    e.connect_stereo(v, good)
    e.connect_stereo(v, good, 2)
    e.update()  # the graph is usable


ACCEPTED = [[], [0.05], GOOD, [1e-6, 0.0, 1.0, 1.0, 0.0], [1000.0, 1.0, 32768.0, 32768.0, 32768.0], [0.05, 0.25, 1.0, 32768.0, 0.0],
            [0.05, 0.25, 32768.0, 1.0, 32768.0]]


@pytest.mark.parametrize("params", ACCEPTED)
@pytest.mark.parametrize("n,k", [(1, 1), (2, 2), (2, 1), (8, 8), (1, 8), (8, 1)])
def test_parameters_and_shapes_accepted_and_set_param_refused(params, n, k):
    e, _ = _host()
    m = e.add_node(DUCKER, n + k, n, params)
    e.update()
    assert e.cx.plan_node_level(m) >= 0
    for slot in range(5):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.set_param(m, slot, 0.5)
        assert ei.value.code == INVALID


# ================================================================================================ the two-sub-mix desk
class Desk(object):
    pass


SALT = 57   # (busnodes._start)


def desk(e, middle, n_music=5, n_dialogue=3, seed=0, duck=(0.05, 0.25, 48.0, 700.0, 100.0)):
    """music voices -> SumNode M, dialogue voices -> SumNode Dg; M -> `middle` -> graph_out 0,1 and Dg -> graph_out 2,3.  middle:
    "duck" (key Dg), "volume" (the twin: a 2 -> 2 volume of 100 % in the ducker's place) or None (the oracle's graph: M itself)"""
    d = Desk()
    d.e, d.samplers, d.seed, d.duck = e, [], seed, None
    d.M = e.sum(n_music + 1)              # (a free port pair for a later voice)
    d.Dg = e.sum(max(2, n_dialogue))
    for p in range(n_music):
        e.connect_stereo(_voice(e, d, [40.0 + 7.0 * p]), d.M, 2 * p)
    d.n_music = n_music
    d.dialogue = []
    for p in range(n_dialogue):
        e.connect_stereo(_voice(e, d, [30.0 + 5.0 * p]), d.Dg, 2 * p)
        d.dialogue.append(d.samplers[-1])
    if middle == "duck":
        d.duck = e.add_node(DUCKER, 4, 2, list(duck))
        e.connect_stereo(d.M, d.duck)
        e.connect_stereo(d.Dg, d.duck, 2)
        e.connect_stereo(d.duck, e.graph_out_node)
    elif middle == "volume":
        v = e.volume(100.0)
        e.connect_stereo(d.M, v)
        e.connect_stereo(v, e.graph_out_node)
    else:
        e.connect_stereo(d.M, e.graph_out_node)
    e.connect_stereo(d.Dg, e.graph_out_node, 2)
    e.update()
    for i, s in enumerate(d.samplers):
        _start(e, s, seed, i, SALT)
    return d


def oracle(mbf):
    return scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf, num_graph_outputs=4))


# ================================================================================================ CPU tier: the planner
def _harness_desk(middle, max_batch):
    e = HostOnlyEngine(max_block_frames=256, num_graph_outputs=4, max_batch=max_batch)
    desk(e, middle)
    return (e,) + harness_run(e, n_out_ch=4)


@pytest.mark.parametrize("max_batch", [64, 3])
def test_a_ducker_changes_no_planner_decision(max_batch):
    """the twin graph, a 2 -> 2 volume in the ducker's place: the same plan kind, fused voices, launches and lazy calls; the level that
    holds the node is launched with bit 5"""
    e0, la0, seen0 = _harness_desk("volume", max_batch)
    e, la, seen = _harness_desk("duck", max_batch)
    assert seen & LB_DUCKER and not seen & ~(LB_DUCKER | LB_LEVEL) and not seen0 & ~LB_LEVEL, (seen, seen0)
    assert e.cx.plan_kind() == e0.cx.plan_kind() and e.cx.plan_fused_voices() == e0.cx.plan_fused_voices()
    assert e.cx.plan_fused_voices() == 8
    assert la == la0, (la, la0)
    assert e.cx.lazy_stats() == e0.cx.lazy_stats(), (e.cx.lazy_stats(), e0.cx.lazy_stats())


def test_node_kinds_end_at_19():
    """fwgpu_add_node: the last kind with a valid shape is accepted, the one behind it and -1 are refused"""
    e, _ = _host()
    assert e.add_node(19, 2, 2, [63.0]) >= 0
    for kind in (20, -1):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.add_node(kind, 2, 2, [])
        assert ei.value.code == INVALID
    e.update()


# ================================================================================================ CPU tier: mirror, header, ffi.rs
def test_typed_mirror_header_and_generated_ffi():
    import firewheel_amd as fa
    from firewheel_amd import graph as G

    node = fa.DuckerNode()
    assert (node.KIND, node.channels, node.key_channels, node.num_inputs) == (DUCKER, 2, 2, 4)
    assert node.params() == [0.05, 0.25, 480.0, 12000.0, 4800.0]
    assert fa.DuckerNode(0.1, 0.5, 7, 100, 3, channels=1, key_channels=3).params() == [0.1, 0.5, 7.0, 100.0, 3.0]
    assert (node.attack_secs(48000), node.release_secs(48000), node.hold_secs(48000)) == (0.01, 0.25, 0.1)
    assert fa.DuckerNode.from_secs(48000, 0.01, 0.25, 0.1).params() == node.params()
    for db in (-26.0, -12.0, 0.0):   # the decibel arguments go through MeterNode.db_to_gain
        dn = fa.DuckerNode(threshold_db=db, depth_db=db / 2)
        assert fwapi.bits(F32(dn.threshold)) == fwapi.bits(G.MeterNode.db_to_gain(db))
        assert fwapi.bits(F32(dn.depth)) == fwapi.bits(G.MeterNode.db_to_gain(db / 2))
    # the node the raw call builds: same kind, same parameter list, accepted by the same checks
    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=0, num_graph_outputs=2)
    v = cx.add_node(2, 2, G.VolumeNode(50.0))
    m = cx.add_node(node.num_inputs, node.channels, node)
    for c in range(2):
        cx.connect(v, c, m, c)
        cx.connect(v, c, m, 2 + c)
        cx.connect(m, c, cx.graph_out_node(), c)
    cx.update()
    with pytest.raises(fa.FwgpuError):
        cx.add_node(2, 2, fa.DuckerNode())
    bad = cx.add_node(4, 2, fa.DuckerNode(threshold=0.0))
    with pytest.raises(fa.FwgpuError):
        cx.update()
    cx.remove_node(bad)
    cx.update()
    cx.close()
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    assert re.search(r"FWGPU_DUCKER = 18\b", hdr)
    types = open(os.path.join(ROOT, "firewheel_amd", "csrc", "fwgpu_types.h")).read()
    assert re.search(r"K_DUCKER = 18\b", types)
    assert re.search(r"#define DUCK_WIN_MAX 32768u", types) and re.search(r"#define DUCK_HOLD_MAX 32768u", types)
    ffi = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "ffi.rs")).read()
    assert "pub const FWGPU_DUCKER: c_int = 18;" in ffi
    assert "ffi::FWGPU_DUCKER" in open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "nodes.rs")).read()


# ================================================================================================ GPU tier
# ---- G1: graph_in(n + k) -> ducker -> graph_out(n) on the level executor
G1 = [  # (max_block_frames, A, R, H, n, k, T, D)
    (64, 1, 1, 0, 1, 1, 0.05, 0.25),          # a plain gate
    (64, 7, 100, 3, 2, 2, 0.05, 0.0),         # small windows
    (64, 64, 333, 129, 2, 1, 0.2, 0.5),       # the window spans eight blocks
    (256, 48, 3000, 500, 8, 8, 0.05, 0.25),   # the window is longer than whole calls: history reaches across several
    (256, 300, 50, 0, 1, 1, 0.01, 0.1),       # A > R
    (96, 33, 1000, 65, 2, 2, 0.05, 0.25),     # a block length that is no multiple of 64, W no multiple of 32
    (512, CAP, CAP, CAP, 2, 1, 0.05, 0.25),   # the caps, on a stream just over 2 x 32768 + 512 x 8 frames
]


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,A,R,H,n,k,T,D", G1)
def test_g1_stream_graphs(mbf, A, R, H, n, k, T, D):
    total = 2 * CAP + 512 * 8 + 1 if A == CAP else None
    calls, x, key, marks = probe(n, k, mbf, T, A, R, H, seed=100 * n + mbf + A, total=total)
    if total:
        assert total <= sum(calls) <= total + 5 * mbf
    want = model(x, key, T, D, A, R, H)
    u = amount(gate(key, T), A, R, H)
    ia, ib = marks["idle"]
    assert not u[ia:ib].any() and (fwapi.bits(want[:, ia:ib]) == 0x80000000).all()
    assert (u[marks["open"][0] + max(A, R) - 1:marks["open"][1]] == 1.0).all()
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=n + k, num_graph_outputs=n, max_batch=8)
    m = g.add_node(DUCKER, n + k, n, [T, D, float(A), float(R), float(H)])
    for c in range(n + k):
        g.connect(g.graph_in_node, c, m, c)
    for c in range(n):
        g.connect(m, c, g.graph_out_node, c)
    g.update()
    assert g.cx.plan_kind() == 0
    inp_all = np.concatenate([x, key], axis=0)
    a = 0
    for i, f in enumerate(calls):
        inp = np.ascontiguousarray(inp_all[:, a:a + f].T).ravel()
        y = planar(g.process_interleaved(f, n_out_ch=n, inp=inp, n_in_ch=n + k), n)
        assert_bits(y, want[:, a:a + f], "n %d k %d mbf %d A %d R %d H %d call %d (%d frames at %d)" % (n, k, mbf, A, R, H, i, f, a))
        a += f


# ---- G2: the desk; the dialogue samplers are stopped and restarted by messages between calls
G2_MBF = 256
G2_CALLS = [3, 4, 2, 4, 3, 4, 2, 4, 3]    # blocks; max_batch 4
G2_STOP_BEFORE, G2_PLAY_BEFORE = (2, 6), (4, 7)


def _g2_run(e, d):
    outs = []
    for i, kb in enumerate(G2_CALLS):
        if i in G2_STOP_BEFORE:
            for s in d.dialogue:
                e.sampler_stop(s)
        if i in G2_PLAY_BEFORE:
            for s in d.dialogue:
                e.sampler_play(s)
        outs.append(np.asarray(e.process_interleaved(kb * G2_MBF, n_out_ch=4)))
    return planar(np.concatenate(outs), 4)


@pytest.mark.gpu
def test_g2_dialogue_ducks_music_on_the_desk():
    o = oracle(G2_MBF)
    ro = _g2_run(o, desk(o, None))
    M, Dg = ro[0:2], ro[2:4]
    level = np.abs(Dg).max(axis=0)
    T = float(F32(np.percentile(level[level > 0], 90)))     # the gate chatters while the dialogue sounds
    A, R, H, D = 48, 700, 100, 0.25
    assert (level == 0).sum() > 2 * G2_MBF                   # ... and the key goes flag-silent while it does not
    u = amount(gate(Dg, T), A, R, H)
    assert u.max() == 1.0 and (u == 0).sum() > 100 and ((u > 0) & (u < 1)).sum() > 1000
    want = np.concatenate([model(M, Dg, T, D, A, R, H), Dg], axis=0)
    t = GpuEngine(max_block_frames=G2_MBF, num_graph_outputs=4, max_batch=4)
    rt = _g2_run(t, desk(t, "volume"))
    assert_bits(rt, ro, "the twin")
    g = GpuEngine(max_block_frames=G2_MBF, num_graph_outputs=4, max_batch=4)
    rg = _g2_run(g, desk(g, "duck", duck=(T, D, float(A), float(R), float(H))))
    assert g.cx.plan_kind() == t.cx.plan_kind() and g.cx.plan_fused_voices() == t.cx.plan_fused_voices() == 8
    assert_bits(rg, want, "[model(M, Dg), Dg]")


# ---- G3: edits
@pytest.mark.gpu
def test_g3_connected_into_a_sounding_graph_replaced_and_carried_across_an_edit():
    mbf = 256
    D, A, R, H = 0.25, 48.0, 700.0, 20.0   # a tenth of the dialogue's frames pass T: a hold of 20 lets the gate chatter, one of 100 never closes it
    duck = {}   # (the threshold is taken from the dialogue bus the oracle renders, before the GPU graph is built)
    phases = [[3 * mbf, 2 * mbf], [4 * mbf, 2 * mbf, 3 * mbf], [2 * mbf, 4 * mbf], [3 * mbf, 4 * mbf, 2 * mbf]]

    def run(e, gpu):
        d = desk(e, None)
        outs = [np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in phases[0]]

        def insert():
            d.duck = e.add_node(DUCKER, 4, 2, [duck["T"], D, A, R, H])
            e.connect_stereo(d.M, d.duck)
            e.connect_stereo(d.Dg, d.duck, 2)
            e.connect_stereo(d.duck, e.graph_out_node)
            e.update()

        if gpu:  # the ducker goes in between M and graph_out
            for c in range(2):
                e.disconnect(d.M, c, e.graph_out_node, c)
            insert()
        outs += [np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in phases[1]]
        if gpu:  # ... is removed and added again in one update: a new node, a fresh history
            e.remove_node(d.duck)
            insert()
        outs += [np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in phases[2]]
        end = _voice(e, d, [55.0])   # one more music voice on M's free ports, while ducked
        e.connect_stereo(end, d.M, 2 * d.n_music)
        e.update()
        _start(e, d.samplers[-1], d.seed, len(d.samplers) - 1, SALT)
        outs += [np.asarray(e.process_interleaved(f, n_out_ch=4)) for f in phases[3]]
        return planar(np.concatenate(outs), 4)

    ro = run(oracle(mbf), False)
    level = np.abs(ro[2:]).max(axis=0)
    T = duck["T"] = float(F32(np.percentile(level, 90)))
    g = GpuEngine(max_block_frames=mbf, num_graph_outputs=4, max_batch=4)
    rg = run(g, True)
    n1 = sum(phases[0])
    n2 = n1 + sum(phases[1])
    n3 = n2 + sum(phases[2])
    assert_bits(rg[:, :n1], ro[:, :n1], "before the ducker")
    assert_bits(rg[2:], ro[2:], "the dialogue bus")
    params = (T, D, int(A), int(R), int(H))
    assert_bits(rg[:2, n1:n2], model(ro[:2, n1:n2], ro[2:, n1:n2], *params), "from the activation on: a history of zeros")
    assert_bits(rg[:2, n2:], model(ro[:2, n2:], ro[2:, n2:], *params), "from the second activation on, across the voice edit")
    u1 = amount(gate(ro[2:, n1:n2], T), *params[2:])
    u2 = amount(gate(ro[2:, n2:], T), *params[2:])
    mid = (u2 > 0) & (u2 < 1)
    assert 0 < u1[-1] < 1 and 0 < u2[n3 - n2 - 1] < 1   # part-way ducked at the swap and at the edit: the windows hold ones and zeros
    assert mid.sum() > 500 and mid[n3 - n2:].sum() > 500   # ... and the gain keeps moving, after the edit too


# ---- G4: fwgpu_node_process
@pytest.mark.gpu
def test_g4_node_process_keeps_the_history_between_calls():
    mbf, f = 256, 100
    T, D, A, R, H = 0.3, 0.25, 20, 150, 40
    g = GpuEngine(max_block_frames=mbf)
    m = g.add_node(DUCKER, 3, 2, [T, D, float(A), float(R), float(H)])
    g.connect_stereo(m, g.graph_out_node)
    g.update()
    rng = np.random.default_rng(8)
    blocks = 6
    x = rng.uniform(-0.5, 0.5, size=(2, blocks * f)).astype(F32)
    key = rng.uniform(-0.25, 0.25, size=(1, blocks * f)).astype(F32)
    key[0, 70:95] *= F32(3.0)        # held and released into the following calls
    key[0, 330:333] = F32(0.9)
    key[0, 480:520] *= F32(4.0)      # across a call boundary
    seen_key, seen_x = key.copy(), x.copy()
    seen_key[0, f:2 * f] = 0.0       # the key is flagged silent in the second call: it counts as +0.0 and is not read
    seen_x[1, 4 * f:5 * f] = 0.0     # main channel 1 is flagged silent in the fifth: zeros out, flagged
    want = model(seen_x, seen_key, T, D, A, R, H)
    u = amount(gate(seen_key, T), A, R, H)
    assert u[f] > 0 and u[5 * f] > 0 and u.max() == 1.0
    for i in range(blocks):
        sl = slice(i * f, (i + 1) * f)
        ins = [x[0, sl], x[1, sl] if i != 4 else np.full(f, 55.0, dtype=F32), key[0, sl] if i != 1 else np.full(f, 77.0, dtype=F32)]
        mask = 0b100 if i == 1 else (0b010 if i == 4 else 0)
        y, om = g.node_process(m, f, ins, 2, in_mask=mask)
        assert om == (0b10 if i == 4 else 0)
        assert_bits(y, want[:, sl], "B1 call %d" % i)


# ---- G5: two duckers, a limiter, a biquad and a volume in one level: every launch bit a level below the sources can have
@pytest.mark.gpu
def test_g5_two_duckers_and_a_limiter_side_by_side():
    from test_limiter import model as limiter_model

    mbf = 256
    calls = [2 * mbf, 4 * mbf, mbf, 3 * mbf + 37, 1, 4 * mbf]
    N = sum(calls)
    rng = np.random.default_rng(12)
    inp = rng.uniform(-0.5, 0.5, size=(8, N)).astype(F32)
    inp[2] *= (rng.uniform(size=N) < 0.02) * F32(1.0) + F32(0.1)     # key of ducker 1: sparse spikes above 0.1
    inp[4:6, :] *= F32(0.1)
    inp[5, 600:750] *= F32(9.0)                                      # key of ducker 2: its second channel only, chattering ...
    inp[5, 750:900] += np.copysign(F32(0.15), inp[5, 750:900])       # ... then above 0.1 in every frame, for longer than max(A, R)
    inp[6:8, 1000:1040] *= F32(5.0)                                  # the limiter's bus passes its ceiling

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
            d1 = e.add_node(DUCKER, 3, 2, [0.1, 0.25, 16.0, 400.0, 30.0])
            d2 = e.add_node(DUCKER, 3, 1, [0.1, 0.0, 100.0, 64.0, 0.0])
            lim = e.add_node(LIMITER, 2, 2, [1.0, 0.0])
            for c in range(3):
                e.connect(gi, c, d1, c)
                e.connect(gi, 3 + c, d2, c)
            for c in range(2):
                e.connect(d1, c, go, 4 + c)
                e.connect(gi, 6 + c, lim, c)
                e.connect(lim, c, go, 7 + c)
            e.connect(d2, 0, go, 6)
        e.update()

    def run(e, n_out):
        a, outs = 0, []
        for f in calls:
            outs.append(np.asarray(e.process_interleaved(f, n_out_ch=n_out, inp=np.ascontiguousarray(inp[:, a:a + f].T).ravel(), n_in_ch=8)))
            a += f
        return planar(np.concatenate(outs), n_out)

    o = OracleEngine(max_block_frames=mbf, num_graph_inputs=8, num_graph_outputs=4, short_blocks=True)
    build(o, False)
    ro = run(o, 4)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=8, num_graph_outputs=9, max_batch=4)
    build(g, True)
    rg = run(g, 9)
    assert_bits(rg[0:4], ro, "the volume and the biquad beside them")
    assert_bits(rg[4:6], model(inp[0:2], inp[2:3], 0.1, 0.25, 16, 400, 30), "ducker 1")
    assert_bits(rg[6:7], model(inp[3:4], inp[4:6], 0.1, 0.0, 100, 64, 0), "ducker 2")
    assert_bits(rg[7:9], limiter_model(inp[6:8], 1.0, 0), "the limiter")
    assert amount(gate(inp[2:3], 0.1), 16, 400, 30).max() == 1.0 and amount(gate(inp[4:6], 0.1), 100, 64, 0).max() == 1.0
