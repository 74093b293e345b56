"""The bus compressor node (FWGPU_COMPRESSOR = 21; SPEC).

The reference for sample values is tests/compressor_model.py: the SPEC's text in numpy, applied to the whole stream since the node's
activation and sliced per call.  Every comparison on the GPU tier is `fwapi.bits` equality.

CPU tier: the model against its brute-force twin, the SPEC's properties, the table, shapes and creation parameters on the host-only
harness (whose launch stubs know a closed list of bus kinds: compressor graphs go as far as update() there), the planner's decision, the
typed Python mirror, the header, fwgpu_types.h, ffi.rs and nodes.rs.

GPU tier: G1 stream graphs on the level executor, G2 a voice bank with a compressor and a limiter in its master chain, G3 graph edits,
G4 fwgpu_node_process, G5 a compressor, a ducker and a limiter at one level.
"""
import math
import os
import re

import numpy as np
import pytest

import compressor_model as cm
import fwapi
from busnodes import DUCKER, LIMITER, _host, _start, _voice, assert_bits, planar
from fwapi import GpuEngine, HostOnlyEngine

COMPRESSOR = 21
INVALID = -20
F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SETS = [(1, 1, 0), (7, 64, 1), (64, 63, 64), (333, 65, 63), (48, 480, 2048), (32768, 1, 0), (1, 32768, 2048)]   # (A, R, H)
RATIOS, KNEES = (1.0, 2.0, 4.0, 8.0, 1000.0), (0.0, 6.0, 12.0, 24.0)
SALT = 83   # (busnodes._start)


def pattern_calls(mbf, at_least):
    pat = [1, 17, mbf - 1, mbf, 2 * mbf + 5, 7 * mbf + 37]
    calls = []
    while sum(calls) < at_least:
        calls.append(pat[len(calls) % len(pat)])
    return calls


def probe(n, mbf, T0, A, R, H, seed, tail=6000):
    """-> (calls, x [n][N], marks).  Noise below T0 with, above it: random bursts (before and behind the quiet stretch, across call and
    block boundaries), one longer than min(max(A, R), 3000) frames, levels of exactly T0 and one ulp to either side, levels on a knot
    and one ulp to either side, levels above 2^20 * T0, an infinity, NaNs, short runs of -0.0; one quiet stretch longer than W."""
    W = max(A, R) + H
    head = 3000
    calls = pattern_calls(mbf, head + W + 150 + tail)
    N = sum(calls)
    rng = np.random.default_rng(seed)
    T0 = F32(T0)
    x = (rng.uniform(-0.8, 0.8, size=(n, N)) * float(T0)).astype(F32)

    def burst(a, b, lo=1.5, hi=60.0):
        for c in range(n):
            x[c, a:b] = (rng.uniform(lo, hi, size=b - a) * float(T0) * rng.choice([-1.0, 1.0], size=b - a)).astype(F32)

    qa, qb = head, head + W + 150
    for lo_, hi_ in ((40, head - 100), (qb + 50, N - 200)):
        for _ in range(10):
            a = int(rng.integers(lo_, hi_))
            burst(a, min(a + int(rng.integers(1, 300)), hi_))
    long_ = min(max(A, R), 3000) + 100
    burst(qb + 200, qb + 200 + long_, 3.9, 4.1)
    p = qb + 200 + long_ + 700
    specials = [T0, np.nextafter(T0, F32(0)), np.nextafter(T0, F32(9)), F32(T0 * F32(8)), np.nextafter(F32(T0 * F32(8)), F32(0)),
                np.nextafter(F32(T0 * F32(8)), F32(1e9)), F32(T0 * F32(1.5)), F32(T0 * F32(2.0 ** 21)), F32(T0 * F32(2.0 ** 20)),
                np.nextafter(F32(T0 * F32(2.0 ** 20)), F32(0)), F32(np.inf), F32(-np.inf)]
    for j, v in enumerate(specials):
        x[:, p + 9 * j] = F32(0)
        x[j % n, p + 9 * j] = v if j % 2 else -v
    x[0, p + 200:p + 203] = F32(np.nan)
    x[:, p + 230] = F32(np.nan)                       # every channel NaN: the key is +0.0
    x[:, 10:20] = F32(-0.0)
    x[:, qa + W + 20:qa + W + 30] = F32(-0.0)
    return calls, x, {"quiet": (qa, qb)}


# ================================================================================================ CPU tier: the model and the table
@pytest.mark.parametrize("A,R,H", SETS)
def test_model_equals_the_brute_force_evaluation(A, R, H):
    rng = np.random.default_rng(A + R + H)
    W = max(A, R) + H
    N = W + 700
    q = np.full(N, 65535, dtype=np.uint32)
    for _ in range(12):
        a = int(rng.integers(0, N - 10))
        q[a:a + int(rng.integers(1, max(2, min(W, 400))))] = rng.integers(0, 65536)
    q[5:9] = rng.integers(0, 65536, size=4)
    g = cm.gains(q, A, R, H)
    frames = sorted(set(list(range(0, 30)) + [int(v) for v in np.linspace(30, N - 1, 50 if W > 4000 else 300)]))
    b = cm.brute_gains(q, A, R, H, frames)
    assert np.array_equal(fwapi.bits(g[frames]), fwapi.bits(b)), (A, R, H)


@pytest.mark.parametrize("A,R,H", SETS[:5])
def test_model_is_unity_bit_for_bit_after_a_quiet_window_and_bounded(A, R, H):
    T, ratio, knee = 0.25, 4.0, 6.0
    T0, G = cm.knee_start(T, knee), cm.table(ratio, knee)
    calls, x, marks = probe(2, 64, T0, A, R, H, seed=5)
    W = max(A, R) + H
    g = cm.gains(cm.target_q(cm.key_of(x), T0, G), A, R, H)
    qa, qb = marks["quiet"]
    assert (cm.key_of(x)[qa:qb] <= T0).all() and qb - qa > W
    assert (fwapi.bits(g[qa + W:qb]) == fwapi.bits(F32(1.0))).all()
    y = cm.model(x, T, ratio, knee, A, R, H, 1.0)
    assert_bits(y[:, qa + W:qb], x[:, qa + W:qb], "quiet: the input bit for bit")
    assert (fwapi.bits(y[:, qa + W + 20:qa + W + 30]) == 0x80000000).all()
    assert g.max() <= 1.0 and g.min() >= float(G[320]) - 1.0 / 65535 and g.min() < 0.5


def test_model_step_response_plateau_and_steady_level():
    """A <= R: down linearly over A, back linearly over R beginning H frames later; a burst shorter than R plateaus at
    1 - (1 - t) * len / R; a steady level settles at q / 65535, within 2^-16 of the curve"""
    A, R, H = 10, 100, 7
    T0, G = cm.knee_start(0.25, 6.0), cm.table(4.0, 6.0)
    key = np.zeros(1500, dtype=F32)
    lvl = F32(0.25 * 10 ** (12 / 20.0))
    key[100:400] = lvl
    key[700:730] = lvl
    q = cm.target_q(key, T0, G)
    g = cm.gains(q, A, R, H).astype(np.float64)
    t = q[100] / 65535.0
    assert abs(t - float(cm.target_t(key[100:101], T0, G)[0])) <= 2.0 ** -16
    assert abs(20 * math.log10(t) + 9.0) < 0.01                                   # 12 dB over at 4:1: 9 dB down
    assert abs(g[100 + A - 1] - t) < 1e-6 and g[100 + A - 2] > t + 1e-4         # full reduction after A frames
    assert np.allclose(np.diff(g[99:100 + A]), -(1 - t) / A, atol=1e-6)          # ... linearly
    assert abs(g[399 + H] - t) < 1e-6 and abs(g[399 + H + 1] - (t + (1 - t) / R)) < 1e-6   # the release begins H frames later
    assert np.allclose(np.diff(g[399 + H:399 + H + R + 1]), (1 - t) / R, atol=1e-6) and g[399 + H + R] == 1.0
    plateau = 1 - (1 - t) * (30 + H) / R                                         # (the hold lengthens the burst by H)
    assert abs(g[729 + H + A] - plateau) < 1e-6 and abs(g[700 + R - 1] - plateau) < 1e-6 and g[729 + H + R] == 1.0
    assert abs(g[350] - q[350] / 65535.0) < 1e-7


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("knee", KNEES)
def test_table_properties(ratio, knee):
    G = cm.table(ratio, knee)
    assert fwapi.bits(G[0]) == fwapi.bits(F32(1.0)) and (np.diff(G) <= 0).all() and G.size == 321
    T0 = cm.knee_start(0.25, knee)
    lv = np.exp(np.linspace(math.log(1e-4), math.log(100.0), 20001)).astype(F32)
    t = cm.target_t(lv, T0, G).astype(np.float64)
    u = lv.astype(np.float64) / float(T0)
    want = np.array([cm.exact_gr_db(20 * math.log10(v), ratio, knee) if v > 1 else 0.0 for v in u])
    sat = u >= 2.0 ** 20
    err = np.abs(20 * np.log10(t) - want)[~sat]
    assert err.max() <= 0.01, err.max()
    if ratio == 1.0:   # the identity times M
        assert (fwapi.bits(G) == fwapi.bits(F32(1.0))).all()
        x = (np.random.default_rng(3).uniform(-50, 50, size=(2, 500))).astype(F32)
        assert_bits(cm.model(x, 0.25, 1.0, knee, 7, 64, 1, 0.5), (x * F32(0.5)).astype(F32), "ratio 1")


# ================================================================================================ CPU tier: shapes and parameters
GOOD = [0.25, 4.0, 6.0, 240.0, 12000.0, 0.0, 1.0]


@pytest.mark.parametrize("n_in,n_out", [(4, 2), (2, 0), (9, 9), (0, 0), (2, 3)])
def test_shapes_refused_at_add_node(n_in, n_out):
    e, _ = _host()
    with pytest.raises(e.fa.FwgpuError) as ei:
        e.add_node(COMPRESSOR, n_in, n_out, GOOD)
    assert ei.value.code == INVALID and "CompressorNode" in str(ei.value)
    e.update()  # nothing was added


def _with(slot, value):
    p = list(GOOD)
    p[slot] = value
    return p


BAD_PARAMS = ([_with(s, float("nan")) for s in range(7)] + [_with(s, float("inf")) for s in range(7)] + [_with(s, float("-inf")) for s in range(7)] +
              [_with(0, 0.0), _with(0, 1001.0), _with(1, 0.99), _with(1, 1001.0), _with(2, -0.1), _with(2, 24.5), _with(3, 0.0), _with(3, 32769.0),
               _with(3, 1.5), _with(4, 0.0), _with(4, 32769.0), _with(4, 100.25), _with(5, -1.0), _with(5, 2049.0), _with(5, 0.5),
               _with(6, 0.0), _with(6, 1001.0), [float("nan")], [0.25, 0.5]])


@pytest.mark.parametrize("params", BAD_PARAMS)
def test_parameters_refused_at_update(params):
    e, v = _host()
    m = e.add_node(COMPRESSOR, 2, 2, params)
    for _ in range(2):  # (still there, still refused)
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.update()
        assert ei.value.code == INVALID and "CompressorNode" in str(ei.value)
    e.remove_node(m)
    good = e.add_node(COMPRESSOR, 2, 2, GOOD)
    e.connect_stereo(v, good)
    e.update()  # the graph is usable


ACCEPTED = [[], [0.25], GOOD, [1e-6, 1.0, 0.0, 1.0, 1.0, 0.0, 0.001], [1000.0, 1000.0, 24.0, 32768.0, 32768.0, 2048.0, 1000.0],
            [0.25, 4.0, 6.0, 32768.0, 1.0, 0.0, 1.0], [0.25, 4.0, 6.0, 1.0, 32768.0, 2048.0, 1.0]]


@pytest.mark.parametrize("params", ACCEPTED)
@pytest.mark.parametrize("n", [1, 2, 8])
def test_parameters_and_shapes_accepted_and_set_param_refused(params, n):
    e, _ = _host()
    m = e.add_node(COMPRESSOR, n, n, params)
    e.update()
    assert e.cx.plan_node_level(m) >= 0
    for slot in range(7):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.set_param(m, slot, 0.5)
        assert ei.value.code == INVALID


def test_node_kinds_end_at_21():
    """fwgpu_add_node: the last kind with a valid shape is accepted, the one behind it and -1 are refused"""
    e, _ = _host()
    assert e.add_node(COMPRESSOR, 2, 2, []) >= 0
    for kind in (22, -1):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.add_node(kind, 2, 2, [])
        assert ei.value.code == INVALID
    e.update()


# ================================================================================================ the voice bank with a master chain
class Bank(object):
    pass


DRY = ["v", "vp", "", "pv", "vc", "v", "vp", "p"]


def bank(e, master, seed=0):
    """eight dry voices -> two leaf sums -> root sum -> the master chain -> graph_out 0,1.  master: a list of ("C", params) |
    ("L", ceiling, hold) | ("v", percent)"""
    b = Bank()
    b.e, b.samplers, b.node = e, [], {}
    rng = np.random.default_rng(7300 + seed)
    ends = [_voice(e, b, sh, i, rng) for i, sh in enumerate(DRY)]
    root = e.sum(2)
    for k in range(2):
        leaf = e.sum(4)
        for p_, nd in enumerate(ends[4 * k:4 * k + 4]):
            e.connect_stereo(nd, leaf, 2 * p_)
        e.connect_stereo(leaf, root, 2 * k)
    cur = root
    for i, spec in enumerate(master):
        nd = e.add_node(COMPRESSOR, 2, 2, list(spec[1])) if spec[0] == "C" else (
            e.add_node(LIMITER, 2, 2, [spec[1], spec[2]]) if spec[0] == "L" else e.volume(spec[1]))
        b.node[i] = nd
        e.connect_stereo(cur, nd)
        cur = nd
    e.connect_stereo(cur, e.graph_out_node)
    e.update()
    for i, s in enumerate(b.samplers):
        _start(e, s, seed, i, SALT)
    return b


def test_a_master_compressor_changes_no_planner_decision():
    """update() only: the twin with a 2 -> 2 volume in the compressor's place has the same plan kind and fused voices"""
    e0 = HostOnlyEngine(max_block_frames=256, max_batch=4)
    bank(e0, [("v", 100.0)])
    e = HostOnlyEngine(max_block_frames=256, max_batch=4)
    b = bank(e, [("C", GOOD)])
    assert e.cx.plan_kind() == e0.cx.plan_kind() == 1 and e.cx.plan_fused_voices() == e0.cx.plan_fused_voices() == 8
    assert e.cx.plan_node_level(b.node[0]) >= 0


# ================================================================================================ CPU tier: mirror, header, ffi.rs
def test_typed_mirror_header_types_and_generated_ffi():
    import firewheel_amd as fa
    from firewheel_amd import graph as G

    node = fa.CompressorNode()
    assert (node.KIND, node.channels) == (COMPRESSOR, 2)
    assert node.params() == GOOD
    assert fa.CompressorNode(0.1, 8, 12, 7, 100, 3, 2.0, channels=1).params() == [0.1, 8.0, 12.0, 7.0, 100.0, 3.0, 2.0]
    assert (node.attack_secs(48000), node.release_secs(48000), node.hold_secs(48000)) == (0.005, 0.25, 0.0)
    assert fa.CompressorNode.from_secs(48000, 0.005, 0.25, 0.0).params() == node.params()
    for db in (-26.0, -12.0, 0.0):   # the decibel arguments go through MeterNode.db_to_gain
        cn = fa.CompressorNode(threshold_db=db, makeup_db=-db / 2)
        assert fwapi.bits(F32(cn.threshold)) == fwapi.bits(G.MeterNode.db_to_gain(db))
        assert fwapi.bits(F32(cn.makeup)) == fwapi.bits(G.MeterNode.db_to_gain(-db / 2))
    # static_gain is the model's table curve
    lv = np.exp(np.linspace(math.log(1e-3), math.log(1e7), 997)).astype(F32)
    for ratio, knee in ((4.0, 6.0), (1000.0, 0.0), (2.0, 24.0)):
        cn = fa.CompressorNode(0.25, ratio, knee)
        assert_bits(cn.table(), cm.table(ratio, knee), "table")
        assert_bits(cn.static_gain(lv), cm.target_t(lv, cm.knee_start(0.25, knee), cm.table(ratio, knee)), "static_gain")
    assert fa.CompressorNode().static_gain(0.1) == 1.0
    # the node the raw call builds: same kind, same parameter list, accepted by the same checks
    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=0, num_graph_outputs=2)
    v = cx.add_node(2, 2, G.VolumeNode(50.0))
    m = cx.add_node(node.channels, node.channels, node)
    for c in range(2):
        cx.connect(v, c, m, c)
        cx.connect(m, c, cx.graph_out_node(), c)
    cx.update()
    with pytest.raises(fa.FwgpuError):
        cx.add_node(4, 2, fa.CompressorNode())
    bad = cx.add_node(2, 2, fa.CompressorNode(ratio=0.5))
    with pytest.raises(fa.FwgpuError):
        cx.update()
    cx.remove_node(bad)
    cx.update()
    cx.close()
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    assert re.search(r"FWGPU_COMPRESSOR = 21\b", hdr)
    assert re.search(r"#define FWGPU_COMPRESSOR_WIN_MAX 32768\b", hdr) and re.search(r"#define FWGPU_COMPRESSOR_HOLD_MAX 2048\b", hdr)
    assert re.search(r"#define FWGPU_COMPRESSOR_CH_MAX 8\b", hdr)
    types = open(os.path.join(ROOT, "firewheel_amd", "csrc", "fwgpu_types.h")).read()
    assert re.search(r"K_COMPRESSOR = 21\b", types) and re.search(r"K_KIND_MAX = K_COMPRESSOR\b", types)
    assert re.search(r"#define COMP_WIN_MAX 32768u", types) and re.search(r"#define COMP_HOLD_MAX 2048u", types) and re.search(r"#define COMP_CH_MAX 8\b", types)
    assert re.search(r"LB_COMPRESSOR = 128\b", types) and re.search(r"if \(kind == K_COMPRESSOR\) return 7;", types)
    assert "comp_state_ok" in types and "comp_ext_len" in types
    ffi = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "ffi.rs")).read()
    assert "pub const FWGPU_COMPRESSOR: c_int = 21;" in ffi and "pub const FWGPU_COMPRESSOR_WIN_MAX: u32 = 32768;" in ffi
    assert "pub const FWGPU_COMPRESSOR_HOLD_MAX: u32 = 2048;" in ffi and "pub const FWGPU_COMPRESSOR_CH_MAX: u32 = 8;" in ffi
    nodes = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "nodes.rs")).read()
    assert "pub struct GpuCompressorNode" in nodes and "ffi::FWGPU_COMPRESSOR" in nodes


# ================================================================================================ GPU tier
# ---- G1: graph_in(n) -> compressor -> graph_out(n) on the level executor
G1 = [  # (max_block_frames, max_batch, n, A, R, H, T, ratio, knee, M)
    (64, 1, 1, 1, 1, 0, 0.25, 4.0, 6.0, 1.0),             # windows shorter than a thread's four frames; one block per launch
    (64, 3, 2, 7, 64, 1, 0.25, 8.0, 0.0, 1.0),            # the release window equals a block; hard knee
    (96, 64, 2, 64, 63, 64, 0.1, 2.0, 12.0, 0.5),         # a block length that is no multiple of 64; A > R; makeup
    (256, 3, 8, 333, 65, 63, 0.25, 4.0, 6.0, 1.0),        # longer than a block; eight channels, one of them disconnected
    (64, 64, 2, 48, 480, 2048, 0.05, 1000.0, 24.0, 1.0),  # the hold at its cap: W longer than the whole batch of most calls
    (256, 64, 1, 32768, 1, 0, 0.25, 4.0, 6.0, 2.0),       # the attack window at its cap
    (96, 3, 2, 1, 32768, 2048, 0.25, 4.0, 6.0, 1.0),      # the release window and the hold at their caps: the largest W
]


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,max_batch,n,A,R,H,T,ratio,knee,M", G1)
def test_g1_stream_graphs(mbf, max_batch, n, A, R, H, T, ratio, knee, M):
    T0 = cm.knee_start(T, knee)
    calls, x, marks = probe(n, mbf, T0, A, R, H, seed=100 * n + mbf + A)
    W = max(A, R) + H
    dead = 5 if n == 8 else -1                     # this input is left unconnected: flagged silent in every block
    silent = np.zeros(x.shape, dtype=bool)
    if dead >= 0:
        silent[dead] = True
    want = cm.model(x, T, ratio, knee, A, R, H, M, silent=silent)
    qa, qb = marks["quiet"]
    if M == 1.0:
        live = [c for c in range(n) if c != dead]
        assert_bits(want[live, qa + W:qb], x[live, qa + W:qb], "the model at rest")
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=n, num_graph_outputs=n, max_batch=max_batch)
    m = g.add_node(COMPRESSOR, n, n, [T, ratio, knee, float(A), float(R), float(H), M])
    for c in range(n):
        if c != dead:
            g.connect(g.graph_in_node, c, m, c)
        g.connect(m, c, g.graph_out_node, c)
    g.update()
    assert g.cx.plan_kind() == 0
    a = 0
    for i, f in enumerate(calls):
        inp = np.ascontiguousarray(x[:, a:a + f].T).ravel()
        y = planar(g.process_interleaved(f, n_out_ch=n, inp=inp, n_in_ch=n), n)
        assert_bits(y, want[:, a:a + f], "n %d mbf %d A %d R %d H %d call %d (%d frames at %d)" % (n, mbf, A, R, H, i, f, a))
        a += f


# ---- G2: a voice bank, a compressor and then a limiter in its master chain
@pytest.mark.gpu
def test_g2_master_chain_of_a_voice_bank():
    from test_limiter import model as limiter_model

    mbf, calls = 256, [3, 4, 2, 4, 1, 4, 3]

    def run(e):
        return planar(np.concatenate([np.asarray(e.process_interleaved(k * mbf)) for k in calls]))

    t = GpuEngine(max_block_frames=mbf, max_batch=4)
    bank(t, [("v", 100.0), ("v", 100.0)])
    dry = run(t)
    level = np.abs(dry).max(axis=0)
    T = float(F32(np.percentile(level, 60)))
    params = [T, 4.0, 6.0, 48.0, 700.0, 20.0, 3.0]
    squeezed = cm.model(dry, T, 4.0, 6.0, 48, 700, 20, 3.0)
    gq = cm.gains(cm.target_q(cm.key_of(dry), cm.knee_start(T, 6.0), cm.table(4.0, 6.0)), 48, 700, 20)
    assert gq.min() < 0.8 and ((gq > gq.min()) & (gq < 1)).sum() > 1000
    want = limiter_model(squeezed, 0.5, 32)
    g = GpuEngine(max_block_frames=mbf, max_batch=4)
    bank(g, [("C", params), ("L", 0.5, 32.0)])
    got = run(g)
    assert g.cx.plan_kind() == t.cx.plan_kind() == 1 and g.cx.plan_fused_voices() == t.cx.plan_fused_voices() == 8
    assert g.cx.lazy_stats() == t.cx.lazy_stats(), (g.cx.lazy_stats(), t.cx.lazy_stats())
    assert_bits(got, want, "limiter(compressor(dry mix))")


# ---- G3: edits
@pytest.mark.gpu
def test_g3_connected_into_a_sounding_graph_replaced_and_carried_across_an_edit():
    mbf = 128
    P = (0.2, 4.0, 6.0, 30, 500, 10, 1.0)
    phases = [[3 * mbf, 2 * mbf], [4 * mbf, 2 * mbf + 5, 3 * mbf], [2 * mbf, 4 * mbf], [3 * mbf, 37, 2 * mbf]]
    N = sum(sum(p_) for p_ in phases)
    rng = np.random.default_rng(31)
    x = (rng.uniform(-1, 1, size=(2, N)) * (0.1 + 0.9 * (rng.uniform(size=N) < 0.3))).astype(F32)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=2, num_graph_outputs=4, max_batch=4)
    v = g.volume(100.0)
    for c in range(2):
        g.connect(g.graph_in_node, c, v, c)
        g.connect(v, c, g.graph_out_node, c)
    g.update()
    pos = [0]

    def run(fs):
        outs = []
        for f in fs:
            inp = np.ascontiguousarray(x[:, pos[0]:pos[0] + f].T).ravel()
            outs.append(np.asarray(g.process_interleaved(f, n_out_ch=4, inp=inp, n_in_ch=2)))
            pos[0] += f
        return planar(np.concatenate(outs), 4)

    def insert():
        m = g.add_node(COMPRESSOR, 2, 2, [float(p_) for p_ in P])
        g.connect_stereo(v, m)
        g.connect_stereo(m, g.graph_out_node)
        g.update()
        return m

    outs = [run(phases[0])]
    for c in range(2):
        g.disconnect(v, c, g.graph_out_node, c)
    m = insert()
    outs.append(run(phases[1]))
    g.remove_node(m)            # removed and added again in one update: a new node, a fresh history
    m = insert()
    outs.append(run(phases[2]))
    w = g.volume(50.0)          # an unrelated edit while the gain is moving
    for c in range(2):
        g.connect(g.graph_in_node, c, w, c)
        g.connect(w, c, g.graph_out_node, 2 + c)
    g.update()
    outs.append(run(phases[3]))
    got = np.concatenate(outs, axis=1)
    n1 = sum(phases[0])
    n2 = n1 + sum(phases[1])
    n3 = n2 + sum(phases[2])
    assert_bits(got[:2, :n1], x[:, :n1], "before the compressor")
    assert_bits(got[:2, n1:n2], cm.model(x[:, n1:n2], *P), "from the activation on: a history of unity")
    assert_bits(got[:2, n2:], cm.model(x[:, n2:], *P), "from the second activation on, across the edit")
    assert_bits(got[2:, n3:], (x[:, n3:] * F32(0.25)).astype(F32), "the other bus")
    g1 = cm.gains(cm.target_q(cm.key_of(x[:, n1:n2]), cm.knee_start(P[0], P[2]), cm.table(P[1], P[2])), *P[3:6])
    g2 = cm.gains(cm.target_q(cm.key_of(x[:, n2:]), cm.knee_start(P[0], P[2]), cm.table(P[1], P[2])), *P[3:6])
    assert g1[-1] < 0.99 and g2[n3 - n2 - 1] < 0.99    # reduced at the swap and at the edit: a wrong history would be heard


# ---- G4: fwgpu_node_process
@pytest.mark.gpu
def test_g4_node_process_keeps_the_history_between_calls():
    mbf, f, blocks = 256, 100, 6
    P = (0.3, 8.0, 6.0, 20, 150, 40, 1.5)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=2, max_batch=8)
    m = g.add_node(COMPRESSOR, 2, 2, [float(p_) for p_ in P])
    m2 = g.add_node(COMPRESSOR, 2, 2, [float(p_) for p_ in P])     # its twin renders the same stream in batches
    g.connect_stereo(g.graph_in_node, m2)
    g.connect_stereo(m2, g.graph_out_node)
    g.update()
    rng = np.random.default_rng(8)
    x = rng.uniform(-0.25, 0.25, size=(2, blocks * f)).astype(F32)
    x[0, 70:95] *= F32(3.0)          # held and released into the following calls
    x[1, 330:333] = F32(0.9)
    x[:, 480:520] *= F32(4.0)        # across a call boundary
    silent = np.zeros(x.shape, dtype=bool)
    silent[1, 4 * f:5 * f] = True    # channel 1 is flagged silent in the fifth call: zeros out, flagged
    want = cm.model(x, *P, silent=silent)
    for i in range(blocks):
        sl = slice(i * f, (i + 1) * f)
        ins = [x[0, sl], x[1, sl] if i != 4 else np.full(f, 55.0, dtype=F32)]
        y, om = g.node_process(m, f, ins, 2, in_mask=0b10 if i == 4 else 0)
        assert om == (0b10 if i == 4 else 0)
        assert_bits(y, want[:, sl], "B1 call %d" % i)
    batch = planar(g.process_interleaved(4 * f, inp=np.ascontiguousarray(x[:, :4 * f].T).ravel(), n_in_ch=2))
    assert_bits(batch, want[:, :4 * f], "the batch render of the first four calls' frames")


# ---- G5: a compressor, a ducker and a limiter in one level
@pytest.mark.gpu
def test_g5_compressor_ducker_and_limiter_side_by_side():
    from test_ducker import model as ducker_model
    from test_limiter import model as limiter_model

    mbf = 256
    calls = [2 * mbf, 4 * mbf, mbf, 3 * mbf + 37, 1, 4 * mbf]
    N = sum(calls)
    rng = np.random.default_rng(12)
    inp = rng.uniform(-0.5, 0.5, size=(7, N)).astype(F32)
    inp[0:2] *= (F32(0.2) + F32(1.5) * (rng.uniform(size=N) < 0.2)).astype(F32)   # the compressor's bus
    inp[4] *= (rng.uniform(size=N) < 0.02) * F32(1.0) + F32(0.1)                  # the ducker's key: sparse spikes above 0.1
    inp[5:7, 1000:1040] *= F32(5.0)                                               # the limiter's bus passes its ceiling
    P = (0.2, 4.0, 6.0, 16, 400, 30, 1.0)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=7, num_graph_outputs=6, max_batch=4)
    gi, go = g.graph_in_node, g.graph_out_node
    comp = g.add_node(COMPRESSOR, 2, 2, [float(p_) for p_ in P])
    duck = g.add_node(DUCKER, 3, 2, [0.1, 0.25, 16.0, 400.0, 30.0])
    lim = g.add_node(LIMITER, 2, 2, [1.0, 0.0])
    for c in range(2):
        g.connect(gi, c, comp, c)
        g.connect(gi, 5 + c, lim, c)
        g.connect(comp, c, go, c)
        g.connect(duck, c, go, 2 + c)
        g.connect(lim, c, go, 4 + c)
    for c in range(3):
        g.connect(gi, 2 + c, duck, c)
    g.update()
    assert g.cx.plan_node_level(comp) == g.cx.plan_node_level(duck) == g.cx.plan_node_level(lim)
    a, outs = 0, []
    for f in calls:
        outs.append(np.asarray(g.process_interleaved(f, n_out_ch=6, inp=np.ascontiguousarray(inp[:, a:a + f].T).ravel(), n_in_ch=7)))
        a += f
    rg = planar(np.concatenate(outs), 6)
    assert_bits(rg[0:2], cm.model(inp[0:2], *P), "the compressor")
    assert_bits(rg[2:4], ducker_model(inp[2:4], inp[4:5], 0.1, 0.25, 16, 400, 30), "the ducker")
    assert_bits(rg[4:6], limiter_model(inp[5:7], 1.0, 0), "the limiter")
