"""The crossfade node (FWGPU_CROSSFADE = 20; SPEC): two buses blended along an automated curve.

The reference for sample values and silence flags is `Model` below: the SPEC's position rule, gains and output rule in numpy float32,
one separately rounded operation at a time, applied block by block to the stream since the node's activation.  What the model takes as
input is obtained without the node: the stream input itself, or the OracleEngine's output of the same graph built without the node
(the oracle does not know the kind).  Every comparison on the GPU tier is `fwapi.bits` equality, silence flags included.

CPU tier: the model's properties; shapes, creation parameters and every refusal of fwgpu_crossfade_to on the host-only harness; the
typed mirror, the header and the generated ffi.rs; the planner on the harness against a 4 -> 2 SumNode twin.

GPU tier: G1 at rest, G2 a linear segment (serial walk, then the frozen path; max_batch 1 against 64), G3 Bezier segments, retargets,
jumps, G4 silence flags, G5 fwgpu_node_process, G6 one-block callbacks, G7 the hybrid plan beside fused voice banks.
"""
import os
import re

import numpy as np
import pytest

import fwapi
import scenarios
from busnodes import HARNESS_CALLS, LB_LEVEL, _host, _start, _voice, assert_bits, harness_batches, harness_run, planar, ragged_calls
from fwapi import GpuEngine, HostOnlyEngine, OracleEngine

CROSSFADE = 20
INVALID = -20
F32 = np.float32
LINEAR_LAW, EQUAL_POWER = 0, 1
XF_ITERS = 24
FRAMES_MAX = 1 << 24
EASE_IN_OUT = (0.42, 0.0, 0.58, 1.0)
OVERSHOOT = (0.3, -0.5, 0.7, 1.5)
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SALT = 83   # (busnodes._start: what tells this file's sources from the other bus nodes')


# ------------------------------------------------------------------------------------------------ the SPEC in numpy
def _bezier(t, a, d):
    """B(t; a, d) = ((q*t + b)*t + c)*t with c = 3*a; b = 3*(d - a) - c; q = (1 - c) - b: float32, one rounding per operation"""
    a, d = F32(a), F32(d)
    c = F32(3.0) * a
    b = F32(3.0) * (d - a) - c
    q = (F32(1.0) - c) - b
    return ((q * t + b) * t + c) * t


class Segment(object):
    def __init__(self, P0, P1, t0=0, dur=0, curve=None):
        self.P0, self.P1, self.t0, self.dur, self.curve = F32(P0), F32(P1), int(t0), int(dur), curve

    def position(self, n):
        """the position of the frames at node times n (int64 array) -> float32 array"""
        n = np.asarray(n, dtype=np.int64)
        p = np.full(n.shape, self.P1, dtype=F32)
        k = n - self.t0
        live = (k < self.dur) if self.dur else np.zeros(n.shape, dtype=bool)
        if not live.any():
            return p
        u = k[live].astype(F32) / F32(self.dur)
        y = u
        if self.curve is not None:
            x1, y1, x2, y2 = self.curve
            lo, hi = np.zeros_like(u), np.ones_like(u)
            for _ in range(XF_ITERS):
                m = (lo + hi) * F32(0.5)
                below = _bezier(m, x1, x2) < u
                lo, hi = np.where(below, m, lo), np.where(below, hi, m)
            y = np.where(u == 0, F32(0.0), _bezier((lo + hi) * F32(0.5), y1, y2)).astype(F32)
        q = self.P0 + ((self.P1 - self.P0) * y)
        p[live] = np.minimum(np.maximum(q, F32(0.0)), F32(1.0))
        return p


def gains(p, law):
    p = np.asarray(p, dtype=F32)
    if law == LINEAR_LAW:
        return F32(1.0) - p, p
    return np.sqrt(F32(1.0) - p), np.sqrt(p)


class Model(object):
    """one crossfader since its activation: `to` is a message at the start of the next block, `block` renders one block"""

    def __init__(self, n, position=0.0, law=EQUAL_POWER):
        self.n, self.law, self.T, self.seg = n, law, 0, Segment(position, position)

    def to(self, position, frames, curve=None):
        self.seg = Segment(self.seg.position([self.T])[0], position, self.T, frames, curve)

    def block(self, A, B, fa=None, fb=None):
        """A, B: [n][F] (None: the bus is unconnected); fa, fb: [n] bool, the channel is flagged silent -> (y [n][F], flags [n])"""
        n = self.n
        F = (A if A is not None else B).shape[1]
        fa = np.ones(n, dtype=bool) if A is None else (np.zeros(n, dtype=bool) if fa is None else np.asarray(fa, dtype=bool))
        fb = np.ones(n, dtype=bool) if B is None else (np.zeros(n, dtype=bool) if fb is None else np.asarray(fb, dtype=bool))
        zero = np.zeros((n, F), dtype=F32)
        A = np.where(fa[:, None], zero, zero if A is None else np.asarray(A, dtype=F32))      # flagged: counts as +0.0
        B = np.where(fb[:, None], zero, zero if B is None else np.asarray(B, dtype=F32))
        s = self.seg
        rest = s.dur == 0 or self.T - s.t0 >= s.dur
        p = s.position(self.T + np.arange(F, dtype=np.int64))
        a, b = gains(p, self.law)
        with np.errstate(invalid="ignore", over="ignore"):
            y = (A * a[None, :]) + (B * b[None, :])
        y = np.where((p == 0)[None, :], A, np.where((p == 1)[None, :], B, y)).astype(F32)
        flags = (fa & fb) | (fa & (rest and s.P1 == 0)) | (fb & (rest and s.P1 == 1))
        assert not fwapi.bits(y[flags]).any()      # what the rule flags is +0.0 throughout
        self.T += F
        return y, flags


def blocks_of(frames, mbf):
    """the block lengths of one process call"""
    return [mbf] * (frames // mbf) + ([frames % mbf] if frames % mbf else [])


def noise(rng, n, N, specials=False):
    """noise with -0.0 and subnormals sprinkled in; specials: both infinities and a NaN with a payload too (for the paths that copy)"""
    x = rng.uniform(-1.0, 1.0, size=(n, N)).astype(F32)
    u = fwapi.bits(x).copy()
    words = [0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x00000000] + ([0x7F800000, 0xFF800000, 0x7FC01234] if specials else [])
    words = np.array(words, dtype=np.uint32)
    where = rng.integers(0, N, size=(n, max(8, N // 10)))
    for c in range(n):
        u[c, where[c]] = words[np.arange(where.shape[1]) % len(words)]
    return u.view(F32).reshape(n, N)


# ================================================================================================ CPU tier: the model's properties
@pytest.mark.parametrize("law", [LINEAR_LAW, EQUAL_POWER])
def test_model_at_rest_at_an_end_is_a_copy_bit_for_bit(law):
    rng = np.random.default_rng(1)
    A, B = noise(rng, 3, 200, specials=True), noise(rng, 3, 200, specials=True)
    y0, f0 = Model(3, 0.0, law).block(A, B)
    y1, f1 = Model(3, 1.0, law).block(A, B)
    assert_bits(y0, A, "at rest at 0")
    assert_bits(y1, B, "at rest at 1")
    assert not f0.any() and not f1.any()
    u = fwapi.bits(A)
    assert (u == 0x80000000).any() and (u == 0x00000001).any() and (u == 0x7FC01234).any()


def test_model_linear_shape_starts_at_exactly_p0():
    for P0, P1 in ((0.3, 0.9), (1.0, 0.0), (0.123456, 0.654321)):
        s = Segment(P0, P1, t0=777, dur=1000)
        assert fwapi.bits(s.position([777])[0]) == fwapi.bits(F32(P0))
        assert fwapi.bits(s.position([1777])[0]) == fwapi.bits(F32(P1)) and fwapi.bits(s.position([10 ** 12])[0]) == fwapi.bits(F32(P1))
        b = Segment(P0, P1, t0=777, dur=1000, curve=EASE_IN_OUT)
        assert fwapi.bits(b.position([777])[0]) == fwapi.bits(F32(P0))     # y = 0 when u == 0


@pytest.mark.parametrize("curve", [None, EASE_IN_OUT, OVERSHOOT])
def test_model_a_retarget_in_mid_fade_starts_where_the_old_segment_stands(curve):
    m = Model(1, 0.1, EQUAL_POWER)
    m.to(0.95, 500, curve)
    x = np.ones((1, 64), dtype=F32)
    for _ in range(3):
        m.block(x, x)
    old = m.seg.position([m.T])[0]
    assert 0.1 < old < 0.95
    m.to(0.2, 300, EASE_IN_OUT)
    assert fwapi.bits(m.seg.P0) == fwapi.bits(old) and m.seg.t0 == 192
    assert fwapi.bits(m.seg.position([m.T])[0]) == fwapi.bits(old)


def test_model_an_overshooting_curve_never_leaves_the_unit_interval():
    raw = _bezier(np.linspace(0, 1, 1001, dtype=F32), OVERSHOOT[1], OVERSHOOT[3])
    assert raw.min() < 0 and raw.max() > 1                      # the curve itself does overshoot
    for P0, P1 in ((0.0, 1.0), (1.0, 0.0), (0.05, 0.97)):
        p = Segment(P0, P1, t0=5, dur=4000, curve=OVERSHOOT).position(np.arange(0, 4100))
        assert p.min() >= 0 and p.max() <= 1 and (p == 0).any() | (p == 1).any()


@pytest.mark.parametrize("curve", [None, EASE_IN_OUT])
def test_model_one_block_of_128_equals_two_blocks_of_64(curve):
    rng = np.random.default_rng(2)
    A, B = noise(rng, 2, 128), noise(rng, 2, 128)
    one, two = Model(2, 0.2), Model(2, 0.2)
    one.to(0.8, 100, curve)
    two.to(0.8, 100, curve)
    y, _ = one.block(A, B)
    ya, _ = two.block(A[:, :64], B[:, :64])
    yb, _ = two.block(A[:, 64:], B[:, 64:])
    assert_bits(np.concatenate([ya, yb], axis=1), y, "128 = 64 + 64")
    assert one.T == two.T == 128


def test_model_flags_follow_the_rule():
    x = np.ones((2, 8), dtype=F32)
    fa, fb = np.array([True, False]), np.array([True, True])
    for pos, want in ((0.0, fa), (1.0, fb), (0.3, fa & fb)):
        _, f = Model(2, pos).block(x, x, fa, fb)
        assert np.array_equal(f, want), pos
    m = Model(2, 0.0)
    m.to(1.0, 100)
    _, f = m.block(x, x, fa, fb)
    assert np.array_equal(f, fa & fb)          # inside a segment only "both flagged" flags


# ================================================================================================ CPU tier: the ABI
def _to(e, node, position, frames, curve=None, at_block=0):
    shape, (x1, y1, x2, y2) = (0, (0.0, 0.0, 1.0, 1.0)) if curve is None else (1, curve)
    e._chk(e.cx.L.fwgpu_crossfade_to(e.cx.c, node, position, frames, shape, x1, y1, x2, y2, at_block))


@pytest.mark.parametrize("n_in,n_out", [(2, 1), (4, 2), (16, 8)])
def test_shapes_accepted(n_in, n_out):
    e, _ = _host()
    m = e.add_node(CROSSFADE, n_in, n_out, [])
    e.update()
    assert e.cx.plan_node_level(m) >= 0 and e.cx.node_latency(m) == 0


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (3, 2), (18, 9), (2, 0)])
def test_shapes_refused_at_add_node(n_in, n_out):
    e, _ = _host()
    with pytest.raises(e.fa.FwgpuError) as ei:
        e.add_node(CROSSFADE, n_in, n_out, [])
    assert ei.value.code == INVALID and "CrossfadeNode" in str(ei.value)
    e.update()  # nothing was added


def test_node_kinds_end_at_20():
    """fwgpu_add_node: the last kind with a valid shape is accepted, the one behind it and -1 are refused"""
    e, _ = _host()
    assert e.add_node(CROSSFADE, 4, 2, []) >= 0
    for kind in (21, -1):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.add_node(kind, 4, 2, [])
        assert ei.value.code == INVALID
    e.update()


@pytest.mark.parametrize("params", [[float("nan")], [-0.01], [1.01], [float("inf")], [0.5, 2.0], [0.5, 0.5], [0.5, float("nan")], [0.5, -1.0]])
def test_creation_parameters_refused_at_update(params):
    e, v = _host()
    m = e.add_node(CROSSFADE, 4, 2, params)
    for _ in range(2):  # (still there, still refused)
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.update()
        assert ei.value.code == INVALID and "CrossfadeNode" in str(ei.value)
    e.remove_node(m)
    good = e.add_node(CROSSFADE, 4, 2, [0.5, 0.0])
    e.connect_stereo(v, good)
    e.update()  # the graph is usable


@pytest.mark.parametrize("params", [[], [0.0], [1.0, 0.0], [0.25, 1.0]])
def test_creation_parameters_accepted(params):
    e, _ = _host()
    e.add_node(CROSSFADE, 2, 1, params)
    e.update()


NAN = float("nan")
REFUSED = [
    ("position", dict(position=-0.001)), ("position", dict(position=1.001)), ("position", dict(position=NAN)),
    ("frames", dict(frames=FRAMES_MAX + 1)), ("shape", dict(shape=2)), ("shape", dict(shape=-1)),
    ("x1", dict(x1=-0.1)), ("x1", dict(x1=1.1)), ("x1", dict(x1=NAN)), ("x2", dict(x2=-0.1)), ("x2", dict(x2=1.1)), ("x2", dict(x2=NAN)),
    ("y1", dict(y1=-1.1)), ("y1", dict(y1=2.1)), ("y1", dict(y1=NAN)), ("y2", dict(y2=-1.1)), ("y2", dict(y2=2.1)), ("y2", dict(y2=NAN)),
]


@pytest.mark.parametrize("what,bad", REFUSED)
def test_crossfade_to_refusals(what, bad):
    e, v = _host()
    m = e.add_node(CROSSFADE, 4, 2, [])
    e.update()
    a = dict(position=0.5, frames=100, shape=1, x1=0.42, y1=0.0, x2=0.58, y2=1.0)
    call = lambda d: e.cx.L.fwgpu_crossfade_to(e.cx.c, m, d["position"], d["frames"], d["shape"], d["x1"], d["y1"], d["x2"], d["y2"], 0)
    assert call(a) == 0
    assert call(dict(a, **bad)) == INVALID, what
    assert "fwgpu_crossfade_to" in e.cx.L.fwgpu_last_error(e.cx.c).decode()


def test_crossfade_to_accepts_the_borders_and_refuses_other_kinds():
    e, v = _host()
    m = e.add_node(CROSSFADE, 4, 2, [])
    L, c = e.cx.L, e.cx.c
    assert L.fwgpu_crossfade_to(c, m, 1.0, FRAMES_MAX, 1, 0.0, -1.0, 1.0, 2.0, 7) == 0      # before the first update, too
    assert L.fwgpu_crossfade_to(c, m, 0.0, 0, 0, 0.0, 0.0, 1.0, 1.0, 0) == 0
    e.update()
    assert L.fwgpu_crossfade_to(c, m, 1.0, FRAMES_MAX, 1, 1.0, 2.0, 0.0, -1.0, 0) == 0
    for other in (v, e.graph_out_node, 12345 << 32):
        assert L.fwgpu_crossfade_to(c, other, 0.5, 10, 0, 0.0, 0.0, 1.0, 1.0, 0) == INVALID
    assert L.fwgpu_crossfade_to(None, m, 0.5, 10, 0, 0.0, 0.0, 1.0, 1.0, 0) == INVALID


def test_set_param_0_is_a_jump_and_other_params_are_refused():
    e, _ = _host()
    m = e.add_node(CROSSFADE, 4, 2, [])
    e.update()
    e.set_param(m, 0, 0.75)
    e.set_param(m, 0, 0.0, at_block=3)
    for bad in (-0.5, 1.5, NAN):        # the same range as the message it is
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.set_param(m, 0, bad)
        assert ei.value.code == INVALID
    for slot in (1, 2, -1):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.set_param(m, slot, 0.5)
        assert ei.value.code == INVALID
    e.process_blocks(4)
    assert e.violation() == ""


def test_typed_mirror_header_and_generated_ffi():
    import firewheel_amd as fa
    from firewheel_amd import _lib as flib

    node = fa.CrossfadeNode()
    assert (node.KIND, node.position, node.law, node.channels, node.num_inputs, node.params()) == (CROSSFADE, 0.0, EQUAL_POWER, 2, 4, [0.0, 1.0])
    assert fa.CrossfadeNode(0.25, fa.CrossfadeNode.LAW_LINEAR, channels=3).params() == [0.25, 0.0]
    assert fa.CrossfadeNode(channels=8).num_inputs == 16 and fa.CrossfadeNode.FRAMES_MAX == FRAMES_MAX
    assert fa.CrossfadeNode.LINEAR is None and fa.CrossfadeNode.EASE_IN_OUT == EASE_IN_OUT
    assert fa.CrossfadeNode.EASE_IN == (0.42, 0.0, 1.0, 1.0) and fa.CrossfadeNode.EASE_OUT == (0.0, 0.0, 0.58, 1.0)
    assert "fwgpu_crossfade_to" in flib.SIGNATURES
    # the node the raw call builds: same kind, same parameter list, accepted by the same checks
    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=0, num_graph_outputs=2)
    v = cx.add_node(2, 2, fa.VolumeNode(50.0))
    m = cx.add_node(node.num_inputs, node.channels, node)
    for c in range(2):
        cx.connect(v, c, m, c)
        cx.connect(m, c, cx.graph_out_node(), c)
    node.crossfade_to(1.0, 480, fa.CrossfadeNode.EASE_IN)      # before the first update
    cx.update()
    assert cx.node_latency(m) == 0 and cx.latency_report() == []
    node.crossfade_to(0.5, 100)
    node.crossfade_to(0.0, 100, fa.CrossfadeNode.EASE_IN_OUT, at_block=2)
    node.crossfade_to_secs(1.0, 0.01, fa.CrossfadeNode.EASE_OUT)
    node.set_position(0.3)
    assert node.position == 0.3
    for bad in (lambda: node.crossfade_to(1.5, 10), lambda: node.crossfade_to(0.5, FRAMES_MAX + 1), lambda: node.crossfade_to(0.5, 10, (2.0, 0, 1, 1)),
                lambda: node.crossfade_to_secs(0.5, 1000.0)):
        with pytest.raises(fa.FwgpuError):
            bad()
    with pytest.raises(fa.FwgpuError):
        cx.add_node(2, 2, fa.CrossfadeNode())
    bad = cx.add_node(4, 2, fa.CrossfadeNode(position=1.5))
    with pytest.raises(fa.FwgpuError):
        cx.update()
    cx.remove_node(bad)
    cx.update()
    cx.close()
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    assert re.search(r"FWGPU_CROSSFADE = 20\b", hdr)
    assert re.search(r"#define FWGPU_CROSSFADE_FRAMES_MAX 16777216\b", hdr) and re.search(r"#define FWGPU_CROSSFADE_CH_MAX 8\b", hdr)
    decl = ("int fwgpu_crossfade_to(fwgpu_ctx* ctx, int64_t node, float position, uint32_t frames, int shape, float x1, float y1, float x2, "
            "float y2,\n                       uint32_t at_block);")
    assert decl in hdr, decl
    types = open(os.path.join(ROOT, "firewheel_amd", "csrc", "fwgpu_types.h")).read()
    assert re.search(r"K_CROSSFADE = 20\b", types) and re.search(r"K_LAST = K_CROSSFADE\b", types) and re.search(r"CMD_XF_TO = 23\b", types)
    assert re.search(r"#define XF_CH_MAX 8\b", types) and re.search(r"#define XF_FRAMES_MAX 16777216u", types) and re.search(r"#define XF_ITERS 24\b", types)
    ffi = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "ffi.rs")).read()
    assert "pub const FWGPU_CROSSFADE: c_int = 20;" in ffi and "pub const FWGPU_CROSSFADE_FRAMES_MAX: u32 = 16777216;" in ffi
    assert "pub const FWGPU_CROSSFADE_CH_MAX: u32 = 8;" in ffi
    assert ("pub fn fwgpu_crossfade_to(ctx: *mut fwgpu_ctx, node: i64, position: f32, frames: u32, shape: c_int, x1: f32, y1: f32, x2: f32, "
            "y2: f32, at_block: u32) -> c_int;") in ffi
    nodes = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "nodes.rs")).read()
    assert "pub struct GpuCrossfadeNode" in nodes and "ffi::FWGPU_CROSSFADE" in nodes and "ffi::fwgpu_crossfade_to" in nodes


# ================================================================================================ the desk: two sub-mixes and a crossfader
class Desk(object):
    pass


SHAPES = ["v", "vp", "", "pv", "vc", "v", "vp", "p"]     # eight dry voices (busnodes._stage)


def desk(e, join, position=0.5, law=EQUAL_POWER, early=None):
    """eight dry voices in two halves -> SumNodes S0 and S1 -> `join` -> graph_out 0,1.  join: "xf" (the crossfader: S0 is bus A, S1 bus B),
    "sum" (the twin: a 4 -> 2 SumNode in its place) or None (the oracle's graph: S0 -> graph_out 0,1 and S1 -> graph_out 2,3).
    Beside the join a VolumeNode that nothing feeds -> graph_out 2,3 (silence): a tree of SumNodes over dry voices and nothing else is the
    voice-bank plan as a whole, so without it the twin would be plan 1 and no like-for-like twin of a graph that is the hybrid plan.
    early: messages (position, frames, curve, at_block) queued before the first update"""
    d = Desk()
    d.e, d.samplers, d.xf, d.seed, d.salt = e, [], None, 0, SALT
    rng = np.random.default_rng(6200)
    d.S = [e.sum(4), e.sum(4)]
    for i, sh in enumerate(SHAPES):
        e.connect_stereo(_voice(e, d, sh, i, rng), d.S[i // 4], 2 * (i % 4))
    if join is None:
        e.connect_stereo(d.S[0], e.graph_out_node, 0)
        e.connect_stereo(d.S[1], e.graph_out_node, 2)
    else:
        d.xf = e.add_node(CROSSFADE, 4, 2, [position, float(law)]) if join == "xf" else e.sum(2)
        e.connect_stereo(d.S[0], d.xf, 0)
        e.connect_stereo(d.S[1], d.xf, 2)
        e.connect_stereo(d.xf, e.graph_out_node)
        d.beside = e.volume(100.0)
        e.connect_stereo(d.beside, e.graph_out_node, 2)
        for msg in early or ():
            _to(e, d.xf, *msg)
    e.update()
    for i, s in enumerate(d.samplers):
        _start(e, s, 0, i, SALT)
    return d


# ================================================================================================ CPU tier: the planner
@pytest.mark.parametrize("max_batch", [1, 3, 64])
def test_a_crossfader_changes_no_planner_decision(max_batch):
    """the twin graph, a 4 -> 2 SumNode in the crossfader's place: the same plan kind, fused voices and launches; the level that holds the
    node is launched with k_level's bits alone; no report with messages queued before the first update, nor with the node removed and
    added again between calls"""
    e0 = HostOnlyEngine(max_block_frames=256, num_graph_outputs=4, max_batch=max_batch)
    desk(e0, "sum")
    la0, seen0 = harness_run(e0, n_out_ch=4)
    e = HostOnlyEngine(max_block_frames=256, num_graph_outputs=4, max_batch=max_batch)
    d = desk(e, "xf", early=[(1.0, 3000, EASE_IN_OUT, 0), (0.2, 0, None, 2)])
    la, seen = harness_run(e, n_out_ch=4)
    assert seen & ~LB_LEVEL == 0 and seen0 & ~LB_LEVEL == 0 and seen & 1, (seen, seen0)
    assert e.cx.plan_kind() == e0.cx.plan_kind() == 3 and e.cx.plan_fused_voices() == e0.cx.plan_fused_voices() == len(SHAPES)
    assert la == la0 and la["leaf_sum"] == harness_batches(max_batch), (la, la0)
    assert e.cx.lazy_stats() == e0.cx.lazy_stats(), (e.cx.lazy_stats(), e0.cx.lazy_stats())
    # messages in flight, then the node leaves and a new one takes its place
    _to(e, d.xf, 0.0, 100000, OVERSHOOT, at_block=1)
    e.process_blocks(HARNESS_CALLS[0], n_out_ch=4)
    e.remove_node(d.xf)
    d.xf = e.add_node(CROSSFADE, 4, 2, [1.0, 0.0])
    e.connect_stereo(d.S[0], d.xf, 0)
    e.connect_stereo(d.S[1], d.xf, 2)
    e.connect_stereo(d.xf, e.graph_out_node)
    _to(e, d.xf, 0.5, 700)
    e.update()
    la2, seen2 = harness_run(e, n_out_ch=4)
    assert seen2 & ~LB_LEVEL == 0 and la2 == la0, (seen2, la2, la0)
    assert e.cx.plan_kind() == 3 and e.cx.plan_fused_voices() == len(SHAPES)


# ================================================================================================ GPU tier
# (max_block_frames, n): both block sizes, every n; with set_max_batch 1, 3 and 64
COMBOS = [(64, 1), (64, 2), (96, 3), (96, 8), (64, 8), (96, 2), (64, 3), (96, 1)]
BATCHES = [1, 3, 64]


def stream_calls(mbf):
    """busnodes.ragged_calls (K in {1, 2, 5}, a 37-frame tail, a 1-frame call), then a call of 19 blocks and one of 70: a wave's run of
    blocks is ragged and more than one wave shares a node"""
    return ragged_calls(mbf, at_least=0) + [19 * mbf, 70 * mbf]


_inputs = {}


def stream_input(n, mbf, specials=False):
    key = (n, mbf, specials)
    if key not in _inputs:
        _inputs[key] = noise(np.random.default_rng(1000 * n + mbf + int(specials)), 2 * n, sum(stream_calls(mbf)), specials)
    return _inputs[key]


def run_stream(mbf, n, max_batch, nodes, x, calls=None):
    """graph_in(2n) -> one crossfader per entry of `nodes`, all fed by the same two buses -> graph_out(len(nodes) * n).
    nodes: dicts position, law, script {call index: [(at_block, position, frames, curve)]} -> (device output, the model's) [.][frames]"""
    calls = calls or stream_calls(mbf)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=2 * n, num_graph_outputs=len(nodes) * n, max_batch=max_batch)
    ids, models = [], []
    for j, nd in enumerate(nodes):
        m = g.add_node(CROSSFADE, 2 * n, n, [nd["position"], float(nd["law"])])
        for c in range(2 * n):
            g.connect(g.graph_in_node, c, m, c)
        for c in range(n):
            g.connect(m, c, g.graph_out_node, j * n + c)
        ids.append(m)
        models.append(Model(n, nd["position"], nd["law"]))
    g.update()
    assert g.cx.plan_kind() == 0
    a, got, want = 0, [], []
    for k, f in enumerate(calls):
        for j, nd in enumerate(nodes):
            for (at_block, position, frames, curve) in nd.get("script", {}).get(k, ()):
                _to(g, ids[j], position, frames, curve, at_block)
        inp = np.ascontiguousarray(x[:, a:a + f].T).ravel()
        got.append(planar(g.process_interleaved(f, n_out_ch=len(nodes) * n, inp=inp, n_in_ch=2 * n), len(nodes) * n))
        rows = []
        for j, nd in enumerate(nodes):
            b0, ys = a, []
            for bi, F in enumerate(blocks_of(f, mbf)):
                for (at_block, position, frames, curve) in nd.get("script", {}).get(k, ()):
                    if at_block == bi:
                        models[j].to(position, frames, curve)
                ys.append(models[j].block(x[:n, b0:b0 + F], x[n:, b0:b0 + F])[0])
                b0 += F
            rows.append(np.concatenate(ys, axis=1))
        want.append(np.concatenate(rows, axis=0))
        a += f
    return np.concatenate(got, axis=1), np.concatenate(want, axis=1)


# ---- G1: at rest at 0, at 1 and at 0.3, under both laws: six nodes on the same two buses
@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", BATCHES)
@pytest.mark.parametrize("mbf,n", COMBOS)
def test_g1_at_rest(mbf, n, max_batch):
    ends = [dict(position=p, law=law) for law in (LINEAR_LAW, EQUAL_POWER) for p in (0.0, 1.0)]
    calls = stream_calls(mbf)
    x = stream_input(n, mbf, specials=True)
    got, want = run_stream(mbf, n, max_batch, ends, x, calls)
    assert_bits(got, want, "at rest at an end, mbf %d n %d K<=%d" % (mbf, n, max_batch))
    assert_bits(got[:n], x[:n, :got.shape[1]], "position 0 is bus A")
    assert_bits(got[n:2 * n], x[n:, :got.shape[1]], "position 1 is bus B")
    u = fwapi.bits(got)
    assert (u == 0x80000000).any() and (u == 0x7F800000).any() and (u == 0x00000001).any() and (u == 0x7FC01234).any()
    between = [dict(position=0.3, law=law) for law in (LINEAR_LAW, EQUAL_POWER)]
    got, want = run_stream(mbf, n, max_batch, between, stream_input(n, mbf), calls)
    assert_bits(got, want, "at rest at 0.3, mbf %d n %d K<=%d" % (mbf, n, max_batch))


# ---- G2: a linear segment of 1000 frames from block 2 of the 5-block call; it ends inside a block of the 19-block call
LINEAR_SCRIPT = {1: [(2, 1.0, 1000, None)]}


@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", BATCHES)
@pytest.mark.parametrize("mbf,n", COMBOS)
def test_g2_a_linear_segment_through_the_serial_walk_and_the_frozen_path(mbf, n, max_batch):
    nodes = [dict(position=0.0, law=law, script=LINEAR_SCRIPT) for law in (LINEAR_LAW, EQUAL_POWER)]
    calls = stream_calls(mbf)
    end = sum(calls[:1]) + 2 * mbf + 1000
    assert sum(calls[:5]) < end < sum(calls[:6]) and (end - sum(calls[:5])) % mbf       # message-free batches, and inside a block
    got, want = run_stream(mbf, n, max_batch, nodes, stream_input(n, mbf))
    assert_bits(got, want, "linear segment, mbf %d n %d K<=%d" % (mbf, n, max_batch))


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,n", [(64, 2), (96, 3)])
def test_g2_max_batch_1_and_64_render_the_same_bits(mbf, n):
    nodes = [dict(position=0.0, law=EQUAL_POWER, script=LINEAR_SCRIPT), dict(position=0.9, law=LINEAR_LAW, script={1: [(2, 0.1, 5000, EASE_IN_OUT)]})]
    one, _ = run_stream(mbf, n, 1, nodes, stream_input(n, mbf))
    many, want = run_stream(mbf, n, 64, nodes, stream_input(n, mbf))
    assert_bits(many, one, "max_batch 64 against 1")
    assert_bits(many, want, "... and the model")


# ---- G3: Bezier segments
def bezier_nodes(mbf):
    return [
        # an ease in and out that runs on into the 70-block call
        dict(position=0.0, law=EQUAL_POWER, script={1: [(2, 1.0, 30 * mbf + 11, EASE_IN_OUT)]}),
        # the overshooting curve, retargeted in mid-fade, then a jump, then a segment of 3 frames
        dict(position=0.2, law=EQUAL_POWER, script={0: [(1, 0.9, 12 * mbf, OVERSHOOT)], 3: [(1, 0.1, 25 * mbf + 5, OVERSHOOT)], 6: [(40, 0.6, 0, None), (50, 0.0, 3, EASE_IN_OUT)]}),
        # two messages on one block, in order; frames == 0; down again through 1.0 -> 0.0 under the linear law
        dict(position=1.0, law=LINEAR_LAW, script={1: [(0, 0.5, 0, None), (0, 0.0, 7 * mbf + 1, EASE_IN_OUT)], 5: [(3, 1.0, 3, OVERSHOOT), (3, 0.25, 900, OVERSHOOT)]}),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", BATCHES)
@pytest.mark.parametrize("mbf,n", COMBOS)
def test_g3_bezier_segments_retargets_and_jumps(mbf, n, max_batch):
    got, want = run_stream(mbf, n, max_batch, bezier_nodes(mbf), stream_input(n, mbf))
    assert_bits(got, want, "Bezier segments, mbf %d n %d K<=%d" % (mbf, n, max_batch))
    assert np.abs(want).max() > 0.5


# ---- G4: silence flags.  sampler -> volume (muted by message for some calls) -> bus A; bus B unconnected: a fade-out and fade-in of A
# (blocks per call.  A volume muted by message alone is never flagged: its smoother settles into Deactivating, and a gain below 1e-5 is
# a mute only while the smoother is Inactive, volume.rs:104-108 — which it becomes when a block arrives with every input silent,
# volume.rs:94-100.  So the sampler is stopped for the first call of each muted stretch and plays again from the next: from there on it
# is the muted volume that clears and flags bus A, over a live input)
G4_CALLS = [3, 4, 2, 5, 1, 4, 3, 6, 2]
G4_STOPPED = (2, 7)                        # calls during which the sampler is stopped
G4_MUTED = (2, 3, 4, 7)                    # calls in front of which the volume is set to 0 (100 % in front of the others)


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,max_batch", [(64, 4), (96, 1), (96, 64)])
@pytest.mark.parametrize("what", ["at rest at 0", "at rest at 1", "inside a segment", "fade out and in"])
def test_g4_output_flags_follow_the_rule(what, mbf, max_batch):
    position = 1.0 if what == "at rest at 1" else 0.0
    script = {"inside a segment": {0: [(0, 0.7, 10 ** 6, EASE_IN_OUT)]},
              "fade out and in": {1: [(1, 1.0, 2 * mbf + 9, None)], 5: [(2, 0.0, 3 * mbf, EASE_IN_OUT)]}}.get(what, {})

    def run(e, with_node):
        s = e.sampler(100.0)
        v = e.volume(100.0)
        e.connect_stereo(s, v)
        m = None
        if with_node:
            m = e.add_node(CROSSFADE, 4, 2, [position, float(EQUAL_POWER)])
            e.connect_stereo(v, m, 0)                  # bus B stays unconnected
            e.connect_stereo(m, e.graph_out_node)
        else:
            e.connect_stereo(v, e.graph_out_node)
        e.update()
        e.sampler_set_sample(s, e.new_sample(fwapi.PLANAR_F32, 2, scenarios.voice_source(77, 5 * mbf + 13, 2)))
        e.sampler_set_loop_range(s, fwapi.LOOP_FULL)
        e.sampler_play(s)
        outs = []
        for i, k in enumerate(G4_CALLS):
            e.set_param(v, 0, 0.0 if i in G4_MUTED else 100.0)
            (e.sampler_stop if i in G4_STOPPED else e.sampler_play)(s)
            if m is not None:
                for (at_block, pos, frames, curve) in script.get(i, ()):
                    _to(e, m, pos, frames, curve, at_block)
            outs.append(e.process_blocks_flags(k))
        return planar(np.concatenate([np.asarray(o[0], F32) for o in outs])), np.concatenate([o[1] for o in outs]).T.astype(bool)

    xo, fo = run(OracleEngine(max_block_frames=mbf), False)
    assert fo.any() and not fo.all()
    assert fo[:, sum(G4_CALLS[:3]):sum(G4_CALLS[:5])].all()      # calls 3 and 4: the sampler plays, the muted volume flags
    model = Model(2, position, EQUAL_POWER)
    ys, fs, b = [], [], 0
    for i, k in enumerate(G4_CALLS):
        for bi in range(k):
            for (at_block, pos, frames, curve) in script.get(i, ()):
                if at_block == bi:
                    model.to(pos, frames, curve)
            y, f = model.block(xo[:, b * mbf:(b + 1) * mbf], None, fo[:, b], None)
            ys.append(y)
            fs.append(f)
            b += 1
    want, want_flags = np.concatenate(ys, axis=1), np.stack(fs, axis=1)
    yg, fg = run(GpuEngine(max_block_frames=mbf, max_batch=max_batch), True)
    assert_bits(yg, want, "%s, mbf %d K<=%d" % (what, mbf, max_batch))
    assert np.array_equal(fg, want_flags), (fg.astype(int), want_flags.astype(int))
    if what == "at rest at 0":
        assert np.array_equal(want_flags, fo)
    elif what == "at rest at 1":
        assert want_flags.all()
    else:
        assert np.array_equal(want_flags, fo) or what == "fade out and in"      # B is flagged throughout: "both flagged" is A's flag
    if what == "fade out and in":
        assert want_flags.sum() > fo.sum() and not want_flags.all()      # at rest at 1 the output is bus B: flagged


# ---- G5: fwgpu_node_process, one block at a time, one of them through a segment's end
@pytest.mark.gpu
@pytest.mark.parametrize("n,f", [(2, 100), (3, 256), (1, 37)])
def test_g5_node_process_leaves_the_state_advanced(n, f):
    g = GpuEngine(max_block_frames=256, num_graph_outputs=n)
    m = g.add_node(CROSSFADE, 2 * n, n, [0.25, float(EQUAL_POWER)])
    for c in range(n):
        g.connect(m, c, g.graph_out_node, c)
    g.update()
    blocks = 8
    x = noise(np.random.default_rng(5 + n), 2 * n, blocks * f)
    model = Model(n, 0.25, EQUAL_POWER)
    fa = np.zeros((n, blocks), dtype=bool)
    fb = np.zeros((n, blocks), dtype=bool)
    fa[0, 2] = fb[0, 2] = True          # both flagged: zero-filled and flagged
    fb[n - 1, 4] = True                 # one flagged: counts as +0.0, not read
    for k in range(blocks):
        if k == 1:
            _to(g, m, 1.0, 2 * f + f // 2, EASE_IN_OUT)      # ends inside call 3
            model.to(1.0, 2 * f + f // 2, EASE_IN_OUT)
        if k == 5:
            _to(g, m, 0.0, 3, None)
            model.to(0.0, 3, None)
        sl = slice(k * f, (k + 1) * f)
        ins = [np.full(f, 77.0, dtype=F32) if (fa[c, k] if c < n else fb[c - n, k]) else x[c, sl] for c in range(2 * n)]
        mask = sum(1 << c for c in range(n) if fa[c, k]) | sum(1 << (n + c) for c in range(n) if fb[c, k])
        y, om = g.node_process(m, f, ins, n, in_mask=mask)
        want, wf = model.block(x[:n, sl], x[n:, sl], fa[:, k], fb[:, k])
        assert om == sum(1 << c for c in range(n) if wf[c]), (k, om, wf)
        assert_bits(y, want, "B1 call %d" % k)
    assert model.seg.dur == 3 and model.T == blocks * f


# ---- G6 / G7: the desk on the hybrid plan
G7_MBF = 256
G7_CALLS = [3, 4, 2, 4, 3]     # blocks; max_batch 4


def _desk_reference(mbf, frames):
    o = scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf, num_graph_outputs=4))
    desk(o, None)
    return planar(np.concatenate([np.asarray(o.process_interleaved(f, n_out_ch=4)) for f in frames]), 4)


@pytest.mark.gpu
def test_g7_a_fade_across_three_calls_beside_the_fused_voice_banks():
    frames = [k * G7_MBF for k in G7_CALLS]
    ro = _desk_reference(G7_MBF, frames)
    t = GpuEngine(max_block_frames=G7_MBF, num_graph_outputs=4, max_batch=4)
    desk(t, "sum")
    for f in frames:
        t.process_interleaved(f, n_out_ch=4)
    g = GpuEngine(max_block_frames=G7_MBF, num_graph_outputs=4, max_batch=4)
    d = desk(g, "xf", position=0.0)
    model = Model(2, 0.0, EQUAL_POWER)
    got, want, b = [], [], 0
    for i, k in enumerate(G7_CALLS):
        if i == 1:      # from block 1 of call 1 to inside call 3
            _to(g, d.xf, 1.0, 8 * G7_MBF + 100, EASE_IN_OUT, at_block=1)
        got.append(planar(np.asarray(g.process_interleaved(k * G7_MBF, n_out_ch=4)), 4)[:2])
        for bi in range(k):
            if i == 1 and bi == 1:
                model.to(1.0, 8 * G7_MBF + 100, EASE_IN_OUT)
            sl = slice(b * G7_MBF, (b + 1) * G7_MBF)
            want.append(model.block(ro[0:2, sl], ro[2:4, sl])[0])
            b += 1
    assert g.cx.plan_kind() == t.cx.plan_kind() == 3 and g.cx.plan_fused_voices() == t.cx.plan_fused_voices() == len(SHAPES)
    got, want = np.concatenate(got, axis=1), np.concatenate(want, axis=1)
    assert_bits(got[:, :G7_MBF], ro[0:2, :G7_MBF], "before the fade: bus A")
    assert_bits(got, want, "the fade across three calls")
    assert_bits(got[:, -G7_MBF:], ro[2:4, -G7_MBF:], "after the fade: bus B")
    assert np.abs(ro[0:2]).max() > 0.01 and np.abs(ro[2:4]).max() > 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("mbf", [64, 96])
def test_g6_one_block_callbacks_on_the_hybrid_graph(mbf):
    callbacks = 14
    ro = _desk_reference(mbf, [mbf] * callbacks)
    g = GpuEngine(max_block_frames=mbf, num_graph_outputs=4)
    d = desk(g, "xf", position=1.0, law=LINEAR_LAW)
    model = Model(2, 1.0, LINEAR_LAW)
    before = g.cx.rt_path_stats()
    for k in range(callbacks):
        if k == 2:
            _to(g, d.xf, 0.0, 5 * mbf + 7, OVERSHOOT)
            model.to(0.0, 5 * mbf + 7, OVERSHOOT)
        y = planar(np.asarray(g.process_interleaved(mbf, n_out_ch=4)), 4)[:2]
        sl = slice(k * mbf, (k + 1) * mbf)
        assert_bits(y, model.block(ro[0:2, sl], ro[2:4, sl])[0], "callback %d" % k)
    after = g.cx.rt_path_stats()
    assert g.cx.plan_kind() == 3
    # which path ran: every callback is a one-block batch of the level executor (the banks by the voice-bank kernels inside it)
    assert tuple(x - y for x, y in zip(after, before)) == (0, 0, 0, callbacks), (before, after)
