"""Gain rides (fwgpu_gain_ride, CMD_GAIN_RIDE = 27; SPEC): a volume's gain or a pan's two ear gains moved every frame
along the crossfader's curve by ONE message.

The reference is tests/gain_ride_model.py: tests/refmodel.py's VolumeNode and PanNode with the ride added (np.float32 operations one at a
time), inside a RefEngine.  Every comparison is bit equality (busnodes.assert_bits), silence flags included: there is no tolerance.

CPU tier: the model's own properties; the g++ build of fwgpu_types.h gain_ride_* against the model; the factored curve against
tests/test_crossfade.py's; the ABI on the host-only harness and the pins; the planner on the fake-HIP harness.

GPU tier: ONE list of rides (script) through the level executor, the fused voice bank at both bank sizes and with every control build,
16-bit interleaved and mono sources, the chain plan (a ride in front of, between and behind the filters), the hybrid plan, a master
volume, one-block calls, fwgpu_node_process, a plan install in mid-ride, the message interplay, a seeded family.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fwapi
import gain_ride_model as gm
import ramps_model
import refmodel
import sampler_fade_model as sfm
from busnodes import assert_bits
from fwapi import LOOP_FULL, PLANAR_F32, GpuEngine, HostOnlyEngine
from gain_ride_model import EASE, OVERSHOOT
from refmodel import pan_gains, percent_volume_to_raw_gain
from scenarios import voice_source

INVALID = -20
F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FUZZ_SEEDS = int(os.environ.get("FWGPU_FUZZ_SEEDS", "20"))
INTERLEAVED_I16 = 0
ULL = C.c_ulonglong
U = C.c_uint
LENGTHS = [1, 2, 3, 63, 64, 65, 257, 1 << 24]
CURVES = [None, EASE, OVERSHOOT]


def fbits(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def ffrom(u):
    return np.array([u], dtype=np.uint32).view(F32)[0]


def peek():
    p, UP = C.c_void_p, C.POINTER(U)
    return fwapi.peek_lib("gain_ride_peek", {
        "grp_ride_book": (None, [p, C.POINTER(ULL)]), "grp_state_bytes": (U, []), "grp_init": (None, [p, U, U]),
        "grp_set_smoother": (None, [p, C.c_int, C.c_int, U, U]), "grp_start": (None, [p, U, U, U, C.c_int, UP]), "grp_end": (None, [p]),
        "grp_behind_block": (None, [p, U]), "grp_frames": (C.c_int, [p, C.c_int, U, U, UP]), "grp_state": (None, [p, UP]),
        "grp_is_fresh": (C.c_int, [p, U, U]), "grp_curve": (None, [C.c_int, UP, U, U, U, UP]), "grp_unpack": (None, [UP, UP]),
        "grp_pins": (None, [UP])})


def _ctl(curve):
    x1, y1, x2, y2 = (0.0, 0.0, 1.0, 1.0) if curve is None else curve
    return (U * 4)(fbits(x1), fbits(y1), fbits(x2), fbits(y2))


# ================================================================================================ CPU tier: the model's properties
def _windows(N):
    """frame ranges near 0, near N and across N"""
    return [(0, min(N, 70)), (max(N - 70, 0), 140), (N // 2, 8)]


@pytest.mark.parametrize("curve", CURVES)
def test_model_ride_0_is_G0_the_value_stays_inside_and_frame_N_on_is_G1(curve):
    rng = np.random.default_rng(11)
    for N in LENGTHS:
        for _ in range(4):
            G0, G1 = F32(rng.uniform(0, 1)), F32(rng.choice([0.0, 1.0, rng.uniform(0, 1)]))
            assert fbits(gm.ride_value(G0, G1, N, 0, curve)) == fbits(G0)                 # a fresh ride starts at G0 bit for bit
            lo, hi = min(G0, G1), max(G0, G1)
            for k, n in _windows(N):
                v = gm.ride_values(G0, G1, N, k, n, curve)
                assert np.all((v >= lo) & (v <= hi)) and np.all(v >= 0), (N, k, curve)
                t = k + np.arange(n)
                assert np.array_equal(fwapi.bits(v[t >= N]), fwapi.bits(np.full(int((t >= N).sum()), G1, dtype=F32)))
                if curve is not OVERSHOOT:                                               # a monotone curve gives a monotone ride
                    d = np.diff(v.astype(np.float64))
                    assert np.all(d >= 0) if G1 >= G0 else np.all(d <= 0), (N, k, curve)
    # the overshooting curve flattens at the ends: it reaches G1 before the ride is over and leaves G0 late
    v = gm.ride_values(F32(0.25), F32(0.75), 1000, 0, 1000, OVERSHOOT)
    assert v.min() == F32(0.25) and v.max() == F32(0.75) and (v == F32(0.75)).sum() > 20 and (v == F32(0.25)).sum() > 20


def _one(F, shape="vp", eng=None, **kw):
    e = eng or gm.RideRefEngine(max_block_frames=F, short_blocks=True)
    return e, build(e, [shape], **kw)


@pytest.mark.parametrize("curve", [None, EASE])
@pytest.mark.parametrize("N", [1, 37, 300])
def test_model_block_splits_give_the_same_samples_and_state(N, curve):
    total = 448
    splits = {"one": [total], "1": [1] * total, "7": [7] * 64, "40": [40] * 11 + [8], "64": [64] * 7, "mixed": [64, 1, 100, 7, 256, 20]}
    runs = {}
    for name, blocks in splits.items():
        e, b = _one(512)
        vol, pan = b.voices[0].stages
        e.ride(vol, 20.0, N, curve)
        e.ride(pan, 0.8, N + 11, curve)
        out = np.concatenate([e.process_interleaved(n) for n in blocks])
        v, p = e.nodes[vol], e.nodes[pan]
        runs[name] = (out, (v.N, v.k, fbits(v.raw_gain), v.smoother.status, fbits(v.smoother.input), fbits(v.smoother.last_output),
                            p.N, p.k, fbits(p.gl), fbits(p.gr), p.sl.status, fbits(p.sr_.last_output)))
    for name in splits:
        assert_bits(runs[name][0], runs["one"][0], name)
        assert runs[name][1] == runs["one"][1], name
    assert runs["one"][1][:2] == (0, 0) and runs["one"][1][6:8] == (0, 0) and np.any(runs["one"][0] != 0)


def test_model_behind_a_ride_the_node_is_a_fresh_node_at_the_target():
    F = 64
    e, b = _one(F)
    vol, pan = b.voices[0].stages
    e.process_blocks(1)
    e.ride(vol, 35.0, 150, EASE)
    e.ride(pan, -0.4, 129)
    a = [e.process_blocks(1) for _ in range(3)]
    f, fb = _one(F)
    f.process_blocks(4)                                      # the same source frames ...
    for node, kind, val in ((fb.voices[0].stages[0], refmodel.VolumeNode, 35.0), (fb.voices[0].stages[1], refmodel.PanNode, -0.4)):
        f.nodes[node] = kind(f, 2, 2, [val])                 # ... into FRESH nodes at the targets
    for n, m in ((e.nodes[vol], f.nodes[fb.voices[0].stages[0]]), (e.nodes[pan], f.nodes[fb.voices[0].stages[1]])):
        assert n.N == 0 and n.k == 0
        for (s, G1), (s2, G2) in zip(n._gains(), gm.RideVolumeNode._gains(m) if isinstance(m, refmodel.VolumeNode) else gm.RidePanNode._gains(m)):
            assert (s.status, fbits(s.input), fbits(s.last_output), fbits(G1)) == (s2.status, fbits(s2.input), fbits(s2.last_output), fbits(G2))
    assert_bits(np.concatenate([e.process_blocks(1) for _ in range(4)]), np.concatenate([f.process_blocks(1) for _ in range(4)]), "behind the rides")
    assert np.any(np.concatenate(a) != 0)


def test_model_without_a_ride_is_refmodels_node():
    def run(e):
        b = build(e, ["vp", "pv", "v"])
        outs = [e.process_blocks(2)]
        e.set_param(b.voices[0].stages[0], 0, 20.0)
        e.set_param(b.voices[1].stages[0], 0, -0.9)
        outs.append(e.process_blocks(3))
        return np.concatenate(outs)
    assert_bits(run(gm.RideRefEngine(max_block_frames=64, short_blocks=True)), run(refmodel.RefEngine(max_block_frames=64, short_blocks=True)), "no ride")


def test_model_messages_during_a_ride():
    F = 64
    e, b = _one(F)
    vol, pan = b.voices[0].stages
    v, p = e.nodes[vol], e.nodes[pan]
    e.process_blocks(1)
    g_start = v.raw_gain
    e.ride(vol, 10.0, 640, EASE)
    G1 = percent_volume_to_raw_gain(10.0)
    assert (v.N, v.k) == (640, 0) and v.smoother.status == refmodel.INACTIVE and fbits(v.smoother.input) == fbits(G1) == fbits(v.smoother.last_output)
    assert fbits(v.G0[0]) == fbits(g_start)
    e.process_blocks(3)
    assert v.k == 192
    mid = gm.ride_value(g_start, G1, 640, 192, EASE)
    e.ride(vol, 90.0, 100)                                   # a second ride starts where the first stands
    assert (v.N, v.k) == (100, 0) and fbits(v.G0[0]) == fbits(mid) and v.curve is None
    e.process_blocks(1)
    now = gm.ride_value(mid, percent_volume_to_raw_gain(90.0), 100, 64)
    e.set_param(vol, 0, 50.0)                                # param 0 ends the ride: the smoother is reset to the ride's value ...
    assert v.N == 0 and fbits(v.smoother.last_output) == fbits(now) == fbits(v.smoother.input) and v.smoother.status == refmodel.INACTIVE
    out = e.process_blocks(1)
    assert v.smoother.status == refmodel.ACTIVE and np.any(out != 0)    # ... and glides on from there
    e.ride(vol, 70.0, 33)                                    # a ride during a one-pole glide starts at what the smoother last gave
    assert fbits(v.G0[0]) == fbits(v.smoother.last_output) or v.smoother.status == refmodel.INACTIVE
    e.ride(pan, 1.0, 0)                                      # frames == 0 is a step: no glide
    assert p.N == 0 and (fbits(p.gl), fbits(p.gr)) == tuple(fbits(g) for g in pan_gains(1.0)) and p.sl.status == refmodel.INACTIVE
    assert fbits(p.sl.last_output) == fbits(p.gl) and fbits(p.sr_.last_output) == fbits(p.gr)
    # a ride to 0, then the mute rule from the block behind it; a silent input still advances k
    e.ride(vol, 0.0, 64)
    _, fl = e.process_blocks_flags(2)
    assert fl.tolist() == [[False, False], [True, True]]
    e.ride(vol, 80.0, 256)
    e.sampler_pause(b.voices[0].sampler)
    e.process_blocks(2)
    assert v.N == 256 and v.k == 128


# ================================================================================================ CPU tier: the g++ build
@pytest.mark.parametrize("curve", CURVES)
def test_the_gxx_build_of_gain_ride_agrees_with_the_model_bit_for_bit(curve):
    P = peek()
    assert P.grp_state_bytes() == 128
    st, st2 = C.create_string_buffer(128), C.create_string_buffer(128)
    big, out = (U * 17)(), (U * 160)()
    rng = np.random.default_rng(7)
    shape = gm.LINEAR if curve is None else gm.BEZIER
    c32 = (0.0, 0.0, 1.0, 1.0) if curve is None else curve
    for N in LENGTHS:
        for trial in range(6):
            pan = trial % 2
            G0 = [F32(rng.uniform(0, 1)), F32(rng.uniform(0, 1)) if pan else F32(0.0)]
            G1 = [F32(rng.choice([0.0, 1.0, rng.uniform(0, 1)])), F32(rng.uniform(0, 1)) if pan else F32(0.0)]
            P.grp_init(st, fbits(G0[0]), fbits(G0[1]))
            if trial == 2:                                   # a smoother on its way: the gain in force is `last`
                P.grp_set_smoother(st, 0, refmodel.ACTIVE, fbits(F32(0.9)), fbits(G0[0]))
            if trial == 3:                                   # through a first ride, stopped in mid-flight: G0 is its value there
                first = [F32(rng.uniform(0, 1)), F32(rng.uniform(0, 1))]
                P.grp_start(st, fbits(first[0]), fbits(first[1]), 1000, shape, _ctl(curve))
                k0 = int(rng.integers(1, 999))
                P.grp_behind_block(st, k0)
                G0 = [gm.ride_value(G0[c], first[c], 1000, k0, curve) for c in range(2)]
            P.grp_start(st, fbits(G1[0]), fbits(G1[1]), N, shape, _ctl(curve))
            P.grp_state(st, big)
            assert list(big[:9]) == [N, 0, shape, fbits(G0[0]), fbits(G0[1])] + [fbits(v) for v in c32], (N, trial, list(big))
            assert list(big[9:]) == [0, fbits(G1[0]), fbits(G1[0]), 0, fbits(G1[1]), fbits(G1[1]), fbits(G1[0]), fbits(G1[1])]   # at rest at the targets
            for k, n in _windows(N):                         # k near 0, near N, across N: from the start, and with the state advanced
                for adv in (0, k):
                    C.memmove(st2, st.raw, 128)
                    if adv:
                        P.grp_behind_block(st2, adv)
                    n4 = (n + 3) & ~3
                    for c in range(2):
                        assert P.grp_frames(st2, c, k - adv, n4, out) == 1                 # gain_ride_value == gain_ride_values<4>
                        want = gm.ride_values(G0[c], G1[c], N, k, n4, curve)
                        assert list(out[:n4]) == [int(x) for x in fwapi.bits(want)], (N, trial, k, adv, c)
            if N <= 1000:
                C.memmove(st2, st.raw, 128)
                P.grp_behind_block(st2, N // 2)
                if N > 1:
                    P.grp_state(st2, big)
                    assert list(big[:2]) == [N, N // 2]
                P.grp_behind_block(st2, N - N // 2)
                assert P.grp_is_fresh(st2, fbits(G1[0]), fbits(G1[1])) == 1                # behind the ride: a node set to the target
    # param 0 in a ride: both smoothers are reset to the ride's current values; at rest it changes nothing
    P.grp_init(st, fbits(0.25), fbits(0.75))
    P.grp_end(st)
    assert P.grp_is_fresh(st, fbits(0.25), fbits(0.75)) == 1
    P.grp_start(st, fbits(1.0), fbits(0.0), 100, shape, _ctl(curve))
    P.grp_behind_block(st, 40)
    P.grp_end(st)
    P.grp_state(st, big)
    now = [fbits(gm.ride_value(F32(0.25), F32(1.0), 100, 40, curve)), fbits(gm.ride_value(F32(0.75), F32(0.0), 100, 40, curve))]
    assert list(big[:2]) == [0, 0] and list(big[9:15]) == [0, now[0], now[0], 0, now[1], now[1]] and list(big[15:]) == [fbits(1.0), fbits(0.0)]
    # frames == 0 is a step; a corrupted message (too long, an unknown shape) is one too
    for frames, shp in ((0, shape), (gm.FRAMES_MAX + 1, shape), (10, 2)):
        P.grp_init(st, fbits(0.5), fbits(0.25))
        P.grp_set_smoother(st, 0, refmodel.ACTIVE, fbits(0.5), fbits(0.1))
        P.grp_start(st, fbits(0.75), fbits(0.125), frames, shp, _ctl(curve))
        assert P.grp_is_fresh(st, fbits(0.75), fbits(0.125)) == 1


def test_the_factored_curve_is_the_crossfaders():
    """fw_curve_y, the function xf_positions now calls, against tests/test_crossfade.py's numpy statement of the crossfader's position on
    the same inputs (P0 = 0, P1 = 1: the position is the clamped curve value); tests/test_crossfade.py itself passes unchanged"""
    import test_crossfade as xf

    P = peek()
    out = (U * 300)()
    for curve in (None, xf.EASE_IN_OUT, xf.OVERSHOOT, (0.0, 2.0, 1.0, -1.0), (1.0, 0.0, 0.0, 1.0)):
        for N in (1, 3, 257, 1000, 1 << 24):
            for k in sorted({0, N // 3, max(N - 300, 0)}):
                n = min(300, N - k)
                P.grp_curve(gm.LINEAR if curve is None else gm.BEZIER, _ctl(curve), k, N, n, out)
                y = np.array(list(out[:n]), dtype=np.uint32).view(F32)
                want = xf.Segment(0.0, 1.0, 0, N, curve).position(k + np.arange(n))
                assert_bits(np.minimum(np.maximum(y, F32(0.0)), F32(1.0)), want, "curve %r N %d k %d" % (curve, N, k))
                assert_bits(y, gm.curve_y((k + np.arange(n)).astype(F32) / F32(N), curve), "model curve %r N %d k %d" % (curve, N, k))


# ------------------------------------------------------------------------------------------------ graphs (any fwapi.Engine)
class Bank(object):
    pass


class Voice(object):
    pass


def _stage(e, tok, rng, v):
    if tok == "v":
        return e.volume(float(rng.uniform(40, 100)))
    if tok == "p":
        return e.pan(float(rng.uniform(-1, 1)))
    if tok == "c":
        return e.hard_clip(-3.0)
    if tok == "B":
        return e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 6000)), float(rng.choice([0.707, 2.0])))
    assert tok == "D"
    return e.delay((64, 129, 300)[v % 3] / float(e.sample_rate), feedback=float(rng.choice([0.0, 0.45])), mix=0.5)


def build(e, shapes, lens=None, loops=None, fmt=PLANAR_F32, ch=2, leaf=4, master="", send=False, spare_port=False, start=True):
    """voices sampler -> the stages of shapes[v] (v volume, p pan, c hard clip, B biquad, D delay) under SumNodes of `leaf` ports -> a root
    SumNode -> the master chain (a string of v / p) -> graph_out.  send: leaf 0's bus goes to the root twice, dry and through a delay —
    the hybrid plan.  Bank.voices[v].stages = the voice's v / p / c nodes in order (the filters are not counted)."""
    rng = np.random.default_rng(99)
    n = len(shapes)
    lens = lens or [3000 + 37 * v for v in range(n)]
    loops = loops or [True] * n
    b = Bank()
    b.voices, ends = [], []
    for v, shape in enumerate(shapes):
        vc = Voice()
        vc.sampler = e.sampler(float(rng.uniform(60, 100)))
        vc.stages, cur = [], vc.sampler
        for tok in shape:
            node = _stage(e, tok, rng, v)
            e.connect_stereo(cur, node)
            cur = node
            if tok in "vpc":
                vc.stages.append(node)
        b.voices.append(vc)
        ends.append(cur)
    mixers = []
    for i in range(0, n, leaf):
        grp = ends[i:i + leaf]
        m = e.sum(max(2, len(grp) + (1 if spare_port and i == 0 else 0)))
        if i == 0:
            b.mixer, b.free_port = m, len(grp)
        for p, node in enumerate(grp):
            e.connect_stereo(node, m, 2 * p)
        mixers.append(m)
    top = mixers[0]
    if len(mixers) > 1 or send or master:
        top = e.sum(max(2, len(mixers) + (1 if send else 0)))
        for p, m in enumerate(mixers):
            e.connect_stereo(m, top, 2 * p)
        if send:
            d = e.delay(300 / float(e.sample_rate), feedback=0.3, mix=1.0)
            e.connect_stereo(mixers[0], d)
            e.connect_stereo(d, top, 2 * len(mixers))
    b.master = []
    for tok in master:
        node = _stage(e, tok, rng, 0)
        e.connect_stereo(top, node)
        top = node
        b.master.append(node)
    e.connect_stereo(top, e.graph_out_node)
    e.update()
    if start:
        for v, vc in enumerate(b.voices):
            start_voice(e, vc.sampler, 7100 + v, lens[v], loops[v], fmt, ch)
    return b


def start_voice(e, s, seed, frames, loop, fmt=PLANAR_F32, ch=2):
    data = voice_source(seed, frames, ch)
    if fmt == INTERLEAVED_I16:
        data = np.round(np.asarray(data, dtype=F32).reshape(ch, frames).T * 32767).astype(np.int16)
    e.sampler_set_sample(s, e.new_sample(fmt, ch, data))
    if loop:
        e.sampler_set_loop_range(s, LOOP_FULL)
    e.sampler_play(s)


# ================================================================================================ CPU tier: the ABI on the harness
def _vol_msg(percent, frames, block, curve=None):
    """the nine words (type, block, f0, i0, i1, d0 low, d0 high, d1 low, d1 high) one call queues for a volume"""
    x1, y1, x2, y2 = (0.0, 0.0, 1.0, 1.0) if curve is None else curve
    return (27, block, fbits(percent_volume_to_raw_gain(percent)), frames | ((0 if curve is None else 1) << 28), 0,
            fbits(x1), fbits(y1), fbits(x2), fbits(y2))


def _pan_msg(pan, frames, block, curve=None):
    x1, y1, x2, y2 = (0.0, 0.0, 1.0, 1.0) if curve is None else curve
    gl, gr = pan_gains(pan)
    return (27, block, fbits(gl), frames | ((0 if curve is None else 1) << 28), fbits(gr), fbits(x1), fbits(y1), fbits(x2), fbits(y2))


def test_abi_the_nine_words_a_call_queues():
    """one Cmd per call.  Read where the ABI keeps the messages of a node no plan holds yet; the words are pinned as literals"""
    P = peek()
    e = HostOnlyEngine(sample_rate=44100, max_block_frames=96, num_graph_inputs=3, num_graph_outputs=2)
    L, c = e.cx.L, e.cx.c
    assert P.fwp_layout_check(c, 44100, 96, 3, 2, 0) == 0
    vol, pan = e.volume(80.0), e.pan(0.0)
    assert fwapi.early_msgs(P, c) == []
    assert L.fwgpu_gain_ride(c, vol, 50.0, 1000, 0, 0.0, 0.0, 1.0, 1.0, 0) == 0
    assert L.fwgpu_gain_ride(c, pan, -1.0, 1 << 24, 1, 0.42, 0.0, 0.58, 1.0, 3) == 0
    assert L.fwgpu_gain_ride(c, pan, 1.0, 0, 1, 0.0, -1.0, 1.0, 2.0, 7) == 0                 # frames == 0; the borders of the control values
    assert L.fwgpu_gain_ride(c, vol, float("nan"), 10, 0, 0.0, 0.0, 1.0, 1.0, 0) == INVALID  # a refused call queues nothing
    got = fwapi.early_msgs(P, c)
    # volume to 50 %: raw gain 0.25; linear: shape 0 and the control values (0, 0, 1, 1)
    assert got[0] == (27, 0, 0x3e800000, 1000, 0, 0x00000000, 0x00000000, 0x3f800000, 0x3f800000)
    # pan hard left: (1, 0); 2^24 frames | Bezier << 28; ease (0.42, 0, 0.58, 1)
    assert got[1] == (27, 3, 0x3f800000, 0x11000000, 0x00000000, 0x3ed70a3d, 0x00000000, 0x3f147ae1, 0x3f800000)
    # pan hard right: (0, 1); a step; (0, -1, 1, 2)
    assert got[2] == (27, 7, 0x00000000, 0x10000000, 0x3f800000, 0x00000000, 0xbf800000, 0x3f800000, 0x40000000)
    assert got == [_vol_msg(50.0, 1000, 0), _pan_msg(-1.0, 1 << 24, 3, EASE), _pan_msg(1.0, 0, 7, (0.0, -1.0, 1.0, 2.0))]
    out = (U * 8)()
    P.grp_unpack((U * 9)(*got[1]), out)                                                     # the readers give the fields back
    assert list(out) == [0x3f800000, 0, 1 << 24, 1, 0x3ed70a3d, 0, 0x3f147ae1, 0x3f800000]
    e.connect_stereo(vol, pan)
    e.connect_stereo(pan, e.graph_out_node)
    e.update()                                                                              # the plan that activates the nodes releases them
    assert fwapi.early_msgs(P, c) == []
    e.process_blocks(4)
    assert e.violation() == ""


def test_abi_refusals():
    e = HostOnlyEngine(max_block_frames=64, max_batch=4)
    b = build(e, ["vp", "c"])
    L, c = e.cx.L, e.cx.c
    vol, pan = b.voices[0].stages
    ok = (0, 0.0, 0.0, 1.0, 1.0)
    for bad, word in ((lambda: L.fwgpu_gain_ride(c, b.voices[0].sampler, 50.0, 10, *ok, 0), "not a VolumeNode or a StereoPanNode"),
                      (lambda: L.fwgpu_gain_ride(c, b.voices[1].stages[0], 50.0, 10, *ok, 0), "not a VolumeNode or a StereoPanNode"),
                      (lambda: L.fwgpu_gain_ride(c, b.mixer, 50.0, 10, *ok, 0), "not a VolumeNode or a StereoPanNode"),
                      (lambda: L.fwgpu_gain_ride(c, vol, float("nan"), 10, *ok, 0), "NaN or infinite"),
                      (lambda: L.fwgpu_gain_ride(c, vol, float("inf"), 10, *ok, 0), "NaN or infinite"),
                      (lambda: L.fwgpu_gain_ride(c, pan, float("-inf"), 10, *ok, 0), "NaN or infinite"),
                      (lambda: L.fwgpu_gain_ride(c, vol, 50.0, (1 << 24) + 1, *ok, 0), "2^24"),
                      (lambda: L.fwgpu_gain_ride(c, vol, 50.0, 10, 2, 0.0, 0.0, 1.0, 1.0, 0), "shape"),
                      (lambda: L.fwgpu_gain_ride(c, vol, 50.0, 10, -1, 0.0, 0.0, 1.0, 1.0, 0), "shape"),
                      (lambda: L.fwgpu_gain_ride(c, pan, 0.5, 10, 1, -0.01, 0.0, 1.0, 1.0, 0), "x1 and x2"),
                      (lambda: L.fwgpu_gain_ride(c, pan, 0.5, 10, 1, 0.0, 0.0, 1.01, 1.0, 0), "x1 and x2"),
                      (lambda: L.fwgpu_gain_ride(c, pan, 0.5, 10, 1, float("nan"), 0.0, 1.0, 1.0, 0), "x1 and x2"),
                      (lambda: L.fwgpu_gain_ride(c, pan, 0.5, 10, 1, 0.0, -1.01, 1.0, 1.0, 0), "y1 and y2"),
                      (lambda: L.fwgpu_gain_ride(c, pan, 0.5, 10, 1, 0.0, 0.0, 1.0, 2.01, 0), "y1 and y2"),
                      (lambda: L.fwgpu_gain_ride(c, pan, 0.5, 10, 0, 0.0, 0.0, 1.0, float("nan"), 0), "y1 and y2"),   # validated for a linear ride too
                      (lambda: L.fwgpu_gain_ride(c, 1 << 40, 50.0, 10, *ok, 0), "unknown node")):
        assert bad() == INVALID
        assert word in L.fwgpu_last_error(c).decode()
    assert L.fwgpu_gain_ride(None, vol, 50.0, 10, *ok, 0) == INVALID
    assert L.fwgpu_gain_ride(c, vol, -5.0, 10, *ok, 0) == 0          # what param 0 takes: a negative percent is 0


def test_abi_a_ride_for_a_node_no_plan_holds_yet_waits_for_the_update():
    P = peek()
    e = HostOnlyEngine(max_block_frames=64)
    vol = e.volume(100.0)
    assert e.cx.L.fwgpu_gain_ride(e.cx.c, vol, 30.0, 100, 0, 0.0, 0.0, 1.0, 1.0, 0) == 0
    assert len(fwapi.early_msgs(P, e.cx.c)) == 1
    e.connect_stereo(vol, e.graph_out_node)
    e.update()
    assert fwapi.early_msgs(P, e.cx.c) == []
    e.process_blocks(1)
    assert e.violation() == ""


def test_typed_mirror():
    import firewheel_amd as fa

    P = peek()
    cx = fwapi.hostonly_ctx(max_block_frames=64)
    vol, pan = fa.VolumeNode(100.0), fa.StereoPanNode(0.0)
    vid, pid = cx.add_node(2, 2, vol), cx.add_node(2, 2, pan)
    vol.ride_to(30.0, 480, EASE)                            # before the first update
    pan.ride_to_secs(-1.0, 0.01, at_block=2)
    assert fwapi.early_msgs(P, cx.c) == [_vol_msg(30.0, 480, 0, EASE), _pan_msg(-1.0, 480, 2)]
    cx.connect(vid, 0, pid, 0)
    cx.connect(pid, 0, cx.graph_out_node(), 0)
    cx.update()
    vol.ride_to_secs(80.0, 2.0)
    pan.ride_to(1.0, 0)
    vol.ride_to(-3.0, 7)
    assert vol.percent_volume == 0.0 and pan.pan == 1.0 and fa.VolumeNode.RIDE_FRAMES_MAX == fa.StereoPanNode.RIDE_FRAMES_MAX == gm.FRAMES_MAX
    for bad in (lambda: vol.ride_to(float("nan"), 10), lambda: pan.ride_to(0.0, gm.FRAMES_MAX + 1), lambda: vol.ride_to(50.0, 10, (2.0, 0.0, 1.0, 1.0))):
        with pytest.raises(fa.FwgpuError) as ei:
            bad()
        assert ei.value.code == INVALID


def test_pins_header_types_ffi_and_lib_agree():
    import firewheel_amd._lib as flib

    rd = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr, types = rd("include", "fwgpu.h"), rd("firewheel_amd", "csrc", "fwgpu_types.h")
    ffi, nodes = rd("rust", "firewheel-gpu", "src", "ffi.rs"), rd("rust", "firewheel-gpu", "src", "nodes.rs")
    assert re.search(r"#define FWGPU_GAIN_RIDE_FRAMES_MAX 16777216\b", hdr)
    assert re.search(r"int fwgpu_gain_ride\(fwgpu_ctx\* ctx, int64_t node, float value, uint32_t frames, int shape, float x1, float y1, float x2, "
                     r"float y2,\s+uint32_t at_block\);", hdr)
    assert "dips in power" in hdr
    assert re.search(r"CMD_GAIN_RIDE = 27\b", types) and re.search(r"#define GAIN_RIDE_FRAMES_MAX 16777216u", types)
    assert re.search(r"K_LAST = K_CROSSFADE\b", types)           # no new node kind
    assert "pub const FWGPU_GAIN_RIDE_FRAMES_MAX: u32 = 16777216;" in ffi
    assert ("pub fn fwgpu_gain_ride(ctx: *mut fwgpu_ctx, node: i64, value: f32, frames: u32, shape: c_int, x1: f32, y1: f32, x2: f32, y2: f32, "
            "at_block: u32) -> c_int;") in ffi
    assert nodes.count("pub fn ride_to(") == 2 and "ffi::fwgpu_gain_ride" in nodes and nodes.count("ffi::FWGPU_GAIN_RIDE_FRAMES_MAX") == 2
    res, args = flib.SIGNATURES["fwgpu_gain_ride"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_float, C.c_uint32, C.c_int] + [C.c_float] * 4 + [C.c_uint32]
    pins = (U * 6)()
    peek().grp_pins(pins)
    assert list(pins) == [27, 20, 20, 128, 40, 1 << 24]        # CMD_GAIN_RIDE, K_LAST == K_CROSSFADE, NodeState, Cmd, the cap


# ================================================================================================ CPU tier: the planner
def _book(P, e):
    out = (ULL * 5)()
    P.grp_ride_book(e.cx.c, out)
    return list(out)


DRY6 = ["vp", "v", "pv", "vc", "p", "vpv"]


@pytest.mark.parametrize("force_generic", [False, True])
def test_planner_a_call_inside_a_ride_is_a_control_batch_and_the_calls_behind_it_are_lazy_again(force_generic):
    P = peek()
    F, K = 64, 4

    def run(ride):
        e = HostOnlyEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)
        b = build(e, DRY6)
        assert e.cx.plan_kind() == (0 if force_generic else 1)
        for _ in range(3):
            e.process_blocks(K)
        e.reset_launches()
        per_call, books, lazy = [], [], []
        for call in range(7):
            if ride and call == 1:
                assert e.cx.L.fwgpu_gain_ride(e.cx.c, b.voices[2].stages[1], 20.0, 2 * K * F + 9, 1, 0.42, 0.0, 0.58, 1.0, 1) == 0   # through calls 1, 2 and into 3
            before, l0 = e.launches(), e.cx.lazy_stats()
            e.process_blocks(K)
            after, l1 = e.launches(), e.cx.lazy_stats()
            per_call.append({k: after[k] - before[k] for k in after})
            lazy.append((l1[0] - l0[0], l1[1] - l0[1]))
            books.append(_book(P, e))
        assert e.violation() == ""
        return per_call, books, lazy

    rode, books, lazy = run(True)
    still, still_books, still_lazy = run(False)
    assert all(bk[1] == 0 and bk[2] == 0 for bk in still_books)
    # the host's book: calls 1, 2 and 3 may meet the ride (it starts one block into call 1), the others cannot
    assert [bk[2] for bk in books] == [0, 1, 1, 1, 0, 0, 0], books
    assert books[1][1] == 4 * K * F + F + 2 * K * F + 9      # four calls done, one block into the fifth, the ride's frames
    assert books[3][3] == 2 * K * F + 9 and books[4][3] == 0
    if not force_generic:
        assert still_lazy == [(1, 0)] * 7, still_lazy        # a bank with no ride: every call lazy, as before the ride existed ...
        assert lazy == [(1, 0), (0, 1), (0, 1), (0, 1), (1, 0), (1, 0), (1, 0)], lazy   # inside the ride a control batch, behind it lazy again
        assert still == [still[0]] * 7                       # ... and launches what it launched
        assert rode[0] == rode[5] == rode[6] == still[0]
        assert all(c["voice_control"] == 1 for c in rode[1:4]) and still[0]["voice_control"] == 0
    else:
        assert rode == still, (rode, still)                  # the level executor: WHICH instantiation runs changes, never how many kernels


def test_planner_a_step_opens_the_book_for_its_call_alone_and_node_process_opens_it_for_good():
    P = peek()
    F, K = 64, 4
    e = HostOnlyEngine(max_block_frames=F, max_batch=K)
    b = build(e, DRY6)
    e.process_blocks(K)
    assert e.cx.L.fwgpu_gain_ride(e.cx.c, b.voices[0].stages[0], 20.0, 0, 0, 0.0, 0.0, 1.0, 1.0, 0) == 0
    e.process_blocks(K)
    assert _book(P, e)[2:4] == [1, 0]                         # the ride builds are the ones that apply a step
    e.process_blocks(K)
    assert _book(P, e)[2:4] == [0, 0]
    ins = [np.zeros(F, dtype=F32), np.zeros(F, dtype=F32)]
    assert e.cx.L.fwgpu_gain_ride(e.cx.c, b.voices[0].stages[0], 90.0, 100, 0, 0.0, 0.0, 1.0, 1.0, 0) == 0
    e.node_process(b.voices[0].stages[0], F, ins, 2)          # the ride moves with that node's calls alone: no frame count bounds it
    assert _book(P, e)[1] == (1 << 64) - 1
    e.process_blocks(K)
    assert _book(P, e)[2] == 1 and e.violation() == ""


def test_planner_a_node_that_leaves_the_plan_in_mid_ride_meets_the_ride_builds_when_it_returns():
    P = peek()
    F, K, N = 64, 4, 10 * 64
    e = HostOnlyEngine(max_block_frames=F, max_batch=K)
    b = build(e, ["v", "vp", "p"], leaf=4)
    vol, pan = b.voices[1].stages
    assert e.cx.L.fwgpu_gain_ride(e.cx.c, pan, 0.9, N, 0, 0.0, 0.0, 1.0, 1.0, 0) == 0
    e.process_blocks(K)
    assert _book(P, e)[:3] == [K * F, N, 1]
    for port in (0, 1):
        e.disconnect(pan, port, b.mixer, 2 + port)
    e.update()                                                    # the node leaves the plan with 384 frames of its ride to go
    live = []
    for _ in range(5):
        e.process_blocks(K)
        live.append(_book(P, e)[2])
    assert live == [1, 1, 1, 0, 0], live                          # the bound was extended by N at the install, then runs out
    assert _book(P, e)[4] == N
    e.connect_stereo(pan, b.mixer, 2)
    e.update()                                                    # ... and the install that brings it back opens it again, for N frames
    live = []
    for _ in range(4):
        e.process_blocks(K)
        live.append(_book(P, e)[2])
    assert live == [1, 1, 1, 0], live
    assert e.violation() == ""


# ================================================================================================ GPU tier: the list of rides
N_CALLS = 5      # call 0 and call 4 carry no message


def _at(K, call, where, plus=0):
    g = call * K + {"first": 0, "mid": K // 2, "last": K - 1}[where] + plus
    return g // K, g % K


def script(F, K):
    """per item: (shape, loops, sample frames, [(call, at_block, stage, message, args)]) — voice v of a bank is item v % len.  The shapes
    are dry; `chain_shape` puts filters between their stages for the chain plan.  Lengths 1, 3, 64, 65, 257 and 1000 end inside a
    lane's four frames, on a wave, on a block, and in mid-block of a later call; each is sent at block 0 and further in."""
    A = lambda where, plus=0, call=1: _at(K, call, where, plus)
    R = lambda pos, st, value, N, curve=None: pos + (st, "ride", (value, N, curve))
    S = lambda pos, st, value: pos + (st, "set", (value,))
    T = lambda pos, what: pos + (0, what, ())
    return [
        ("v", True, 3000, [R(A("first"), 0, 30.0, 1), R(A("first", call=2), 0, 90.0, 3, OVERSHOOT)]),
        ("vp", True, 3100, [R(A("mid"), 1, 1.0, 3, EASE), R(A("mid"), 0, 55.0, 64, EASE)]),
        ("pv", True, 2900, [R(A("first"), 1, 0.0, 64), R(A("first", call=3), 1, 80.0, 65, OVERSHOOT)]),       # to 0 (then the mute rule), and up from muted
        ("vp", True, 3000, [S(A("first", call=0), 1, -1.0), R(A("last"), 1, 1.0, 257, OVERSHOOT)]),             # hard left to hard right
        ("v", True, 3050, [R(A("first"), 0, 20.0, 1000, EASE)]),                                               # spans calls
        ("vp", True, 3000, [R(A("first"), 0, 10.0, 6 * F), R(A("first", 2), 0, 95.0, 2 * F + 5, EASE)]),        # a ride during a ride
        ("vp", True, 2800, [R(A("first"), 1, 0.8, 6 * F, EASE), S(A("first", 3), 1, -0.5)]),                    # param 0 during a ride
        ("v", True, 3000, [S(A("mid"), 0, 15.0), R(A("mid", 1), 0, 85.0, 65)]),                                 # a ride during a one-pole glide
        ("vc", True, 3000, [R(A("last"), 0, 45.0, 0)]),                                                        # frames == 0: a step
        ("vp", False, 9 * F + 11 if K > 1 else 3 * F + 11, [R(A("first"), 0, 25.0, 40 * F), R(A("first"), 1, -0.7, 1000, EASE)]),   # a one-shot ends inside
        ("v", True, 3000, [R(A("mid"), 0, 10.0, 2 * F), R(A("mid"), 0, 70.0, F + 3, EASE)]),                    # two rides for one block
        ("pv", True, 3000, [R(A("first"), 0, -0.9, 5 * F), T(A("first", 1), "pause"), T(A("first", 3), "play")]),   # the source pauses: the ride goes on
        ("vpv", True, 3000, [R(A("first"), 0, 35.0, 257, EASE), R(A("mid"), 1, 0.6, 3 * F + 7, OVERSHOOT), R(A("last"), 2, 5.0, 1000)]),
        ("vp", True, 3000, [R(A("first"), 0, 0.0, 65, EASE), T(A("first", 1), "stop"), R(A("first", 2), 0, 60.0, 3)]),   # a stopped source: k still moves
        ("v", True, 3000, []),                                                                                  # never rode
        ("", True, 3000, []),
    ]


def chain_shape(shape, v):
    """a dry shape with filters put in: a ride in front of, between and behind them (the chain plan's grammar)"""
    return {"v": ["vB", "Bv", "vBD"][v % 3], "vp": ["vBp", "vpBD", "BvDp"][v % 3], "pv": ["pBv", "DBpv"][v % 2], "vc": "vBc", "vpv": "vBpDv",
            "": ["B", ""][v % 2]}[shape]


def run_script(e, F, K, n_voices, n_calls=N_CALLS, chain=False, **kw):
    items = script(F, K)
    pick = [items[v % len(items)] for v in range(n_voices)]
    b = build(e, [chain_shape(p[0], v) if chain else p[0] for v, p in enumerate(pick)], lens=[p[2] for p in pick], loops=[p[1] for p in pick], **kw)
    outs, flags = [], []
    for call in range(n_calls):
        for v, p in enumerate(pick):
            vc = b.voices[v]
            for c, at, st, what, args in p[3]:
                if c != call:
                    continue
                if what == "ride":
                    e.ride(vc.stages[st], args[0], args[1], args[2], at_block=at)
                elif what == "set":
                    e.set_param(vc.stages[st], 0, args[0], at_block=at)
                else:
                    getattr(e, "sampler_" + what)(vc.sampler, at_block=at)
        if b.master and call in (1, 2):                      # the master chain rides too
            e.ride(b.master[0], 40.0 if call == 1 else 100.0, 3 * F + 5, EASE, at_block=K - 1)
        o, f = e.process_blocks_flags(K)
        outs.append(np.asarray(o))
        flags.append(np.asarray(f, dtype=bool))
    return np.concatenate(outs), np.concatenate(flags), b


_refs = {}


def reference(F, K, n_voices, n_calls=N_CALLS, **kw):
    key = (F, K, n_voices, n_calls, tuple(sorted(kw.items())))
    if key not in _refs:
        out, fl, _ = run_script(gm.Tagged(gm.RideRefEngine(max_block_frames=F, short_blocks=True)), F, K, n_voices, n_calls, **kw)
        out.setflags(write=False)
        fl.setflags(write=False)
        assert np.any(out != 0)
        _refs[key] = (out, fl)
    return _refs[key]


def check(g, F, K, V, what, n_calls=N_CALLS, plan=None, **kw):
    got, gf, b = run_script(gm.GpuRide(g), F, K, V, n_calls, **kw)
    if plan is not None:
        assert g.cx.plan_kind() == plan, (g.cx.plan_kind(), plan)
    want, wf = reference(F, K, V, n_calls, **kw)
    assert np.array_equal(gf, wf), (what, gf.T, wf.T)
    assert_bits(got, want, what)
    return b


COMBOS = [(64, 1, 5), (64, 3, 40), (64, 7, 5), (256, 1, 40), (256, 3, 5), (256, 7, 40)]      # F, K, voices


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g1_level_executor(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K, force_generic=True)
    check(g, F, K, V, "level executor", n_calls=12 if K == 1 else N_CALLS, plan=0, master="vp")


@pytest.mark.gpu
def test_g1_level_executor_blocks_of_more_than_256_frames():
    """k_level's 256-frame chunk loop: max_block_frames 512, calls of 300 frames"""
    F, V = 512, 5

    def run(e):
        b = build(e, ["vp", "v", "pv", "vpv", "p"], master="v")
        outs = []
        for call in range(9):
            if call == 1:
                e.ride(b.voices[0].stages[0], 10.0, 257, EASE)
                e.ride(b.voices[0].stages[1], 1.0, 1000, OVERSHOOT)
                e.ride(b.voices[2].stages[0], -1.0, 300)
                e.ride(b.master[0], 30.0, 650, EASE)
            if call == 4:
                e.ride(b.voices[3].stages[2], 0.0, 299)
                e.set_param(b.voices[0].stages[1], 0, 0.0)
            outs.append(np.asarray(e.process_interleaved(300)))
        return np.concatenate(outs)

    want = run(gm.Tagged(gm.RideRefEngine(max_block_frames=F, short_blocks=True)))
    assert_bits(run(gm.GpuRide(GpuEngine(max_block_frames=F, force_generic=True))), want, "300-frame calls")


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", [None, "0", "1"])
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g2_plan_1_at_both_bank_sizes_with_every_control_build(F, K, V, ahead, monkeypatch):
    """launch_voice_control's rule: the small build runs beside the render of the call before (control-ahead mode), the big one
    otherwise.  FWGPU_CTL_AHEAD=0: every call the big build; =1: every multi-block call the small one; unset: the calls with messages
    the small one and the calls in mid-ride the big one"""
    if ahead is None:
        monkeypatch.delenv("FWGPU_CTL_AHEAD", raising=False)
    else:
        monkeypatch.setenv("FWGPU_CTL_AHEAD", ahead)
    g = GpuEngine(max_block_frames=F, max_batch=K)
    check(g, F, K, V, "voice bank, planar f32, FWGPU_CTL_AHEAD=%s" % ahead, n_calls=12 if K == 1 else N_CALLS, plan=1)
    assert g.cx.plan_fused_voices() == V


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,ch", [(INTERLEAVED_I16, 2), (PLANAR_F32, 1), (INTERLEAVED_I16, 1)])
def test_g2_plan_1_on_16_bit_interleaved_and_mono_sources(fmt, ch):
    F, K, V = 64, 3, 40
    check(GpuEngine(max_block_frames=F, max_batch=K), F, K, V, "format %d, %d channel(s)" % (fmt, ch), plan=1, fmt=fmt, ch=ch)


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", [(64, 3, 16), (256, 7, 5), (64, 1, 16)])
def test_g3_plan_2_a_ride_in_front_of_between_and_behind_the_filters(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    check(g, F, K, V, "chain plan", n_calls=12 if K == 1 else N_CALLS, plan=2, chain=True)


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", [(64, 3, 16), (256, 7, 8)])      # (the planner takes a send bank of eight voices or more)
def test_g4_plan_3_a_hybrid_plan_with_a_send(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    check(g, F, K, V, "hybrid plan", plan=3, send=True, master="v")


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["master", "voice"])
def test_g5_a_master_volume_ride_under_plan_1_and_the_calls_around_it(where, monkeypatch):
    """lazy calls before and after, a control kernel during.  "master": the ride is the master volume's, which the level executor renders
    behind the bank.  "voice": a bank without a master chain, whose steady calls take the grouped path (leaves and root in one kernel: a
    tree with a master chain is not its shape) — fwgpu_plan_group_stats stands still during the ride and moves again behind it.  The
    loops are whole blocks long, which is what a lazy record needs"""
    F, K, V = 64, 4, 8
    monkeypatch.setenv("FWGPU_LEAF_GROUP_MIN", "1")          # (calls of a few blocks are grouped)

    def run(e):
        b = build(e, ["vp", "v", "pv", "vc", "p", "vpv", "v", ""], master="v" if where == "master" else "", lens=[F * (6 + v) for v in range(V)])
        outs, marks = [], []
        for call in range(14):
            if call == 5:
                e.ride(b.master[0] if where == "master" else b.voices[2].stages[1], 30.0, 2 * K * F + 9, EASE, at_block=1)   # through calls 5, 6, into 7
            outs.append(np.asarray(e.process_blocks(K)))
            if hasattr(e, "cx"):
                marks.append(e.cx.lazy_stats() + (e.cx.group_stats(),))
        return np.concatenate(outs), marks

    want, _ = run(gm.Tagged(gm.RideRefEngine(max_block_frames=F, short_blocks=True)))
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got, marks = run(gm.GpuRide(g))
    assert g.cx.plan_kind() == 1
    assert_bits(got, want, "fourteen calls")
    if os.environ.get("FWGPU_LAZY") == "0":
        return
    lazy, ctl, grouped = ([marks[i][n] - marks[i - 1][n] for i in range(1, 14)] for n in range(3))     # index i: call i + 1
    assert lazy[1:4] == [1, 1, 1] and ctl[1:4] == [0, 0, 0], marks                  # calls 2 .. 4: lazy
    assert ctl[4:7] == [1, 1, 1] and lazy[4:7] == [0, 0, 0], marks                  # calls 5 .. 7: inside the ride
    assert lazy[-3:] == [1, 1, 1] and ctl[-3:] == [0, 0, 0], marks                  # behind it: lazy again
    if where == "voice" and os.environ.get("FWGPU_LEAF_GROUP") != "0":
        assert grouped[1:4] == [1, 1, 1] and grouped[4:7] == [0, 0, 0] and grouped[-3:] == [1, 1, 1], marks   # the grouped path resumes


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 256])
def test_g6_one_block_calls_take_the_launch_sequence_during_a_ride_and_the_resident_kernel_comes_back(F):
    V = 8

    def run(e):
        b = build(e, ["vp", "v", "pv", "vc", "p", "vpv", "v", ""])
        outs, paths = [], []
        for call in range(40):
            if call == 10:
                e.ride(b.voices[0].stages[0], 20.0, 5 * F + 3, EASE)
                e.ride(b.voices[2].stages[0], 1.0, 3 * F)
            if call == 30:
                e.ride(b.voices[5].stages[1], -1.0, 0)
            outs.append(np.asarray(e.process_interleaved(F)))
            if hasattr(e, "cx"):
                paths.append(e.cx.rt_path_stats())
        return np.concatenate(outs), paths

    want, _ = run(gm.Tagged(gm.RideRefEngine(max_block_frames=F, short_blocks=True)))
    g = GpuEngine(max_block_frames=F)
    got, paths = run(gm.GpuRide(g))
    assert g.cx.plan_kind() == 1
    assert_bits(got, want, "one-block calls")
    seq = [paths[i][2] - paths[i - 1][2] for i in range(1, 40)]
    assert seq[9:15] == [1] * 6, seq                                                # calls 10 .. 15: the launch sequence
    assert seq[29] == 1 and sum(seq[16:29]) == 0 and sum(seq[31:]) == 0, seq        # a step takes it for its call alone
    assert paths[9][3] == paths[-1][3] == 0
    if os.environ.get("FWGPU_RT_PERSIST") != "0":
        assert paths[29][0] > paths[16][0] and paths[-1][0] > paths[31][0], paths    # the resident kernel comes back behind the ride


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["volume", "pan", "mono volume"])
@pytest.mark.parametrize("F", [40, 64, 100, 256])
def test_g7_node_process(F, kind):
    """fwgpu_node_process (k_single_node): one node, one block per call, every kind of message between the calls — samples and out mask
    of every block against the model's process"""
    g = GpuEngine(max_block_frames=256)
    e = gm.RideRefEngine(max_block_frames=256, short_blocks=True)
    ch = 1 if kind == "mono volume" else 2
    mk = (lambda x: x.pan(-0.3)) if kind == "pan" else (lambda x: x.volume(80.0, ch=ch))
    gn, mn = mk(g), mk(e)
    g.connect(gn, 0, g.graph_out_node, 0)
    g.update()
    node = e.nodes[mn]
    gg = gm.GpuRide(g)
    rng = np.random.default_rng(F)
    val = (lambda a, b: b) if kind == "pan" else (lambda a, b: a)
    rode = 0
    steps = {1: (val(20.0, 0.9), 2 * F + F // 2, EASE), 5: (val(100.0, -1.0), 3, None), 7: (val(0.0, 1.0), 4 * F + 1, OVERSHOOT), 9: (val(60.0, 0.2), 3 * F, None),
             12: (val(33.0, -0.6), 0, None), 13: (val(70.0, 0.0), 65, EASE)}
    for k in range(17):
        if k in steps:
            gg.ride(gn, *steps[k])
            e.ride(mn, *steps[k])
        if k == 10:                                             # param 0 in mid-ride
            g.set_param(gn, 0, val(45.0, 0.5))
            e.set_param(mn, 0, val(45.0, 0.5))
        rode += node.N != 0
        in_mask = (1 << ch) - 1 if k in (3, 14) else 0          # a block whose input is flagged silent: k still moves
        ins = [rng.uniform(-1, 1, F).astype(F32) for _ in range(ch)]
        y, om = g.node_process(gn, F, ins, ch, in_mask=in_mask)
        outs = [np.zeros(F, dtype=F32) for _ in range(ch)]
        wm = node.process(F, ins, outs, in_mask)
        assert om == wm, (k, om, wm)
        assert_bits(y, np.stack(outs), "block %d" % k)
    assert rode >= 8 and node.N == 0


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g8_the_ride_carries_over_a_plan_install(force_generic):
    F, K = 64, 3

    def run(e):
        b = build(e, ["vp", "pv", "v", "vc", "p"], leaf=8, spare_port=True)
        outs = [np.asarray(e.process_blocks(K))]
        e.ride(b.voices[0].stages[0], 15.0, 8 * F + 9, EASE, at_block=1)
        e.ride(b.voices[1].stages[0], 1.0, 8 * F + 9, OVERSHOOT, at_block=2)
        outs.append(np.asarray(e.process_blocks(K)))
        s, vol = e.sampler(80.0), e.volume(70.0)               # a voice is added to the mixer's free port between two calls of the rides
        e.connect_stereo(s, vol)
        e.connect_stereo(vol, b.mixer, 2 * b.free_port)
        e.update()
        start_voice(e, s, 50, 900, True)
        e.ride(vol, 20.0, 100)
        for _ in range(3):
            outs.append(np.asarray(e.process_blocks(K)))
        return np.concatenate(outs)

    want = run(gm.Tagged(gm.RideRefEngine(max_block_frames=F, short_blocks=True)))
    g = GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)
    got = run(gm.GpuRide(g))
    assert g.cx.plan_kind() == (0 if force_generic else 1)
    assert_bits(got, want, "a plan install between two calls of a ride")


# ------------------------------------------------------------------------------------------------ rides and sampler fades together
class RideRampsEngine(gm.RideRefEngine, ramps_model.RampsRefEngine):
    def add_node(self, kind, n_in, n_out, params=()):
        if kind in gm.NODE_CLASSES:
            return gm.RideRefEngine.add_node(self, kind, n_in, n_out, params)
        return ramps_model.RampsRefEngine.add_node(self, kind, n_in, n_out, params)


class TaggedBoth(gm.Tagged, ramps_model.Tagged):
    pass


class GpuBoth(gm.GpuRide, sfm.GpuFade):
    pass


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g9_a_ride_on_a_voice_whose_sampler_is_inside_a_fade_or_stopped(force_generic):
    F, K = 64, 3

    def run(e):
        b = build(e, ["vp", "v", "pv"])
        outs, fls = [], []
        for call in range(6):
            if call == 1:
                e.fade(b.voices[0].sampler, 0.0, 5 * F + 7, sfm.PAUSE, at_block=1)     # a declicked pause ...
                e.ride(b.voices[0].stages[0], 20.0, 7 * F + 1, EASE, at_block=1)        # ... under a ride that outlasts it: silent input, k moves
                e.ride(b.voices[0].stages[1], -1.0, 4 * F)
                e.sampler_stop(b.voices[1].sampler, at_block=2)
                e.ride(b.voices[1].stages[0], 0.0, 2 * F + 3, at_block=2)
            if call == 3:
                e.sampler_play(b.voices[1].sampler)
                e.ride(b.voices[1].stages[0], 90.0, 65, OVERSHOOT)                      # up from muted
                e.fade(b.voices[2].sampler, 0.3, 257, sfm.NONE)
                e.ride(b.voices[2].stages[1], 10.0, 257)
            o, f = e.process_blocks_flags(K)
            outs.append(np.asarray(o))
            fls.append(np.asarray(f, dtype=bool))
        return np.concatenate(outs), np.concatenate(fls)

    want, wf = run(TaggedBoth(RideRampsEngine(max_block_frames=F, short_blocks=True)))
    got, gf = run(GpuBoth(GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)))
    assert np.array_equal(gf, wf), (gf.T, wf.T)
    assert_bits(got, want, "rides and fades")
    assert np.any(want != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g9_a_ride_to_0_mutes_from_the_next_block_and_a_ride_comes_up_from_muted(force_generic):
    F, K = 64, 4

    def run(e):
        b = build(e, ["v"])
        vol = b.voices[0].stages[0]
        e.ride(vol, 0.0, 2 * F, at_block=1)                     # blocks 1 and 2 ride down; block 3 is the first muted one
        a, fa = e.process_blocks_flags(K)
        e.ride(vol, 100.0, F + 1, EASE, at_block=2)             # two muted blocks, then up: the ride's blocks are not flagged, 0.0 gain or not
        c, fc = e.process_blocks_flags(K)
        return np.concatenate([np.asarray(a), np.asarray(c)]), np.concatenate([np.asarray(fa, dtype=bool), np.asarray(fc, dtype=bool)])

    want, wf = run(gm.Tagged(gm.RideRefEngine(max_block_frames=F, short_blocks=True)))
    assert wf[:, 0].tolist() == [False, False, False, True, True, True, False, False]
    got, gf = run(gm.GpuRide(GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)))
    assert np.array_equal(gf, wf), (gf.T, wf.T)
    assert_bits(got, want, "to 0 and back")


# ------------------------------------------------------------------------------------------------ the seeded family
def fuzz(e, seed, F):
    rng = np.random.default_rng(52_000 + seed)
    V = 14
    shapes = [str(rng.choice(["v", "vp", "pv", "vc", "p", "vpv", "vv"])) for _ in range(V)]
    lens = [int(rng.choice([37, 700, 3000])) for _ in range(V)]
    loops = [bool(rng.random() < 0.7) and lens[v] >= 700 for v in range(V)]      # (a loop shorter than a block is outside the sampler's domain)
    b = build(e, shapes, lens=lens, loops=loops, leaf=8, spare_port=True, master=str(rng.choice(["", "v", "vp"])))
    rideable = [(vc.sampler, n, shapes[v][i]) for v, vc in enumerate(b.voices) for i, n in enumerate(vc.stages) if shapes[v][i] in "vp"]
    rideable += [(None, n, "vp"[i]) for i, n in enumerate(b.master)]
    outs = []
    value = lambda kind: float(rng.choice([0.0, 3.0, 50.0, 100.0, 140.0])) if kind == "v" else float(rng.choice([-1.0, -0.3, 0.0, 0.6, 1.0]))
    curve = lambda: [None, EASE, OVERSHOOT, (0.0, 2.0, 1.0, -1.0)][int(rng.integers(0, 4))]
    for call in range(5):
        K = int(rng.integers(1, 5))
        if call == 2:                                        # a graph edit: one more voice on the first mixer's free port
            s, vol = e.sampler(70.0), e.volume(60.0)
            e.connect_stereo(s, vol)
            e.connect_stereo(vol, b.mixer, 2 * b.free_port)
            e.update()
            start_voice(e, s, 600 + seed, 800, True)
            rideable.append((s, vol, "v"))
        for _ in range(int(rng.integers(0, 16))):
            (s, node, kind), at = rideable[int(rng.integers(0, len(rideable)))], int(rng.integers(0, K))
            what = rng.random()
            if what < 0.55:
                N = int(rng.choice([1, 3, F - 1, F, F + 1, 257, 3 * F + 7, int(rng.integers(1, 8 * F))]))
                e.ride(node, value(kind), N, curve(), at_block=at)
            elif what < 0.75:
                e.set_param(node, 0, value(kind), at_block=at)
            elif what < 0.85:
                e.ride(node, value(kind), 0, curve(), at_block=at)
            elif s is not None and what < 0.93:
                e.sampler_pause(s, at_block=at)
            elif s is not None:
                e.sampler_play(s, at_block=at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_g10_seeded_rides_params_transport_and_graph_edits_on_plans_0_and_1(seed):
    F = [64, 256, 128, 64][seed % 4]
    want = fuzz(gm.Tagged(gm.RideRefEngine(max_block_frames=F, short_blocks=True)), seed, F)
    for force_generic in (False, True):
        g = GpuEngine(max_block_frames=F, max_batch=4, force_generic=force_generic)
        got = fuzz(gm.GpuRide(g), seed, F)
        assert g.cx.plan_kind() == (0 if force_generic else 1)
        assert_bits(got, want, "seed %d, %s" % (seed, "level executor" if force_generic else "voice bank"))
