"""The spatialiser's move (fwgpu_spatial_move, CMD_SP_MOVE = 26; SPEC): a source's place in the stereo image moved
every frame by ONE message — the ear gains linearly, the per-ear delays as 32.32 fractions of a frame read with a two-tap blend.

The reference is tests/sp_move_model.py: tests/refmodel.py's SpatialNode with the move added (integers for the delays, np.float32
operations one at a time), inside a RefEngine.  Every comparison is bit equality (busnodes.assert_bits): there is no tolerance to choose.

CPU tier: the closed form against the iteration and against the g++ build of fwgpu_types.h sp_move_*; the model's own properties (block
splits, the state behind a move, no move = refmodel.SpatialNode, a set_position inside a move); the ABI on the host-only harness; the
pins; the planner on the fake-HIP harness.

GPU tier: ONE list of moves (script) through the level executor, the fused voice bank on planar f32, planar i16 and mono sources,
one-block calls, ragged calls, fwgpu_node_process; the accounting of calls around a move; a graph edit inside a move; silence flags
behind a one-shot; a seeded family.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import busnodes
import fwapi
import refmodel
import sp_move_model as sm
from busnodes import assert_bits
from fwapi import LOOP_FULL, PLANAR_F32, PLANAR_I16, GpuEngine, HostOnlyEngine
from refmodel import spatial_params
from scenarios import voice_source

INVALID = -20
F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FUZZ_SEEDS = int(os.environ.get("FWGPU_FUZZ_SEEDS", "20"))
ITD = 32                                   # round(0.00066 * 48000): the largest per-ear delay at 48 kHz
ULL = C.c_ulonglong


def fbits(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def ffrom(u):
    return np.array([u], dtype=np.uint32).view(F32)[0]


def peek():
    u, p = C.c_uint, C.c_void_p
    return fwapi.peek_lib("sp_move_peek", {
        "spp_move_book": (None, [p, C.POINTER(ULL)]), "spp_state_bytes": (u, []), "spp_init": (None, [p, u, u, C.c_int, C.c_int]),
        "spp_set_smoother": (None, [p, C.c_int, C.c_int, u, u]), "spp_start": (None, [p, u, u, C.c_int, C.c_int, u]), "spp_stop": (None, [p]),
        "spp_advance": (None, [p, u]), "spp_frame": (None, [p, u, C.POINTER(ULL)]), "spp_state": (None, [p, C.POINTER(ULL)]),
        "spp_tap": (u, [u, u, ULL]), "spp_unpack": (None, [C.POINTER(u), C.POINTER(u)]), "spp_pins": (None, [C.POINTER(u)])})


# ================================================================================================ CPU tier: the arithmetic
def _random_moves():
    """(G0l, G0r, G1l, G1r, D0l, D0r, d1l, d1r, N)"""
    rng = np.random.default_rng(2026)
    g = lambda: F32(rng.uniform(0.0, 1.0))
    cases = [
        (g(), g(), g(), g(), 0, ITD << 32, ITD, 0, 1),                                   # N == 1, a cross
        (g(), g(), g(), g(), ITD << 32, 0, 0, ITD, sm.FRAMES_MAX),                       # N == 2^24, a cross
        (g(), g(), g(), g(), 7 << 32, 0, 7, 0, 500),                                     # equal delays at both ends: inc == 0
        (F32(0.25), F32(0.25), F32(0.25), F32(0.25), 63 << 32, 0, 0, 63, 64),            # equal gains; the widest delays
        (g(), g(), g(), g(), (5 << 32) + 0x12345678, (31 << 32) + 0xffffff00, 32, 0, 777),   # a retarget from a fractional D0
        (g(), g(), g(), g(), (62 << 32) + 0xffffffff, 1, 63, 0, 3),
    ]
    while len(cases) < 200:
        kind = len(cases) % 5
        N = 1 if kind == 0 else int(rng.integers(1, 3000))
        D0 = [int(rng.integers(0, ITD + 1)) << 32 for _ in range(2)]
        if kind == 1:                                                                    # in mid-move: fractional
            D0 = [int(rng.integers(0, (ITD << 32) + 1)) for _ in range(2)]
        d1 = [int(rng.integers(0, ITD + 1)) for _ in range(2)]
        if kind == 2:                                                                    # |d1 << 32 - D0| < N: inc == 0
            D0 = [min(max((d1[e] << 32) + int(rng.integers(-N + 1, N)), 0), 63 << 32) for e in range(2)]
        cases.append((g(), g(), g(), g(), D0[0], D0[1], d1[0], d1[1], N))
    return cases


def _frames_to_check(N):
    return sorted(set(range(min(N, 130))) | set(range(max(N - 130, 0), N)) | {N // 2, N // 3})


def test_closed_form_equals_the_iteration_and_the_move_ends_exactly_on_the_target():
    zero_inc = one_frame = fractional = 0
    for G0l, G0r, G1l, G1r, D0l, D0r, d1l, d1r, N in _random_moves():
        one_frame += N == 1
        for G0, G1, D0, d1 in ((G0l, G1l, D0l, d1l), (G0r, G1r, D0r, d1r)):
            inc = sm.start(D0, d1, N)
            T = d1 << 32
            assert inc == (abs(T - D0) // N) * (1 if T >= D0 else -1)
            zero_inc += inc == 0 and T != D0
            fractional += (D0 & 0xffffffff) != 0
            lo, hi = min(D0, T), max(D0, T)
            glo, ghi = min(G0, G1), max(G0, G1)
            if N <= 4096:
                at = sm.iterate(D0, inc, d1, N, N + 3)
                assert at[N:] == [T, T, T]                                   # exactly the target, whatever the division left over
                assert all(at[t] == sm.delay_value(D0, inc, d1, N, t) for t in range(N))
            for t in _frames_to_check(N):
                D = sm.delay_value(D0, inc, d1, N, t)
                assert lo <= D <= hi, (D0, d1, N, t)
                q, f = sm.whole_frac(D)
                assert f == 0 or q <= 62, (D0, d1, N, t)
                assert 0 <= float(f) < 1 and float(f) * (1 << 24) == ((D & 0xffffffff) >> 8)       # 24 bits, exact
                gv = sm.gain_value(G0, G1, N, t)
                assert glo <= gv <= ghi, (G0, G1, N, t)
            assert sm.delay_value(D0, inc, d1, N, N) == T and fbits(sm.gain_value(G0, G1, N, N)) == fbits(G1)
            assert fbits(sm.gain_value(G0, G1, N, 0)) == fbits(G0)
    assert zero_inc >= 20 and one_frame >= 30 and fractional >= 40


def test_the_gxx_build_of_sp_move_agrees_with_the_model_bit_for_bit():
    P = peek()
    assert P.spp_state_bytes() == 128
    st, st2 = C.create_string_buffer(128), C.create_string_buffer(128)
    out, big = (ULL * 4)(), (ULL * 16)()
    rng = np.random.default_rng(7)
    for G0l, G0r, G1l, G1r, D0l, D0r, d1l, d1r, N in _random_moves():
        # reach (G0, D0) the way a node does: at rest for whole delays, through a first move for fractional ones
        whole = (D0l & 0xffffffff) == 0 and (D0r & 0xffffffff) == 0
        if whole:
            P.spp_init(st, fbits(G0l), fbits(G0r), D0l >> 32, D0r >> 32)
            if N % 2:                                   # a smoother on its way: the gain in force is `last`
                P.spp_set_smoother(st, 0, refmodel.ACTIVE, fbits(F32(0.9)), fbits(G0l))
            G0, D0 = [G0l, G0r], [D0l, D0r]
        else:
            P.spp_init(st, fbits(G0l), fbits(G0r), 0, ITD)
            P.spp_start(st, fbits(G1l), fbits(G1r), ITD, 0, 1000)
            k0 = int(rng.integers(1, 999))
            P.spp_advance(st, k0)
            i0 = [sm.start(0, ITD, 1000), sm.start(ITD << 32, 0, 1000)]
            D0 = [sm.delay_value(0, i0[0], ITD, 1000, k0), sm.delay_value(ITD << 32, i0[1], 0, 1000, k0)]
            G0 = [sm.gain_value(G0l, G1l, 1000, k0), sm.gain_value(G0r, G1r, 1000, k0)]
            G1l, G1r = F32(rng.uniform(0, 1)), F32(rng.uniform(0, 1))
        P.spp_start(st, fbits(G1l), fbits(G1r), d1l, d1r, N)
        inc = [sm.start(D0[0], d1l, N), sm.start(D0[1], d1r, N)]
        P.spp_state(st, big)
        assert list(big[:8]) == [N, 0, D0[0], D0[1], inc[0] & sm.M64, inc[1] & sm.M64, d1l, d1r], (list(big[:8]), D0, inc)
        assert list(big[8:16]) == [0, fbits(G1l), fbits(G1l), 0, fbits(G1r), fbits(G1r), fbits(G1l), fbits(G1r)]   # the smoothers rest at the target
        # frames of a first block, then of a block further on (the state advanced), then behind the move
        split = min(N - 1, 100) if N > 1 else 0
        for t in _frames_to_check(N) + [N, N + 5]:
            if t >= split and split:
                memo = bytes(st.raw)
                C.memmove(st2, memo, 128)
                P.spp_advance(st2, split)
                P.spp_frame(st2, t - split, out)
            else:
                P.spp_frame(st, t, out)
            want = [fbits(sm.gain_value(G0[0], G1l, N, t)), fbits(sm.gain_value(G0[1], G1r, N, t)),
                    sm.delay_value(D0[0], inc[0], d1l, N, t), sm.delay_value(D0[1], inc[1], d1r, N, t)]
            assert list(out) == want, (N, t, list(out), want)
        P.spp_advance(st, N)
        P.spp_state(st, big)
        assert list(big[:2]) == [0, 0] and list(big[6:8]) == [d1l, d1r]                  # at rest at the target
    for D in (0, 5 << 32, (5 << 32) + 0x100, (5 << 32) + 0xff, (62 << 32) + 0xffffffff, (31 << 32) + 0x80000000):
        for a, b in ((0.5, -0.25), (1.0, 1.0), (-0.0, 0.0), (3e-39, 1.0)):
            assert P.spp_tap(fbits(a), fbits(b), D) == fbits(sm.tap(F32(a), F32(b), D)), (D, a, b)
    # a corrupted message is a step
    P.spp_init(st, fbits(0.5), fbits(0.25), 3, 0)
    for bad in (0, sm.FRAMES_MAX + 1):
        P.spp_start(st, fbits(0.75), fbits(0.125), 0, 9, bad)
        P.spp_state(st, big)
        assert list(big[:2]) == [0, 0] and list(big[6:8]) == [0, 9] and big[14] == fbits(0.75)


def test_trunc_div_is_cxx_division():
    for a, b, q in ((7, 2, 3), (-7, 2, -3), (0, 5, 0), (-1, 1 << 24, 0), (-(63 << 32), 1, -(63 << 32)), ((63 << 32) - 1, 1 << 24, (63 << 8) - 1)):
        assert sm.trunc_div(a, b) == q


# ------------------------------------------------------------------------------------------------ graphs (any fwapi.Engine)
POS = [(-3.0, 0.0, -1.0), (2.5, 0.5, -2.0), (0.0, 0.0, -1.0), (-0.4, 0.2, -0.3), (6.0, -1.0, 3.0), (-4.0, 0.0, -0.5), (0.7, 0.0, 0.1)]


def build(e, n_voices, lens=None, loops=None, fmt=PLANAR_F32, ch=2, leaf=20, spare_port=False, unmoved_extra=False):
    """voices sampler -> [volume] -> spatialiser under SumNodes of `leaf` ports -> graph_out; returns [(sampler, spatialiser)]"""
    rng = np.random.default_rng(99)
    lens = lens or [3000 + 37 * v for v in range(n_voices)]
    loops = loops or [True] * n_voices
    voices, ends = [], []
    for v in range(n_voices):
        s = e.sampler(float(rng.uniform(60, 100)))
        cur = s
        if v % 3 == 1:
            vol = e.volume(float(rng.uniform(40, 100)))
            e.connect_stereo(cur, vol)
            cur = vol
        x, y, z = POS[v % len(POS)]
        sp = e.spatial(x, y, z, n_in=2)
        e.connect_stereo(cur, sp)
        voices.append((s, sp))
        ends.append(sp)
    mixers = []
    for i in range(0, n_voices, leaf):
        grp = ends[i:i + leaf]
        m = e.sum(len(grp) + (1 if spare_port and i == 0 else 0))
        if i == 0:
            e.the_mixer, e.the_free_port = m, len(grp)
        for p, n in enumerate(grp):
            e.connect_stereo(n, m, 2 * p)
        mixers.append(m)
    top = mixers[0]
    if len(mixers) > 1:
        top = e.sum(len(mixers))
        for p, m in enumerate(mixers):
            e.connect_stereo(m, top, 2 * p)
    e.connect_stereo(top, e.graph_out_node)
    e.update()
    for v, (s, _) in enumerate(voices):
        start_voice(e, s, 7100 + v, lens[v], loops[v], fmt, ch)
    return voices


def start_voice(e, s, seed, frames, loop, fmt=PLANAR_F32, ch=2):
    data = voice_source(seed, frames, ch)
    smp = e.new_sample(fmt, ch, np.round(data * 32767).astype(np.int16) if fmt == PLANAR_I16 else data)
    e.sampler_set_sample(s, smp)
    if loop:
        e.sampler_set_loop_range(s, LOOP_FULL)
    e.sampler_play(s)


def set_position(e, sp, x, y, z, at_block=0):
    for i, v in enumerate((x, y, z)):
        e.set_param(sp, i, v, at_block=at_block)


def _model(F, n_voices=1, **kw):
    e = sm.MoveRefEngine(max_block_frames=F, short_blocks=True)
    return e, build(e, n_voices, **kw)


# ================================================================================================ CPU tier: the model
@pytest.mark.parametrize("N", [1, 37, 300])
def test_model_block_splits_give_the_same_samples_and_state(N):
    total = 448
    splits = {"one": [total], "1": [1] * total, "7": [7] * 64, "40": [40] * 11 + [8], "64": [64] * 7, "mixed": [64, 1, 100, 7, 256, 20]}
    runs = {}
    for name, blocks in splits.items():
        assert sum(blocks) == total
        e, ((_, sp),) = _model(512)
        e.move(sp, 4.0, 0.0, -0.5, N)
        out = np.concatenate([e.process_interleaved(b) for b in blocks])
        n = e.nodes[sp]
        runs[name] = (out, (n.N, n.k, n.dl, n.dr, fbits(n.gl), fbits(n.gr), n.sl.status, fbits(n.sl.input), fbits(n.sl.last_output), bytes(n.hist)))
    for name in splits:
        assert_bits(runs[name][0], runs["one"][0], name)
        assert runs[name][1] == runs["one"][1], name
    assert runs["one"][1][:2] == (0, 0) and np.any(runs["one"][0] != 0)


def test_model_behind_a_move_the_node_is_a_fresh_node_at_the_target_fed_the_same_history():
    F = 64
    e, ((_, sp),) = _model(F)
    e.process_blocks(1)
    e.move(sp, 2.0, 0.3, -0.7, 150)
    a = [e.process_blocks(1) for _ in range(3)]
    n = e.nodes[sp]
    assert n.N == 0 and n.k == 0
    f, ((_, fp),) = _model(F)
    f.process_blocks(4)                                      # the same source frames; its own position does not matter ...
    m = f.nodes[fp]
    fresh = refmodel.SpatialNode(f, 2, 2, [2.0, 0.3, -0.7])   # ... because the node is replaced by a FRESH one at the target
    fresh.hist = m.hist.copy()
    f.nodes[fp] = fresh
    assert (n.gl, n.gr, n.dl, n.dr) == (fresh.gl, fresh.gr, fresh.dl, fresh.dr) and np.array_equal(fwapi.bits(n.hist), fwapi.bits(fresh.hist))
    assert_bits(np.concatenate([e.process_blocks(1) for _ in range(4)]), np.concatenate([f.process_blocks(1) for _ in range(4)]), "behind the move")
    assert np.any(np.concatenate(a) != 0)


def test_model_without_a_move_is_refmodels_spatialiser():
    def run(e):
        vs = build(e, 3)
        outs = [e.process_blocks(2)]
        set_position(e, vs[1][1], 3.0, 0.0, 1.0)
        outs.append(e.process_blocks(3))
        return np.concatenate(outs)
    assert_bits(run(sm.MoveRefEngine(max_block_frames=64, short_blocks=True)), run(refmodel.RefEngine(max_block_frames=64, short_blocks=True)), "no move")


def test_model_messages_during_a_move():
    F = 64
    e, ((_, sp),) = _model(F)
    n = e.nodes[sp]
    e.process_blocks(1)
    g_start = (n.gl, n.gr)
    e.move(sp, 4.0, 0.0, -0.5, 640)
    tl, tr, dl, dr = spatial_params(4.0, 0.0, -0.5, 48000)
    assert (n.N, n.k, n.dl, n.dr) == (640, 0, dl, dr) and n.sl.status == refmodel.INACTIVE and n.sl.input == tl == n.sl.last_output
    assert (fbits(n.G0[0]), fbits(n.G0[1])) == (fbits(g_start[0]), fbits(g_start[1]))
    e.process_blocks(3)
    assert n.k == 192 and n.D[0] == 192 * n.inc[0] + (0 << 32) and n.D[0] & 0xffffffff      # fractional by now
    mid_g = sm.gain_value(n.G0[0], tl, 640, 192)
    mid_D = list(n.D)
    e.move(sp, -4.0, 0.0, -0.5, 100)                         # a retarget starts from where the first move stands
    assert (n.N, n.k) == (100, 0) and n.D == mid_D and fbits(n.G0[0]) == fbits(mid_g)
    assert n.inc[0] == sm.trunc_div((n.dl << 32) - mid_D[0], 100)
    e.process_blocks(1)
    now_g = sm.gain_value(n.G0[1], n.gr, 100, 64)
    e.set_param(sp, 0, 1.0)                                  # a plain set_position ends the move ...
    assert n.N == 0 and n.k == 0 and fbits(n.sr_.last_output) == fbits(now_g) and n.sr_.status == refmodel.INACTIVE
    want = spatial_params(1.0, 0.0, -0.5, 48000)
    assert (n.gl, n.gr, n.dl, n.dr) == want                   # ... the delays step, the gains glide on from the move's values
    out = e.process_blocks(1)
    assert n.sr_.status == refmodel.ACTIVE and np.any(out != 0)
    e.move(sp, 0.0, 1.0, 0.0, 0)                             # frames == 0 is a step
    assert n.N == 0 and (n.gl, n.gr, n.dl, n.dr) == spatial_params(0.0, 1.0, 0.0, 48000)


# ================================================================================================ CPU tier: the ABI on the harness
def _early(P, c):
    """[(type, block, f0 bits, i0, i1, d0 bits)] of the messages waiting for their node's first plan"""
    return [(w[0], w[1], w[2], w[3], w[4], w[5] | (w[6] << 32)) for w in fwapi.early_msgs(P, c)]


def _move_msg(x, y, z, frames, block, sr=48000):
    gl, gr, dl, dr = spatial_params(x, y, z, sr)
    return (sm.CMD_SP_MOVE, block, 0, dl | (dr << 6), frames, fbits(gl) | (fbits(gr) << 32))


def _step_msgs(x, y, z, block, sr=48000):
    gl, gr, dl, dr = spatial_params(x, y, z, sr)
    return [(sm.CMD_SET_P0, block, fbits(gl), 0, 0, 0), (sm.CMD_SET_P1, block, fbits(gr), 0, 0, 0), (sm.CMD_SP_ITD, block, fbits(gr), dl, dr, 0)]


def test_abi_what_a_call_queues():
    """one Cmd per call: CMD_SP_MOVE with what spatial_params yields for the target; frames == 0 queues the three messages that the
    last of three fwgpu_node_set_param calls for that position queues (the six in front of them are overwritten by them).  Read where
    the ABI keeps the messages of a node no plan holds yet."""
    P = peek()
    e = HostOnlyEngine(sample_rate=44100, max_block_frames=96, num_graph_inputs=3, num_graph_outputs=2)
    L, c = e.cx.L, e.cx.c
    assert P.fwp_layout_check(c, 44100, 96, 3, 2, 0) == 0
    assert P.fwp_layout_check(c, 44100, 64, 3, 2, 0) == 2
    sp = e.spatial(-3.0, 0.0, -1.0, n_in=2)
    assert _early(P, c) == []
    assert L.fwgpu_spatial_move(c, sp, 4.0, 0.0, -0.5, sm.FRAMES_MAX, 0) == 0               # the longest move
    assert L.fwgpu_spatial_move(c, sp, -1e9, 0.0, 0.0, 1, 3) == 0                            # any coordinates but NaN
    assert L.fwgpu_spatial_move(c, sp, 0.5, 2.0, -0.25, 0, 2) == 0                           # frames == 0 ...
    assert L.fwgpu_spatial_move(c, sp, float("nan"), 0.0, 0.0, 10, 0) == INVALID             # a refused call queues nothing
    assert L.fwgpu_spatial_move(c, sp, 0.0, 0.0, float("nan"), 0, 0) == INVALID
    assert L.fwgpu_spatial_move(c, sp, 1.0, 0.0, 0.0, sm.FRAMES_MAX + 1, 0) == INVALID
    e.set_param(sp, 1, 7.0, at_block=5)                                                     # ... and a later set_param starts from the target
    got = _early(P, c)
    want = ([_move_msg(4.0, 0.0, -0.5, sm.FRAMES_MAX, 0, 44100), _move_msg(-1e9, 0.0, 0.0, 1, 3, 44100)] + _step_msgs(0.5, 2.0, -0.25, 2, 44100) +
            _step_msgs(0.5, 7.0, -0.25, 5, 44100))
    assert got == want, (got, want)
    # ... which is what three set_param calls queue (the last three of their nine are the position's)
    f = HostOnlyEngine(sample_rate=44100, max_block_frames=96, num_graph_inputs=3, num_graph_outputs=2)
    fp = f.spatial(-3.0, 0.0, -1.0, n_in=2)
    set_position(f, fp, 0.5, 2.0, -0.25, at_block=2)
    assert _early(P, f.cx.c)[-3:] == _step_msgs(0.5, 2.0, -0.25, 2, 44100)
    # the reader gives the message's fields back
    words, out = (C.c_uint * 9)(*fwapi.early_msgs(P, c)[0]), (C.c_uint * 5)()
    P.spp_unpack(words, out)
    gl, gr, dl, dr = spatial_params(4.0, 0.0, -0.5, 44100)
    assert list(out) == [fbits(gl), fbits(gr), dl, dr, sm.FRAMES_MAX]
    e.connect_stereo(sp, e.graph_out_node)
    e.update()                                                                              # the plan that activates the node releases them
    assert _early(P, c) == []
    e.process_blocks(4)
    assert e.violation() == ""


def test_abi_refusals():
    e = HostOnlyEngine(max_block_frames=64, max_batch=4)
    vs = build(e, 3)
    L, c = e.cx.L, e.cx.c
    vol = e.volume(50.0)
    sp = vs[0][1]
    for bad, word in ((lambda: L.fwgpu_spatial_move(c, vol, 1.0, 0.0, 0.0, 10, 0), "not a SpatialNode"),
                      (lambda: L.fwgpu_spatial_move(c, vs[0][0], 1.0, 0.0, 0.0, 10, 0), "not a SpatialNode"),
                      (lambda: L.fwgpu_spatial_move(c, sp, float("nan"), 0.0, 0.0, 10, 0), "NaN"),
                      (lambda: L.fwgpu_spatial_move(c, sp, 0.0, float("nan"), 0.0, 10, 0), "NaN"),
                      (lambda: L.fwgpu_spatial_move(c, sp, 1.0, 0.0, 0.0, sm.FRAMES_MAX + 1, 0), "2^24"),
                      (lambda: L.fwgpu_spatial_move(c, 1 << 40, 1.0, 0.0, 0.0, 10, 0), "unknown node")):
        assert bad() == INVALID
        assert word in L.fwgpu_last_error(c).decode()
    assert L.fwgpu_spatial_move(None, sp, 1.0, 0.0, 0.0, 10, 0) == INVALID


def test_abi_a_move_for_a_node_no_plan_holds_yet_waits_for_the_update():
    P = peek()
    e = HostOnlyEngine(max_block_frames=64)
    sp = e.spatial(1.0, 0.0, -1.0, n_in=2)
    assert e.cx.L.fwgpu_spatial_move(e.cx.c, sp, -2.0, 0.0, -1.0, 100, 0) == 0
    assert len(_early(P, e.cx.c)) == 1
    e.connect_stereo(sp, e.graph_out_node)
    e.update()
    assert _early(P, e.cx.c) == []
    e.process_blocks(1)
    assert e.violation() == ""


def test_typed_mirror():
    import firewheel_amd as fa

    cx = fwapi.hostonly_ctx(max_block_frames=64)
    node = fa.SpatialNode(1.0, 0.0, -1.0)
    nid = cx.add_node(2, 2, node)
    node.move_to(-2.0, 0.0, -1.0, 480)                     # before the first update
    cx.connect(nid, 0, cx.graph_out_node(), 0)
    cx.update()
    node.move_to(0.5, 0.5, 0.5, 100, at_block=2)
    node.move_to_secs(3.0, 0.0, 0.0, 0.01)
    node.move_to(2.0, 0.0, 0.0, 0)
    assert node.pos == [2.0, 0.0, 0.0] and fa.SpatialNode.MOVE_FRAMES_MAX == sm.FRAMES_MAX
    for bad in (lambda: node.move_to(float("nan"), 0.0, 0.0, 10), lambda: node.move_to(1.0, 0.0, 0.0, sm.FRAMES_MAX + 1)):
        with pytest.raises(fa.FwgpuError) as ei:
            bad()
        assert ei.value.code == INVALID
    assert "glide_to(doppler_ratio(" in fa.SpatialNode.move_to.__doc__       # the fly-by


def test_pins_header_types_ffi_and_lib_agree():
    import firewheel_amd._lib as flib

    rd = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr, types = rd("include", "fwgpu.h"), rd("firewheel_amd", "csrc", "fwgpu_types.h")
    ffi, nodes = rd("rust", "firewheel-gpu", "src", "ffi.rs"), rd("rust", "firewheel-gpu", "src", "nodes.rs")
    assert re.search(r"#define FWGPU_SPATIAL_MOVE_FRAMES_MAX 16777216\b", hdr)
    assert "int fwgpu_spatial_move(fwgpu_ctx* ctx, int64_t node, float x, float y, float z, uint32_t frames, uint32_t at_block);" in hdr
    assert re.search(r"CMD_SP_MOVE = 26\b", types) and re.search(r"#define SP_MOVE_FRAMES_MAX 16777216u", types)
    assert re.search(r"K_LAST = K_CROSSFADE\b", types)           # no new node kind
    assert "pub const FWGPU_SPATIAL_MOVE_FRAMES_MAX: u32 = 16777216;" in ffi
    assert "pub fn fwgpu_spatial_move(ctx: *mut fwgpu_ctx, node: i64, x: f32, y: f32, z: f32, frames: u32, at_block: u32) -> c_int;" in ffi
    assert "pub fn move_to" in nodes and "ffi::fwgpu_spatial_move" in nodes
    res, args = flib.SIGNATURES["fwgpu_spatial_move"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32]
    pins = (C.c_uint * 6)()
    peek().spp_pins(pins)
    assert list(pins) == [26, 20, 20, 128, 40, 1 << 24]        # CMD_SP_MOVE, K_LAST == K_CROSSFADE, NodeState, Cmd, the cap


# ================================================================================================ CPU tier: the planner
def _book(P, e):
    out = (ULL * 3)()
    P.spp_move_book(e.cx.c, out)
    return list(out)


@pytest.mark.parametrize("force_generic", [False, True])
def test_planner_a_call_inside_a_move_runs_the_control_kernel_and_a_bank_without_one_launches_what_it_launched(force_generic):
    P = peek()
    F, K = 64, 4

    def run(move):
        e = HostOnlyEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)
        vs = build(e, 6)
        assert e.cx.plan_kind() == (0 if force_generic else 1)
        e.process_blocks(K)
        e.reset_launches()
        per_call, books = [], []
        for call in range(6):
            if move and call == 1:
                assert e.cx.L.fwgpu_spatial_move(e.cx.c, vs[2][1], 4.0, 0.0, -0.5, 2 * K * F + 9, 1) == 0    # through calls 1, 2 and into call 3
            before = e.launches()
            e.process_blocks(K)
            after = e.launches()
            per_call.append({k: after[k] - before[k] for k in after})
            books.append(_book(P, e))
        assert e.violation() == ""
        return per_call, books

    moved, books = run(True)
    still, still_books = run(False)
    assert all(b[2] == 0 and b[1] == 0 for b in still_books)
    # the host's book: calls 1, 2 and 3 may meet the move (it starts one block into call 1), the others cannot
    assert [b[2] for b in books] == [0, 1, 1, 1, 0, 0], books
    assert books[1][1] == 2 * K * F + F + 2 * K * F + 9      # two calls done, one block into the third, the move's frames
    if not force_generic:
        assert all(c["voice_control"] == 1 and c["leaf_sum"] == 1 for c in moved), moved
    # by kind, the never-moved bank launches what the moved one launches: the move changes WHICH instantiation runs, never how many kernels
    assert moved == still, (moved, still)


def test_planner_an_unrelated_never_moved_spatialiser_voice_changes_no_launch_and_opens_no_book():
    """the same bank with and without one more spatialiser voice that never moves: launches by kind per call are the same, and the
    host's book never opens (the launch stubs count launches by kind, not by instantiation: which build a launch picks follows
    DevView / FusedView::sp_moves, which is the book's live flag)"""
    P = peek()
    F, K = 64, 4

    def run(n):
        e = HostOnlyEngine(max_block_frames=F, max_batch=K)
        vs = build(e, n)
        set_position(e, vs[0][1], 1.0, 0.0, 2.0)                  # a plain step is no move
        e.process_blocks(K)
        e.reset_launches()
        per_call = []
        for _ in range(4):
            before = e.launches()
            e.process_blocks(K)
            after = e.launches()
            per_call.append({k: after[k] - before[k] for k in after})
            assert _book(P, e)[1:] == [0, 0]
        assert e.violation() == "" and e.cx.plan_kind() == 1
        return per_call

    assert run(6) == run(7)


def test_planner_a_spatialiser_that_leaves_the_plan_in_mid_move_meets_the_move_builds_when_it_returns():
    """the host's bound counts frames from the message on; a node that is disconnected in mid-move keeps its move in its state slot, so
    the plan install that may bring it back opens the book again for the move's length"""
    P = peek()
    F, K, N = 64, 4, 10 * 64
    e = HostOnlyEngine(max_block_frames=F, max_batch=K)
    vs = build(e, 3)
    s, sp = vs[1]
    assert e.cx.L.fwgpu_spatial_move(e.cx.c, sp, 4.0, 0.0, -0.5, N, 0) == 0
    e.process_blocks(K)
    assert _book(P, e) == [K * F, N, 1]
    for port in (0, 1):
        e.disconnect(sp, port, e.the_mixer, 2 + port)
    e.update()                                                    # the node leaves the plan with 384 frames of its move to go
    live = []
    for _ in range(5):
        e.process_blocks(K)
        live.append(_book(P, e)[2])
    assert live == [1, 1, 1, 0, 0], live                          # the bound was extended by N at the install, then runs out
    e.connect_stereo(sp, e.the_mixer, 2)
    e.update()                                                    # ... and the install that brings it back opens it again, for N frames
    live = []
    for _ in range(4):
        e.process_blocks(K)
        live.append(_book(P, e)[2])
    assert live == [1, 1, 1, 0], live
    assert e.violation() == ""


# ================================================================================================ GPU tier: the list of moves
N_CALLS = 5      # call 0 and call 4 carry no message


def _at(K, call, where, plus=0):
    """(call, at_block) of block `where` ('first' / 'mid' / 'last') of `call`, `plus` blocks further on"""
    g = call * K + {"first": 0, "mid": K // 2, "last": K - 1}[where] + plus
    return g // K, g % K


def script(F, K):
    """per item: (loops, sample frames, [(call, at_block, message, args)]) — voice v of a bank plays item v % len from POS[v % len(POS)]"""
    A = lambda where, plus=0, call=1: _at(K, call, where, plus)
    M = lambda pos, x, y, z, N: pos + ("move", (x, y, z, N))
    S = lambda pos, x, y, z: pos + ("set", (x, y, z))
    T = lambda pos, what: pos + (what, ())
    return [
        (True, 3000, [M(A("first"), 3.0, 0.0, -1.0, 1)]),                                              # N = 1
        (True, 3100, [M(A("mid"), 0.5, 1.0, 2.0, 37)]),                                                # ends inside a block
        (True, 2900, [M(A("first"), -5.0, 0.0, 0.5, 5000)]),                                           # spans calls
        (True, 3000, [M(A("first"), 4.0, 0.0, -0.5, 6 * F), M(A("first", 2), -4.0, 0.3, -0.5, 2 * F + 5)]),   # a retarget in mid-move
        (True, 3050, [M(A("first"), 4.0, 0.0, -0.5, 6 * F), S(A("first", 3), -1.0, 0.0, -1.0)]),       # a set_position in mid-move
        (True, 3000, [S(A("first", call=0), -4.0, 0.0, -0.5), M(A("mid"), 4.0, 0.0, -0.5, 3 * F + 7)]),   # a cross in front of the listener
        (True, 2800, [M(A("last"), 2.0, 0.0, -2.0, 0)]),                                               # frames == 0: a step
        (False, 9 * F + 11 if K > 1 else 3 * F + 11, [M(A("first"), -3.0, 0.0, 2.0, 40 * F)]),         # a one-shot ends inside the move
        (True, 3000, [M(A("mid"), 1.0, 0.0, -1.0, 2 * F), M(A("mid"), 1.0, 0.0, -1.0, F + 3)]),        # two moves for one block
        (True, 3000, [M(A("first"), -2.0, 0.0, -1.0, 5 * F), T(A("first", 1), "pause"), T(A("first", 3), "play")]),   # the source pauses: the move goes on
        (True, 3000, [S(A("mid"), 2.0, 0.0, 0.0), M(A("mid", 1), -2.0, 0.0, 0.0, 4 * F + 1)]),         # from a smoother still on its way
        (True, 3000, []),                                                                              # never moved
    ]


def run_script(e, F, K, n_voices, n_calls=N_CALLS, calls=None, **kw):
    items = script(F, K)
    pick = [items[v % len(items)] for v in range(n_voices)]
    vs = build(e, n_voices, lens=[p[1] for p in pick], loops=[p[0] for p in pick], **kw)
    outs = []
    for call in range(n_calls):
        for v, p in enumerate(pick):
            s, sp = vs[v]
            for c, at, what, args in p[2]:
                if c != call:
                    continue
                if calls is not None:
                    at = 0                          # (ragged calls take their messages at their first block)
                if what == "move":
                    e.move(sp, args[0], args[1], args[2], args[3], at_block=at)
                elif what == "set":
                    set_position(e, sp, args[0], args[1], args[2], at_block=at)
                elif what == "pause":
                    e.sampler_pause(s, at_block=at)
                else:
                    e.sampler_play(s, at_block=at)
        outs.append(np.asarray(e.process_blocks(K) if calls is None else e.process_interleaved(calls[call])))
    return np.concatenate(outs)


_refs = {}


def reference(F, K, n_voices, n_calls=N_CALLS, calls=None, **kw):
    key = (F, K, n_voices, n_calls, None if calls is None else tuple(calls), tuple(sorted(kw.items())))
    if key not in _refs:
        out = run_script(sm.Tagged(sm.MoveRefEngine(max_block_frames=F, short_blocks=True)), F, K, n_voices, n_calls, calls, **kw)
        out.setflags(write=False)
        assert np.any(out != 0)
        _refs[key] = out
    return _refs[key]


COMBOS = [(40, 3, 5), (64, 5, 37), (100, 1, 37), (512, 3, 5), (64, 1, 5), (100, 5, 5), (256, 3, 37), (128, 5, 5)]      # F, K, voices
SMALL = [(64, 3, 37), (512, 1, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g1_level_executor(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K, force_generic=True)
    got = run_script(sm.GpuMove(g), F, K, V)
    assert g.cx.plan_kind() == 0
    assert_bits(got, reference(F, K, V), "level executor")


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g2_fused_voice_bank_planar_f32(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(sm.GpuMove(g), F, K, V)
    # (a spatialiser voice is a voice-bank shape when the block is whole 64-frame tiles: fwgpu_plan_detect.cpp; blocks of 40 and 100
    #  frames go through whatever plan the product picks for them, and must give the same bits)
    if F % 64 == 0:
        assert g.cx.plan_kind() == 1 and g.cx.plan_fused_voices() == V
    assert_bits(got, reference(F, K, V), "voice bank, planar f32")


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", SMALL)
@pytest.mark.parametrize("fmt,ch", [(PLANAR_I16, 2), (PLANAR_F32, 1), (PLANAR_I16, 1)])
def test_g3_planar_i16_and_mono_sources(fmt, ch, F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(sm.GpuMove(g), F, K, V, fmt=fmt, ch=ch)
    assert g.cx.plan_kind() == 1
    assert_bits(got, reference(F, K, V, fmt=fmt, ch=ch), "format %d, %d channel(s)" % (fmt, ch))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 256])
def test_g4_one_block_calls(F):
    V, K, calls = 37, 1, 12
    g = GpuEngine(max_block_frames=F)
    got = run_script(sm.GpuMove(g), F, K, V, n_calls=calls)
    assert g.cx.plan_kind() == 1
    assert_bits(got, reference(F, K, V, n_calls=calls), "one-block calls")


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
@pytest.mark.parametrize("F", [40, 64])
def test_g5_ragged_calls(F, force_generic):
    calls = busnodes.ragged_calls(F, at_least=20 * F)
    g = GpuEngine(max_block_frames=F, max_batch=5, force_generic=force_generic)
    got = run_script(sm.GpuMove(g), F, 5, 5, n_calls=len(calls), calls=calls)
    assert_bits(got, reference(F, 5, 5, n_calls=len(calls), calls=calls), "ragged calls")


@pytest.mark.gpu
@pytest.mark.parametrize("F", [40, 64, 100, 256])
def test_g6_node_process(F):
    """fwgpu_node_process (k_single_node): one spatialiser, one block per call, every kind of message between the calls — samples and
    out mask of every block against MoveSpatialNode.process"""
    g = GpuEngine(max_block_frames=256)
    sp = g.spatial(-3.0, 0.0, -1.0, n_in=2)
    g.connect_stereo(sp, g.graph_out_node)
    g.update()
    e = sm.MoveRefEngine(max_block_frames=256, short_blocks=True)
    mp = e.spatial(-3.0, 0.0, -1.0, n_in=2)
    node = e.nodes[mp]
    gg = sm.GpuMove(g)
    rng = np.random.default_rng(F)
    moved = 0
    for k in range(14):
        if k == 1:
            gg.move(sp, 4.0, 0.0, -0.5, 2 * F + F // 2)    # ends inside call 3
            e.move(mp, 4.0, 0.0, -0.5, 2 * F + F // 2)
        if k == 5:
            gg.move(sp, -4.0, 0.0, -0.5, 3)
            e.move(mp, -4.0, 0.0, -0.5, 3)
        if k == 7:
            gg.move(sp, 1.0, 2.0, 0.5, 4 * F + 1)
            e.move(mp, 1.0, 2.0, 0.5, 4 * F + 1)
        if k == 9:                                          # a retarget, then a set_position in mid-move
            gg.move(sp, -1.0, 0.0, 0.0, 3 * F)
            e.move(mp, -1.0, 0.0, 0.0, 3 * F)
        if k == 10:
            set_position(g, sp, 3.0, 0.0, 1.0)
            set_position(e, mp, 3.0, 0.0, 1.0)
        moved += node.N != 0
        ins = [rng.uniform(-1, 1, F).astype(F32), rng.uniform(-1, 1, F).astype(F32)]
        y, om = g.node_process(sp, F, ins, 2)
        outs = [np.zeros(F, dtype=F32), np.zeros(F, dtype=F32)]
        wm = node.process(F, ins, outs, 0)
        assert om == wm == 0
        assert_bits(y, np.stack(outs), "block %d" % k)
    assert moved >= 7 and node.N == 0


# ------------------------------------------------------------------------------------------------ calls around a move
@pytest.mark.gpu
def test_g7_voices_that_do_not_move_keep_their_accounting():
    """a bank in which three voices of twelve move: bit-exact over twelve calls, and the calls are counted exactly as the same calls of
    the same bank without a move are (include/fwgpu.h fwgpu_lazy_stats: a bank with spatialiser stages runs its control kernel in
    every call — the steady voices take its cached path, which the bits of the calls behind the move go through again)"""
    F, K, V = 64, 4, 12

    def run(e, move):
        vs = build(e, V)
        outs, marks = [], []
        for call in range(12):
            if move and call == 4:
                for v in (0, 5, 11):
                    e.move(vs[v][1], 4.0 - v, 0.0, -0.5, 9 * F + 3, at_block=1)      # through calls 4, 5 and into call 6
            outs.append(np.asarray(e.process_blocks(K)))
            if hasattr(e, "cx"):
                marks.append(e.cx.lazy_stats())
        return np.concatenate(outs), marks

    want, _ = run(sm.Tagged(sm.MoveRefEngine(max_block_frames=F, short_blocks=True)), True)
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got, marks = run(sm.GpuMove(g), True)
    assert g.cx.plan_kind() == 1
    assert_bits(got, want, "twelve calls")
    _, still = run(sm.GpuMove(GpuEngine(max_block_frames=F, max_batch=K)), False)
    assert marks == still, (marks, still)


# ------------------------------------------------------------------------------------------------ a graph edit inside a move
@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g8_the_move_carries_over_a_plan_install(force_generic):
    F, K, V = 64, 3, 6

    def run(e):
        vs = build(e, V, leaf=8, spare_port=True)
        outs = [np.asarray(e.process_blocks(K))]
        e.move(vs[0][1], 4.0, 0.0, -0.5, 8 * F + 9, at_block=1)
        e.move(vs[1][1], -4.0, 1.0, 0.5, 8 * F + 9, at_block=2)
        outs.append(np.asarray(e.process_blocks(K)))
        # a voice is added to the mixer's free port between two calls of the move
        s = e.sampler(80.0)
        sp = e.spatial(1.0, 0.0, 1.0, n_in=2)
        e.connect_stereo(s, sp)
        e.connect_stereo(sp, e.the_mixer, 2 * e.the_free_port)
        e.update()
        start_voice(e, s, 50, 900, True)
        for _ in range(3):
            outs.append(np.asarray(e.process_blocks(K)))
        return np.concatenate(outs)

    want = run(sm.Tagged(sm.MoveRefEngine(max_block_frames=F, short_blocks=True)))
    g = GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)
    got = run(sm.GpuMove(g))
    assert g.cx.plan_kind() == (0 if force_generic else 1)
    assert_bits(got, want, "a plan install between two calls of a move")


# ------------------------------------------------------------------------------------------------ silence flags behind a one-shot
@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g9_a_one_shot_that_ends_inside_a_move_leaves_the_output_unflagged(force_generic):
    F, K = 64, 6

    def run(e):
        ((s, sp),) = build(e, 1, lens=[3 * F + 20], loops=[False])
        e.move(sp, 4.0, 0.0, -0.5, 20 * F, at_block=1)
        a, fa = e.process_blocks_flags(K)
        b, fb = e.process_blocks_flags(K)
        return np.concatenate([np.asarray(a), np.asarray(b)]), np.concatenate([np.asarray(fa, dtype=bool), np.asarray(fb, dtype=bool)])

    want, wf = run(sm.Tagged(sm.MoveRefEngine(max_block_frames=F, short_blocks=True)))
    got, gf = run(sm.GpuMove(GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)))
    assert not wf.any() and np.any(want != 0)               # the spatialiser never flags its output: the history drains, the move goes on
    assert np.array_equal(gf, wf), (gf.T, wf.T)
    assert_bits(got, want, "one-shot")
    tail = want.reshape(-1, 2)[5 * F:]
    assert np.all(tail == 0)                                 # drained


# ------------------------------------------------------------------------------------------------ the seeded family
def fuzz(e, seed, F):
    rng = np.random.default_rng(41_000 + seed)
    V = 18
    lens = [int(rng.choice([37, 700, 3000])) for _ in range(V)]
    loops = [bool(rng.random() < 0.7) and lens[v] >= 700 for v in range(V)]      # (a loop shorter than a block is outside the sampler's domain)
    vs = build(e, V, lens=lens, loops=loops, leaf=10, spare_port=True)
    outs = []
    coord = lambda: float(rng.choice([-6.0, -1.5, -0.2, 0.0, 0.3, 2.0, 5.0]))
    for call in range(5):
        K = int(rng.integers(1, 5))
        if call == 2:                                        # a graph edit: one more voice on the first mixer's free port
            s = e.sampler(70.0)
            sp = e.spatial(coord(), 0.0, coord(), n_in=2)
            e.connect_stereo(s, sp)
            e.connect_stereo(sp, e.the_mixer, 2 * e.the_free_port)
            e.update()
            start_voice(e, s, 600 + seed, 800, True)
            vs.append((s, sp))
        for _ in range(int(rng.integers(0, 16))):
            (s, sp), at = vs[int(rng.integers(0, len(vs)))], int(rng.integers(0, K))
            what = rng.random()
            if what < 0.55:
                N = int(rng.choice([1, 3, F - 1, F, F + 1, 3 * F + 7, int(rng.integers(1, 8 * F))]))
                e.move(sp, coord(), coord(), coord(), N, at_block=at)
            elif what < 0.75:
                set_position(e, sp, coord(), coord(), coord(), at_block=at)
            elif what < 0.85:
                e.move(sp, coord(), coord(), coord(), 0, at_block=at)
            elif what < 0.93:
                e.sampler_pause(s, at_block=at)
            else:
                e.sampler_play(s, at_block=at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_g10_seeded_moves_steps_pauses_and_graph_edits_on_both_plans(seed):
    F = [64, 100, 40, 256][seed % 4]
    want = fuzz(sm.Tagged(sm.MoveRefEngine(max_block_frames=F, short_blocks=True)), seed, F)
    for force_generic in (False, True):
        g = GpuEngine(max_block_frames=F, max_batch=4, force_generic=force_generic)
        got = fuzz(sm.GpuMove(g), seed, F)
        assert g.cx.plan_kind() == (0 if force_generic else 1) or F % 64 != 0
        assert_bits(got, want, "seed %d, %s" % (seed, "level executor" if force_generic else "voice bank"))
