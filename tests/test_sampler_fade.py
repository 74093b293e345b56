"""The sampler's gain envelope (fwgpu_sampler_fade, CMD_SMP_FADE = 16; SPEC): "fade out over N frames, then stop"
in ONE message — a linear envelope per voice, multiplied into the gains the render kernels already read.

The reference is tests/sampler_fade_model.py: tests/refmodel.py's SamplerNode with the envelope added (numpy f32, one separately
rounded operation after the other, the state moved frame by frame), inside a RefEngine.  Every comparison is `fwapi.bits` equality: the
arithmetic is a handful of f32 operations over exact integers, so there is no tolerance to choose.

CPU tier: the envelope's properties on random (E0, E1, N), and the functions the kernels compile (fwgpu_types.h smp_env_*, built on the
host) against the model; the model's own properties (block splits, a retarget, the reset rules); the ABI on the host-only harness; the
header, fwgpu_types.h, ffi.rs, nodes.rs and _lib.py agree; the typed mirror's three-message fade-in.

GPU tier: ONE list of fades (script) through the level executor, the fused voice bank on planar f32, planar i16, interleaved f32 and
mono sources, voices that end in a spatialiser, chain-plan voices, one-block calls, fwgpu_node_process; lazy calls around a fade; a graph
edit inside a fade; the silence flags behind a fade that stops; a seeded family.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fwapi
import sampler_fade_model as fm
from busnodes import assert_bits
from fwapi import INTERLEAVED_F32, LOOP_FULL, LOOP_NONE, LOOP_RANGE_SECS, PLANAR_F32, PLANAR_I16, GpuEngine, HostOnlyEngine
from scenarios import voice_source

INVALID = -20
F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FUZZ_SEEDS = int(os.environ.get("FWGPU_FUZZ_SEEDS", "20"))
NONE, PAUSE, STOP = fm.NONE, fm.PAUSE, fm.STOP
SR = 48000


def fbits(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


# ================================================================================================ CPU tier: the arithmetic
def _random_fades():
    rng = np.random.default_rng(2025)
    cases = [(0.0, 1.0, 1), (1.0, 0.0, 1), (0.0, 1.0, 3), (1.0, 0.0, 1 << 24), (0.25, 0.25, 100), (0.1, 0.7, 1 << 24), (1.0, float(np.nextafter(F32(1), F32(0))), 4096),
             (0.0, float(np.nextafter(F32(0), F32(1))), 77), (float(F32(1) / F32(3)), float(F32(2) / F32(3)), 3)]
    while len(cases) < 300:
        E0, E1 = (float(F32(rng.random())) for _ in range(2))
        if len(cases) % 5 == 0:
            E1 = float(np.nextafter(F32(E0), F32(rng.integers(0, 2))))          # one ulp apart: d * u rounds every which way
        N = int(rng.choice([1, 2, 3, 63, 64, 65, 100, 4097, int(rng.integers(1, 5000)), int(rng.integers(1, 1 << 24))]))
        cases.append((E0, E1, N))
    return cases


def _sample_ks(N, rng):
    if N <= 600:
        return list(range(N))
    ks = set(range(260)) | set(range(N - 260, N)) | set(int(x) for x in rng.integers(0, N, 200))
    for x in rng.integers(0, N - 70, 4):
        ks |= set(range(int(x), int(x) + 64))
    return sorted(ks)


def test_env_starts_on_e0_is_monotone_stays_inside_and_rests_on_e1():
    rng = np.random.default_rng(7)
    clamped = 0
    for E0, E1, N in _random_fades():
        E0, E1 = F32(E0), F32(E1)
        lo, hi = min(E0, E1), max(E0, E1)
        assert fwapi.bits(fm.env_value(E0, E1, N, 0, 0)) == fwapi.bits(E0), (E0, E1, N)         # env(0) of a fresh fade is E0, bit for bit
        ks = _sample_ks(N, rng)
        v = np.array([fm.env_value(E0, E1, N, k, 0) for k in ks], dtype=F32)
        assert np.all(v >= lo) and np.all(v <= hi), (E0, E1, N)
        d = np.diff(v.astype(np.float64))
        assert np.all(d >= 0) if E1 >= E0 else np.all(d <= 0), (E0, E1, N)                      # monotone (over the sampled, sorted k)
        for k in (N, N + 1, N + 1000):
            assert fwapi.bits(fm.env_value(E0, E1, N, k, 0)) == fwapi.bits(E1)                  # E1 from k = N on
        assert fwapi.bits(fm.env_value(E0, E1, N, 5, 3)) == fwapi.bits(fm.env_value(E0, E1, N, 8, 0))   # a function of k + j
        # (the clamp is there for a reason: the unclamped value can leave the range)
        if N > 1:
            k = N - 1
            raw = F32(E0 + F32(F32(E1 - E0) * F32(F32(k) / F32(N))))
            clamped += not (lo <= raw <= hi)
    assert fwapi.bits(fm.env_value(0.3, 0.8, 0, 0, 5)) == fwapi.bits(F32(0.8))                  # at rest: E1
    print("fades whose last unclamped value leaves [min, max]:", clamped)


def _peek_lib():
    """tests/host_harness/sampler_fade_peek.cpp beside the harness library: the messages a ctx keeps for nodes no plan holds yet, and
    the envelope functions of fwgpu_types.h — the ones the kernels compile — built for the host"""
    up = C.POINTER(C.c_uint)
    return fwapi.peek_lib("sampler_fade_peek", {"sfp_env_values": (None, [up, C.c_uint, up]), "sfp_env_start": (None, [up, C.c_uint, C.c_uint, C.c_int]),
                                                "sfp_env_behind_block": (None, [up, C.c_uint])})


def _st(env, playing=1, has_loop=0, playhead=0, loop_start=0):
    """an Envelope as the NodeState fields the helper takes"""
    return (C.c_uint * 8)(fbits(env.E0), fbits(env.E1), env.N | (env.then << 28), env.k, playing, has_loop, playhead, loop_start)


def test_the_kernels_own_statement_equals_the_model():
    """fwgpu_types.h smp_env_of / _value / _start / _behind_block, compiled for the host, against Envelope: values, the message (a
    retarget included), the advance, `then`, the reset — on the states a random run of messages and blocks passes through"""
    P = _peek_lib()
    rng = np.random.default_rng(99)
    then_fired = resets = 0
    for case in range(60):
        env = fm.Envelope()
        playing, playhead, has_loop, loop_start = 1, 1000, case % 2, 40
        for step in range(30):
            if rng.random() < 0.4:
                N = int(rng.choice([0, 1, 3, 64, 100, 257, 1000, 1 << 24]))
                then = int(rng.integers(0, 3)) if N else NONE
                tgt = F32(rng.choice([0.0, 1.0, 0.25, float(rng.random())]))
                st = _st(env, playing, has_loop, playhead, loop_start)
                env.start(tgt, N, then)
                P.sfp_env_start(st, fbits(tgt), N, then)
                assert list(st)[:4] == [fbits(env.E0), fbits(env.E1), env.N | (env.then << 28), env.k], (case, step)
            F = int(rng.choice([1, 37, 64, 100, 256]))
            st = _st(env, playing, has_loop, playhead, loop_start)
            got = (C.c_uint * F)()
            P.sfp_env_values(st, F, got)
            want = [fbits(env.value(j)) for j in range(F)]
            assert list(got) == want, (case, step)
            due = NONE
            for _ in range(F):
                t = env.step()
                due = t or due
            if due == PAUSE:
                playing = 0
            elif due == STOP:
                playing, playhead = 0, (loop_start if has_loop else 0)
            if not playing:
                env.reset()
            P.sfp_env_behind_block(st, F)
            assert list(st) == [fbits(env.E0) if env.N else st[0], fbits(env.E1), env.N | (env.then << 28), env.k, playing, has_loop, playhead, loop_start], (case, step)
            then_fired += due != NONE
            if not playing:
                resets += 1
                playing, playhead = 1, 1000
    assert then_fired >= 20 and resets >= 20


# ------------------------------------------------------------------------------------------------ graphs (any fwapi.Engine)
def _sample(e, seed, frames, fmt=PLANAR_F32, ch=2):
    data = voice_source(6100 + seed, frames, ch)
    if fmt == PLANAR_I16:
        return e.new_sample(fmt, ch, np.round(data * 32767).astype(np.int16))
    if fmt == INTERLEAVED_F32:
        return e.new_sample(fmt, ch, data.T.copy())
    return e.new_sample(fmt, ch, data)


def build(e, items, fmt=PLANAR_F32, ch=2, variant="bank", leaf=20):
    """one voice per item — sampler -> volume -> [pan] ("bank"), sampler -> spatialiser ("spatial") or sampler -> biquad -> delay
    ("chain", as tests/test_chain_grammar.py builds them) — under SumNodes of `leaf` ports -> graph_out; the item says which sample, which
    loop range, whether the voice plays.  Returns [(sampler, [sample A, sample B])]."""
    rng = np.random.default_rng(78)
    smps, ends = [], []
    for v, it in enumerate(items):
        s = e.sampler(it.get("pv", 80.0))
        if variant == "spatial":
            cur = e.spatial(float(rng.uniform(-4, 4)), float(rng.uniform(-1, 1)), float(rng.uniform(-4, 4)), n_in=2)
            e.connect_stereo(s, cur)
        elif variant == "chain":
            bq = e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 8000)), 0.707)
            e.connect_stereo(s, bq)
            cur = e.delay([64, 129, 300][v % 3] / float(SR), feedback=float(rng.choice([0.0, 0.45])), mix=0.5)
            e.connect_stereo(bq, cur)
        else:
            cur = e.volume(float(rng.uniform(30, 100)))
            e.connect_stereo(s, cur)
            if v % 2:
                p = e.pan(float(rng.uniform(-1, 1)))
                e.connect_stereo(cur, p)
                cur = p
        smps.append(s)
        ends.append(cur)
    mixers = []
    for i in range(0, len(items), leaf):
        m = e.sum(max(2, len(ends[i:i + leaf])))
        for p, n in enumerate(ends[i:i + leaf]):
            e.connect_stereo(n, m, 2 * p)
        mixers.append(m)
    top = mixers[0]
    if len(mixers) > 1:
        top = e.sum(len(mixers))
        for p, m in enumerate(mixers):
            e.connect_stereo(m, top, 2 * p)
    e.connect_stereo(top, e.graph_out_node)
    e.update()
    out = []
    for v, it in enumerate(items):
        a, b = _sample(e, v, it.get("len", 5000), fmt, ch), _sample(e, 500 + v, 3000, fmt, ch)
        e.sampler_set_sample(smps[v], a)
        loop = it.get("loop", (LOOP_FULL,))
        if loop[0] != LOOP_NONE:
            e.sampler_set_loop_range(smps[v], *loop)
        if it.get("playing", True):
            e.sampler_play(smps[v])
        out.append((smps[v], [a, b]))
    return out


def send(e, voice, what, args, at):
    s, samples = voice
    if what == "fade":
        e.fade(s, args[0], args[1], args[2] if len(args) > 2 else NONE, at_block=at)
    elif what == "pv":
        e.set_param(s, 0, args[0], at_block=at)
    elif what == "play":
        e.sampler_play(s, at_block=at)
    elif what == "pause":
        e.sampler_pause(s, at_block=at)
    elif what == "stop":
        e.sampler_stop(s, at_block=at)
    elif what == "seek":
        e.sampler_set_playhead_secs(s, args[0], at_block=at)
    elif what == "loop":
        e.sampler_set_loop_range(s, *args, at_block=at)
    elif what == "sample":
        e.sampler_set_sample(s, samples[args[0]], args[1], at_block=at)
    else:
        raise ValueError(what)


def _model(F, items, **kw):
    e = fm.FadeRefEngine(max_block_frames=F)
    return e, build(e, items, **kw)


# ================================================================================================ CPU tier: the model
@pytest.mark.parametrize("loop,frames,then", [((LOOP_FULL,), 549, NONE), ((LOOP_FULL,), 5000, STOP), ((LOOP_NONE,), 5000, PAUSE), ((LOOP_NONE,), 300, NONE)])
def test_model_block_splits_give_the_same_samples_and_state(loop, frames, then):
    """a fade's `then` takes effect behind the BLOCK the fade ends in, so the splits compared here all put a block boundary on the
    fade's last frame (frame 300) — and on the one-shot's end; everything in between may fall anywhere"""
    total = 448
    splits = {"one": [300, 148], "1": [1] * total, "4": [4] * 112, "100": [100, 100, 100, 148], "mixed": [64, 1, 100, 7, 128, 20, 128]}
    runs = {}
    for name, blocks in splits.items():
        assert sum(blocks) == total and 300 in np.cumsum(blocks)
        e, (vc,) = _model(512, [dict(len=frames, loop=loop)])
        e.set_param(vc[0], 0, 35.0)                    # the smoother ramps under the fade
        e.fade(vc[0], 0.125, 300, then)
        out = np.concatenate([e.process_interleaved(b) for b in blocks])
        node = e.nodes[vc[0]]
        runs[name] = (out, (node.env.state(), node.playing, node.playhead))
    for name in splits:
        assert_bits(runs[name][0], runs["one"][0], name)
        assert runs[name][1] == runs["one"][1], name
    env, playing, _ = runs["one"][1]
    assert env[1:] == (0, 0, NONE) and playing == (then == NONE and frames != 300)
    assert env[0][1] == (fbits(0.125) if playing else fbits(1.0))          # at rest at E1 while it plays on; a transient otherwise
    assert np.any(runs["one"][0] != 0)


def test_model_a_retarget_continues_from_where_the_fade_stands():
    e, (vc,) = _model(64, [dict()])
    n = e.nodes[vc[0]]
    e.fade(vc[0], 0.0, 640)
    e.process_blocks(3)
    mid = n.env.value(0)
    assert n.env.k == 192 and 0.0 < mid < 1.0 and fwapi.bits(mid) == fwapi.bits(fm.env_value(1.0, 0.0, 640, 192, 0))
    e.fade(vc[0], 1.0, 100, PAUSE)
    e.process_blocks(1)                             # (the message applies at the block's first frame)
    assert fwapi.bits(n.env.E0) == fwapi.bits(mid) and (n.env.E1, n.env.N, n.env.k, n.env.then) == (1.0, 100, 64, PAUSE)
    e.fade(vc[0], 0.5, 0)                           # a step: at rest at the target, then = NONE
    e.process_blocks(1)
    assert n.env.state() == ([n.env.state()[0][0], fbits(0.5)], 0, 0, NONE) and n.playing
    e.fade(vc[0], -0.0, 0)
    e.process_blocks(1)
    assert fbits(n.env.E1) == 0                     # -0.0 counts as +0.0


def test_model_the_envelope_is_a_transient():
    """pause, stop, set_sample with stop and a one-shot's end put it back to rest at 1.0, then = NONE; play, a seek, a loop range, the
    volume and set_sample without stop leave it alone; a paused voice's envelope does not move"""
    REST1 = ([0, fbits(1.0)], 0, 0, NONE)

    def fresh(**item):
        e, (vc,) = _model(64, [dict(**item)])
        e.fade(vc[0], 0.25, 640, STOP)
        e.process_blocks(2)
        n = e.nodes[vc[0]]
        assert (n.env.N, n.env.k, n.env.then) == (640, 128, STOP)
        return e, vc, n

    for what, args in (("pause", ()), ("stop", ()), ("sample", (1, True))):
        e, vc, n = fresh()
        send(e, vc, what, args, 0)
        e.process_blocks(1)
        assert n.env.state()[1:] == REST1[1:] and n.env.E1 == 1.0 and not n.playing, what
        e.sampler_play(vc[0])
        want = e.process_blocks(1)
        assert n.env.at_rest() and np.any(want != 0)
    for what, args in (("play", ()), ("seek", (0.01,)), ("loop", (LOOP_RANGE_SECS, 0.001, 0.01)), ("pv", (40.0,)), ("sample", (1, False))):
        e, vc, n = fresh()
        send(e, vc, what, args, 0)
        e.process_blocks(1)
        assert (n.env.N, n.env.k, n.env.then) == (640, 192, STOP) and n.playing, what
    # a one-shot that ends inside the fade (sampler.rs:499-513), and one found past its end (:486-497)
    e, vc, n = fresh(len=64 * 3 + 10, loop=(LOOP_NONE,))
    e.process_blocks(2)
    assert not n.playing and n.env.state()[1:] == REST1[1:] and n.env.E1 == 1.0
    e, vc, n = fresh(len=5000, loop=(LOOP_NONE,))
    e.sampler_set_playhead_secs(vc[0], 6000.0 / SR)
    e.process_blocks(1)
    assert not n.playing and n.env.at_rest() and n.env.E1 == 1.0
    # paused: nothing moves; the fade goes on when the voice plays again only if it was sent while paused
    e, (vc,) = _model(64, [dict(playing=False)])
    n = e.nodes[vc[0]]
    e.fade(vc[0], 0.0, 0)
    e.fade(vc[0], 1.0, 200)
    e.process_blocks(3)
    assert (n.env.N, n.env.k) == (200, 0) and n.env.E0 == 0.0
    e.sampler_play(vc[0])
    out = e.process_blocks(4)
    assert n.env.state() == ([0, fbits(1.0)], 0, 0, NONE) and out[0] == 0.0 and np.any(out != 0)


def test_model_a_muted_voice_holds_its_playhead_while_the_envelope_runs_on_and_then_still_fires():
    """the reference's mute test (sampler.rs:437) needs an INACTIVE smoother below 1e-5.  A smoother that has glided to 0 stays
    Deactivating for good (smoother.rs:159-194: nothing but reset() takes it to Inactive, and the sampler never resets its own), so the
    early-out is met by a voice CREATED at volume 0 — a volume of 0 sent later renders x * 0 through the ordinary path"""
    e, (vc,) = _model(64, [dict(pv=0.0, loop=(LOOP_RANGE_SECS, 100.0 / SR, 900.0 / SR))])
    n = e.nodes[vc[0]]
    e.process_blocks(2)
    assert n.playing and n.playhead == 0            # muted: the playhead has not moved
    e.fade(vc[0], 0.0, 64 * 4 + 1, STOP)
    for b in range(4):
        e.process_blocks(1)
        assert n.playing and n.playhead == 0 and n.env.k == 64 * (b + 1)        # ... and does not, while the envelope runs on
    e.process_blocks(1)
    assert not n.playing and n.playhead == 100 and n.env.state()[1:] == (0, 0, NONE) and n.env.E1 == 1.0    # `then` fired: the loop start
    e.set_param(vc[0], 0, 70.0)
    e.sampler_play(vc[0])
    assert np.any(e.process_blocks(1) != 0)
    # a volume of 0 sent in mid-fade: Deactivating, never muted — the playhead moves on
    e, (vc,) = _model(64, [dict()])
    n = e.nodes[vc[0]]
    e.fade(vc[0], 0.5, 64 * 200)
    e.set_param(vc[0], 0, 0.0)
    e.process_blocks(150)
    assert n.gain_smoother.is_active() and n.gain_smoother.last_output == 0.0 and n.playhead == (150 * 64) % 5000 and n.env.k == 150 * 64


# ================================================================================================ CPU tier: the ABI on the harness
def _early(P, c):
    """[(type, block, i0, f0 bits, i1)] of the messages waiting for their node's first plan"""
    return [(w[0], w[1], w[3], w[2], w[4]) for w in fwapi.early_msgs(P, c)]


def test_abi_what_a_call_queues():
    """one Cmd per call: CMD_SMP_FADE with the target in f0, frames in i0, `then` in i1.  Read where the ABI keeps the messages of a node
    that no plan holds yet."""
    P = _peek_lib()
    e = HostOnlyEngine(sample_rate=44100, max_block_frames=96, num_graph_inputs=3, num_graph_outputs=2)
    L, c = e.cx.L, e.cx.c
    assert P.fwp_layout_check(c, 44100, 96, 3, 2, 0) == 0
    assert P.fwp_layout_check(c, 44100, 64, 3, 2, 0) == 2 and P.fwp_layout_check(c, 48000, 96, 2, 2, 0) == 5      # (and it does look)
    s = e.sampler(100.0)
    assert _early(P, c) == []
    assert L.fwgpu_sampler_fade(c, s, 0.0, fm.FRAMES_MAX, STOP, 0) == 0            # the longest fade
    assert L.fwgpu_sampler_fade(c, s, 1.0, 1, PAUSE, 3) == 0
    assert L.fwgpu_sampler_fade(c, s, 0.37, 0, NONE, 2) == 0                       # a step
    assert L.fwgpu_sampler_fade(c, s, -0.0, 5, NONE, 1) == 0                       # -0.0 counts as +0.0
    assert L.fwgpu_sampler_fade(c, s, float("nan"), 10, NONE, 0) == INVALID        # a refused call queues nothing
    assert L.fwgpu_sampler_fade(c, s, 0.5, 0, STOP, 0) == INVALID
    got = _early(P, c)
    assert got == [(fm.CMD_SMP_FADE, 0, fm.FRAMES_MAX, fbits(0.0), STOP), (fm.CMD_SMP_FADE, 3, 1, fbits(1.0), PAUSE),
                   (fm.CMD_SMP_FADE, 2, 0, fbits(0.37), NONE), (fm.CMD_SMP_FADE, 1, 5, 0, NONE)], got
    e.connect_stereo(s, e.graph_out_node)
    e.update()                                                                     # the plan that activates the node releases them
    assert _early(P, c) == []
    e.process_blocks(4)
    assert e.violation() == ""


def _harness_bank(n=3):
    e = HostOnlyEngine(max_block_frames=64, max_batch=4)
    return e, build(e, [dict(len=900)] * n)


def test_abi_refusals_and_a_good_call_reaches_the_control_kernel():
    e, voices = _harness_bank()
    L, c = e.cx.L, e.cx.c
    assert e.cx.plan_kind() == 1
    seen = fwapi.hostonly_lib().fwh_cmds_seen           # messages the control kernel's launches would apply
    seen.restype = C.c_ulonglong
    s0 = voices[0][0]
    vol = e.volume(50.0)
    rs = e.resampler(voices[0][1][0], 1.0, loop=True, n_out=2)
    tiny = float(np.nextafter(F32(0), F32(-1)))
    for bad, word in ((lambda: L.fwgpu_sampler_fade(c, vol, 1.0, 10, NONE, 0), "not a SamplerNode"),
                      (lambda: L.fwgpu_sampler_fade(c, rs, 1.0, 10, NONE, 0), "not a SamplerNode"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, float("nan"), 10, NONE, 0), "0..1"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, float("inf"), 10, NONE, 0), "0..1"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, float("-inf"), 10, NONE, 0), "0..1"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, float(np.nextafter(F32(1), F32(2))), 10, NONE, 0), "0..1"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, tiny, 10, NONE, 0), "0..1"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, 0.5, fm.FRAMES_MAX + 1, NONE, 0), "2^24"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, 0.5, 10, 3, 0), "then"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, 0.5, 10, -1, 0), "then"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, 0.5, 0, PAUSE, 0), "no end"),
                      (lambda: L.fwgpu_sampler_fade(c, s0, 0.5, 0, STOP, 0), "no end"),
                      (lambda: L.fwgpu_sampler_fade(c, 1 << 40, 0.5, 10, NONE, 0), "unknown node")):
        assert bad() == INVALID
        assert word in L.fwgpu_last_error(c).decode(), (word, L.fwgpu_last_error(c).decode())
    assert L.fwgpu_sampler_fade(None, s0, 1.0, 10, NONE, 0) == INVALID
    e.process_blocks(2)
    n0 = seen()
    assert L.fwgpu_sampler_fade(c, s0, 0.0, fm.FRAMES_MAX, STOP, 0) == 0
    assert L.fwgpu_sampler_fade(c, voices[1][0], 1.0, 1, PAUSE, 1) == 0
    assert L.fwgpu_sampler_fade(c, voices[1][0], -0.0, 5, NONE, 1) == 0
    assert L.fwgpu_sampler_fade(c, voices[2][0], 0.5, 0, NONE, 0) == 0
    e.process_blocks(2)
    assert seen() == n0 + 4                              # the refused calls above queued nothing
    e.process_blocks(1)
    assert seen() == n0 + 4 and e.violation() == ""


def test_abi_the_sampler_message_ring_fills_as_for_the_other_sampler_messages():
    e, voices = _harness_bank(1)
    L, c = e.cx.L, e.cx.c
    s = voices[0][0]
    e.process_blocks(1)
    rcs = [L.fwgpu_sampler_fade(c, s, 0.5, 10, NONE, 0) for _ in range(129)]
    assert rcs[:128] == [0] * 128 and rcs[128] == -21 and L.fwgpu_sampler_stop(c, s, 0) == -21       # FWGPU_ERR_QUEUE_FULL, shared
    e.process_blocks(1)
    assert L.fwgpu_sampler_fade(c, s, 0.5, 10, NONE, 0) == 0 and e.violation() == ""


def test_abi_a_fade_for_a_node_no_plan_holds_yet_waits_for_the_update():
    e = HostOnlyEngine(max_block_frames=64)
    s = e.sampler(100.0)
    assert e.cx.L.fwgpu_sampler_fade(e.cx.c, s, 0.5, 100, PAUSE, 0) == 0
    e.connect_stereo(s, e.graph_out_node)
    e.update()
    e.process_blocks(1)
    assert e.violation() == ""


def test_typed_mirror_fade_in_queues_its_three_messages_in_order():
    import firewheel_amd as fa

    P = _peek_lib()
    cx = fwapi.hostonly_ctx(max_block_frames=64)
    assert P.fwp_layout_check(cx.c, 48000, 64, 0, 2, 0) == 0
    node = fa.SamplerNode(100.0)
    nid = cx.add_node(0, 2, node)
    node.fade_in(480, at_block=2)                       # before the first update: the three wait, in order
    assert _early(P, cx.c) == [(fm.CMD_SMP_FADE, 2, 0, 0, NONE), (11, 2, 0, 0, 0), (fm.CMD_SMP_FADE, 2, 480, fbits(1.0), NONE)]
    assert node.is_playing()
    node.fade_out(300)
    assert _early(P, cx.c)[3] == (fm.CMD_SMP_FADE, 0, 300, 0, STOP) and not node.is_playing()
    node.fade_to(0.25, 100, "pause", at_block=1)
    node.fade_to_secs(0.5, 0.01)
    assert _early(P, cx.c)[4:] == [(fm.CMD_SMP_FADE, 1, 100, fbits(0.25), PAUSE), (fm.CMD_SMP_FADE, 0, 480, fbits(0.5), NONE)]
    cx.connect(nid, 0, cx.graph_out_node(), 0)
    cx.update()
    assert _early(P, cx.c) == [] and fa.SamplerNode.FADE_FRAMES_MAX == fm.FRAMES_MAX
    for bad in (lambda: node.fade_to(float("nan"), 10), lambda: node.fade_to(1.5, 10), lambda: node.fade_to(0.5, fm.FRAMES_MAX + 1),
                lambda: node.fade_to(0.5, 0, "stop")):
        with pytest.raises(fa.FwgpuError) as ei:
            bad()
        assert ei.value.code == INVALID
    with pytest.raises(ValueError):
        node.fade_to(0.5, 10, "halt")


def test_header_types_ffi_and_lib_agree():
    import firewheel_amd._lib as flib

    rd = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr, types = rd("include", "fwgpu.h"), rd("firewheel_amd", "csrc", "fwgpu_types.h")
    ffi, nodes = rd("rust", "firewheel-gpu", "src", "ffi.rs"), rd("rust", "firewheel-gpu", "src", "nodes.rs")
    assert re.search(r"#define FWGPU_SAMPLER_FADE_FRAMES_MAX 16777216\b", hdr)
    assert "enum fwgpu_fade_then { FWGPU_FADE_NONE = 0, FWGPU_FADE_PAUSE = 1, FWGPU_FADE_STOP = 2 };" in hdr
    assert "int fwgpu_sampler_fade(fwgpu_ctx* ctx, int64_t node, float target, uint32_t frames, int then, uint32_t at_block);" in hdr
    assert re.search(r"CMD_SMP_FADE = 16\b", types) and re.search(r"#define SMP_FADE_FRAMES_MAX 16777216u", types)
    for name, val in (("NONE", 0), ("PAUSE", 1), ("STOP", 2)):
        assert re.search(r"#define SMP_FADE_%s %d\b" % (name, val), types)
        assert "pub const FWGPU_FADE_%s: c_int = %d;" % (name, val) in ffi
    assert re.search(r"K_LAST = K_CROSSFADE\b", types)           # no new node kind
    assert "static_assert(sizeof(NodeState) == 128" in types
    assert "pub const FWGPU_SAMPLER_FADE_FRAMES_MAX: u32 = 16777216;" in ffi
    assert "pub fn fwgpu_sampler_fade(ctx: *mut fwgpu_ctx, node: i64, target: f32, frames: u32, then: c_int, at_block: u32) -> c_int;" in ffi
    assert "pub fn fade_to" in nodes and "ffi::fwgpu_sampler_fade" in nodes
    res, args = flib.SIGNATURES["fwgpu_sampler_fade"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_float, C.c_uint32, C.c_int, C.c_uint32]
    assert (fm.CMD_SMP_FADE, fm.FRAMES_MAX, fm.NONE, fm.PAUSE, fm.STOP) == (16, 1 << 24, 0, 1, 2)


# ================================================================================================ GPU tier: the list of fades
N_CALLS = 5      # call 0 and call 4 carry no message


def _at(K, call, where, plus=0):
    """(call, at_block) of block `where` ('first' / 'mid' / 'last') of `call`, `plus` blocks further on"""
    g = call * K + {"first": 0, "mid": K // 2, "last": K - 1}[where] + plus
    return g // K, g % K


def script(F, K):
    """per item: the voice (sample frames, loop range, playing, percent volume) and its messages [(call, at_block, what, args)] —
    voice v of a bank plays item v % len.  Messages fall into calls 1 to 3."""
    A = lambda where, plus=0, call=1: _at(K, call, where, plus)
    M = lambda pos, what, *args: pos + (what, args)
    span3 = (K - K // 2) * F + K * F + F // 2                # from the middle of call 1 to inside call 3
    rng_loop = (LOOP_RANGE_SECS, 100.0 / SR, 900.0 / SR)
    return [
        dict(msgs=[M(A("mid"), "fade", 0.0, F + 1, PAUSE), M(A("first", call=3), "play")]),
        dict(msgs=[M(A("first"), "fade", 0.5, 1)]),
        dict(msgs=[M(A("last"), "fade", 0.0, 3, STOP), M(A("mid", call=3), "play")]),
        # a voice muted from its creation (the one way to an Inactive smoother below 1e-5: see the model's test): the mute early-out holds
        # the playhead while the envelope runs on, and `then` still fires — the voice is heard from its loop start
        dict(pv=0.0, loop=rng_loop, msgs=[M(A("first"), "fade", 0.0, 3 * F + 1, STOP), M(A("first", call=3), "pv", 70.0), M(A("first", call=3), "play")]),
        dict(msgs=[M(A("first"), "fade", 0.0, 5 * F + 7, STOP)]),
        dict(msgs=[M(A("mid"), "fade", 0.1, span3)]),                                                   # spans three calls
        dict(msgs=[M(A("first"), "fade", 0.25, 6 * F), M(A("first", 2), "fade", 1.0, 3 * F + 5)]),      # a retarget two blocks on
        dict(playing=False, msgs=[M(A("mid"), "fade", 0.0, 0), M(A("mid"), "play"), M(A("mid"), "fade", 1.0, 4 * F + 3)]),   # the fade-in triple
        dict(msgs=[M(A("last"), "fade", 0.3, F - 1)]),
        dict(msgs=[M(A("first"), "fade", 0.3, F)]),
        dict(msgs=[M(A("mid"), "fade", 0.2, 3 * F), M(A("mid"), "fade", 0.9, 2 * F + 1, PAUSE)]),       # two fades for one block
        dict(msgs=[M(A("first"), "pv", 30.0), M(A("first"), "fade", 0.4, 5 * F)]),                      # ramp times envelope
        dict(msgs=[M(A("first"), "fade", 0.1, 8 * F), M(A("first", 2), "pv", 55.0)]),                   # ... in mid-fade
        dict(msgs=[M(A("first"), "fade", 0.2, 6 * F), M(A("first", 1), "pause"), M(A("first", 2), "play")]),     # full gain afterwards
        dict(msgs=[M(A("first"), "fade", 0.2, 6 * F), M(A("first", 2), "stop"), M(A("first", call=3), "play")]),
        # a loop that wraps inside the fade, in nearly every block at another frame: 37 frames longer than a block (a sampler's loop
        # SHORTER than a block wraps more than once per block, which the reference does not survive: DESIGN.md Q8 — 37 frames as such
        # are the resampler's case)
        dict(len=F + 37, msgs=[M(A("first"), "fade", 0.3, 5 * F + 7)]),
        dict(loop=(LOOP_NONE,), msgs=[M(A("first"), "seek", (5000 - 2 * F - 5) / float(SR)), M(A("first"), "fade", 0.2, 8 * F),
                                      M(A("first", call=3), "play")]),                                  # a one-shot ends inside the fade
        dict(loop=rng_loop, msgs=[M(A("mid"), "fade", 0.0, 2 * F + 9, STOP), M(A("mid", call=3), "play")]),      # back to the loop start
        dict(msgs=[M(A("first"), "fade", 0.3, 6 * F), M(A("first", 2), "sample", 1, False)]),           # set_sample without stop in mid-fade
        dict(msgs=[M(A("first"), "fade", 0.25, 2 * F + 3)]),                                            # rests at 0.25 through the last call
        dict(msgs=[M(A("first"), "fade", 0.1, 8 * F, STOP), M(A("first", 1), "pv", 0.0)]),              # a volume of 0 in mid-fade
    ]


def run_script(e, F, K, n_voices, n_calls=N_CALLS, warm=0, ready=None, **kw):
    items = script(F, K)
    pick = [items[v % len(items)] for v in range(n_voices)]
    voices = build(e, pick, **kw)
    outs = [np.asarray(e.process_blocks(1)) for _ in range(warm)]
    if ready:
        ready()
    for call in range(n_calls):
        for v, p in enumerate(pick):
            for c, at, what, args in p["msgs"]:
                if c == call:
                    send(e, voices[v], what, args, at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


_refs = {}


def reference(F, K, n_voices, n_calls=N_CALLS, **kw):
    key = (F, K, n_voices, n_calls, tuple(sorted(kw.items())))
    if key not in _refs:
        out = run_script(fm.Tagged(fm.FadeRefEngine(max_block_frames=F)), F, K, n_voices, n_calls, **kw)
        out.setflags(write=False)
        assert np.any(out != 0)
        _refs[key] = out
    return _refs[key]


COMBOS = [(64, 70, 8), (100, 3, 40), (256, 3, 20), (512, 1, 18), (64, 1, 1)]      # F, K, voices
SMALL = [(100, 3, 18), (256, 1, 18)]


def test_the_script_sends_no_message_in_its_first_and_last_call_and_the_model_meets_what_it_is_for():
    for F, K, _ in COMBOS + SMALL:
        for it in script(F, K):
            assert it["msgs"] and all(1 <= c <= 3 and 0 <= at < K for c, at, _, _ in it["msgs"]), (F, K, it)
    # the muted voice's `then` fires while it is muted
    F, K = 64, 3
    e = fm.Tagged(fm.FadeRefEngine(max_block_frames=F))
    items = script(F, K)
    voices = build(e, items)
    node = e.e.nodes[voices[3][0]]
    e.process_blocks(K)
    for c, at, what, args in items[3]["msgs"]:
        if c == 1:
            send(e, voices[3], what, args, at)
    e.process_blocks(K)
    assert node.playing and node.playhead == 0 and node.env.k == 3 * F
    e.process_blocks(K)
    assert not node.playing and node.playhead == 100 and node.env.E1 == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g1_level_executor(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K, force_generic=True)
    got = run_script(fm.GpuFade(g), F, K, V)
    assert g.cx.plan_kind() == 0
    assert_bits(got, reference(F, K, V), "level executor")


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g2_fused_voice_bank_planar_f32(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(fm.GpuFade(g), F, K, V)
    assert g.cx.plan_kind() == 1 and g.cx.plan_fused_voices() == V
    assert_bits(got, reference(F, K, V), "voice bank, planar f32")


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", SMALL)
@pytest.mark.parametrize("fmt,ch", [(PLANAR_I16, 2), (INTERLEAVED_F32, 2), (PLANAR_F32, 1), (PLANAR_I16, 1)])
def test_g3_other_formats_and_mono_sources(fmt, ch, F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(fm.GpuFade(g), F, K, V, fmt=fmt, ch=ch)
    assert g.cx.plan_kind() == 1
    assert_bits(got, reference(F, K, V, fmt=fmt, ch=ch), "format %d, %d channel(s)" % (fmt, ch))


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", [(64, 3, 20), (256, 1, 18)])
def test_g4_voices_that_end_in_a_spatialiser(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(fm.GpuFade(g), F, K, V, variant="spatial")
    assert g.cx.plan_kind() == 1
    assert_bits(got, reference(F, K, V, variant="spatial"), "sampler -> spatialiser")


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", [(64, 3, 20), (64, 70, 8), (256, 1, 18)])
def test_g5_chain_plan_voices(F, K, V):
    """sampler -> biquad -> delay: a fade whose `then` is STOP clears the source, and the filter tails ring on"""
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(fm.GpuFade(g), F, K, V, variant="chain")
    assert g.cx.plan_kind() == 2
    assert_bits(got, reference(F, K, V, variant="chain"), "chain plan")


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 256])
def test_g6_one_block_calls(F):
    """40 voices under two leaves and a root: the tree the one-launch edge takes.  One block sets the voices up; of the 12 calls
    counted, calls 1, 2 and 3 carry messages (the launch sequence: include/fwgpu.h fwgpu_rt_path_stats); the others — fades in flight
    among them — are one launch or a doorbell."""
    V, K, calls = 40, 1, 12
    g = GpuEngine(max_block_frames=F)
    before = []
    got = run_script(fm.GpuFade(g), F, K, V, n_calls=calls, warm=1, ready=lambda: before.append(g.cx.rt_path_stats()))
    delta = tuple(a - b for a, b in zip(g.cx.rt_path_stats(), before[0]))
    print("one-block launch batches by path (resident, one launch, fused sequence, level executor):", delta)
    assert g.cx.plan_kind() == 1
    assert_bits(got, reference(F, K, V, n_calls=calls, warm=1), "one-block calls")
    assert sum(delta) == calls and delta[3] == 0 and delta[2] <= 3 and delta[0] + delta[1] >= calls - 3, delta


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 100, 256])
def test_g7_node_process_every_item_of_the_script(F):
    """fwgpu_node_process (k_single_node, an instantiation of its own with its own apply_cmds_from): EVERY item of script(), one node
    per item, one block per call, the item's messages sent between the calls exactly as run_script sends them at K = 1 — samples
    and out mask of every block against FadeSamplerNode.process."""
    K, calls = 1, 12
    items = script(F, K)
    g = GpuEngine(max_block_frames=F)
    e = fm.FadeRefEngine(max_block_frames=F)
    gg = fm.GpuFade(g)
    gv, mv = build(gg, items), build(e, items)
    masks, fading, thens = set(), 0, 0
    for call in range(calls):
        for v, p in enumerate(items):
            node = e.nodes[mv[v][0]]
            for c, at, what, args in p["msgs"]:
                assert at == 0
                if c == call:
                    send(gg, gv[v], what, args, 0)
                    send(e, mv[v], what, args, 0)
            y, om = g.node_process(gv[v][0], F, [], 2)
            outs = [np.full(F, np.nan, dtype=F32), np.full(F, np.nan, dtype=F32)]
            then_before = node.env.then if node.playing else NONE
            was_playing = node.playing or any(m[0] == "play" for m in node.msgs)
            wm = node.process(F, [], outs, 0)
            assert om == wm, (v, call, om, wm)
            assert_bits(y, np.stack(outs), "item %d, call %d" % (v, call))
            masks.add(wm)
            fading += not node.env.at_rest() and node.playing
            thens += bool(then_before) and was_playing and not node.playing
    assert fading >= 25 and masks == {0, 3} and thens >= 3, (fading, masks, thens)


# ------------------------------------------------------------------------------------------------ lazy calls around a fade
@pytest.mark.gpu
def test_g8_a_call_inside_a_fade_runs_the_control_kernel_and_lazy_calls_resume_behind_it():
    F, K, V = 64, 4, 12
    items = [dict(len=5120)] * V                           # a loop of 80 whole blocks: lazy-capable

    def run(e):
        voices = build(e, items)
        outs, marks = [], []
        for call in range(12):
            if call == 4:
                e.fade(voices[0][0], 0.25, 9 * F + 3, at_block=1)       # through calls 4, 5 and into call 6; rests at 0.25 from there on
                e.fade(voices[5][0], 1.0, 9 * F + 3, at_block=1)        # 1.0 -> 1.0: in flight all the same; rests at 1.0
                e.fade(voices[11][0], 0.6, 3 * F, at_block=1)
            outs.append(np.asarray(e.process_blocks(K)))
            if hasattr(e, "cx"):
                marks.append(e.cx.lazy_stats())
        return np.concatenate(outs), marks

    m = fm.Tagged(fm.FadeRefEngine(max_block_frames=F))
    want, _ = run(m)
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got, marks = run(fm.GpuFade(g))
    assert g.cx.plan_kind() == 1
    assert_bits(got, want, "twelve calls")
    if os.environ.get("FWGPU_LAZY") == "0":
        return
    lazy, ctl = [m[0] for m in marks], [m[1] for m in marks]
    assert lazy[3] > lazy[1], marks                     # quiet calls in front of the fade are lazy
    assert lazy[6] == lazy[3] and ctl[6] - ctl[3] == 3, marks     # calls 4, 5, 6: a fade in flight (or ending): the control kernel, no lazy batch
    assert lazy[11] - lazy[7] == 4, marks               # ... and lazy again behind it — at rest at 0.25, 0.6 and 1.0 —, bit-exact (above)


# ------------------------------------------------------------------------------------------------ a graph edit inside a fade
@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g9_the_envelope_carries_over_a_plan_install(force_generic):
    F, K, V = 64, 3, 6

    def run(e):
        voices = build(e, [dict()] * V, leaf=8)
        outs = [np.asarray(e.process_blocks(K))]
        e.fade(voices[0][0], 0.0, 8 * F + 9, STOP, at_block=1)
        e.fade(voices[1][0], 0.3, 8 * F + 9, at_block=2)
        e.fade(voices[2][0], 0.5, F, at_block=0)                 # at rest at 0.5 when the plan changes
        outs.append(np.asarray(e.process_blocks(K)))
        # a voice is added to the mixer's free port between two calls of the fades
        extra = e.sampler(90.0)
        vol = e.volume(60.0)
        e.connect_stereo(extra, vol)
        e.connect_stereo(vol, e.the_mixer, 2 * V)
        e.update()
        e.sampler_set_sample(extra, _sample(e, 50, 900))
        e.sampler_set_loop_range(extra, LOOP_FULL)
        e.sampler_play(extra)
        for _ in range(3):
            outs.append(np.asarray(e.process_blocks(K)))
        return np.concatenate(outs)

    class Eng(object):          # (build() makes the mixer; keep its id and give it one port more)
        def __init__(self, e):
            self._e = e

        def __getattr__(self, name):
            return getattr(self._e, name)

        def sum(self, ports, ch=2):
            self.the_mixer = self._e.sum(ports + 1, ch)
            return self.the_mixer

        def connect_stereo(self, src, dst, dst_port0=0, src_port0=0):
            return fwapi.Engine.connect_stereo(self, src, dst, dst_port0, src_port0)

    want = run(Eng(fm.Tagged(fm.FadeRefEngine(max_block_frames=F))))
    g = GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)
    got = run(Eng(fm.GpuFade(g)))
    assert g.cx.plan_kind() == (0 if force_generic else 1)
    assert_bits(got, want, "a plan install between two calls of a fade")


# ------------------------------------------------------------------------------------------------ silence flags behind a fade
@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
@pytest.mark.parametrize("then", [STOP, NONE])
def test_g10_behind_a_fade_that_stops_the_output_is_flagged_silent_from_the_next_block(then, force_generic):
    F, K = 64, 6

    def run(e):
        (vc,) = build(e, [dict()])
        e.fade(vc[0], 0.0, 3 * F + 5, then, at_block=1)         # ends inside block 4 of the first call
        a, fa = e.process_blocks_flags(K)
        b, fb = e.process_blocks_flags(K)
        return np.concatenate([np.asarray(a), np.asarray(b)]), np.concatenate([np.asarray(fa, dtype=bool), np.asarray(fb, dtype=bool)])

    want, wf = run(fm.Tagged(fm.FadeRefEngine(max_block_frames=F)))
    got, gf = run(fm.GpuFade(GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)))
    if then == STOP:
        assert not wf[:5].any() and wf[5:].all()            # the block the fade ended in was rendered whole; flagged from the next one
    else:
        assert not wf.any()                                 # no envelope-driven silence: a voice that rests at 0 renders zeros
    assert np.all(want[2 * 5 * F:] == 0) and np.any(want[:2 * 4 * F] != 0)
    assert np.array_equal(gf, wf), (gf.T, wf.T)
    assert_bits(got, want, "flags")


# ------------------------------------------------------------------------------------------------ the seeded family
def fuzz(e, seed, F):
    rng = np.random.default_rng(41_000 + seed)
    V = 40
    items = []
    for _ in range(V):
        ln = int(rng.choice([F + 37, 700, 5000]))       # (every loop at least a block long: one wrap per block)
        loop = (LOOP_FULL,) if rng.random() < 0.6 else ((LOOP_NONE,) if rng.random() < 0.5 or ln < 700 else (LOOP_RANGE_SECS, 64.0 / SR, 640.0 / SR))
        items.append(dict(len=ln, loop=loop, playing=bool(rng.random() < 0.8), pv=float(rng.choice([100.0, 60.0, 0.0]))))
    voices = build(e, items)
    outs = []
    for call in range(5):
        K = int(rng.integers(1, 5))
        n_msgs = int(rng.integers(0, 30))
        ats = sorted(int(rng.integers(0, K)) for _ in range(n_msgs))     # (a node's messages go out in non-decreasing block order)
        for at in ats:
            vc = voices[int(rng.integers(0, V))]
            what = rng.random()
            if what < 0.5:
                N = int(rng.choice([0, 1, 3, F - 1, F, F + 1, 3 * F + 7, int(rng.integers(1, 8 * F))]))
                then = int(rng.integers(0, 3)) if N else NONE
                send(e, vc, "fade", (float(rng.choice([0.0, 1.0, 0.25, 0.5, float(F32(rng.random()))])), N, then), at)
            elif what < 0.62:
                send(e, vc, "pv", (float(rng.choice([0.0, 35.0, 100.0])),), at)
            elif what < 0.74:
                send(e, vc, "play", (), at)
            elif what < 0.8:
                send(e, vc, "pause", (), at)
            elif what < 0.86:
                send(e, vc, "stop", (), at)
            elif what < 0.91:
                send(e, vc, "seek", (float(rng.integers(0, 30)) / SR,), at)
            elif what < 0.96:
                send(e, vc, "loop", [(LOOP_NONE,), (LOOP_FULL,)][int(rng.integers(0, 2))], at)
            else:
                send(e, vc, "sample", (int(rng.integers(0, 2)), bool(rng.random() < 0.5)), at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_g11_seeded_fades_volumes_and_transport_on_both_plans(seed):
    F = [64, 100, 256][seed % 3]
    want = fuzz(fm.Tagged(fm.FadeRefEngine(max_block_frames=F)), seed, F)
    for force_generic in (False, True):
        g = GpuEngine(max_block_frames=F, max_batch=4, force_generic=force_generic)
        got = fuzz(fm.GpuFade(g), seed, F)
        assert g.cx.plan_kind() == (0 if force_generic else 1)
        assert_bits(got, want, "seed %d, %s" % (seed, "level executor" if force_generic else "voice bank"))
