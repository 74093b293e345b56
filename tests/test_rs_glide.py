"""The resampler's ratio glide (fwgpu_resampler_glide, CMD_RS_GLIDE = 24; SPEC): the pitch of a resampling source
moved every frame by ONE message — the 32.32 position a quadratic in the frame index, in integers.

The reference is tests/rs_glide_model.py: tests/refmodel.py's ResamplerNode with the glide added (Python integers, the state moved
frame by frame, `fma32` for the taps), inside a RefEngine.  Every comparison is `fwapi.bits` equality: the arithmetic is integers plus
the resampler's own fmaf chain, so there is no tolerance to choose.

CPU tier: the closed form against the iteration; the model's own properties (block splits, the state behind a glide); the ABI on the
host-only harness; the header, fwgpu_types.h, ffi.rs, nodes.rs and _lib.py agree; doppler_ratio.

GPU tier: ONE list of glides (SCRIPT) through the level executor, the fused voice bank on planar f32 (steady blocks on the window
path, glide blocks frame by frame), on planar i16 and interleaved f32, mono sources, voices that end in a spatialiser, one-block calls,
fwgpu_node_process; lazy calls around a glide; a graph edit inside a glide; silence flags behind a one-shot; a seeded family.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fwapi
import rs_glide_model as gm
from busnodes import assert_bits
from fwapi import INTERLEAVED_F32, PLANAR_F32, PLANAR_I16, GpuEngine, HostOnlyEngine
from refmodel import resampler_step
from scenarios import voice_source

INVALID = -20
F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FUZZ_SEEDS = int(os.environ.get("FWGPU_FUZZ_SEEDS", "20"))
LO, HI = 1 << 24, 1 << 40          # resampler_step's range: ratios 1/256 and 256


# ================================================================================================ CPU tier: the arithmetic
def _random_glides():
    rng = np.random.default_rng(2024)
    cases = [(LO, HI, 1, 0), (HI, LO, 1, 12345), (LO, LO + 5, 100, (1 << 64) - 7), (HI, HI - 1000, 4096, 99), (1 << 32, 1 << 32, 50, 1)]
    while len(cases) < 200:
        S, S1 = (int(rng.integers(LO, HI + 1)) for _ in range(2))
        kind = len(cases) % 4
        if kind == 0:                      # |S1 - S| < N: inc == 0
            N = int(rng.integers(2, 3000))
            S1 = min(max(S + int(rng.integers(-N + 1, N)), LO), HI)
        elif kind == 1:
            N = 1
        else:
            N = int(rng.integers(1, 3000))
        cases.append((S, S1, N, int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))))
    return cases


def test_closed_form_equals_the_iteration_and_ends_exactly_on_the_target():
    zero_inc = one_frame = 0
    for S, S1, N, pos in _random_glides():
        inc, left, target = gm.glide_start(S, S1, N)
        assert inc == (abs(S1 - S) // N) * (1 if S1 >= S else -1) and target == S1 and left == N
        zero_inc += inc == 0 and S1 != S
        one_frame += N == 1
        p, s, l = pos, S, left
        lo, hi = min(S, S1), max(S, S1)
        for i in range(N):
            at, step_i = gm.closed_form(pos, S, inc, i)
            assert at == p and step_i == s and lo <= s <= hi, (S, S1, N, i)
            (took,), p, s, l = gm.iterate(p, s, inc, l, target, 1)
            assert took == at
        assert s == S1 and l == 0                                   # exactly the target, whatever the division left over
        assert gm.closed_form(pos, S, inc, N)[0] == p               # the first frame behind the glide
        assert gm.iterate(p, s, inc, l, target, 3)[0] == [p, (p + S1) & gm.M64, (p + 2 * S1) & gm.M64]
    assert zero_inc >= 20 and one_frame >= 40


@pytest.mark.parametrize("ratio", [0.5, 2.0, 1.0 / 256.0, 256.0, 1e-9, 1e9, 0.999, 44100.0 / 48000.0])
def test_after_n_frames_the_step_is_resampler_step_of_the_ratio(ratio):
    e, nodes = _model_bank(1, 64, loops=[True], lens=[5000])
    n = e.nodes[nodes[0]]
    e.glide(nodes[0], ratio, 777)
    for _ in range(13):             # 832 frames
        e.process_blocks(1)
    assert n.left == 0 and n.step == resampler_step(F32(ratio)) and LO <= n.step <= HI


def test_trunc_div_is_cxx_division():
    for a, b, q in ((7, 2, 3), (-7, 2, -3), (7, -2, -3), (-7, -2, 3), (0, 5, 0), (-1, 1 << 24, 0), ((1 << 40) - 1, 1 << 24, (1 << 16) - 1)):
        assert gm.trunc_div(a, b) == q


# ------------------------------------------------------------------------------------------------ graphs (any fwapi.Engine)
def _sample(e, v, frames, fmt=PLANAR_F32, ch=2):
    data = voice_source(5100 + v, frames, ch)
    if fmt == PLANAR_I16:
        return e.new_sample(fmt, ch, np.round(data * 32767).astype(np.int16))
    if fmt == INTERLEAVED_F32:
        return e.new_sample(fmt, ch, data.T.copy())
    return e.new_sample(fmt, ch, data)


def build(e, n_voices, ratios, loops, lens, fmt=PLANAR_F32, ch=2, spatial=False, leaf=20):
    """voices resampler -> volume -> [pan] (or resampler -> spatialiser) under SumNodes of `leaf` ports -> graph_out"""
    rng = np.random.default_rng(77)
    srcs, ends = [], []
    for v in range(n_voices):
        smp = _sample(e, v, lens[v], fmt, ch)
        s = e.resampler(smp, ratios[v], loop=loops[v], n_out=2)
        if spatial:
            cur = e.spatial(float(rng.uniform(-4, 4)), float(rng.uniform(-1, 1)), float(rng.uniform(-4, 4)), n_in=2)
            e.connect_stereo(s, cur)
        else:
            cur = e.volume(float(rng.uniform(30, 100)))
            e.connect_stereo(s, cur)
            if v % 2:
                p = e.pan(float(rng.uniform(-1, 1)))
                e.connect_stereo(cur, p)
                cur = p
        srcs.append(s)
        ends.append(cur)
    mixers = []
    for i in range(0, n_voices, leaf):
        m = e.sum(len(ends[i:i + leaf]))
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
    return srcs


def _model_bank(n_voices, F, ratios=None, loops=None, lens=None, **kw):
    e = gm.GlideRefEngine(max_block_frames=F)
    nodes = build(e, n_voices, ratios or [1.0] * n_voices, loops or [True] * n_voices, lens or [5000] * n_voices, **kw)
    return e, nodes


# ================================================================================================ CPU tier: the model
@pytest.mark.parametrize("loop,frames", [(True, 37), (True, 5000), (False, 37), (False, 5000)])
def test_model_block_splits_give_the_same_samples_and_state(loop, frames):
    total = 448
    splits = {"one": [total], "1": [1] * total, "7": [7] * 64, "64": [64] * 7, "mixed": [64, 1, 100, 7, 256, 20]}
    runs = {}
    for name, blocks in splits.items():
        assert sum(blocks) == total
        e, (n,) = _model_bank(1, 512, ratios=[0.5], loops=[loop], lens=[frames])
        e.glide(n, 2.0, 300)
        out = np.concatenate([e.process_interleaved(b) for b in blocks])
        node = e.nodes[n]
        runs[name] = (out, (node.pos, node.step, node.left, node.playing_ctl))
    for name in splits:
        assert_bits(runs[name][0], runs["one"][0], name)
        # (a one-shot that runs out stops behind the BLOCK that carries it past the end, so where the 37-frame one's position comes to
        #  rest depends on the split; what it renders behind its end is +0.0 either way)
        if loop or frames == 5000:
            assert runs[name][1] == runs["one"][1], name
        assert runs[name][1][1:3] == (resampler_step(2.0), 0) or not runs[name][1][3], name
    assert np.any(runs["one"][0] != 0)


def test_model_behind_a_glide_the_node_is_a_fresh_node_at_that_position_and_ratio():
    e, (n,) = _model_bank(1, 64, ratios=[0.5], lens=[5000])
    e.glide(n, 1.75, 150)
    for _ in range(3):
        e.process_blocks(1)
    node = e.nodes[n]
    assert node.left == 0
    f, (m,) = _model_bank(1, 64, ratios=[1.0], lens=[5000])
    f.set_param(m, 1, 1.75)
    f.nodes[m].pos = node.pos
    assert_bits(np.concatenate([e.process_blocks(1) for _ in range(4)]), np.concatenate([f.process_blocks(1) for _ in range(4)]), "behind the glide")


def test_model_messages_during_a_glide():
    e, (n,) = _model_bank(1, 64, ratios=[0.5], lens=[5000])
    node = e.nodes[n]
    e.glide(n, 2.0, 640)
    e.process_blocks(3)
    mid = node.step
    assert node.left == 640 - 192 and resampler_step(0.5) < mid < resampler_step(2.0)
    e.glide(n, 0.25, 100)                       # a second glide starts from the step the first has reached
    assert node.left == 100 and node.inc == gm.trunc_div(resampler_step(0.25) - mid, 100) and node.step == mid
    e.set_param(n, 4, 40.0)                     # a seek leaves the glide as it is
    e.set_param(n, 3, 0.0)                      # paused: nothing advances, the glide included
    e.process_blocks(2)
    assert node.left == 100 and node.step == mid
    e.set_param(n, 3, 1.0)
    e.process_blocks(1)
    assert node.left == 36 and node.pos >> 32 >= 40
    e.set_param(n, 1, 1.5)                      # a step ends the glide
    assert node.left == 0 and node.step == resampler_step(1.5)
    e.glide(n, 3.0, 0)                          # frames == 0 is a step
    assert node.left == 0 and node.step == resampler_step(3.0)


# ================================================================================================ CPU tier: the ABI on the harness
def _harness_bank(n=3):
    e = HostOnlyEngine(max_block_frames=64, max_batch=4)
    srcs = build(e, n, [1.0] * n, [True] * n, [900] * n)
    return e, srcs


def _early(P, c):
    """[(type, block, i0, d0 bits)] of the messages waiting for their node's first plan"""
    return [(w[0], w[1], w[3], w[5] | (w[6] << 32)) for w in fwapi.early_msgs(P, c)]


def test_abi_what_a_call_queues():
    """one Cmd per call: CMD_RS_GLIDE with S1 = resampler_step(ratio) as the bits of d0 and frames in i0; frames == 0 is CMD_RS_STEP,
    the message param 1 queues.  Read where the ABI keeps the messages of a node that no plan holds yet."""
    P = fwapi.peek_lib("rs_glide_peek")
    e = HostOnlyEngine(sample_rate=44100, max_block_frames=96, num_graph_inputs=3, num_graph_outputs=2)
    L, c = e.cx.L, e.cx.c
    # the helper and the harness library are two builds of fwgpu_ctx: members in front of and behind early_msgs must read as they were set
    assert P.fwp_layout_check(c, 44100, 96, 3, 2, 0) == 0
    assert P.fwp_layout_check(c, 44100, 64, 3, 2, 0) == 2 and P.fwp_layout_check(c, 48000, 96, 2, 2, 0) == 5      # (and it does look)
    s = e.resampler(_sample(e, 0, 900), 1.0, loop=True, n_out=2)
    assert _early(P, c) == []
    assert L.fwgpu_resampler_glide(c, s, 2.0, gm.FRAMES_MAX, 0) == 0               # the longest glide
    assert L.fwgpu_resampler_glide(c, s, 1e9, 1, 3) == 0                           # any ratio but NaN: clamped, as param 1 clamps
    assert L.fwgpu_resampler_glide(c, s, float("-inf"), 5, 1) == 0
    assert L.fwgpu_resampler_glide(c, s, 0.37, 0, 2) == 0                          # frames == 0 ...
    e.set_param(s, 1, 0.37, at_block=2)                                            # ... is param 1's message
    assert L.fwgpu_resampler_glide(c, s, float("nan"), 10, 0) == INVALID           # a refused call queues nothing
    assert L.fwgpu_resampler_glide(c, s, 1.0, gm.FRAMES_MAX + 1, 0) == INVALID
    got = _early(P, c)
    assert got == [(gm.CMD_RS_GLIDE, 0, gm.FRAMES_MAX, resampler_step(2.0)), (gm.CMD_RS_GLIDE, 3, 1, HI), (gm.CMD_RS_GLIDE, 1, 5, LO),
                   (gm.CMD_RS_STEP, 2, 0, resampler_step(0.37)), (gm.CMD_RS_STEP, 2, 0, resampler_step(0.37))], got
    e.connect_stereo(s, e.graph_out_node)
    e.update()                                                                     # the plan that activates the node releases them
    assert _early(P, c) == []
    e.process_blocks(4)
    assert e.violation() == ""


def test_abi_refusals_and_a_good_call_reaches_the_control_kernel():
    e, srcs = _harness_bank()
    L, c = e.cx.L, e.cx.c
    assert e.cx.plan_kind() == 1
    seen = fwapi.hostonly_lib().fwh_cmds_seen           # messages the control kernel's launches would apply
    seen.restype = C.c_ulonglong
    vol = e.volume(50.0)
    for bad, word in ((lambda: L.fwgpu_resampler_glide(c, vol, 1.0, 10, 0), "not a resampling source"),
                      (lambda: L.fwgpu_resampler_glide(c, srcs[0], float("nan"), 10, 0), "NaN"),
                      (lambda: L.fwgpu_resampler_glide(c, srcs[0], 1.0, gm.FRAMES_MAX + 1, 0), "2^24"),
                      (lambda: L.fwgpu_resampler_glide(c, 1 << 40, 1.0, 10, 0), "unknown node")):
        assert bad() == INVALID
        assert word in L.fwgpu_last_error(c).decode()
    assert L.fwgpu_resampler_glide(None, srcs[0], 1.0, 10, 0) == INVALID
    e.process_blocks(2)
    n0 = seen()
    assert L.fwgpu_resampler_glide(c, srcs[0], 2.0, gm.FRAMES_MAX, 0) == 0
    assert L.fwgpu_resampler_glide(c, srcs[1], 1e9, 1, 1) == 0
    assert L.fwgpu_resampler_glide(c, srcs[1], float("inf"), 5, 1) == 0
    assert L.fwgpu_resampler_glide(c, srcs[2], 0.5, 0, 0) == 0
    e.process_blocks(2)
    assert seen() == n0 + 4                              # the refused calls above queued nothing
    e.process_blocks(1)
    assert seen() == n0 + 4 and e.violation() == ""


def test_abi_a_glide_for_a_node_no_plan_holds_yet_waits_for_the_update():
    e = HostOnlyEngine(max_block_frames=64)
    smp = _sample(e, 0, 900)
    s = e.resampler(smp, 1.0, loop=True, n_out=2)
    assert e.cx.L.fwgpu_resampler_glide(e.cx.c, s, 1.5, 100, 0) == 0
    e.connect_stereo(s, e.graph_out_node)
    e.update()
    e.process_blocks(1)
    assert e.violation() == ""


def test_typed_mirror_and_doppler_ratio():
    import firewheel_amd as fa
    from firewheel_amd import graph

    cx = fwapi.hostonly_ctx(max_block_frames=64)
    node = fa.ResamplerNode(cx.new_sample(PLANAR_F32, 2, voice_source(1, 500, 2)), ratio=1.0, loop=True)
    nid = cx.add_node(0, 2, node)
    node.glide_to(1.5, 480)                     # before the first update
    cx.connect(nid, 0, cx.graph_out_node(), 0)
    cx.update()
    node.glide_to(0.5, 100, at_block=2)
    node.glide_to(2.0, 0)
    assert node.ratio == 2.0 and fa.ResamplerNode.GLIDE_FRAMES_MAX == gm.FRAMES_MAX
    for bad in (lambda: node.glide_to(float("nan"), 10), lambda: node.glide_to(1.0, gm.FRAMES_MAX + 1)):
        with pytest.raises(fa.FwgpuError) as ei:
            bad()
        assert ei.value.code == INVALID
    d = graph.doppler_ratio
    assert d(1.0, 0.0) == 1.0 and d(2.0, 343.0) == 1.0 and d(1.0, -171.5) == 2.0 and d(0.5, 10.0, 340.0) == 0.5 * 340.0 / 350.0
    assert d(1.0, 34.3) < 1.0 < d(1.0, -34.3)                 # receding: the pitch drops
    for v in (-343.0, -400.0, float("nan")):
        with pytest.raises(ValueError):
            d(1.0, v)
    assert fa.doppler_ratio is d


def test_header_types_ffi_and_lib_agree():
    import firewheel_amd._lib as flib

    rd = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr, types = rd("include", "fwgpu.h"), rd("firewheel_amd", "csrc", "fwgpu_types.h")
    ffi, nodes = rd("rust", "firewheel-gpu", "src", "ffi.rs"), rd("rust", "firewheel-gpu", "src", "nodes.rs")
    assert re.search(r"#define FWGPU_RESAMPLER_GLIDE_FRAMES_MAX 16777216\b", hdr)
    assert "int fwgpu_resampler_glide(fwgpu_ctx* ctx, int64_t node, float ratio, uint32_t frames, uint32_t at_block);" in hdr
    assert re.search(r"CMD_RS_GLIDE = 24\b", types) and re.search(r"CMD_RS_STEP = 20\b", types) and re.search(r"#define RS_GLIDE_FRAMES_MAX 16777216u", types)
    assert re.search(r"K_LAST = K_CROSSFADE\b", types)           # no new node kind
    assert "pub const FWGPU_RESAMPLER_GLIDE_FRAMES_MAX: u32 = 16777216;" in ffi
    assert "pub fn fwgpu_resampler_glide(ctx: *mut fwgpu_ctx, node: i64, ratio: f32, frames: u32, at_block: u32) -> c_int;" in ffi
    assert "pub fn glide_to" in nodes and "ffi::fwgpu_resampler_glide" in nodes
    res, args = flib.SIGNATURES["fwgpu_resampler_glide"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_float, C.c_uint32, C.c_uint32]


# ================================================================================================ GPU tier: the list of glides
N_CALLS = 5      # call 0 and call 4 carry no message


def _at(K, call, where, plus=0):
    """(call, at_block) of block `where` ('first' / 'mid' / 'last') of `call`, `plus` blocks further on"""
    g = call * K + {"first": 0, "mid": K // 2, "last": K - 1}[where] + plus
    return g // K, g % K


def script(F, K):
    """per item: (initial ratio, sample frames, loops, [(call, at_block, message, args)]) — voice v of a bank plays item v % len"""
    A = lambda where, plus=0, call=1: _at(K, call, where, plus)
    G = lambda pos, ratio, N: pos + ("glide", (ratio, N))
    P = lambda pos, param, value: pos + ("param", (param, value))
    tiny = float(np.nextafter(F32(1.0), F32(2.0)))           # 512 steps of 2^-32 over 4096 frames: inc == 0
    span3 = (K - K // 2) * F + K * F + F // 2                # from the middle of call 1 to inside call 3
    return [
        (0.5, 5000, True, [G(A("first"), 2.0, 1)]),
        (2.0, 5000, True, [G(A("mid"), 0.5, 3)]),
        (0.5, 5000, True, [G(A("last"), 2.0, F - 1)]),
        (2.0, 5000, True, [G(A("first"), 0.5, F)]),
        (0.5, 5000, True, [G(A("mid"), 2.0, F + 1)]),
        (2.0, 5000, True, [G(A("first"), 0.5, 5 * F + 7)]),
        (0.8, 5000, True, [G(A("mid"), 1.6, span3)]),
        (1.0 / 256.0, 5000, True, [G(A("first"), 256.0, 4 * F)]),                       # the window grows beyond what LDS stages
        (1.0, 5000, True, [G(A("first"), tiny, 4096)]),
        (0.7, 5000, True, [G(A("first"), 1.9, 6 * F), G(A("first", 2), 0.6, 2 * F + 5)]),   # a retarget in mid-glide
        (0.7, 5000, True, [G(A("first"), 1.9, 6 * F), P(A("first", 3), 1, 1.3)]),           # set_ratio in mid-glide
        (1.2, 5000, True, [G(A("first"), 0.4, 6 * F), P(A("first", 2), 4, 100.0)]),         # a seek in mid-glide
        (1.2, 5000, True, [G(A("first"), 0.4, 6 * F), P(A("first", 1), 3, 0.0), P(A("first", 3), 3, 1.0)]),   # pause and resume
        (1.0, 5000, True, [G(A("mid"), 1.7, 3 * F), G(A("mid"), 0.8, 2 * F + 1)]),          # two glides for one block
        (0.5, 37, True, [G(A("first"), 2.0, 5 * F + 7)]),                                   # the loop wraps inside the glide, many times
        (1.0, 5000, False, [P(A("first"), 4, float(5000 - 3 * F)), G(A("first"), 2.0, 8 * F)]),   # a one-shot ends inside the glide
        (0.25, 37, False, [P(A("first"), 4, 0.0), P(A("first"), 3, 1.0), G(A("first"), 1.0, 4 * F)]),
        (1.9, 5000, True, [G(A("last", call=2), 0.3, 5 * F + 7)]),                          # the 5000-frame loop wraps inside the glide
    ]


def run_script(e, F, K, n_voices, n_calls=N_CALLS, **kw):
    items = script(F, K)
    pick = [items[v % len(items)] for v in range(n_voices)]
    srcs = build(e, n_voices, [p[0] for p in pick], [p[2] for p in pick], [p[1] for p in pick], **kw)
    outs = []
    for call in range(n_calls):
        for v, p in enumerate(pick):
            for c, at, what, args in p[3]:
                if c == call and what == "glide":
                    e.glide(srcs[v], args[0], args[1], at_block=at)
                elif c == call:
                    e.set_param(srcs[v], args[0], args[1], at_block=at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


_refs = {}


def reference(F, K, n_voices, n_calls=N_CALLS, **kw):
    key = (F, K, n_voices, n_calls, tuple(sorted(kw.items())))
    if key not in _refs:
        out = run_script(gm.Tagged(gm.GlideRefEngine(max_block_frames=F)), F, K, n_voices, n_calls, **kw)
        out.setflags(write=False)
        assert np.any(out != 0)
        _refs[key] = out
    return _refs[key]


COMBOS = [(64, 70, 8), (100, 3, 40), (256, 3, 20), (512, 1, 18), (64, 1, 1)]      # F, K, voices
SMALL = [(100, 3, 18), (256, 1, 18)]


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g1_level_executor(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K, force_generic=True)
    got = run_script(gm.GpuGlide(g), F, K, V)
    assert g.cx.plan_kind() == 0
    assert_bits(got, reference(F, K, V), "level executor")


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g2_fused_voice_bank_planar_f32(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(gm.GpuGlide(g), F, K, V)
    assert g.cx.plan_kind() == 1 and g.cx.plan_fused_voices() == V
    assert_bits(got, reference(F, K, V), "voice bank, planar f32")


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", SMALL)
@pytest.mark.parametrize("fmt,ch", [(PLANAR_I16, 2), (INTERLEAVED_F32, 2), (PLANAR_F32, 1), (PLANAR_I16, 1)])
def test_g3_g4_other_formats_and_mono_sources(fmt, ch, F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(gm.GpuGlide(g), F, K, V, fmt=fmt, ch=ch)
    assert g.cx.plan_kind() == 1
    assert_bits(got, reference(F, K, V, fmt=fmt, ch=ch), "format %d, %d channel(s)" % (fmt, ch))


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", [(64, 3, 18), (256, 1, 18)])
def test_g5_voices_that_end_in_a_spatialiser(F, K, V):
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_script(gm.GpuGlide(g), F, K, V, spatial=True)
    assert_bits(got, reference(F, K, V, spatial=True), "resampler -> spatialiser")


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 256])
def test_g6_one_block_calls(F):
    """40 voices under two leaves and a root: the tree the one-launch edge takes.  Calls 1, 2 and 3 carry messages (the launch
    sequence: include/fwgpu.h fwgpu_rt_path_stats); the others — glides in flight among them — are one launch or a doorbell."""
    V, K, calls = 40, 1, 12
    g = GpuEngine(max_block_frames=F)
    before = g.cx.rt_path_stats()
    got = run_script(gm.GpuGlide(g), F, K, V, n_calls=calls)
    delta = tuple(a - b for a, b in zip(g.cx.rt_path_stats(), before))
    print("one-block launch batches by path (resident, one launch, fused sequence, level executor):", delta)
    assert g.cx.plan_kind() == 1
    assert_bits(got, reference(F, K, V, n_calls=calls), "one-block calls")
    assert sum(delta) == calls and delta[3] == 0 and delta[2] <= 3 and delta[0] + delta[1] >= calls - 3, delta


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 100, 256])
def test_g7_node_process_every_item_of_the_script(F):
    """fwgpu_node_process (k_single_node, an instantiation of its own with its own apply_cmds_from): EVERY item of script(), one node
    per item, one block per call, the item's messages sent between the calls exactly as run_script sends them at K = 1 — samples
    and out mask of every block against GlideResamplerNode.process."""
    K, calls = 1, 12
    items = script(F, K)
    g = GpuEngine(max_block_frames=F)
    e = gm.GlideRefEngine(max_block_frames=F)
    gg = gm.GpuGlide(g)
    gs = build(g, len(items), [p[0] for p in items], [p[2] for p in items], [p[1] for p in items])
    ms = build(e, len(items), [p[0] for p in items], [p[2] for p in items], [p[1] for p in items])
    masks, glided, ended = set(), 0, 0
    for call in range(calls):
        for v, p in enumerate(items):
            node = e.nodes[ms[v]]
            for c, at, what, args in p[3]:
                assert at == 0
                if c == call and what == "glide":
                    gg.glide(gs[v], args[0], args[1])
                    e.glide(ms[v], args[0], args[1])
                elif c == call:
                    g.set_param(gs[v], args[0], args[1])
                    e.set_param(ms[v], args[0], args[1])
            glided += node.left > 0 and node.playing_ctl
            was_playing = node.playing_ctl
            y, om = g.node_process(gs[v], F, [], 2)
            outs = [np.full(F, np.nan, dtype=F32), np.full(F, np.nan, dtype=F32)]
            wm = node.process(F, [], outs, 0)
            assert om == wm, (v, call, om, wm)
            assert_bits(y, np.stack(outs), "item %d, call %d" % (v, call))
            masks.add(wm)
            ended += was_playing and not node.playing_ctl and not p[2]
    # (what the run must have met: blocks inside a glide, blocks flagged silent — a pause, a one-shot behind its end —, one-shots that ran out)
    assert glided >= 40 and masks == {0, 3} and ended >= 2, (glided, masks, ended)


@pytest.mark.gpu
@pytest.mark.parametrize("F,loop,frames", [(100, True, 5000), (256, False, 5000), (37, True, 37)])
def test_g7_node_process(F, loop, frames):
    g = GpuEngine(max_block_frames=256)
    smp = _sample(g, 3, frames)
    s = g.resampler(smp, 0.5, loop=loop, n_out=2)
    g.connect_stereo(s, g.graph_out_node)
    g.update()
    e = gm.GlideRefEngine(max_block_frames=256)
    m = e.resampler(_sample(e, 3, frames), 0.5, loop=loop, n_out=2)
    node = e.nodes[m]
    gg = gm.GpuGlide(g)
    for k in range(9):
        if k == 1:
            gg.glide(s, 2.0, 2 * F + F // 2)          # ends inside call 3
            e.glide(m, 2.0, 2 * F + F // 2)
        if k == 5:
            gg.glide(s, 0.75, 3)
            e.glide(m, 0.75, 3)
        if k == 7:
            gg.glide(s, 1.0 / 256.0, 2 * F + 1)
            e.glide(m, 1.0 / 256.0, 2 * F + 1)
        y, om = g.node_process(s, F, [], 2)
        outs = [np.zeros(F, dtype=F32), np.zeros(F, dtype=F32)]
        wm = node.process(F, [], outs, 0)
        assert om == wm
        assert_bits(y, np.stack(outs), "block %d" % k)
    assert node.left == 1 and node.step != resampler_step(0.5)


# ------------------------------------------------------------------------------------------------ lazy calls around a glide
@pytest.mark.gpu
def test_g8_a_call_inside_a_glide_runs_the_control_kernel_and_lazy_calls_resume_behind_it():
    F, K, V = 64, 4, 12
    ratios = [0.5 + 0.1 * v for v in range(V)]

    def run(e):
        srcs = build(e, V, ratios, [True] * V, [5000] * V)
        outs, marks = [], []
        for call in range(12):
            if call == 4:
                for v in (0, 5, 11):
                    e.glide(srcs[v], 1.7 - 0.1 * v, 9 * F + 3, at_block=1)      # through calls 4, 5 and into call 6
            outs.append(np.asarray(e.process_blocks(K)))
            if hasattr(e, "cx"):
                marks.append(e.cx.lazy_stats())
        return np.concatenate(outs), marks

    want, _ = run(gm.Tagged(gm.GlideRefEngine(max_block_frames=F)))
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got, marks = run(gm.GpuGlide(g))
    assert g.cx.plan_kind() == 1
    assert_bits(got, want, "twelve calls")
    if os.environ.get("FWGPU_LAZY") == "0":
        return
    lazy, ctl = [m[0] for m in marks], [m[1] for m in marks]
    assert lazy[3] > lazy[1], marks                     # quiet calls in front of the glide are lazy
    assert lazy[6] == lazy[3] and ctl[6] - ctl[3] == 3, marks     # calls 4, 5, 6: a glide in flight (or ending): the control kernel, no lazy batch
    assert lazy[11] - lazy[7] == 4, marks               # ... and lazy again behind it, bit-exact (above) over these calls


# ------------------------------------------------------------------------------------------------ a graph edit inside a glide
@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g9_the_glide_carries_over_a_plan_install(force_generic):
    F, K, V = 64, 3, 6

    def run(e):
        srcs = build(e, V, [1.5, 0.5, 1.0, 2.0, 0.7, 1.1], [True] * V, [5000] * V, leaf=8)
        outs = [np.asarray(e.process_blocks(K))]
        e.glide(srcs[0], 0.4, 8 * F + 9, at_block=1)          # a falling ratio: inc < 0, both halves of it in use
        e.glide(srcs[1], 1.9, 8 * F + 9, at_block=2)
        outs.append(np.asarray(e.process_blocks(K)))
        # a voice is added to the mixer's free port between two calls of the glide
        extra = e.resampler(_sample(e, 50, 900), 1.25, loop=True, n_out=2)
        vol = e.volume(60.0)
        e.connect_stereo(extra, vol)
        e.connect_stereo(vol, e.the_mixer, 2 * V)
        e.update()
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

    want = run(Eng(gm.Tagged(gm.GlideRefEngine(max_block_frames=F))))
    g = GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)
    got = run(Eng(gm.GpuGlide(g)))
    assert g.cx.plan_kind() == (0 if force_generic else 1)
    assert_bits(got, want, "a plan install between two calls of a glide")


# ------------------------------------------------------------------------------------------------ silence flags behind a one-shot
@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g10_a_one_shot_that_ends_inside_a_glide_stays_silent_and_flagged(force_generic):
    F, K = 64, 6

    def run(e):
        (s,) = build(e, 1, [1.0], [False], [5000])
        e.set_param(s, 4, float(5000 - 5 * F))
        e.glide(s, 2.0, 20 * F, at_block=1)
        a, fa = e.process_blocks_flags(K)
        b, fb = e.process_blocks_flags(K)
        return np.concatenate([np.asarray(a), np.asarray(b)]), np.concatenate([np.asarray(fa, dtype=bool), np.asarray(fb, dtype=bool)])

    want, wf = run(gm.Tagged(gm.GlideRefEngine(max_block_frames=F)))
    got, gf = run(gm.GpuGlide(GpuEngine(max_block_frames=F, max_batch=K, force_generic=force_generic)))
    assert not wf[:3].any() and wf[-6:].all() and np.any(want != 0)
    assert np.array_equal(gf, wf), (gf.T, wf.T)
    assert_bits(got, want, "one-shot")


# ------------------------------------------------------------------------------------------------ the seeded family
def fuzz(e, seed, F):
    rng = np.random.default_rng(31_000 + seed)
    V = 40
    lens = [int(rng.choice([37, 700, 5000])) for _ in range(V)]
    loops = [bool(rng.random() < 0.7) for _ in range(V)]
    ratios = [float(rng.choice([0.25, 0.5, 0.9, 1.0, 1.5, 1.93, 3.0])) for _ in range(V)]
    srcs = build(e, V, ratios, loops, lens)
    outs = []
    for call in range(4):
        K = int(rng.integers(1, 5))
        for _ in range(int(rng.integers(0, 25))):
            s, at = srcs[int(rng.integers(0, V))], int(rng.integers(0, K))
            what = rng.random()
            if what < 0.55:
                N = int(rng.choice([1, 3, F - 1, F, F + 1, 3 * F + 7, int(rng.integers(1, 8 * F))]))
                e.glide(s, float(rng.choice([1.0 / 256.0, 0.3, 0.77, 1.0, 1.0000001, 1.4, 2.5, 8.0])), N, at_block=at)
            elif what < 0.7:
                e.set_param(s, 1, float(rng.uniform(0.3, 2.5)), at_block=at)
            elif what < 0.85:
                e.set_param(s, 4, float(rng.integers(0, 600)), at_block=at)
            else:
                e.set_param(s, 3, float(rng.integers(0, 2)), at_block=at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_g11_seeded_glides_steps_seeks_and_pauses_on_both_plans(seed):
    F = [64, 100, 256][seed % 3]
    want = fuzz(gm.Tagged(gm.GlideRefEngine(max_block_frames=F)), seed, F)
    for force_generic in (False, True):
        g = GpuEngine(max_block_frames=F, max_batch=4, force_generic=force_generic)
        got = fuzz(gm.GpuGlide(g), seed, F)
        assert g.cx.plan_kind() == (0 if force_generic else 1)
        assert_bits(got, want, "seed %d, %s" % (seed, "level executor" if force_generic else "voice bank"))
