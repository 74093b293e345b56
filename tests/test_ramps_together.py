"""Fades, glides, sweeps, moves and streams in flight TOGETHER: the five messages that move a value every frame
each have a model and a bit-exact test file of their own, and each of those files keeps the other four features at rest.  On the
device they share ramp rows, fields, host bounds and kernel instantiations; here they meet in one voice and in one call.

The reference is tests/ramps_model.py: ONE RefEngine whose add_node picks the five model files' node classes by kind.  Every comparison
is bit equality (busnodes.assert_bits): there is no tolerance to choose.

CPU tier: the combined engine equals each single engine on that feature's own script (bits and silence flags); the script of this file
is not vacuous (per pair of features, counted block by block from the model's state: blocks with both in flight, a block in which one
ends while the other goes on, a call boundary crossed with both in flight); the planner on the host-only harness (a mixed bank with a
move, a sweep and a move in one level-executor call, a fade and a sweep on a chain bank).

GPU tier: ONE script of items (bank_items / chain_items) through the level executor, the fused mixed bank (k_leaf_sum_rs_sp_spm), the
source formats, the chain plan at both tile sizes, the hybrid plan, one-block calls, ragged calls, a plan install in mid-flight, the
accounting of lazy calls, a seeded family.

Three things the models decide: a spatialiser never flags its output, so behind a fade's STOP inside a move the graph output plays the
tail out and then holds exact zeros UNFLAGGED; the end of a stream puts the envelope back to rest, so a stream and its fade-out end in
the same block (a second, short fade comes to rest while the stream goes on); the sweep model reports no silence flags, so its scripts are compared sample for sample only.
"""
import ctypes as C
import os

import numpy as np
import pytest

import busnodes
import fwapi
import ramps_model as rm
import refmodel
import sampler_fade_model as sfm
import stream_source_model as ssm
import test_bq_sweep as t_sweep
import test_rs_glide as t_glide
import test_sampler_fade as t_fade
import test_sp_move as t_move
import test_stream_source as t_stream
from busnodes import assert_bits
from fwapi import INTERLEAVED_I16, LOOP_FULL, PLANAR_F32, PLANAR_I16, GpuEngine, HostOnlyEngine
from sampler_fade_model import NONE, PAUSE, STOP
from scenarios import voice_source
from test_sp_move import POS, set_position

FUZZ_SEEDS = int(os.environ.get("FWGPU_FUZZ_SEEDS", "20"))
SR = 48000
ULL = C.c_ulonglong
N_CALLS = 5
LEAF = 20            # ports of a leaf mixer: 37 voices are two leaves and a top mixer


def model(F):
    return rm.Tagged(rm.RampsRefEngine(max_block_frames=F, short_blocks=True))


# ================================================================================================ CPU tier: the engine is the five engines
def _same(a, b, what, F=None):
    """samples and silence flags of two runs are the same: both runs hold a row of flags for EVERY block of F frames they rendered.
    F=None only where the single model reports no flags (the sweep's): samples alone"""
    (oa, fa), (ob, fb) = a, b
    assert_bits(oa, ob, what)
    if F is None:
        assert fb is None, what
        return
    assert fa is not None and fb is not None and fa.shape == fb.shape == (len(oa) // (2 * F), 2) and len(fa) > 0, what
    assert np.array_equal(fa, fb), what


def _with_flags(e, run):
    """run(e) with every process_blocks call of `e` routed through process_blocks_flags -> (samples, flags); flags None where the engine
    reports none (the sweep model's)"""
    flags = []
    plain = e.process_blocks
    if not hasattr(e.e, "process_blocks_flags"):
        return np.asarray(run(e)), None

    def process_blocks(k, n_out_ch=2):
        if n_out_ch != 2:
            return plain(k, n_out_ch)
        o, f = e.process_blocks_flags(k, n_out_ch)
        flags.append(np.asarray(f, dtype=bool))
        return o
    e.process_blocks = process_blocks
    out = run(e)
    return np.asarray(out), (np.concatenate(flags) if flags else None)


def test_the_combined_engine_equals_the_fade_engine_on_the_fade_script():
    F, K, V = t_fade.COMBOS[1]
    run = lambda e: t_fade.run_script(e, F, K, V)
    _same(_with_flags(rm.Tagged(rm.RampsRefEngine(max_block_frames=F)), run), _with_flags(sfm.Tagged(sfm.FadeRefEngine(max_block_frames=F)), run), "fades", F)


def test_the_combined_engine_equals_the_glide_engine_on_the_glide_script():
    F, K, V = t_glide.COMBOS[1]
    run = lambda e: t_glide.run_script(e, F, K, V)
    _same(_with_flags(rm.Tagged(rm.RampsRefEngine(max_block_frames=F)), run),
          _with_flags(t_glide.gm.Tagged(t_glide.gm.GlideRefEngine(max_block_frames=F)), run), "glides", F)


def test_the_combined_engine_equals_the_move_engine_on_the_move_script():
    F, K, V = t_move.COMBOS[0]
    run = lambda e: t_move.run_script(e, F, K, V)
    _same(_with_flags(model(F), run), _with_flags(t_move.sm.Tagged(t_move.sm.MoveRefEngine(max_block_frames=F, short_blocks=True)), run), "moves", F)


@pytest.mark.parametrize("name", ["BB both", "BD"])
def test_the_combined_engine_equals_the_sweep_engine_on_the_sweep_scripts(name):
    """test_bq_sweep.py has no script(F, K): its chain bank (F, K and 40 voices of its own) and its bus graph are its scripts"""
    bm, F = t_sweep.bm, t_sweep.F
    run = lambda e: t_sweep.run_chain(e, name)
    _same(_with_flags(rm.Tagged(rm.RampsRefEngine(max_block_frames=F)), run), _with_flags(bm.Tagged(bm.SweepRefEngine(max_block_frames=F)), run), name)
    msgs = t_sweep.INTERPLAY["retarget in mid-sweep"]
    bus = lambda e: t_sweep.run_bus(e, 2, msgs, tail_frames=37)
    _same(_with_flags(model(F), bus), _with_flags(bm.Tagged(bm.SweepRefEngine(max_block_frames=F, short_blocks=True)), bus), "bus")


def test_the_combined_engine_equals_the_stream_engine_on_the_stream_files_bank_case():
    """tests/test_stream_source.py test_with_the_other_voice_features, plan "bank": its graph, its writes and its messages, with the end
    of the stream added; samples, flags and the stream's accounting"""
    B, K = t_stream.B, 3
    variant, n, streamed, _, _ = t_stream.PLANS["bank"]
    script = {1: [("pv", 35.0, 1)], 3: [("pv", 0.0, 0)], 8: [("pv", 90.0, 2)], 9: [("pause", None, 1)], 10: [("play", None, 0)],
              11: [("stop", None, 2)], 12: [("play", None, 1)], 13: [("fade", (0.0, 150, STOP), 0)], 15: [("play", None, 0)]}
    runs = []
    for e in (sfm.Tagged(ssm.StreamRefEngine(max_block_frames=B)), rm.Tagged(rm.RampsRefEngine(max_block_frames=B))):
        feeds = t_stream._build(e, variant, n, streamed, t_stream.P_F32, 2, 12 * B + 24, t_stream.RowsOf(t_stream.P_F32, 2, 40 * B + 17, streamed))
        outs, fls, sts = [], [], []
        for call in range(18):
            for v in streamed:
                f = feeds[v]
                f.write(min(3 * K * B, f.R - B - (f.pos - f.status()[1])))
                if f.pos == len(f.rows) and not f.ended:
                    f.end()
            for what, arg, at in script.get(call, []):
                smp = feeds[streamed[0]].sampler
                if what == "pv":
                    e.set_param(smp, 0, arg, at_block=at)
                elif what == "fade":
                    e.fade(smp, arg[0], arg[1], arg[2], at_block=at)
                else:
                    getattr(e, "sampler_" + what)(smp, at_block=at)
            o, f = e.process_blocks_flags(K)
            outs.append(o)
            fls.append(f)
            sts.append([feeds[v].status() for v in streamed])
        runs.append((np.concatenate(outs), np.concatenate(fls), sts))
    assert_bits(runs[1][0], runs[0][0], "streams")
    assert np.array_equal(runs[1][1], runs[0][1]) and runs[1][2] == runs[0][2]
    assert all(st[3] for st in runs[0][2][-1]) and np.any(runs[0][0] != 0)          # every stream finished


# ================================================================================================ the script
def _at(K, call, where, plus=0):
    """(call, at_block) of block `where` ('first' / 'mid' / 'last') of `call`, `plus` blocks further on"""
    g = call * K + {"first": 0, "mid": K // 2, "last": K - 1}[where] + plus
    return g // K, g % K


def spans(F, K):
    """(S, LONG): a ramp of S frames started anywhere in call 1 goes on over the call's end and ends INSIDE a block of call 2 (K = 1: of
    call 3); one of LONG frames started with it goes on for three and a half blocks more"""
    S = (2 if K == 1 else K + 1) * F + F // 2 + 1
    return S, S + 3 * F + 8


def stream_plan(F, K):
    """a streamed voice's data and its writer: (frames in all, the frames written before calls 0 .. 3).  One block short before call 2
    — that call's last block is starved —, the rest and the end before call 3, whose last block is the end block (F // 2 + 5 frames)"""
    total = (4 * K - 2) * F + F // 2 + 5
    return total, [K * F, 2 * K * F, 3 * K * F - F, total]


def ring_frames(F, K):
    return (K + 3) * F + 24          # the wrap falls inside a block


def _M(pos, what, *args):
    return pos + (what, args)


def bank_items(F, K):
    """plan 1.  kind "sp": sampler -> [volume] -> spatialiser; kind "rs": resampler -> volume -> [pan].  Voice v plays item v % len:
    the first five hold a resampler voice between moving spatialiser voices, so a bank of 5 voices has both kinds."""
    A = lambda where, plus=0, call=1: _at(K, call, where, plus)
    S, LONG = spans(F, K)
    shot = (2 if K == 1 else K + 1) * F + F // 3             # a one-shot that ends inside that block
    return [
        # 0: fade and move start in the same block; the fade ends inside a block in mid-move
        dict(name="fade ends in mid-move", kind="sp", msgs=[_M(A("mid"), "fade", 0.3, S), _M(A("mid"), "move", 4.0, 0.0, -0.5, LONG)]),
        # 1: a resampler voice gliding while its port neighbours' spatialisers move
        dict(name="glide beside moves", kind="rs", ratio=0.7, pan=True, msgs=[_M(A("first"), "glide", 1.9, S)]),
        # 2: a stream under a moving spatialiser: a short fade that comes to rest over the live ring, a starved block in mid-move, the end
        #    inside the move, a fade-out across the end (a starved block holds the envelope, so the fade is still going when the stream
        #    ends; the end puts the envelope back to rest)
        dict(name="stream under a move", kind="sp", vol=True, stream=True,
             msgs=[_M(A("first", call=0), "fade", 0.6, F // 2 + 3), _M(A("first"), "move", -4.0, 0.3, -0.5, 3 * K * F + F // 2 + 7),
                   _M(A("last"), "fade", 0.0, (2 * K + 1) * F + 9)]),
        # 3: then = STOP inside a move at its widest delay: from hard left to hard right, one ear's delay falls from ITD = 32 frames as
        #    the other's rises, fractional all the way; the spatialiser's 63-frame tail plays out under per-frame delays
        dict(name="stop in a wide move", kind="sp", msgs=[_M(A("first", call=0), "set", -6.0, 0.0, 0.0), _M(A("first"), "move", 6.0, 0.0, 0.0, LONG),
                                                           _M(A("first", 1), "fade", 0.0, S - F, STOP)]),
        # 4: three ramped stages in one voice: the volume's smoother, the fade, the move
        dict(name="three ramps", kind="sp", vol=True, msgs=[_M(A("mid"), "vol", 30.0), _M(A("mid"), "fade", 0.4, S), _M(A("mid"), "move", -3.0, 0.0, 2.0, S + F)]),
        # 5: a glide whose one-shot ends in a call with a move
        dict(name="gliding one-shot", kind="rs", ratio=1.0, loop=False, len=5000,
             msgs=[_M(A("first"), "rsp", 4, float(5000 - 3 * F)), _M(A("first"), "glide", 2.0, LONG)]),
        # 6: the reverse order: the move ends inside a block in mid-fade
        dict(name="move ends in mid-fade", kind="sp", vol=True, msgs=[_M(A("first"), "move", -5.0, 0.0, 0.5, S), _M(A("first"), "fade", 0.25, LONG)]),
        # 7: then = PAUSE, then play and a fade-in, all inside one long move
        dict(name="pause and fade-in in a move", kind="sp", vol=True,
             msgs=[_M(A("first"), "move", 2.0, 0.5, -2.0, LONG + 2 * F), _M(A("first"), "fade", 0.0, F // 2 + 3, PAUSE),
                   _M(A("first", 2), "fade", 0.0, 0), _M(A("first", 2), "play"), _M(A("first", 2), "fade", 1.0, F + F // 2)]),
        # 8: a one-shot that ends inside both a fade and a move
        dict(name="one-shot in fade and move", kind="sp", loop=False, len=shot, msgs=[_M(A("first"), "fade", 0.5, LONG), _M(A("first"), "move", 0.5, 1.0, 2.0, LONG)]),
        # 9: a resampler voice that never glides beside moving voices
        dict(name="steady resampler", kind="rs", ratio=1.3, msgs=[]),
        # 10: a retarget of the move while the fade runs
        dict(name="move retargeted in a fade", kind="sp", msgs=[_M(A("first"), "fade", 0.2, LONG), _M(A("first"), "move", 4.0, 0.0, -0.5, LONG),
                                                                 _M(A("first", 1), "move", -4.0, 0.3, -0.5, S)]),
        # 11: a set_position in mid-move while the fade runs: the move ends there, the smoothers take over
        dict(name="set_position in fade and move", kind="sp", vol=True, msgs=[_M(A("first"), "fade", 0.6, LONG), _M(A("first"), "move", 3.0, 0.0, 1.0, LONG),
                                                                               _M(A("first", 2), "set", -1.0, 0.0, -1.0)]),
        # 12: receives nothing
        dict(name="untouched", kind="sp", msgs=[]),
    ]


def chain_items(F, K):
    """plan 2.  `shape`: the stages behind the sampler (v volume, B biquad, D delay); a sweep names its biquad by position"""
    A = lambda where, plus=0, call=1: _at(K, call, where, plus)
    S, LONG = spans(F, K)
    shot = (2 if K == 1 else K + 1) * F + F // 3
    return [
        # 0: fade and sweep start in the same block; the fade ends inside a block while the sweep goes on
        dict(name="fade ends in mid-sweep", shape="vBDv", msgs=[_M(A("mid"), "fade", 0.3, S), _M(A("mid"), "sweep", 0, 6000.0, 3.0, LONG)]),
        # 1: ... and the sweep (of the second biquad) ends while the fade goes on
        dict(name="sweep ends in mid-fade", shape="BB", msgs=[_M(A("first"), "sweep", 1, 300.0, 2.0, S), _M(A("first"), "fade", 0.25, LONG)]),
        # 2: then = STOP in mid-sweep: the source is cleared, the sweep still reaches its target, the filter and the delay ring on
        dict(name="stop in mid-sweep", shape="BDv", msgs=[_M(A("first"), "sweep", 0, 7000.0, 3.0, LONG), _M(A("first", 1), "fade", 0.0, S - F, STOP)]),
        # 3, 4: a stream under a sweep, planar f32 and planar i16: a starved block, the end
        dict(name="f32 stream under a sweep", shape="vBDv", stream=PLANAR_F32, msgs=[_M(A("first"), "sweep", 0, 5000.0, 2.0, 3 * K * F + F // 2 + 7)]),
        dict(name="i16 stream under a sweep", shape="BB", stream=PLANAR_I16,
             msgs=[_M(A("first", call=0), "fade", 0.6, F // 2 + 3), _M(A("first"), "sweep", 0, 250.0, 4.0, 3 * K * F + F // 2 + 7),
                   _M(A("last"), "fade", 0.0, (2 * K + 1) * F + 9)]),
        # 5: a pause / play pair inside a sweep, with a fade-in
        dict(name="pause and fade-in in a sweep", shape="BDv",
             msgs=[_M(A("first"), "sweep", 0, 900.0, 5.0, LONG + 2 * F), _M(A("first", 1), "pause"),
                   _M(A("first", 2), "fade", 0.0, 0), _M(A("first", 2), "play"), _M(A("first", 2), "fade", 1.0, F + F // 2)]),
        # 6: a volume ramp between the two biquads during a sweep of the second
        dict(name="volume ramp between biquads", shape="BvB", msgs=[_M(A("mid"), "vol", 35.0), _M(A("mid"), "sweep", 1, 5000.0, 2.0, S + F)]),
        # 7: a one-shot ending inside a sweep and a fade
        dict(name="one-shot in fade and sweep", shape="BDv", loop=False, len=shot, msgs=[_M(A("first"), "fade", 0.5, LONG), _M(A("first"), "sweep", 0, 4000.0, 1.0, LONG)]),
        # 8: receives nothing
        dict(name="untouched", shape="vBDv", msgs=[]),
    ]


# ------------------------------------------------------------------------------------------------ graphs (any fwapi.Engine)
class Voice(object):
    def __init__(self, item):
        self.it, self.s, self.vol, self.sp, self.bqs, self.feed, self.end = item, None, None, None, [], None, None


def _sample(e, seed, frames, fmt=PLANAR_F32, ch=2):
    data = voice_source(8100 + seed, frames, ch)
    if fmt in (PLANAR_I16, INTERLEAVED_I16):
        data = np.round(data * 32767).astype(np.int16)
    return e.new_sample(fmt, ch, data.T.copy() if fmt == INTERLEAVED_I16 else data)


class Built(list):
    """the voices of a graph, with the tree above them: `top` (the mixer that feeds graph_out), `mixer` (the first leaf mixer) and
    `free_port` (its spare port, if one was asked for)"""


def _mix(e, ends, leaf, spare_port):
    """-> (top mixer, first leaf mixer, that mixer's first free port)"""
    mixers = []
    for i in range(0, len(ends), leaf):
        grp = ends[i:i + leaf]
        m = e.sum(max(2, len(grp) + (1 if spare_port and i == 0 else 0)))
        for p, n in enumerate(grp):
            e.connect_stereo(n, m, 2 * p)
        mixers.append(m)
    top = mixers[0]
    if len(mixers) > 1:
        top = e.sum(len(mixers))
        for p, m in enumerate(mixers):
            e.connect_stereo(m, top, 2 * p)
    return top, mixers[0], min(len(ends), leaf)


def _bank_voice(e, it, v, rng, fmt, ch):
    vo = Voice(it)
    pct, pan = float(rng.uniform(40, 100)), float(rng.uniform(-1, 1))
    if it["kind"] == "rs":
        vo.s = e.resampler(_sample(e, v, it.get("len", 3000 + 37 * v), fmt, ch), it["ratio"], loop=it.get("loop", True), n_out=2)
        vo.vol = e.volume(pct)
        e.connect_stereo(vo.s, vo.vol)
        vo.end = vo.vol
        if it.get("pan"):
            vo.end = e.pan(pan)
            e.connect_stereo(vo.vol, vo.end)
        return vo
    vo.s = e.sampler(float(rng.uniform(60, 100)))
    cur = vo.s
    if it.get("vol"):
        vo.vol = e.volume(pct)
        e.connect_stereo(cur, vo.vol)
        cur = vo.vol
    x, y, z = POS[v % len(POS)]
    vo.sp = vo.end = e.spatial(x, y, z, n_in=2)
    e.connect_stereo(cur, vo.sp)
    return vo


def chain_delays(F):
    """a voice's delay in frames, by voice index.  k_chain's tile is 128 frames when the block is whole 128-frame tiles AND every delay
    of the bank holds one (fwgpu_plan_install.cpp chain_nq_for), else 64: so blocks of 128 and 256 frames get the large-tile build by
    default, blocks of 64 the small one; SMALL_TILE_DELAYS at a block of 128 keeps the small tile there"""
    return (128, 129, 300) if F % 128 == 0 else SMALL_TILE_DELAYS


SMALL_TILE_DELAYS = (64, 129, 300)


def _chain_voice(e, it, v, rng, delays):
    vo = Voice(it)
    vo.s = e.sampler(85.0)
    cur = vo.s
    for t in it["shape"]:
        if t == "B":
            n = e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 6000)), float(rng.choice([0.707, 2.0, 5.0])))
            vo.bqs.append(n)
        elif t == "D":
            n = e.delay(delays[v % len(delays)] / float(SR), feedback=float(rng.choice([0.0, 0.45])), mix=0.5)
        else:
            n = e.volume(float(rng.uniform(40, 100)))
            vo.vol = n if vo.vol is None else vo.vol         # (the "vol" message goes to the shape's first volume)
        e.connect_stereo(cur, n)
        cur = n
    vo.end = cur
    return vo


def _start(e, vo, v, F, K, fmt, ch):
    """the sampler's source: a stream of stream_plan's frames, or a sample (a loop unless the item says otherwise)"""
    it = vo.it
    if it.get("kind") == "rs":
        return
    if it.get("stream") is not None:
        sf = fmt if it["stream"] is True else it["stream"]            # (True: the bank's format)
        total, _ = stream_plan(F, K)
        vo.feed = t_stream.Feed(e, vo.s, sf, ch, ring_frames(F, K), t_stream.rows_for(sf, ch, total, 900 + v))
    else:
        e.sampler_set_sample(vo.s, _sample(e, v, it.get("len", 3000 + 37 * v), fmt, ch))
        if it.get("loop", True):
            e.sampler_set_loop_range(vo.s, LOOP_FULL)
    e.sampler_play(vo.s)


def build(e, plan, F, K, n_voices, fmt=PLANAR_F32, ch=2, with_rs=True, spare_port=False, update=True, items=None, delays=None):
    """`n_voices` voices of the plan's items under SumNodes of LEAF ports -> graph_out (update=False: -> nothing yet; the caller wires
    the top mixer).  Returns Built([Voice])."""
    items = items or (bank_items(F, K) if plan == "bank" else chain_items(F, K))
    if not with_rs:
        items = [it for it in items if it.get("kind") != "rs"]
    rng = np.random.default_rng(1234)
    delays = delays or chain_delays(F)
    voices = Built(_bank_voice(e, items[v % len(items)], v, rng, fmt, ch) if plan == "bank" else _chain_voice(e, items[v % len(items)], v, rng, delays)
                   for v in range(n_voices))
    voices.top, voices.mixer, voices.free_port = _mix(e, [vo.end for vo in voices], LEAF, spare_port)
    if update:
        e.connect_stereo(voices.top, e.graph_out_node)
        e.update()
        start(e, voices, F, K, fmt, ch)
    return voices


def start(e, voices, F, K, fmt=PLANAR_F32, ch=2, first=0):
    for v, vo in enumerate(voices):
        _start(e, vo, first + v, F, K, fmt, ch)


def send(e, vo, what, args, at):
    if what == "fade":
        e.fade(vo.s, args[0], args[1], args[2] if len(args) > 2 else NONE, at_block=at)
    elif what == "move":
        e.move(vo.sp, args[0], args[1], args[2], args[3], at_block=at)
    elif what == "set":
        set_position(e, vo.sp, args[0], args[1], args[2], at_block=at)
    elif what == "vol":
        e.set_param(vo.vol, 0, args[0], at_block=at)
    elif what == "glide":
        e.glide(vo.s, args[0], args[1], at_block=at)
    elif what == "rsp":
        e.set_param(vo.s, args[0], args[1], at_block=at)
    elif what == "sweep":
        e.sweep(vo.bqs[args[0]], args[1], args[2], args[3], at_block=at)
    elif what in ("play", "pause", "stop"):
        getattr(e, "sampler_" + what)(vo.s, at_block=at)
    else:
        raise ValueError(what)


def feed_step(vo, call, F, K, strict=True):
    """the scripted writer of a streamed voice, in front of call `call` (strict=False: on the host-only harness, where nothing plays and
    a ring fills up)"""
    W = stream_plan(F, K)[1]
    if vo.feed is None or call >= len(W):
        return
    n = W[call] - vo.feed.pos
    assert n <= 0 or vo.feed.write(n) == n or not strict, (call, n)
    if call == len(W) - 1:
        assert vo.feed.end() or not strict


def feed_ahead(vo, F):
    """the writer where the calls are not the script's (ragged calls, the seeded family): all that fits beside the end's padding, from
    the consumed count both the model and the product report; behind the last frame, the end"""
    f = vo.feed
    if f is None or f.ended:
        return
    n = min(len(f.rows) - f.pos, f.R - F - (f.pos - f.status()[1]))
    assert n <= 0 or f.write(n) == n, n
    if f.pos == len(f.rows):
        assert f.end()


def run_script(e, plan, F, K, n_voices, n_calls=N_CALLS, calls=None, flags=False, **kw):
    """-> samples (flags: (samples, silence flags per block)); calls: frames per call (ragged calls: messages at the first block)"""
    voices = build(e, plan, F, K, n_voices, **kw)
    outs, fls = [], []
    for call in range(n_calls):
        for vo in voices:
            feed_step(vo, call, F, K) if calls is None else feed_ahead(vo, F)
            for c, at, what, args in vo.it["msgs"]:
                if c == call:
                    send(e, vo, what, args, at if calls is None else 0)
        if flags:
            o, f = e.process_blocks_flags(K)
            fls.append(np.asarray(f, dtype=bool))
        else:
            o = e.process_blocks(K) if calls is None else e.process_interleaved(calls[call])
        outs.append(np.asarray(o))
    return (np.concatenate(outs), np.concatenate(fls)) if flags else np.concatenate(outs)


_refs = {}


def reference(plan, F, K, n_voices, n_calls=N_CALLS, calls=None, flags=False, **kw):
    key = (plan, F, K, n_voices, n_calls, None if calls is None else tuple(calls), flags, tuple(sorted(kw.items())))
    if key not in _refs:
        out = run_script(model(F), plan, F, K, n_voices, n_calls, calls, flags, **kw)
        for a in (out if flags else (out,)):
            a.setflags(write=False)
        assert np.any((out[0] if flags else out) != 0)
        _refs[key] = out
    return _refs[key]


def gpu(F, K=None, **kw):
    g = GpuEngine(max_block_frames=F, **(dict(kw, max_batch=K) if K else kw))
    return g, rm.GpuRamps(g)


# ================================================================================================ CPU tier: the script is not vacuous
FK = [(F, K) for F in (64, 128, 256) for K in (1, 3, 5)]
COMBOS = [(64, 3, 37), (128, 5, 5), (256, 1, 37), (64, 5, 5), (256, 3, 5), (128, 1, 5)]           # F, K, voices of the GPU tier
BANK_PAIRS = [("fade", "move"), ("vol", "move"), ("vol", "fade"), ("stream", "move"), ("stream", "fade"), ("glide", "move beside")]
CHAIN_PAIRS = [("fade", "sweep"), ("stream", "sweep"), ("vol", "sweep"), ("stream", "fade")]


def _in_flight(e, vo, voices, v):
    """the features in flight on voice v, from the model's state behind a block"""
    n = e.nodes
    s = n[vo.s]
    on = set()
    if vo.it.get("kind") == "rs":
        if s.left > 0:
            on.add("glide")
        if any(0 <= w < len(voices) and voices[w].sp is not None and n[voices[w].sp].N > 0 for w in (v - 1, v + 1)):
            on.add("move beside")
        return on
    if s.env.N > 0:
        on.add("fade")
    if s.stream is not None and not s.finished:
        on.add("stream")
    if vo.sp is not None and n[vo.sp].N > 0:
        on.add("move")
    if vo.vol is not None and n[vo.vol].smoother.status != refmodel.INACTIVE:
        on.add("vol")
    if any(n[b].sw.N > 0 for b in vo.bqs):
        on.add("sweep")
    return on


RAMPS = ("fade", "move", "glide", "sweep")           # their last argument (the fade's second) is the ramp's frames: 0 is a step


def trace(plan, F, K):
    """the script through the model ONE block per call, each message in front of its block (which is what `Tagged` does with at_block):
    -> (samples, per voice and block: (in flight in the block, still in flight behind it), the voices, the model)"""
    m = model(F)
    e = m.e
    n_items = len(bank_items(F, K) if plan == "bank" else chain_items(F, K))
    voices = build(m, plan, F, K, n_items)
    outs, rows = [], [[] for _ in voices]
    # (a stream is bound in front of block 0: the sampler hears of it at the top of that block)
    behind = [_in_flight(e, vo, voices, v) | ({"stream"} if vo.feed is not None else set()) for v, vo in enumerate(voices)]
    for call in range(N_CALLS):
        for vo in voices:
            feed_step(vo, call, F, K)
        for b in range(K):
            started = [set() for _ in voices]
            for v, vo in enumerate(voices):
                for c, at, what, args in vo.it["msgs"]:
                    if (c, at) == (call, b):
                        send(m, vo, what, args, 0)
                        if what == "vol" or (what in RAMPS and args[1 if what == "fade" else -1] != 0):
                            started[v].add(what)
            for v, vo in enumerate(voices):          # a neighbour's move that starts in this block
                if vo.it.get("kind") == "rs" and any(0 <= w < len(voices) and "move" in started[w] for w in (v - 1, v + 1)):
                    started[v].add("move beside")
            outs.append(np.asarray(m.process_blocks(1)))
            for v, vo in enumerate(voices):
                now = _in_flight(e, vo, voices, v)
                rows[v].append((behind[v] | started[v], now))
                behind[v] = now
    return np.concatenate(outs), rows, voices, m


def overlap(rows, K, x, y):
    """over every voice: (blocks with x and y both in flight, blocks in which one of them ends while the other goes on, call boundaries
    crossed with both in flight)"""
    both = one_ends = crossed = 0
    for r in rows:
        for b, (during, behind) in enumerate(r):
            if x in during and y in during:
                both += 1
                one_ends += (x in behind) != (y in behind)
                crossed += (b + 1) % K == 0 and b + 1 < len(r) and x in behind and y in behind
    return both, one_ends, crossed


@pytest.mark.parametrize("F,K", FK)
@pytest.mark.parametrize("plan", ["bank", "chain"])
def test_the_script_holds_every_pair_of_features_in_flight_together(plan, F, K):
    out, rows, voices, m = trace(plan, F, K)
    V = len(voices)
    assert_bits(out, reference(plan, F, K, V), "one block per call = K blocks per call")     # K = 1 and K > 1 meet the same edges
    for x, y in (BANK_PAIRS if plan == "bank" else CHAIN_PAIRS):
        both, one_ends, crossed = overlap(rows, K, x, y)
        assert both >= 3 and one_ends >= 1 and crossed >= 1, (plan, F, K, x, y, both, one_ends, crossed)
    for vo in voices:
        if vo.feed is not None:                      # one starved block, the end reached
            assert vo.feed.status()[2:] == (1, True), (vo.it["name"], vo.feed.status())
    if plan == "bank":
        wide = [vo for vo in voices if vo.it["name"] == "stop in a wide move"][0]
        assert refmodel.spatial_params(-6.0, 0.0, 0.0, SR)[2:] == (0, t_move.ITD) or refmodel.spatial_params(-6.0, 0.0, 0.0, SR)[2:] == (t_move.ITD, 0)
        assert refmodel.spatial_params(6.0, 0.0, 0.0, SR)[2:] == refmodel.spatial_params(-6.0, 0.0, 0.0, SR)[2:][::-1]
        assert not m.e.nodes[wide.s].playing                                          # the fade's STOP has fired


def _stop_in_a_wide_move(e, F, K):
    """the item alone under the mixer -> (samples, silence flags of the graph output per block)"""
    items = [it for it in bank_items(F, K) if it["name"] == "stop in a wide move"]
    return run_script(e, "bank", F, K, 1, flags=True, items=items)


def test_model_the_stop_inside_a_wide_move_plays_the_spatialisers_tail_out():
    """the fade reaches 0.0 inside a block, which is rendered whole (env = 0.0 behind the fade's last frame), then STOP; the spatialiser
    plays its history out under the move's per-frame delays — up to 32 frames and a fraction — and goes on moving.  A spatialiser
    never flags its output (refmodel.SpatialNode, and tests/test_sp_move.py g9): the graph output stays unflagged and holds exact
    zeros once the tail has gone."""
    F, K = 64, 3
    out, fl = _stop_in_a_wide_move(model(F), F, K)
    S, _ = spans(F, K)
    stop_block = K + 1 + (S - F - 1) // F                   # the block in which the fade's last frame falls: rendered whole, then STOP
    o = out.reshape(-1, 2)
    assert not fl.any()
    r = stop_block * F + (S - F) % F                        # the first frame whose envelope is 0.0
    assert np.any(o[r - 8:r] != 0) and np.any(o[r + 1:r + 9] != 0), "the tail"
    assert np.all(o[r + t_move.ITD + 2:] == 0), "behind the tail"


# ================================================================================================ CPU tier: the planner on the harness
def _move_book(e):
    out = (ULL * 3)()
    t_move.peek().spp_move_book(e.cx.c, out)
    return list(out)                                  # frames done, the bound, live


def _sweep_book(e):
    out = (ULL * 3)()
    t_sweep._peek_lib().bsp_sweep_book(e.cx.c, out)
    return list(out)


def _calls(e, n, K, before=None):
    """n calls of K blocks -> per call (launches by kind, move book, sweep book, lazy stats)"""
    rows = []
    for call in range(n):
        if before:
            before(call)
        a = e.launches()
        e.process_blocks(K)
        b = e.launches()
        rows.append(({k: b[k] - a[k] for k in b}, _move_book(e), _sweep_book(e), e.cx.lazy_stats()))
    report = e.violation()
    fwapi.hostonly_lib().fwh_violation_reset()
    assert report == "", report
    return rows


QUIET = [dict(name="rs", kind="rs", ratio=0.9, msgs=[]), dict(name="sp", kind="sp", msgs=[]), dict(name="sp vol", kind="sp", vol=True, msgs=[])]


def test_planner_a_mixed_bank_with_one_move_launches_what_its_twin_launches_and_opens_the_move_book_for_the_moves_calls():
    F, K = 64, 4

    def run(move):
        e = rm.GpuRamps(HostOnlyEngine(max_block_frames=F, max_batch=K))
        vs = build(e, "bank", F, K, 7, items=QUIET)
        assert e.cx.plan_kind() == 1 and e.cx.plan_fused_voices() == 7
        e.process_blocks(K)
        e.reset_launches()
        N = 2 * K * F + 9                                           # from block 1 of call 1 through call 2 and into call 3
        return _calls(e, 6, K, lambda call: move and call == 1 and e.move(vs[1].sp, 4.0, 0.0, -0.5, N, at_block=1))

    moved, still = run(True), run(False)
    assert [r[0] for r in moved] == [r[0] for r in still]
    assert [r[1][2] for r in moved] == [0, 1, 1, 1, 0, 0] and all(r[1][2] == 0 for r in still), moved
    assert all(r[0]["voice_control"] == 1 and r[0]["leaf_sum"] == 1 for r in moved), moved


def _refused(e, F):
    """sampler -> spatialiser -> biquad (a refused shape) twice, under a SumNode"""
    out = []
    m = e.sum(2)
    for v in range(2):
        s = e.sampler(80.0)
        sp = e.spatial(*POS[v], n_in=2)
        bq = e.biquad(0, 900.0 + 700 * v, 2.0)
        e.connect_stereo(s, sp)
        e.connect_stereo(sp, bq)
        e.connect_stereo(bq, m, 2 * v)
        out.append((s, sp, bq))
    e.connect_stereo(m, e.graph_out_node)
    e.update()
    for v, (s, _, _) in enumerate(out):
        e.sampler_set_sample(s, _sample(e, 70 + v, 3000 + 11 * v))
        e.sampler_set_loop_range(s, LOOP_FULL)
        e.sampler_play(s)
    return out


def test_planner_a_sweep_and_a_move_overlap_in_level_executor_calls_and_each_book_closes_at_its_own_bound():
    F, K = 64, 4

    def run(msgs):
        e = rm.GpuRamps(HostOnlyEngine(max_block_frames=F, max_batch=K, force_generic=True))
        vs = _refused(e, F)
        assert e.cx.plan_kind() == 0
        e.process_blocks(K)
        e.reset_launches()

        def before(call):
            if msgs and call == 1:
                e.sweep(vs[0][2], 6000.0, 3.0, K * F + 5, at_block=2)          # ends 5 frames into block 2 of call 2
            if msgs and call == 2:
                e.move(vs[0][1], 4.0, 0.0, -0.5, 2 * K * F - 7, at_block=1)    # from block 1 of call 2 to the last block of call 4
        return _calls(e, 7, K, before)

    both, still = run(True), run(False)
    assert [r[0] for r in both] == [r[0] for r in still]
    assert [r[2][2] for r in both] == [0, 1, 1, 0, 0, 0, 0], both               # the sweep: calls 1 and 2
    assert [r[1][2] for r in both] == [0, 0, 1, 1, 1, 0, 0], both               # the move: calls 2, 3 and 4; call 2 has both
    done = lambda call: (call + 1) * K * F                                      # (one call ran before the count)
    assert both[2][2][1] == done(1) + 2 * F + K * F + 5 and both[4][1][1] == done(2) + F + 2 * K * F - 7


def test_planner_on_a_chain_bank_a_call_inside_a_fade_and_a_sweep_runs_one_control_batch_and_lazy_calls_resume_behind_the_later_one():
    F, K, V = 64, 4, 6

    def run(e, behind_call):
        vs = build(e, "chain", F, K, V, items=[dict(name="q", shape="BDv", len=8 * F, msgs=[])])      # loops of whole blocks: lazy-capable
        rows = []
        for call in range(12):
            if call == 3:
                e.fade(vs[1].s, 0.3, 2 * K * F + 9, at_block=1)                 # ends in call 5 ...
                e.sweep(vs[1].bqs[0], 5000.0, 2.0, 3 * K * F + 5, at_block=2)   # ... the sweep in call 6
            e.process_blocks(K)
            rows.append(behind_call(e, vs[1]))
        return rows

    # from the model: behind which call is each ramp still in flight?
    m = model(F)
    going = run(m, lambda e, vo: (m.e.nodes[vo.s].env.N > 0, m.e.nodes[vo.bqs[0]].sw.N > 0))
    last_fade = max(c for c in range(12) if going[c][0]) + 1                     # the call in which it ends
    last_sweep = max(c for c in range(12) if going[c][1]) + 1
    assert (last_fade, last_sweep) == (5, 6), going
    e = rm.GpuRamps(HostOnlyEngine(max_block_frames=F, max_batch=K))
    rows = run(e, lambda e, vo: e.cx.lazy_stats())
    assert e.cx.plan_kind() == 2 and e.violation() == ""
    if os.environ.get("FWGPU_LAZY") == "0":
        return
    lazy, ctl = [r[0] for r in rows], [r[1] for r in rows]
    later = max(last_fade, last_sweep)
    assert lazy[2] > lazy[0], rows                                               # quiet calls in front are lazy
    assert lazy[later] == lazy[2] and ctl[later] - ctl[2] == later - 2, rows     # one control batch per call from the messages to the later end
    assert lazy[11] - lazy[later + 1] == 11 - later - 1 and ctl[11] == ctl[later + 1], rows    # ... and lazy again behind it


# ================================================================================================ GPU tier
SMALL = [(64, 3, 37), (128, 1, 5)]


def _rendered_both(e, F):
    """sampler -> spatialiser -> biquad voices (a refused shape) through two calls with a sweep and a move live in the same blocks"""
    vs = _refused(e, F)
    outs = [np.asarray(e.process_blocks(3))]
    for v, (s, sp, bq) in enumerate(vs):
        e.move(sp, 4.0 - 8 * v, 0.0, -0.5, 4 * F + 9, at_block=1)
        e.sweep(bq, 6000.0, 3.0, 3 * F + 5, at_block=1 + v)
        e.fade(s, 0.3, 2 * F + 1, at_block=v)
    for _ in range(3):
        outs.append(np.asarray(e.process_blocks(3)))
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", COMBOS)
@pytest.mark.parametrize("plan", ["bank", "chain"])
def test_g1_level_executor(plan, F, K, V):
    g, e = gpu(F, K, force_generic=True)
    got = run_script(e, plan, F, K, V)
    assert g.cx.plan_kind() == 0
    assert_bits(got, reference(plan, F, K, V), "level executor, " + plan)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 256])
def test_g1_one_level_launch_renders_a_sweeping_biquad_behind_a_moving_spatialiser(F):
    """k_level<1, true> with no_walkers set: both host bounds live in one call"""
    g, e = gpu(F, 3, force_generic=True)
    got = _rendered_both(e, F)
    assert g.cx.plan_kind() == 0
    assert_bits(got, _rendered_both(model(F), F), "sampler -> spatialiser -> biquad")


_books = {}


def host_move_book(F, K, V, with_rs):
    """per call of the bank script: is the host's move book live?  Read on the host-only harness — the same host code given the same
    graph and the same calls; the book is a function of the messages and the frames done, and nothing of the device's — because the
    library has no call that reports it.  -> (plan kind, fused voices, [live per call])"""
    key = (F, K, V, with_rs)
    if key not in _books:
        e = rm.GpuRamps(HostOnlyEngine(max_block_frames=F, max_batch=K))
        voices = build(e, "bank", F, K, V, with_rs=with_rs)
        live = []
        for call in range(N_CALLS):
            for vo in voices:
                feed_step(vo, call, F, K, strict=False)
                for c, at, what, args in vo.it["msgs"]:
                    if c == call:
                        send(e, vo, what, args, at)
            e.process_blocks(K)
            live.append(_move_book(e)[2])
        report = e.violation()
        fwapi.hostonly_lib().fwh_violation_reset()
        assert report == "", report
        _books[key] = (e.cx.plan_kind(), e.cx.plan_fused_voices(), live)
    return _books[key]


@pytest.mark.parametrize("with_rs", [True, False])
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_planner_the_bank_script_opens_the_move_book_in_its_message_calls(F, K, V, with_rs):
    kind, fused, live = host_move_book(F, K, V, with_rs)
    assert (kind, fused) == (1, V) and live[0] == 0 and live[1:4] == [1, 1, 1], (kind, fused, live)


@pytest.mark.gpu
@pytest.mark.parametrize("with_rs", [True, False])
@pytest.mark.parametrize("F,K,V", COMBOS)
def test_g2_fused_mixed_bank(F, K, V, with_rs):
    """launch_leaf_sum picks k_leaf_sum_rs_sp_spm when the plan is the voice bank, the bank holds resampler voices and spatialiser voices
    and a move may be live: the assertions in front of the comparison are those conditions, so a planner change that drops one of them
    fails here (with_rs = False: k_leaf_sum_sp_spm, with fades in its stage-0 ramp rows)"""
    g, e = gpu(F, K)
    voices = build(e, "bank", F, K, V, with_rs=with_rs)
    assert g.cx.plan_kind() == 1 and g.cx.plan_fused_voices() == V
    kinds = [vo.it["kind"] for vo in voices]
    assert "sp" in kinds and ("rs" in kinds) == with_rs
    kind, fused, live = host_move_book(F, K, V, with_rs)
    assert (kind, fused) == (1, V) and live[1:4] == [1, 1, 1], live            # the move book is live in the message calls
    outs = []
    for call in range(N_CALLS):
        for vo in voices:
            feed_step(vo, call, F, K)
            for c, at, what, args in vo.it["msgs"]:
                if c == call:
                    send(e, vo, what, args, at)
        outs.append(np.asarray(e.process_blocks(K)))
    assert_bits(np.concatenate(outs), reference("bank", F, K, V, with_rs=with_rs), "voice bank")


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_g2_the_stop_inside_a_wide_move_sample_for_sample_and_flag_for_flag(force_generic):
    F, K = 64, 3
    want, wf = _stop_in_a_wide_move(model(F), F, K)
    g, e = gpu(F, K, force_generic=force_generic)
    got, gf = _stop_in_a_wide_move(e, F, K)
    assert g.cx.plan_kind() == (0 if force_generic else 1)
    assert np.array_equal(gf, wf), (gf.T, wf.T)
    assert_bits(got, want, "stop in a wide move")


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", SMALL)
@pytest.mark.parametrize("fmt,ch", [(PLANAR_I16, 2), (PLANAR_F32, 1), (PLANAR_I16, 1)])
def test_g3_bank_source_formats(fmt, ch, F, K, V):
    g, e = gpu(F, K)
    got = run_script(e, "bank", F, K, V, fmt=fmt, ch=ch)
    assert g.cx.plan_kind() == 1
    assert_bits(got, reference("bank", F, K, V, fmt=fmt, ch=ch), "format %d, %d channel(s)" % (fmt, ch))


# F, K, voices, delays (None: chain_delays(F)), k_chain's tile in units of 64 frames
CHAIN_CASES = [(64, 3, 37, None, 1), (64, 1, 5, None, 1), (128, 5, 5, None, 2), (128, 3, 37, None, 2), (128, 3, 37, SMALL_TILE_DELAYS, 1), (256, 1, 5, None, 2)]
_nqs = {}


def host_chain_nq(F, K, V, delays):
    """the k_chain instantiation the planner picks for the chain script's bank (PlanImage::chain_nq: bits 0..1 the tile, bit 2 a second
    recurrence stage, bit 3 the five-site stage logic), read on the host-only harness — the same planner given the same graph —
    because the library has no call that reports it.  -> (plan kind, fused voices, chain_nq)"""
    key = (F, K, V, delays)
    if key not in _nqs:
        P = fwapi.peek_lib("ramps_peek", {"rmp_chain_nq": (C.c_int, [C.c_void_p])})
        e = rm.GpuRamps(HostOnlyEngine(max_block_frames=F, max_batch=K))
        build(e, "chain", F, K, V, delays=delays)
        e.process_blocks(K)
        report = e.violation()
        fwapi.hostonly_lib().fwh_violation_reset()
        assert report == "", report
        _nqs[key] = (e.cx.plan_kind(), e.cx.plan_fused_voices(), int(P.rmp_chain_nq(e.cx.c)))
    return _nqs[key]


@pytest.mark.parametrize("F,K,V,delays,tile", CHAIN_CASES)
def test_planner_the_chain_script_takes_the_tile_its_case_names(F, K, V, delays, tile):
    assert "FWGPU_CHAIN_NQ" not in os.environ                     # (the switch that forces the small tile)
    kind, fused, nq = host_chain_nq(F, K, V, delays)
    assert (kind, fused, nq & 3) == (2, V, tile), (kind, fused, nq)
    assert nq & 4                                                 # "BB" voices: the second recurrence stage
    assert bool(nq & 8) == (V > 6)                                # "BvB" (item 6): the site logic, with ramp rows live in the script


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [PLANAR_F32, INTERLEAVED_I16])
@pytest.mark.parametrize("F,K,V,delays,tile", CHAIN_CASES)
def test_g4_chain_plan(F, K, V, delays, tile, fmt):
    """both k_chain tiles: 128 frames where the block is whole 128-frame tiles and every delay holds one, else 64 (a 64-frame delay in
    a bank at a block of 128 keeps the small tile there: the twin of the large-tile case).  The tile is asserted, from the planner on
    the host-only harness, so a change of the delays or of the planner's rule that drops a tile fails here."""
    kind, fused, nq = host_chain_nq(F, K, V, delays)
    assert (kind, fused, nq & 3) == (2, V, tile), (kind, fused, nq)
    g, e = gpu(F, K)
    got = run_script(e, "chain", F, K, V, fmt=fmt, delays=delays)
    assert g.cx.plan_kind() == 2 and g.cx.plan_fused_voices() == V
    assert_bits(got, reference("chain", F, K, V, fmt=fmt, delays=delays), "chain plan, format %d, tile %d" % (fmt, 64 * tile))


def run_hybrid(e, F, K, V):
    """the bank and the chain bank under one master SumNode -> biquad -> volume -> graph_out; the master biquad sweeps (and the master
    volume ramps) while the voices below fade, move, glide, sweep and stream"""
    bank = build(e, "bank", F, K, V, update=False)
    chain = build(e, "chain", F, K, V, update=False)
    master = e.sum(2)
    e.connect_stereo(bank.top, master, 0)
    e.connect_stereo(chain.top, master, 2)
    bq = e.biquad(0, 2500.0, 1.5)
    vol = e.volume(80.0)
    e.connect_stereo(master, bq)
    e.connect_stereo(bq, vol)
    e.connect_stereo(vol, e.graph_out_node)
    e.update()
    start(e, bank, F, K)
    start(e, chain, F, K, first=100)
    S, LONG = spans(F, K)
    outs = []
    for call in range(N_CALLS):
        if call == 1:
            e.sweep(bq, 400.0, 4.0, LONG + K * F, at_block=K // 2)
            e.set_param(vol, 0, 45.0, at_block=K - 1)
        for vo in bank + chain:
            feed_step(vo, call, F, K)
            for c, at, what, args in vo.it["msgs"]:
                if c == call:
                    send(e, vo, what, args, at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("F,K,V", [(64, 3, 37), (128, 1, 5), (256, 5, 5)])
def test_g5_hybrid(F, K, V):
    key = ("hybrid", F, K, V)
    if key not in _refs:
        _refs[key] = run_hybrid(model(F), F, K, V)
        _refs[key].setflags(write=False)
    g, e = gpu(F, K)
    got = run_hybrid(e, F, K, V)
    assert g.cx.plan_kind() == 3
    assert_bits(got, _refs[key], "hybrid")


@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 256])
@pytest.mark.parametrize("plan", ["bank", "chain"])
def test_g6_one_block_calls(plan, F):
    """K = 1 with the default max_batch: the realtime launch sequence"""
    V, calls = 37, 12
    g, e = gpu(F)
    got = run_script(e, plan, F, 1, V, n_calls=calls)
    assert g.cx.plan_kind() == (1 if plan == "bank" else 2)
    assert_bits(got, reference(plan, F, 1, V, n_calls=calls), "one-block calls")


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
@pytest.mark.parametrize("F", [40, 64])
@pytest.mark.parametrize("plan", ["bank", "chain"])
def test_g7_ragged_calls(plan, F, force_generic):
    """the short tail block changes owner with two ramps in flight; the two host bounds over-estimate (a short block counts as a whole
    one): that costs kernels, never bits"""
    calls = busnodes.ragged_calls(F, at_least=20 * F)
    g, e = gpu(F, 5, force_generic=force_generic)
    got = run_script(e, plan, F, 5, 13, n_calls=len(calls), calls=calls)
    assert_bits(got, reference(plan, F, 5, 13, n_calls=len(calls), calls=calls), "ragged calls")


def run_install(e, plan, F, K):
    """one more voice on the first mixer's free port while the script's ramps are in flight"""
    V = 13
    voices = build(e, plan, F, K, V, spare_port=True)
    items = bank_items(F, K) if plan == "bank" else chain_items(F, K)
    outs = []
    for call in range(N_CALLS):
        if call == 2:
            rng = np.random.default_rng(5)
            vo = _bank_voice(e, items[0], 3, rng, PLANAR_F32, 2) if plan == "bank" else _chain_voice(e, items[0], 3, rng, chain_delays(F))
            e.connect_stereo(vo.end, voices.mixer, 2 * voices.free_port)
            e.update()
            _start(e, vo, 77, F, K, PLANAR_F32, 2)
            send(e, vo, "fade", (0.5, 3 * F + 1), K - 1)
        for vo in voices:
            feed_step(vo, call, F, K)
            for c, at, what, args in vo.it["msgs"]:
                if c == call:
                    send(e, vo, what, args, at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
@pytest.mark.parametrize("plan", ["bank", "chain"])
def test_g8_every_ramp_carries_over_a_plan_install(plan, force_generic):
    F, K = 64, 3
    key = ("install", plan)
    if key not in _refs:
        _refs[key] = run_install(model(F), plan, F, K)
        _refs[key].setflags(write=False)
    g, e = gpu(F, K, force_generic=force_generic)
    got = run_install(e, plan, F, K)
    assert g.cx.plan_kind() == (0 if force_generic else (1 if plan == "bank" else 2))
    assert_bits(got, _refs[key], "a plan install in mid-flight")


def _plain_bank(e, F, V):
    """sampler -> volume voices under one SumNode: loops of whole blocks, so the bank is lazy-capable (as test_sampler_fade.py g8's)"""
    vs = Built()
    for v in range(V):
        vo = Voice(dict(msgs=[]))
        vo.s = e.sampler(80.0)
        vo.vol = vo.end = e.volume(60.0 + v)
        e.connect_stereo(vo.s, vo.vol)
        vs.append(vo)
    vs.top = vs.mixer = e.sum(V)
    for p, vo in enumerate(vs):
        e.connect_stereo(vo.end, vs.top, 2 * p)
    e.connect_stereo(vs.top, e.graph_out_node)
    e.update()
    for v, vo in enumerate(vs):
        e.sampler_set_sample(vo.s, _sample(e, 300 + v, 80 * F))
        e.sampler_set_loop_range(vo.s, LOOP_FULL)
        e.sampler_play(vo.s)
    return vs


def run_accounting(e, plan, F, K):
    """two kinds of ramp in the calls 4 to 6 — bank: fades, and a stream that voice 5 is handed in front of call 4 (9 blocks and 5 frames,
    written and ended at once: it finishes in call 6, and a voice that holds a stream is never steady); chain: fades and sweeps, in
    one voice and in two.  -> (samples, lazy stats behind each call, the stream's status at the end)"""
    V = 12
    vs = _plain_bank(e, F, V) if plan == "bank" else build(e, "chain", F, K, V, items=[dict(name="q", shape="BDv", len=8 * F, msgs=[])])
    outs, marks = [], []
    for call in range(12):
        if call == 4:
            e.fade(vs[0].s, 0.25, 5 * F + 3, at_block=1)                       # ends in call 5
            if plan == "bank":
                feed = vs[5].feed = t_stream.Feed(e, vs[5].s, PLANAR_F32, 2, 12 * F, t_stream.rows_for(PLANAR_F32, 2, 9 * F + 5, 77))
                assert feed.write(9 * F + 5) == 9 * F + 5 and feed.end()       # ... the stream in call 6
                e.fade(vs[5].s, 0.5, 3 * F, at_block=1)                        # a fade on the streaming voice
            else:
                e.fade(vs[5].s, 0.5, 9 * F + 3, at_block=1)                    # ... in call 6
                e.sweep(vs[0].bqs[0], 6000.0, 3.0, 9 * F + 3, at_block=2)      # in the fading voice; ends in call 6
                e.sweep(vs[7].bqs[0], 300.0, 2.0, 3 * F, at_block=0)
        outs.append(np.asarray(e.process_blocks(K)))
        status = vs[5].feed.status() if vs[5].feed is not None else None          # (the control side sees `finished` when it looks)
        if hasattr(e, "cx"):
            marks.append(e.cx.lazy_stats())
    return np.concatenate(outs), marks, status


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["bank", "chain"])
def test_g9_lazy_calls_resume_behind_the_last_ramp(plan):
    """the counters are fwgpu_lazy_stats (launch batches without and with a control kernel).  The library exposes no counter for a
    voice's steady cache: that the voices which were sent nothing keep theirs is not read here — the evidence is that the calls are
    lazy again behind the last ramp (a lazy call has nothing but the per-voice records to render from) and that every call's mix is
    bit-equal to the model's."""
    F, K = 64, 4
    want, _, wst = run_accounting(model(F), plan, F, K)
    g, e = gpu(F, K)
    got, marks, st = run_accounting(e, plan, F, K)
    assert g.cx.plan_kind() == (1 if plan == "bank" else 2)
    assert_bits(got, want, "twelve calls")
    assert st == wst and (plan == "chain" or (st[2], st[3]) == (0, True)), (st, wst)      # no block starved, the stream finished
    if os.environ.get("FWGPU_LAZY") == "0":
        return
    lazy, ctl = [m[0] for m in marks], [m[1] for m in marks]
    assert lazy[3] > lazy[1], marks                                   # quiet calls in front are lazy
    assert lazy[6] == lazy[3] and ctl[6] - ctl[3] == 3, marks         # calls 4, 5 and 6: a ramp in flight or ending
    assert lazy[11] - lazy[7] == 4, marks                             # ... and lazy again behind the last one


def fuzz(e, plan, seed, F):
    rng = np.random.default_rng(53_000 + seed)
    V = 16
    K0 = 4
    quiet = [dict(it, msgs=[]) for it in (bank_items(F, K0) if plan == "bank" else chain_items(F, K0))]      # the voices; the messages are drawn
    for it in quiet:                                                  # (one-shots long enough to end somewhere inside the run)
        if it.get("len") and it.get("kind") != "rs":
            it["len"] = int(rng.integers(3, 9)) * F + 11
    voices = build(e, plan, F, K0, V, items=quiet)
    coord = lambda: float(rng.choice([-6.0, -1.5, -0.2, 0.0, 0.3, 2.0, 5.0]))
    length = lambda: int(rng.choice([0, 1, 3, F - 1, F, F + 1, 3 * F + 7, int(rng.integers(1, 8 * F))]))
    outs = []
    for call in range(6):
        K = int(rng.integers(1, K0 + 1))
        for vo in voices:
            if rng.random() < 0.8:                                    # (a writer that sometimes falls behind)
                feed_ahead(vo, F)
        msgs = []          # (at_block, call, arguments): a node's messages are sent in non-decreasing at_block order (include/fwgpu.h)
        for _ in range(int(rng.integers(0, 20))):
            vo, at = voices[int(rng.integers(0, len(voices)))], int(rng.integers(0, K))
            what = rng.random()
            rs = vo.it.get("kind") == "rs"
            if what < 0.25 and rs:
                msgs.append((at, e.glide, (vo.s, float(rng.choice([0.4, 0.9, 1.0, 1.7, 2.5])), length(),)))
            elif what < 0.32 and rs:
                msgs.append((at, e.set_param, (vo.s, 1, float(rng.choice([0.5, 1.1, 2.0])),)))
            elif rs:
                msgs.append((at, e.set_param, (vo.s, 3, float(rng.random() < 0.7),)))
            elif what < 0.3:
                N = length()
                then = int(rng.choice([NONE, NONE, PAUSE, STOP])) if N else NONE
                msgs.append((at, e.fade, (vo.s, float(rng.choice([0.0, 0.2, 0.7, 1.0])), N, then,)))
            elif what < 0.55 and vo.sp is not None:
                msgs.append((at, e.move, (vo.sp, coord(), coord(), coord(), length(),)))
            elif what < 0.65 and vo.sp is not None:
                msgs.append((at, set_position, (e, vo.sp, coord(), coord(), coord(),)))
            elif what < 0.65 and vo.bqs:
                msgs.append((at, e.sweep, (vo.bqs[int(rng.integers(0, len(vo.bqs)))], float(rng.choice([150.0, 900.0, 5000.0, 9000.0])), float(rng.choice([0.7, 2.0, 6.0])), length(),)))
            elif what < 0.72 and vo.bqs:
                msgs.append((at, e.set_param, (vo.bqs[0], 1, float(rng.choice([300.0, 2000.0])),)))
            elif what < 0.8 and vo.vol is not None:
                msgs.append((at, e.set_param, (vo.vol, 0, float(rng.choice([0.0, 25.0, 70.0, 100.0])),)))
            elif what < 0.9:
                msgs.append((at, e.sampler_pause, (vo.s,)))
            else:
                msgs.append((at, e.sampler_play, (vo.s,)))
        for at, fn, args in sorted(msgs, key=lambda m: m[0]):
            fn(*args, at_block=at)
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_g10_seeded_messages_of_all_five_kinds_on_both_plans(seed):
    F = [64, 128, 256, 64][seed % 4]
    plan = "bank" if seed % 2 == 0 else "chain"
    want = fuzz(model(F), plan, seed, F)
    got = []
    for force_generic in (False, True):
        g, e = gpu(F, 4, force_generic=force_generic)
        got.append(fuzz(e, plan, seed, F))
        assert g.cx.plan_kind() == (0 if force_generic else (1 if plan == "bank" else 2))
        assert_bits(got[-1], want, "seed %d, %s" % (seed, "level executor" if force_generic else "fused plan"))
    assert_bits(got[0], got[1], "seed %d, the two plans" % seed)
