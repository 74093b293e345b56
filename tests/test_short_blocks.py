"""Short blocks through sampler graphs: a process call whose length is no whole number of blocks ends in a
block of frames < max_block_frames.  The reference's sampler panics there (sampler.rs:435 assert_eq!(gain.values.len(), frames)) unless
its gain happens to be gliding; the product renders the block, from the first `frames` smoothed gain values.  Both CPU restatements
keep the assertion by default and drop it behind a per-engine switch (OracleEngine / RefEngine `short_blocks=True`).

CPU tier (this file):
* the relaxed oracle against the relaxed independent model, bit for bit, on 50 seeds of ragged call sequences through the six graphs
  below with messages tagged at random blocks — calls shorter than one block among them;
* stream invariance: for steady voices the relaxed oracle fed ragged calls produces the very stream the DEFAULT oracle produces in
  whole blocks.  That ties the switch to code that never ran with it: a short block computes what the assertion-keeping oracle computes
  for the same frames.

The graphs (one builder, `build`, also used by test_gpu_short_blocks.py — each is the smallest graph of its fused plan):
  bank     plain voice-bank plan: planar-f32 stereo, mono behind MonoToStereo and interleaved 16-bit sources in every leaf
  spatial  voice-bank plan with spatialiser voices beside dry ones
  rs       resampler-pure bank, ratios 0.5 0.8 1.0 1.25 1.93 2.5
  chain    chain plan: B, BD, DB, BBD with gain / pan / clip stages in front of, between and behind the filters; delays of exactly 64
           frames, of 129 and of more than a block, feedback 0 and 0.45
  hybrid   two banks, a send bus with a bus biquad, a master mixer that takes voices on its leading ports and buses behind them
  master   bank -> volume -> hard clip [-> 2->2 meter, product only] as the master chain
"""
import numpy as np
import pytest

import fwapi
import scenarios
from fwapi import INTERLEAVED_I16, LOOP_FULL, LOOP_NONE, LOOP_RANGE_SECS, PLANAR_F32, OracleEngine

METER = 16
GRAPHS = ("bank", "spatial", "rs", "chain", "hybrid", "master")
PLAN_KIND = dict(bank=1, spatial=1, rs=1, chain=2, hybrid=3, master=1)
SHAPES = dict(
    bank=["vp", "mvp", "v", "p", "", "vpc"] * 2,
    spatial=["vs", "s", "ps", "vp", "ws", "cs", "vs", "v", "s", "pvs"],
    rs=["rvp", "rv", "rp", "r", "rvp", "rpv"] * 2,
    chain=["B", "BD", "DB", "BBD", "vBcBD", "pBv", "DcBv", "BvD", "vBDv", "BDc"],
    master=["vp", "v", "", "pv", "vp", "v", "", "vp", "v"],
)
RADIX = dict(bank=6, spatial=5, rs=6, chain=5, master=3)
RATIOS = (0.5, 0.8, 1.0, 1.25, 1.93, 2.5)
DELAYS = (64, 300, 129, 700)  # frames: the shortest delay line there is, more than a block of 64 / 128, one frame over a chain tile


class Rig(object):
    """what `build` made: voices = [dict(kind 's' sampler | 'r' resampler, src, frames, ch, vols, pans, clips, bqs, dls, sp, end)]"""


def _sample(e, seed, frames, ch, fmt=PLANAR_F32):
    data = scenarios.voice_source(seed, frames, ch)
    if fmt == INTERLEAVED_I16:
        data = np.round(data * 32767).astype(np.int16).T.copy()
    return e.new_sample(fmt, ch, data)


def src_frames(i, mbf):
    """sources of 5 .. 12 blocks, never a whole number of them: loops wrap inside blocks, and sooner or later inside a short one"""
    return (5 + i % 7) * mbf + 17 + 13 * i


def _voice(e, shape, i, seed, mbf, frames, one_shot, planar=False, ratios=RATIOS):
    rng = np.random.default_rng(7000 + 97 * seed + i)
    vc = dict(kind="s", vols=[], pans=[], clips=[], bqs=[], dls=[], sp=None, loop=not one_shot, frames=frames, i=i)
    if shape.startswith("r"):
        vc["kind"], vc["ch"] = "r", 1 if i % 5 == 3 else 2
        vc["ratio"] = ratios[i % len(ratios)]
        smp = _sample(e, 1000 * seed + i, frames, vc["ch"], INTERLEAVED_I16 if (i % 4 == 1 and not planar) else PLANAR_F32)
        cur = vc["src"] = e.resampler(smp, vc["ratio"], loop=not one_shot, playing=True, n_out=2)
        shape = shape[1:]
    elif shape.startswith("m"):
        vc["ch"] = 1
        vc["src"] = e.sampler(100.0, n_out=1)
        cur = e.add_node(fwapi.MONO_TO_STEREO, 1, 2)
        e.connect(vc["src"], 0, cur, 0)
        shape = shape[1:]
    else:
        vc["ch"] = 2
        cur = vc["src"] = e.sampler(float(rng.uniform(60, 100)))
    n_dl = 0
    for t in shape:
        if t == "v":
            n = e.volume(float(rng.uniform(30, 100)))
            vc["vols"].append(n)
        elif t == "p":
            n = e.pan(float(rng.uniform(-1, 1)))
            vc["pans"].append(n)
        elif t == "c":
            n = e.hard_clip(-14.0)  # low enough to bite
            vc["clips"].append(n)
        elif t == "w":
            n = e.width(1.3)
        elif t == "B":
            n = e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 8000)), float(rng.choice([0.707, 1.8])))
            vc["bqs"].append(n)
        elif t == "D":
            n = e.delay(DELAYS[(i + n_dl) % len(DELAYS)] / float(e.sample_rate), feedback=0.45 if i % 3 else 0.0, mix=0.5)
            vc["dls"].append(n)
            n_dl += 1
        elif t == "s":
            n = e.spatial(float(rng.uniform(-5, 5)), float(rng.uniform(-1, 1)), float(rng.uniform(-5, 5)), n_in=2)
            vc["sp"] = n
        else:
            raise ValueError(t)
        e.connect_stereo(cur, n)
        cur = n
    vc["end"] = cur
    return vc


def build(e, graph, seed=0, meter=False, frames=None, one_shots=(), planar=False, ratios=RATIOS):
    """-> Rig.  frames: {voice index: source frames} overriding src_frames; one_shots: voice indices that do not loop; planar: resampling
    sources are planar f32, all of them; ratios: theirs, in turn.  Every source is set, looped (unless a one-shot) and started: the first process call carries those messages."""
    mbf = e.max_block_frames
    frames = frames or {}
    r = Rig()
    r.e, r.graph, r.meter, r.master_vol, r.bus_bq = e, graph, None, None, None

    def voices(shapes, first=0):
        return [_voice(e, sh, first + k, seed, mbf, frames.get(first + k, src_frames(first + k, mbf)), (first + k) in one_shots, planar, ratios) for k, sh in enumerate(shapes)]

    def mixer(ends, ports=None):
        m = e.sum(max(2, ports or len(ends)))
        for p, n in enumerate(ends):
            e.connect_stereo(n, m, 2 * p)
        return m

    if graph == "hybrid":
        a, b, lead = voices(["vp", "v", "mvp", "p", "vp"]), voices(["vpc", "vw", "vp", "cv"], 5), voices(["v", "vp"], 9)
        r.voices = a + b + lead
        sum_a, sum_b = mixer([v["end"] for v in a]), mixer([v["end"] for v in b])
        send = mixer([sum_a, sum_b])  # both banks' buses are consumed twice: dry into the master and through the send
        r.bus_bq = e.biquad(0, 2500.0)
        e.connect_stereo(send, r.bus_bq)
        root = mixer([v["end"] for v in lead] + [sum_a, sum_b, r.bus_bq])  # a split mixer: voices in front, buses behind
    else:
        r.voices = voices(SHAPES[graph])
        rad = RADIX[graph]
        leaves = [mixer([v["end"] for v in r.voices[k:k + rad]]) for k in range(0, len(r.voices), rad)]
        assert len(leaves) >= 2
        root = mixer(leaves)
    cur = root
    if graph == "master":
        r.master_vol = e.volume(85.0)
        clip = e.hard_clip(-9.0)
        e.connect_stereo(cur, r.master_vol)
        e.connect_stereo(r.master_vol, clip)
        cur = clip
        if meter:
            r.meter = e.add_node(METER, 2, 2, [64])
            e.connect_stereo(cur, r.meter)
            cur = r.meter
    e.connect_stereo(cur, e.graph_out_node)
    e.update()
    for vc in r.voices:
        if vc["kind"] == "s":
            fmt = INTERLEAVED_I16 if (vc["ch"] == 2 and vc["i"] % 3 == 2) else PLANAR_F32
            vc["sample"] = _sample(e, 1000 * seed + vc["i"], vc["frames"], vc["ch"], fmt)
            e.sampler_set_sample(vc["src"], vc["sample"])
            if vc["loop"]:
                e.sampler_set_loop_range(vc["src"], LOOP_FULL)
            e.sampler_play(vc["src"])
    r.samplers = [vc for vc in r.voices if vc["kind"] == "s"]
    r.resamplers = [vc for vc in r.voices if vc["kind"] == "r"]
    return r


def relaxed(mbf, model=False):
    if model:
        import refmodel

        return scenarios.TaggedOracle(refmodel.RefEngine(max_block_frames=mbf, short_blocks=True))
    return scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf, short_blocks=True))


def assert_calls_equal(want, got, what):
    """call by call, bit for bit; something must have sounded"""
    assert len(want) == len(got)
    off = 0
    for k, (a, b) in enumerate(zip(want, got)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        bad = np.nonzero(fwapi.bits(a) != fwapi.bits(b))[0]
        assert bad.size == 0, "%s: call %d (%d frames, stream frame %d): %d of %d samples differ, first at frame %d: %r vs %r" % (
            what, k, a.size // 2, off, bad.size, a.size, bad[0] // 2, a[bad[0]], b[bad[0]])
        off += a.size // 2
    assert any(np.any(np.asarray(a) != 0) for a in want), what + ": nothing sounded"


# ================================================================================================ the switch itself
def test_the_switch_is_off_by_default_and_only_moves_the_q5_assertion():
    """with the switch on, whole-block calls are what they were (the committed digests run with it off: tests/golden/*.json)"""
    outs = []
    for sb in (False, True):
        e = OracleEngine(max_block_frames=64, short_blocks=sb)
        assert e.short_blocks is sb and scenarios.TaggedOracle(e).short_blocks is sb
        build(e, "bank")
        outs.append([e.process_interleaved(n) for n in (128, 64, 320)])
    assert_calls_equal(outs[0], outs[1], "whole blocks, switch off / on")
    assert OracleEngine().short_blocks is False


# ================================================================================================ oracle against the independent model
def ragged_fuzz(e, seed):
    """one of the six graphs, call lengths from 1 frame to 3 blocks and a bit, every kind of message at random blocks of them"""
    rng = np.random.default_rng(31_000 + seed)
    graph = GRAPHS[seed % len(GRAPHS)]
    mbf = e.max_block_frames
    one_shots = [int(v) for v in rng.choice(9, size=2, replace=False)]
    r = build(e, graph, seed=seed, one_shots=one_shots)
    outs = []
    for call in range(7):
        pick = int(rng.integers(0, 5))
        n = int([rng.integers(1, mbf), mbf * rng.integers(1, 3) + rng.integers(1, mbf), mbf - 1, mbf * rng.integers(1, 4), mbf + 1][pick])
        nb = (n + mbf - 1) // mbf
        for _ in range(int(rng.integers(0, 5))):
            vc = r.voices[int(rng.integers(0, len(r.voices)))]
            at = int(rng.integers(0, nb + 1))  # (nb: carried over to block 0 of the next call)
            what = int(rng.integers(0, 8))
            if vc["kind"] == "r":
                if what < 3:
                    e.set_param(vc["src"], 1, float(rng.uniform(0.3, 3.0)), at_block=at)
                elif what < 5:
                    e.set_param(vc["src"], 4, float(rng.integers(0, vc["frames"])), at_block=at)
                else:
                    e.set_param(vc["src"], 3, float(rng.integers(0, 2)), at_block=at)
            elif what == 0:
                e.sampler_pause(vc["src"], at_block=at)
            elif what == 1:
                e.sampler_play(vc["src"], at_block=at)
            elif what == 2:
                e.sampler_stop(vc["src"], at_block=at)
            elif what == 3:
                e.sampler_set_playhead_secs(vc["src"], float(rng.integers(0, vc["frames"])) / e.sample_rate, at_block=at)
            elif what == 4:
                e.set_param(vc["src"], 0, float(rng.choice([0.0, 40.0, 100.0])), at_block=at)
            elif what == 5:
                lo = float(rng.integers(0, vc["frames"] // 2)) / e.sample_rate
                e.sampler_set_loop_range(vc["src"], int(rng.choice([LOOP_NONE, LOOP_FULL, LOOP_RANGE_SECS])), lo, lo + float(rng.integers(1, 2 * mbf)) / e.sample_rate, at_block=at)
            elif what == 6:
                e.sampler_set_sample(vc["src"], vc["sample"], stop_playback=bool(rng.integers(0, 2)), at_block=at)
            for t, nodes, prm, val in (("v", vc["vols"], 0, float(rng.uniform(0, 110))), ("p", vc["pans"], 0, float(rng.uniform(-1, 1))),
                                       ("B", vc["bqs"], 1, float(rng.uniform(200, 9000))), ("D", vc["dls"], 1, float(rng.uniform(0, 0.6)))):
                if nodes and what == 7:
                    e.set_param(nodes[0], prm, val, at_block=at)
            if vc["sp"] is not None and what >= 6:
                e.set_param(vc["sp"], 0, float(rng.uniform(-5, 5)), at_block=at)
        if r.master_vol is not None and call == 2:
            e.set_param(r.master_vol, 0, 40.0, at_block=nb - 1)
        if r.bus_bq is not None and call == 3:
            e.set_param(r.bus_bq, 1, 900.0, at_block=0)
        outs.append(np.asarray(e.process_interleaved(n)))
    return outs


def test_relaxed_oracle_and_relaxed_model_agree_on_50_ragged_seeds():
    fails = []
    for seed in range(50):
        mbf = int(np.random.default_rng(seed).choice([64, 100, 128]))
        want, got = ragged_fuzz(relaxed(mbf), seed), ragged_fuzz(relaxed(mbf, model=True), seed)
        try:
            assert_calls_equal(want, got, "seed %d (%s, mbf %d)" % (seed, GRAPHS[seed % len(GRAPHS)], mbf))
        except AssertionError as ex:
            fails.append(str(ex))
    assert not fails, fails[:5]


# ================================================================================================ stream invariance
def ragged_calls(mbf):
    """the stretch the invariance is stated for: K whole blocks + a tail, calls shorter than a block, a call one frame short of one — and
    a last call that pads the stretch to whole blocks"""
    calls = [2 * mbf + 17, 1, mbf - 1, 5, 2 * mbf, 3, 2 * mbf - 3]
    return calls + [-sum(calls) % mbf + mbf]


def steady_stream(e, graph, calls, mbf):
    """gains constant from the start, no message after the first block, sources longer than a block (Q8 wraps once per block); voices 1
    and 4 are one-shots that end inside the stretch (src_frames: 6 and 9 blocks and a bit), the loops wrap inside it"""
    build(e, graph, seed=3, one_shots=(1, 4))
    return [np.asarray(e.process_interleaved(n)) for n in [2 * mbf] + list(calls)]


@pytest.mark.parametrize("graph", ["bank", "rs", "chain"])
@pytest.mark.parametrize("mbf", [64, 128])
def test_steady_voices_in_ragged_calls_equal_the_default_oracle_in_whole_blocks(graph, mbf):
    calls = ragged_calls(mbf)
    total = 2 * mbf + sum(calls)
    assert total % mbf == 0 and total > src_frames(4, mbf) > src_frames(1, mbf)  # (both one-shots end inside the stretch)
    got = np.concatenate(steady_stream(relaxed(mbf), graph, calls, mbf))
    want = steady_stream(OracleEngine(max_block_frames=mbf), graph, [mbf] * (sum(calls) // mbf), mbf)
    assert_calls_equal([np.concatenate(want)], [got], "%s mbf %d: ragged calls against whole blocks" % (graph, mbf))
