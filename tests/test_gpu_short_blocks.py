"""GPU tier (-m gpu): short blocks through sampler graphs on every fused plan.

A process call whose length is no whole number of blocks ends in a short block.  On a fused plan the whole blocks are rendered by the
fused kernels and the short one by the level executor (fwgpu_run.cpp run_blocks_impl: run_fused_batch while a whole block is left, then
run_generic_batch(K = 1, frames < max_block_frames)) — playheads, smoothers and ramp rows, biquad and delay state, delay-ring positions,
spatial histories, resampler positions, the lazy records and the control-ahead stream all change owner in the middle of a call, and
back at the next one.  The reference panics on such a block in a sampler (Q5); what the product renders there is stated by the two CPU
restatements' `short_blocks` switch (test_short_blocks.py, which also holds the six graphs used here).

Every test compares the product through the C ABI with OracleEngine(short_blocks=True) bit for bit and call by call, asserts the plan
kind it means, and asserts that the level executor's one-block counter (rt_path_stats()[3]) grew by the number of short blocks — a planner
that quietly moved the graph to the levels would be seen.  (On the hybrid plan whole blocks run inside run_generic_batch too, the banks
rendered by the voice-bank kernels: its one-block batches of whole blocks are counted as well, `level_singles`.)

T1 one call = K whole blocks + a tail           T2 around lazy calls               T3 messages in and around the tail
T4 ends and wraps inside the tail               T5 the realtime edge               T6 the level executor alone (force_generic)
T7 the product's ragged calls against the DEFAULT oracle's whole blocks (steady voices): independent of the switch
"""
import os

import numpy as np
import pytest

import test_short_blocks as T
from fwapi import LOOP_NONE, LOOP_RANGE_SECS, GpuEngine, OracleEngine
from test_meter import assert_readings, model, planar
from test_short_blocks import GRAPHS, PLAN_KIND, assert_calls_equal

pytestmark = pytest.mark.gpu


def level_singles(graph, calls, mbf, max_batch):
    """how often run_generic_batch runs with K = 1 over these calls: once per short block — and, on the hybrid plan, once per one-block
    batch of whole blocks"""
    n = sum(1 for c in calls if c % mbf)
    if graph == "hybrid":
        n += sum(1 for c in calls if (c // mbf) % (max_batch or 64) == 1)
    return n


def run(e, graph, calls, script=None, **kw):
    """script(e, rig, i) runs before call i -> rig, [output of each call]"""
    r = T.build(e, graph, **kw)
    outs = []
    for i, n in enumerate(calls):
        if script is not None:
            script(e, r, i)
        outs.append(np.asarray(e.process_interleaved(n)))
    return r, outs


def check(graph, mbf, max_batch, calls, script=None, generic=False, what="", **kw):
    _, want = run(T.relaxed(mbf), graph, calls, script, **kw)
    g = GpuEngine(max_block_frames=mbf, max_batch=max_batch, force_generic=generic)
    r, got = run(g, graph, calls, script, meter=graph == "master", **kw)
    assert g.cx.plan_kind() == (0 if generic else PLAN_KIND[graph])
    assert_calls_equal(want, got, "%s %s mbf %d K<=%s calls %s" % (what, graph, mbf, max_batch, calls))
    if not generic:
        assert g.cx.rt_path_stats()[3] == level_singles(graph, calls, mbf, max_batch), (g.cx.rt_path_stats(), calls)
    return g, r, want, got


# ================================================================================================ T1 / T6
def _t1_sets():
    """(mbf, tail) from (64, 1) (64, 63) (128, 3) (128, 17) (128, 127) (100, 37) [(512, 257): one 256-frame resampler piece + 1 frame] x
    max_batch default | 2, pairwise: every graph sees a tail of 1, tails that are no multiple of 4, mbf - 1, both block sizes, both
    batchings.  (Blocks of 100 frames: the plans that take them — spatialiser and chain banks go to the hybrid plan there.)"""
    sets = []
    for k, graph in enumerate(GRAPHS):
        a, b = (None, 2) if k % 2 == 0 else (2, None)
        sets += [(graph, 64, 1, a), (graph, 64, 63, b), (graph, 128, 3 if k % 2 == 0 else 17, b), (graph, 128, 127, a)]
    sets += [("bank", 100, 37, None), ("rs", 100, 37, 2), ("hybrid", 100, 37, 2), ("master", 100, 37, None), ("rs", 512, 257, None)]
    return sets


def t1_calls(mbf, tail, max_batch):
    k = 5 if max_batch == 2 else 3  # (5 whole blocks in batches of 2: 2, 2 and 1 before the tail)
    return [2 * mbf, k * mbf + tail, 2 * mbf, mbf]


@pytest.mark.parametrize("graph,mbf,tail,max_batch", _t1_sets())
def test_t1_whole_blocks_and_a_tail_in_one_call(graph, mbf, tail, max_batch):
    calls = t1_calls(mbf, tail, max_batch)
    g, r, want, got = check(graph, mbf, max_batch, calls, what="T1")
    if graph == "master":  # the meter's block count includes the short block: its record holds `tail` frames
        n = sum((c + mbf - 1) // mbf for c in calls)
        rd, done = g.cx.meter_read(r.meter, 0, n)
        assert done == n and rd.shape[0] == n, (done, rd.shape, n)
        assert list(rd["frames"][:, 0]) == [mbf if f == 0 else f for c in calls for f in [0] * (c // mbf) + ([c % mbf] if c % mbf else [])]
        assert_readings(rd, np.concatenate([model(planar(x), mbf) for x in want]), "master meter, tail %d" % tail)


@pytest.mark.parametrize("graph,mbf,tail,max_batch", [("bank", 64, 63, 2), ("spatial", 128, 17, None), ("rs", 128, 3, 2), ("chain", 64, 1, 2),
                                                      ("hybrid", 128, 127, None), ("master", 100, 37, None)])
def test_t6_the_level_executor_alone_renders_the_same_calls(graph, mbf, tail, max_batch):
    """fails here too: the level executor's short sampler block is wrong; fails in T1 only: the hand-over is"""
    check(graph, mbf, max_batch, t1_calls(mbf, tail, max_batch), generic=True, what="T6")


# ================================================================================================ T2
@pytest.mark.parametrize("graph,mbf,p,max_batch", [("bank", 64, 1, None), ("bank", 128, 127, 2), ("rs", 128, 17, None), ("rs", 64, 63, 2),
                                                   ("chain", 128, 3, None), ("chain", 64, 63, 2)])
def test_t2_short_blocks_between_lazy_calls(graph, mbf, p, max_batch):
    """three message-free calls (the later ones render from the lazy records), a tail-only call, three more, a block + a tail, two more:
    the short block flushes the records, must not strand them, and nothing stale is used afterwards.

    The voices are the ones that can still be rendered lazily once a short block has moved their playheads off the block grid
    (k_control.hip.h lazy_record): one-shots that outlast the run, planar-f32 or interleaved 16-bit — a loop qualifies only while it is
    entered on a block boundary — and resampling sources in planar f32 whose ratio is below 2 (a 32.32 step of 2^33 or more never
    leaves a record, whole blocks or not: of the bank's six ratios 2.5 is left out here, T1 / T3 / T4 / T7 keep it)."""
    calls = [2 * mbf] + [2 * mbf] * 3 + [p] + [2 * mbf] * 3 + [mbf + p] + [2 * mbf] * 2
    n = len(T.SHAPES[graph])
    total = sum(calls) + mbf
    ratios = tuple(x for x in T.RATIOS if x < 2.0)
    frames = {i: int(total * (ratios[i % len(ratios)] if graph == "rs" else 1)) + 17 + 13 * i for i in range(n)}
    marks = {}

    def script(e, r, i):
        if hasattr(e, "cx") and i in (1, 4, 5, 8):
            marks[i] = e.cx.lazy_stats()[0]

    check(graph, mbf, max_batch, calls, script, what="T2", frames=frames, one_shots=range(n), planar=True, ratios=ratios)
    if os.environ.get("FWGPU_LAZY") != "0":
        assert marks[4] > marks[1] and marks[8] > marks[5], marks


# ================================================================================================ T3
def _some(voices, key=None, step=2):
    vs = [vc for vc in voices if key is None or vc[key]]
    return vs[::step] or vs


def m_volume(at):
    def send(e, r, k, i):
        if i != 1:
            return
        at_block = k + at
        for vc in _some(r.samplers, "vols"):
            e.set_param(vc["vols"][0], 0, 35.0, at_block=at_block)
        for vc in _some(r.samplers, "pans"):
            e.set_param(vc["pans"][0], 0, -0.7, at_block=at_block)
        e.set_param(r.samplers[1]["src"], 0, 45.0, at_block=at_block)  # a sampler's own gain: the smoother whose length Q5 asserts
        if r.master_vol is not None:
            e.set_param(r.master_vol, 0, 30.0, at_block=at_block)
        if r.bus_bq is not None:
            e.set_param(r.bus_bq, 1, 900.0, at_block=at_block)
        for vc in r.voices:
            if vc["sp"] is not None:
                e.set_param(vc["sp"], 0, 4.5, at_block=at_block)
    return send


def m_transport(e, r, k, i):
    a, b, c = r.samplers[0], r.samplers[2], r.samplers[3]
    if i == 1:
        e.sampler_pause(b["src"], at_block=0)
        e.sampler_pause(a["src"], at_block=k)
        e.sampler_play(b["src"], at_block=k)
        e.sampler_stop(c["src"], at_block=k)
    if i == 2:
        e.sampler_play(a["src"], at_block=1)
        e.sampler_play(c["src"], at_block=0)


def m_playhead(e, r, k, i):
    if i == 1:
        for j, vc in enumerate(r.samplers[:4]):  # the last of them to 9 frames before its end: the loop wraps in the tail or right behind it
            e.sampler_set_playhead_secs(vc["src"], (100 + 37 * j if j < 3 else vc["frames"] - 9) / float(e.sample_rate), at_block=k)


def m_set_sample(e, r, k, i):
    st = [vc for vc in r.samplers if vc["ch"] == 2]
    if i == 1:
        e.sampler_set_sample(st[0]["src"], st[1]["sample"], stop_playback=True, at_block=k)
        e.sampler_set_sample(st[2]["src"], st[3]["sample"], stop_playback=False, at_block=k)
    if i == 2:
        e.sampler_play(st[0]["src"], at_block=0)


def m_loop_range(e, r, k, i):
    if i == 1:
        mbf, sr = e.max_block_frames, float(e.sample_rate)
        a, b, c = r.samplers[0], r.samplers[2], r.samplers[3]
        e.sampler_set_loop_range(a["src"], LOOP_RANGE_SECS, 10 / sr, (10 + 2 * mbf + 5) / sr, at_block=k)    # the playhead is past it: back to its start
        e.sampler_set_loop_range(b["src"], LOOP_RANGE_SECS, 0.0, (b["frames"] - 3) / sr, at_block=k)         # the playhead is inside it: Q7 snaps
        e.sampler_set_loop_range(c["src"], LOOP_NONE, at_block=k)                                            # a one-shot from here on


def m_cutoff(e, r, k, i):
    if i == 1:
        for j, vc in enumerate(_some(r.voices, "bqs")):
            e.set_param(vc["bqs"][-1], 1, 700.0 + 450.0 * j, at_block=k)


def m_delay(e, r, k, i):
    if i == 1:
        for j, vc in enumerate(vc for vc in r.voices if vc["dls"]):
            e.set_param(vc["dls"][0], 1 + j % 2, 0.3 if j % 2 == 0 else 0.8, at_block=k)  # feedback / mix


def m_resampler(e, r, k, i):
    if i == 1:
        for j, vc in enumerate(r.resamplers[:9]):
            if j % 3 == 0:
                e.set_param(vc["src"], 1, [0.7, 1.6, 2.2][j // 3], at_block=k)      # ratio
            elif j % 3 == 1:
                e.set_param(vc["src"], 4, float(50 + 111 * j), at_block=k)          # seek
            else:
                e.set_param(vc["src"], 3, 0.0, at_block=k)                          # pause
    if i == 2:
        e.set_param(r.resamplers[2]["src"], 3, 1.0, at_block=1)


MESSAGES = dict(volume_in_tail=m_volume(0), volume_before_tail=m_volume(-1), transport=m_transport, playhead=m_playhead, set_sample=m_set_sample,
                loop_range=m_loop_range, cutoff=m_cutoff, delay=m_delay, resampler=m_resampler)
_SHAPES3 = [(64, 1, None), (128, 17, 2), (64, 63, 2), (128, 127, None), (128, 3, None), (64, 63, None), (128, 127, 2)]


def _t3_sets():
    sets = []
    for a, graph in enumerate(("bank", "spatial", "chain", "hybrid", "master")):
        for b, msg in enumerate(("volume_in_tail", "volume_before_tail", "transport", "playhead", "set_sample", "loop_range")):
            sets.append((graph, msg) + _SHAPES3[(3 * a + b) % len(_SHAPES3)])
    sets += [("chain", "cutoff", 64, 63, 2), ("chain", "cutoff", 128, 3, None), ("chain", "delay", 128, 127, 2), ("chain", "delay", 64, 1, None)]
    sets += [("rs", "resampler", 64, 1, 2), ("rs", "resampler", 128, 17, None), ("rs", "resampler", 512, 257, None), ("rs", "volume_in_tail", 128, 127, 2)]
    return sets


@pytest.mark.parametrize("graph,msg,mbf,tail,max_batch", _t3_sets())
def test_t3_messages_in_and_around_the_tail(graph, msg, mbf, tail, max_batch):
    """K whole blocks in front; the messages carry at_block = K (the tail) or K - 1 (a glide runs through the tail into the next call)"""
    k = 5 if max_batch == 2 else 3
    send = MESSAGES[msg]
    if graph == "rs" and msg == "volume_in_tail":
        def send(e, r, k_, i):
            if i == 1:
                for vc in _some(r.voices, "vols"):
                    e.set_param(vc["vols"][0], 0, 35.0, at_block=k_)
    check(graph, mbf, max_batch, [2 * mbf, k * mbf + tail, 2 * mbf, mbf, 2 * mbf], lambda e, r, i: send(e, r, k, i), what="T3 " + msg)


@pytest.mark.parametrize("graph,mbf,p,max_batch", [("bank", 128, 17, None), ("bank", 64, 63, 2), ("chain", 64, 1, None), ("chain", 128, 127, 2)])
def test_t3_a_tail_only_call_right_behind_the_control_ahead_stream(graph, mbf, p, max_batch):
    """a call of four whole blocks with messages (its control kernels run ahead on their own stream), followed at once by a short call"""
    def script(e, r, i):
        if i == 1:
            for j, vc in enumerate(_some(r.samplers, "vols")):
                e.set_param(vc["vols"][0], 0, 25.0 + 10.0 * j, at_block=1 + j % 3)
            e.sampler_pause(r.samplers[0]["src"], at_block=2)
            e.sampler_play(r.samplers[0]["src"], at_block=3)
            for vc in _some(r.voices, "bqs"):
                e.set_param(vc["bqs"][0], 1, 1500.0, at_block=3)

    check(graph, mbf, max_batch, [2 * mbf, 4 * mbf, p, 2 * mbf, mbf], script, what="T3 ahead")


# ================================================================================================ T4
@pytest.mark.parametrize("graph,mbf,tail,max_batch", [("bank", 64, 63, None), ("bank", 128, 17, 2), ("chain", 128, 127, None), ("chain", 64, 3, 2),
                                                      ("rs", 128, 17, None), ("rs", 64, 63, 2), ("rs", 512, 257, None)])
def test_t4_ends_and_wraps_inside_the_tail(graph, mbf, tail, max_batch):
    k = 5 if max_batch == 2 else 3
    t0 = (2 + k) * mbf  # frames rendered before the tail
    if graph == "rs":
        # one-shot resampling sources of every ratio that run out inside the tail (position = frames * ratio), two loops that wrap in it
        ratio = lambda i: T.RATIOS[i % len(T.RATIOS)]
        frames = {i: int((t0 + tail / 2.0) * ratio(i)) for i in range(8)}
        one_shots = range(6)
    else:
        frames = {0: t0 + (tail + 1) // 2,   # a one-shot whose last frame falls inside the tail
                  1: t0 + 1,                 # (the mono voice of the bank) ... on the tail's first frame
                  2: t0 + tail,              # ... exactly on the tail's last frame (Q9: it stops a block later)
                  4: t0,                     # ... on the last frame the fused kernels render: the tail finds playhead == length
                  3: t0 + tail // 2 + 1,     # a loop whose wrap falls inside the tail (Q8)
                  5: t0 + tail}              # a loop whose end is the tail's end: it wraps at the top of the next call
        one_shots = (0, 1, 2, 4)
    check(graph, mbf, max_batch, [2 * mbf, k * mbf + tail, 2 * mbf, mbf], frames=frames, one_shots=one_shots, what="T4")


# ================================================================================================ T5
@pytest.mark.parametrize("p", [37, 255])
def test_t5_a_short_callback_between_callbacks_of_the_resident_kernel(p):
    from test_rt_resident import MBF, _bank

    calls = [MBF] * 10 + [p] + [MBF] * 10

    def rt(e):
        _bank(e)
        outs, stats = [], []
        for n in calls:
            outs.append(np.asarray(e.process_interleaved(n)))
            if hasattr(e, "cx"):
                stats.append(e.cx.rt_resident_stats())
        return outs, stats

    want, _ = rt(OracleEngine(max_block_frames=MBF, short_blocks=True))
    g = GpuEngine(max_block_frames=MBF)
    got, stats = rt(g)
    assert g.cx.plan_kind() == 1
    assert_calls_equal(want, got, "T5 callbacks of %d x 10, %d, %d x 10" % (MBF, p, MBF))
    assert g.cx.rt_path_stats()[3] == 1, g.cx.rt_path_stats()
    if os.environ.get("FWGPU_RT_PERSIST") != "0":
        (l0, d0), (l1, d1), (l2, d2) = stats[9], stats[10], stats[-1]
        assert l0 >= 1 and d0 >= 1, stats        # the resident kernel served the first stretch ...
        assert (l1, d1) == (l0, d0), stats       # ... not the short callback, which ended it ...
        assert l2 > l1 and d2 > d1, stats        # ... and it was launched again behind it


# ================================================================================================ T7
@pytest.mark.parametrize("graph", ["bank", "rs", "chain"])
@pytest.mark.parametrize("mbf,max_batch", [(64, None), (128, 2)])
def test_t7_ragged_calls_equal_the_default_oracle_in_whole_blocks(graph, mbf, max_batch):
    """steady voices (test_short_blocks.steady_stream): nothing here depends on the short_blocks switch"""
    calls = T.ragged_calls(mbf)
    want = T.steady_stream(OracleEngine(max_block_frames=mbf), graph, [mbf] * (sum(calls) // mbf), mbf)
    g = GpuEngine(max_block_frames=mbf, max_batch=max_batch)
    got = T.steady_stream(g, graph, calls, mbf)
    assert g.cx.plan_kind() == PLAN_KIND[graph]
    assert_calls_equal([np.concatenate(want)], [np.concatenate(got)], "T7 %s mbf %d" % (graph, mbf))
    assert g.cx.rt_path_stats()[3] == level_singles(graph, calls, mbf, max_batch)
