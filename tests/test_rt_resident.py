"""GPU tier (-m gpu): the resident realtime kernel (k_rt_persist, include/fwgpu.h `fwgpu_rt_resident_stats`) — one-block
callbacks on the voice-bank plan are served through a doorbell by a kernel that stays on the device; everything that is not a
steady callback ends it first; its watchdog ends it when nobody calls.  Every test compares with the oracle bit for bit: the
kernel runs the same device functions as the one-launch edge, so a difference means the hand-over lost or repeated a block."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import scenarios
from fwapi import LOOP_FULL, LOOP_RANGE_SECS, PLANAR_F32, GpuEngine, OracleEngine
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu
MBF = 256


def _bank(e, n_voices=96):
    voices = scenarios.build_voice_bank(e, n_voices, radix=32, src_frames=5000, mono_every=7)
    for v, vc in enumerate(voices):
        if v % 5 != 3:
            e.sampler_set_loop_range(vc["sampler"], LOOP_FULL)  # (v % 5 == 3: one-shots, they end inside the run)
        if v % 9 != 4:
            e.sampler_play(vc["sampler"])
    return voices


def _run(e, script):
    """script(e, voices, i) is called before callback i; returns the concatenated one-block callbacks"""
    voices = _bank(e)
    outs = []
    for i in range(script.n):
        script(e, voices, i)
        outs.append(np.asarray(e.process_interleaved(MBF)))
    return np.concatenate(outs)


class Steady:
    n = 40

    def __call__(self, e, voices, i):
        pass


class Traffic:
    """messages, a call of another size and a graph edit between the callbacks"""
    n = 60

    def __call__(self, e, voices, i):
        if i == 7:
            e.set_param(voices[2]["volume"], 0, 35.0)          # a glide: ~21 callbacks that are not steady for that voice
        if i == 19:
            e.sampler_pause(voices[5]["sampler"])
        if i == 23:
            e.sampler_play(voices[5]["sampler"])
        if i == 31:
            extra = e.process_interleaved(3 * MBF)              # not one block: the launch sequence, the resident kernel ended first
            self.extra = np.asarray(extra)
        if i == 40:
            e.set_param(voices[11]["pan"], 0, -0.6)
        if i == 48:                                             # a graph edit: a new plan, adopted by the next callback
            e.remove_node(voices[20]["pan"])                    # (its mixer port is left unconnected: silence from there)
            e.update()


def test_consecutive_callbacks_ride_the_doorbell_and_match_the_oracle():
    g, o = GpuEngine(max_block_frames=MBF), OracleEngine(max_block_frames=MBF)
    out_g, out_o = _run(g, Steady()), _run(o, Steady())
    assert g.cx.plan_kind() == 1
    assert_bits_equal(out_o, out_g, "steady callbacks")
    launches, doorbells = g.cx.rt_resident_stats()
    if os.environ.get("FWGPU_RT_PERSIST") == "0":
        assert (launches, doorbells) == (0, 0)
    else:
        # the one-shots end inside the run (a voice that needs its state machines is still a steady CALLBACK: no message on the
        # device); what may cut the run short is the watchdog, when the test machine stalls for its whole idle time
        # (the first callback carries the play / set-sample messages: an ordinary launch)
        assert launches >= 1 and Steady.n - 2 <= launches + doorbells <= Steady.n, (launches, doorbells)
        if int(os.environ.get("FWGPU_RT_IDLE_MS", "20")) >= 20:
            assert launches <= 3, (launches, doorbells)


@pytest.mark.parametrize("n_voices,radix,mbf", [(96, 4, 256), (200, 8, 64), (70, 4, 1024), (33, 2, 128)])
def test_one_launch_edge_walks_mixer_trees_of_any_depth(n_voices, radix, mbf):
    """Round 5: the one-launch / resident edge was the leaves + root tree's; now whoever completes a mixer's children renders the mixer
    and carries on at ITS consumer (k_rt.hip.h) — trees of 3 to 7 levels (radix 2 .. 8: BASELINE configs[4]'s shard is 256 + 8 + 1),
    blocks of 64 to 1024 frames, ragged last mixers, voices that never start, one-shots that end inside the run, a glide and a pause
    between callbacks.  Every callback against the oracle; the counters say the callbacks rode the doorbell / the one launch."""
    def run(e):
        voices = scenarios.build_voice_bank(e, n_voices, radix=radix, src_frames=mbf * 7 + 33, mono_every=5)
        for v, vc in enumerate(voices):
            if v % 5 != 3:
                e.sampler_set_loop_range(vc["sampler"], LOOP_FULL)
            if v % 9 != 4:
                e.sampler_play(vc["sampler"])
        outs = []
        for i in range(24):
            if i == 6:
                e.set_param(voices[1]["volume"], 0, 30.0)
            if i == 11:
                e.sampler_pause(voices[2]["sampler"])
            if i == 15:
                e.sampler_play(voices[2]["sampler"])
            outs.append(np.asarray(e.process_interleaved(mbf)))
        return np.concatenate(outs)

    g, o = GpuEngine(max_block_frames=mbf), OracleEngine(max_block_frames=mbf)
    out_g, out_o = run(g), run(o)
    assert g.cx.plan_kind() == 1
    assert_bits_equal(out_o, out_g, "callbacks on a deep mixer tree")
    rk, one, seq, lev = g.cx.rt_path_stats()
    assert lev == 0 and seq == 0 and rk + one == 24, (rk, one, seq, lev)


def test_rt_path_stats_say_which_path_the_one_block_calls_took():
    """fwgpu_rt_path_stats: the doorbell / one-launch edge exists for the plain voice-bank plan only — a host whose
    callbacks run on the launch sequence (chain plan) or on the level executor (forced generic) sees it in the counters."""
    g = GpuEngine(max_block_frames=MBF)
    _run(g, Steady())
    rk, one, seq, lev = g.cx.rt_path_stats()
    assert lev == 0 and rk + one + seq == Steady.n, (rk, one, seq, lev)
    if os.environ.get("FWGPU_RT_PERSIST") != "0":
        assert rk >= Steady.n - 4, (rk, one, seq, lev)
    c = GpuEngine(max_block_frames=128, max_batch=4)
    scenarios.scenario_chain_steady(c, 12, 4, radix=4, src_frames=700, first_delay_frames=128, min_delay_frames=128)
    assert c.cx.plan_kind() == 2
    before = c.cx.rt_path_stats()
    for _ in range(5):
        c.process_interleaved(128)
    after = c.cx.rt_path_stats()
    assert after[2] - before[2] == 5 and after[0] == before[0] and after[1] == before[1] and after[3] == before[3], (before, after)
    f = GpuEngine(max_block_frames=MBF, force_generic=True)
    _bank(f, 8)
    for _ in range(3):
        f.process_interleaved(MBF)
    assert f.cx.rt_path_stats()[3] == 3 and sum(f.cx.rt_path_stats()[:3]) == 0


def test_messages_other_sizes_and_edits_end_the_kernel_and_nothing_is_lost():
    sg, so = Traffic(), Traffic()
    g, o = GpuEngine(max_block_frames=MBF), OracleEngine(max_block_frames=MBF)
    out_g, out_o = _run(g, sg), _run(o, so)
    assert_bits_equal(out_o, out_g, "callbacks with traffic")
    assert_bits_equal(so.extra, sg.extra, "the three-block call in between")
    launches, doorbells = g.cx.rt_resident_stats()
    if os.environ.get("FWGPU_RT_PERSIST") != "0":
        assert launches >= 4 and doorbells >= 20, (launches, doorbells)   # ended and launched again around every event


def test_an_in_place_rewire_between_callbacks_ends_the_kernel_and_nothing_is_lost():
    """the callback path's share of tests/test_gpu_rewire.py, one block per call under the resident kernel: two sounding voices — one of
    them muted and settled — get their volume and pan swapped (sampler -> pan -> volume) with the same nodes.  The kernel ends, the next
    callback adopts the new plan, the two voices leave their steady caches behind and everybody else's travels."""
    def run(e, rewire=True):
        # (scenarios.build_voice_bank keeps its mixers to itself: the bank is wired here, 96 voices under three leaf sums of 32)
        rng = np.random.default_rng(1234)
        voices, leaves = [], []
        for v in range(96):
            if v % 32 == 0:
                leaves.append(e.sum(32))
            s, vol, pan = e.sampler(100.0), e.volume(float(rng.uniform(10, 100))), e.pan(float(rng.uniform(-1, 1)))
            e.connect_stereo(s, vol)
            e.connect_stereo(vol, pan)
            e.connect_stereo(pan, leaves[-1], 2 * (v % 32))
            voices.append((s, vol, pan))
        root = e.sum(3)
        for p, m in enumerate(leaves):
            e.connect_stereo(m, root, 2 * p)
        e.connect_stereo(root, e.graph_out_node)
        e.update()
        for v, (s, _, _) in enumerate(voices):
            e.sampler_set_sample(s, e.new_sample(PLANAR_F32, 2, scenarios.voice_source(300 + v, 5000, 2)))
            e.sampler_set_loop_range(s, LOOP_FULL)
            e.sampler_play(s)
        outs = []
        for i in range(46):
            if i == 6:
                e.set_param(voices[7][1], 0, 0.0)               # muted, and settled ~21 callbacks later
            if i == 34 and rewire:
                for v in (7, 40):
                    s, vol, pan = voices[v]
                    for ch in (0, 1):
                        e.disconnect(s, ch, vol, ch)
                        e.disconnect(vol, ch, pan, ch)
                        e.disconnect(pan, ch, leaves[v // 32], 2 * (v % 32) + ch)
                    e.connect_stereo(s, pan)
                    e.connect_stereo(pan, vol)
                    e.connect_stereo(vol, leaves[v // 32], 2 * (v % 32))
                e.update()
            if i == 39:
                e.set_param(voices[7][1], 0, 80.0)
            outs.append(np.asarray(e.process_interleaved(MBF)))
        return np.concatenate(outs)

    g, o = GpuEngine(max_block_frames=MBF), OracleEngine(max_block_frames=MBF)
    out_g, out_o = run(g), run(o)
    assert g.cx.plan_kind() == 1
    assert_bits_equal(out_o, out_g, "callbacks around an in-place rewire")
    plain = run(OracleEngine(max_block_frames=MBF), rewire=False)
    lo = 34 * MBF * 2
    assert np.array_equal(out_o[:lo], plain[:lo]) and np.any(out_o[lo:] != plain[lo:])   # the oracle hears the rewire
    launches, doorbells = g.cx.rt_resident_stats()
    if os.environ.get("FWGPU_RT_PERSIST") != "0":
        assert launches >= 3 and doorbells >= 20, (launches, doorbells)


@pytest.mark.parametrize("idle_ms,pause_ms", [(1, 0.7), (1, 1.0), (1, 1.4), (2, 2.0)])
def test_watchdog_ends_the_kernel_and_a_late_doorbell_loses_no_block(idle_ms, pause_ms):
    """pauses around the watchdog's length between callbacks: the kernel ends by itself, sometimes while the next doorbell is on its
    way (the host then finds alive == 0 with the completion flag unchanged and renders the block with an ordinary launch)"""
    code = r'''
import sys, time
sys.path.insert(0, %r)
import numpy as np
from fwapi import GpuEngine, OracleEngine
from test_rt_resident import _bank, MBF
from test_gpu_parity import assert_bits_equal
g, o = GpuEngine(max_block_frames=MBF), OracleEngine(max_block_frames=MBF)
_bank(g), _bank(o)
rng = np.random.default_rng(5)
outs_g, outs_o = [], []
for i in range(150):
    outs_g.append(np.asarray(g.process_interleaved(MBF)))
    outs_o.append(np.asarray(o.process_interleaved(MBF)))
    t = %f * 1e-3 * float(rng.uniform(0.8, 1.2)) if i %% 3 else 0.0
    end = time.perf_counter() + t
    while time.perf_counter() < end:
        pass
assert_bits_equal(np.concatenate(outs_o), np.concatenate(outs_g), "callbacks around the watchdog")
launches, doorbells = g.cx.rt_resident_stats()
assert launches >= %d and launches + doorbells <= 150, (launches, doorbells)
print("OK", launches, doorbells)
''' % (os.path.dirname(os.path.abspath(__file__)), pause_ms, 20 if pause_ms > 1.3 * idle_ms else 1)
    if os.environ.get("FWGPU_RT_PERSIST") == "0":
        pytest.skip("the resident kernel is switched off")
    env = dict(os.environ, FWGPU_RT_IDLE_MS=str(idle_ms))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_destroy_and_idle_leave_no_kernel_behind():
    g = GpuEngine(max_block_frames=MBF)
    _bank(g)
    for _ in range(5):
        g.process_interleaved(MBF)
    t0 = time.perf_counter()
    g.cx.synchronize()     # the ctx stream: the resident kernel runs on its own, this does not wait for it
    assert time.perf_counter() - t0 < 0.015
    g.cx.close()           # ends it (doorbell | quit) and waits
    import torch

    t0 = time.perf_counter()
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 0.010, "a resident kernel outlived its context"


# ------------------------------------------------------------------ more shapes through the resident kernel
def _varied_bank(e, n_voices, fx, src_frames):
    """loops of odd lengths (wraps at every offset inside a block), one-shots that end inside the run, mono samples, voices that
    never play (silent ports), a voice muted by a fade, loop ranges; a last leaf of 4 ports (the unmasked SumNode path)"""
    def voice_fx(e_, v, rng):
        if not fx:
            return []
        return [e_.width(float(rng.uniform(0.3, 1.7)))] if v % 3 == 0 else ([e_.hard_clip(-4.0)] if v % 3 == 1 else [])

    voices = scenarios.build_voice_bank(e, n_voices, radix=32, src_frames=src_frames, mono_every=5, voice_fx=voice_fx if fx else None)
    for v, vc in enumerate(voices):
        if v % 7 == 3:
            pass                                                   # a one-shot: ends after src_frames
        elif v % 7 == 5:
            e.sampler_set_loop_range(vc["sampler"], LOOP_RANGE_SECS, (13 + v) / 48000.0, (src_frames - 29 - v) / 48000.0)
        else:
            e.sampler_set_loop_range(vc["sampler"], LOOP_FULL)
        if v % 11 != 6:
            e.sampler_play(vc["sampler"])                          # v % 11 == 6: never plays
        if v == 9:
            e.set_param(vc["volume"], 0, 0.0)                      # fades to silence: muted from then on
    return voices


@pytest.mark.parametrize("mbf,n_voices,fx,src_frames,n_cb", [(64, 100, False, 701, 260), (64, 132, True, 997, 200), (128, 260, False, 1500, 120),
                                                              (256, 1024, False, 4099, 60)])
def test_varied_banks_through_the_resident_kernel_match_the_oracle(mbf, n_voices, fx, src_frames, n_cb):
    """(the scenario that showed a resident kernel with a second rendering path compiled in writing garbage from its ORDINARY
    block — scripts/experiments/r03_rt_sliced_kernel.patch)"""
    g, o = GpuEngine(max_block_frames=mbf), OracleEngine(max_block_frames=mbf)
    outs_g, outs_o = [], []
    for e, outs in ((g, outs_g), (o, outs_o)):
        _varied_bank(e, n_voices, fx, src_frames)
        for _ in range(n_cb):
            outs.append(np.asarray(e.process_interleaved(mbf)))
    assert g.cx.plan_kind() == 1
    assert_bits_equal(np.concatenate(outs_o), np.concatenate(outs_g), "varied bank %d voices block %d" % (n_voices, mbf))
    if os.environ.get("FWGPU_RT_PERSIST") != "0":
        launches, doorbells = g.cx.rt_resident_stats()
        assert doorbells >= n_cb // 2, (launches, doorbells)


def test_control_calls_that_free_device_memory_do_not_wait_for_a_fed_resident_kernel():
    """hipFree / hipHostFree / hipDeviceSynchronize wait for EVERY stream, and the resident kernel ends only when
    told to or 20 ms after its last doorbell — a steady stream of callbacks kept it alive for ever, and with it an fwgpu_update
    that had to grow a table (or a sample_create that grew the sample table: the audio thread then sat at its gate until the
    watchdog fired).  Now the control call raises RtMailbox::hold first (RtHold): the kernel ends at its next poll, callbacks go
    out as ordinary launches meanwhile.  Audio thread = the library's own callback loop (fwgpu_stream_run, no GIL held), control
    side = this thread: a graph edit that grows every table of the voice-bank plan, then 40 new samples (the table doubles)."""
    import threading

    if os.environ.get("FWGPU_RT_PERSIST") == "0":
        pytest.skip("the resident kernel is switched off")
    g = GpuEngine(max_block_frames=MBF)

    def leaf(first):
        m = g.sum(32)
        vs = []
        for p in range(32):
            s, vol = g.sampler(100.0), g.volume(40.0 + p)
            g.connect_stereo(s, vol)
            g.connect_stereo(vol, m, 2 * p)
            vs.append(s)
        return m, vs

    root = g.sum(8)   # six of its stereo ports stay free for the edit (unconnected = the cleared buffer: still the voice-bank plan)
    samplers = []
    for p in range(2):
        m, vs = leaf(32 * p)
        g.connect_stereo(m, root, 2 * p)
        samplers += vs
    g.connect_stereo(root, g.graph_out_node)
    g.update()
    for v, s in enumerate(samplers):
        g.sampler_set_sample(s, g.new_sample(scenarios.PLANAR_F32, 2, scenarios.voice_source(v, 4000, 2)))
        g.sampler_set_loop_range(s, LOOP_FULL)
        g.sampler_play(s)
    for _ in range(3):
        g.process_interleaved(MBF)
    assert g.cx.plan_kind() == 1
    st = g.cx.open_stream(0, 2)
    st.run(MBF, 20, 0.0)
    l0, d0 = g.cx.rt_resident_stats()
    assert d0 > 0, "the resident kernel is not in use: nothing to test"
    res = {}
    N = 240000   # ~6 s of back-to-back callbacks at ~25 us each: the doorbell never rests for the watchdog's 20 ms

    def audio():
        res["run"] = st.run(MBF, N, 21 * MBF / 48000.0)

    th = threading.Thread(target=audio)
    th.start()
    time.sleep(0.3)
    t0 = time.perf_counter()
    for p in range(2, 6):   # 128 more voices: node / voice / record tables all grow (DevBuf::ensure frees the old ones)
        m, _ = leaf(32 * p)
        g.connect_stereo(m, root, 2 * p)
    g.update()
    t_update = time.perf_counter() - t0
    t1 = time.perf_counter()
    ids = [g.new_sample(scenarios.PLANAR_F32, 2, scenarios.voice_source(900 + i, 512, 2)) for i in range(80)]
    t_samples = time.perf_counter() - t1
    alive_after = th.is_alive()
    th.join(timeout=60)
    assert not th.is_alive(), "the callback loop never returned"
    assert alive_after, "the stream ended before the control calls did: nothing was measured (%.2f s, %.2f s)" % (t_update, t_samples)
    assert g.cx.plan_kind() == 1
    # bounds far above what the calls take (tens of ms) and far below "until the stream stops" (seconds)
    assert t_update < 1.5, "fwgpu_update waited %.2f s beside a fed resident kernel" % t_update
    assert t_samples < 1.5, "%d sample_create calls took %.2f s beside a fed resident kernel" % (len(ids), t_samples)
    l1, d1 = g.cx.rt_resident_stats()
    assert d1 - d0 > N // 2 and l1 > l0, (l0, d0, l1, d1)   # ended (hold) and launched again; doorbells carried the rest
    cbs, unders, _ = st.stats()
    assert cbs == 20 + N
    st.close()
    g.cx.close()
