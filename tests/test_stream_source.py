"""Streaming sample sources (fwgpu_sample_create_stream / _stream_write / _stream_end / _stream_status, CMD_SMP_STREAM = 17; SPEC,
DESIGN.md section 6): a sampler that plays a ring fed while it plays.

CPU tier: the stream's one statement (fwgpu_types.h smp_stream_*, built for the host beside the harness: tests/host_harness/
stream_source_peek.cpp) against the model (tests/stream_source_model.py, on tests/refmodel.py's SamplerNode) over seeded schedules;
the host half on the fake-HIP harness (refusals, what a write queues, the split at the ring's end in the ring's bytes, a full message
ring); a stand-alone program under AddressSanitizer + UBSan that drives the write / free-space / publish accounting
(tests/host_harness/stream_driver.cpp); the header, fwgpu_types.h, _lib.py and ffi.rs agree.

GPU tier, every comparison `fwapi.bits` equality, max_block_frames 64.  The yardsticks are twins that run on code that existed before
streams did: a second context that holds the same frames as a whole sample played as a one-shot (fed ahead), or that gets `pause` at
each starved block and `play` where the data arrives (starved); the numpy model for the cases with fades, glides and mutes.

Rings: the fed-ahead cases take R = (K + 2) * 64 + 24 and (K + 2) * 64, but never less than the 4 * max_block_frames the ABI asks for —
for K = 1 that is 4 * 64 + 24 and 4 * 64 (3 * 64 would be refused): the wrap still falls inside a block with the one and on an edge
with the other.

Known limit (include/fwgpu.h, rule 4): the block the end falls into is rendered as a one-shot's last block unless the ring's wrap falls
in front of the end inside that same block; there the frames behind the end are read from the padding, which is 0.0 for the signed and
float formats and 0x8000 = 1.5e-5 for the unsigned 16-bit formats (no u16 element decodes to 0.0).  The model restates the rule, and
test_end_block_with_the_wrap_in_front_of_the_end lands there on purpose, in a signed and an unsigned format.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fwapi
import sampler_fade_model as fm
import stream_source_model as sm
from fwapi import GpuEngine, HostOnlyEngine

INVALID, QUEUE_FULL = -20, -21
F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HARNESS = os.path.join(ROOT, "tests", "host_harness")
FUZZ_SEEDS = int(os.environ.get("FWGPU_FUZZ_SEEDS", "20"))
I_I16, I_U16, I_F32, P_I16, P_U16, P_F32 = range(6)
FMT_NAMES = ["i_i16", "i_u16", "i_f32", "p_i16", "p_u16", "p_f32"]
B = 64  # max_block_frames of every GPU case


def rows_for(fmt, channels, frames, seed):
    """[frames][channels] raw elements of the format, seeded"""
    rng = np.random.default_rng(4200 + seed)
    if fmt in (I_F32, P_F32):
        return rng.uniform(-0.9, 0.9, (frames, channels)).astype(F32)
    if fmt in (I_I16, P_I16):
        return rng.integers(-30000, 30000, (frames, channels)).astype(np.int16)
    return rng.integers(1, 65535, (frames, channels)).astype(np.uint16)


# ================================================================================================ CPU tier 1: the state machine
def _peek_lib():
    ull = C.POINTER(C.c_ulonglong)
    return fwapi.peek_lib("stream_source_peek", {
        "ssp_ring_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_char_p]),
        "ssp_stream_rec": (C.c_int, [C.c_void_p, C.c_int, ull]), "ssp_stream_pub_n": (C.c_int, [C.c_void_p]), "ssp_init": (None, [C.c_void_p]),
        "ssp_bind": (None, [C.c_void_p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_int]), "ssp_unbind": (None, [C.c_void_p, C.c_int]),
        "ssp_msg": (None, [C.c_void_p, C.c_ulonglong, C.c_int, C.c_ulonglong]), "ssp_transport": (None, [C.c_void_p, C.c_int]),
        "ssp_block": (C.c_uint, [C.c_void_p, C.c_uint, C.c_int]), "ssp_get": (None, [C.c_void_p, ull])})


def _get(P, st):
    o = (C.c_ulonglong * 10)()
    P.ssp_get(st, o)
    return dict(W=o[0], C=o[1], E=o[2], U=o[3], flags=o[4], playing=bool(o[5]), playhead=o[6], has_loop=o[7], loop=(o[8], o[9]))


def _model_voice(F, pv=100.0):
    e = sm.StreamRefEngine(max_block_frames=F)
    s = e.sampler(pv)
    e.connect_stereo(s, e.graph_out_node)
    e.update()
    return e, s


@pytest.mark.parametrize("seed", range(8))
def test_state_machine_equals_the_model(seed):
    """fwgpu_types.h smp_stream_bind / _msg / _starved / _block_data / _behind_block and smp_pause / smp_stop — the functions the
    kernels compile — against StreamSamplerNode over a seeded schedule of writes, calls, pauses, stops, mutes and an end: C, U,
    playing, finished and the playhead are equal after every block; so is which blocks were starved and how much of the end block is
    data"""
    P = _peek_lib()
    rng = np.random.default_rng(900 + seed)
    F = int(rng.choice([16, 64]))
    R = int(rng.choice([4 * F, 4 * F + 5, 7 * F + F // 2]))
    e, s = _model_voice(F)
    node = e.nodes[s]
    ring = e.new_stream(P_F32, 2, R)
    st = C.create_string_buffer(128)
    P.ssp_init(st)
    pre = int(rng.integers(0, 2 * F))
    ring.write(np.ones((pre, 2), dtype=F32))
    e.sampler_set_stream(s, ring)
    P.ssp_bind(st, 0, R, ring.written, 0)
    e.sampler_play(s)
    P.ssp_transport(st, 0)
    starved = played = 0
    muted = False
    for blk in range(260):
        r = rng.random()
        # the writer: between blocks, with the consumed count as the model has it (an exact count is the least lagging one)
        if not ring.ended and r < 0.35:
            n = ring.write(np.full((int(rng.integers(0, 3 * F)), 2), 0.5, dtype=F32))
            if n:
                P.ssp_msg(st, ring.written, 0, 0)
        elif not ring.ended and blk > 200 and r < 0.45:
            if ring.end():
                P.ssp_msg(st, ring.written, 1, ring.written - F)
        t = rng.random()
        if t < (0.06 if node.playing else 0.4):
            (e.sampler_pause if node.playing else e.sampler_play)(s)
            P.ssp_transport(st, 1 if node.playing else 0)
        elif t > 0.97:
            e.sampler_stop(s)
            P.ssp_transport(st, 2)
        elif 0.5 < t < 0.55:
            muted = not muted
            e.set_param(s, 0, 0.0 if muted else 100.0)
        # (the smoother needs blocks to settle: the helper's `muted` is "the playhead holds", which the model decides)
        ph0, c0 = node.playhead, node.C
        u0 = node.U
        e.process_blocks(1)
        holds = node.playhead == ph0
        what = P.ssp_block(st, F, 1 if holds else 0)
        g = _get(P, st)
        assert (g["C"], g["U"], g["playing"], bool(g["flags"] & 4), g["playhead"]) == (node.C, node.U, node.playing, node.finished, node.playhead), (seed, blk)
        assert g["has_loop"] == 1 and g["loop"] == (0, R) and g["W"] == node.W
        assert (what & 0xff) == (1 if node.U != u0 else what & 0xff)
        starved += node.U != u0
        played += node.C != c0
    assert played >= 40 and starved >= 3, (played, starved)


def test_state_machine_end_block_and_leaving_a_stream():
    P = _peek_lib()
    st = C.create_string_buffer(128)
    P.ssp_init(st)
    P.ssp_bind(st, 3, 256, 0, 1)
    P.ssp_transport(st, 0)
    assert P.ssp_block(st, 64, 0) == 1 and _get(P, st)["U"] == 1          # nothing written: starved, playing stays 1
    assert _get(P, st)["playing"]
    P.ssp_msg(st, 64 + 17 + 64, 1, 64 + 17)                                # 81 frames of data + the padding
    assert P.ssp_block(st, 64, 0) == (2 | (64 << 8))
    assert P.ssp_block(st, 64, 0) == (2 | (17 << 8))                       # the end block: 17 frames of data
    g = _get(P, st)
    assert (g["C"], g["playing"], g["flags"] & 4, g["playhead"]) == (128, False, 4, 128)   # stopped where it stands, finished
    P.ssp_transport(st, 0)
    assert not _get(P, st)["playing"]                                      # play on a finished stream is ignored
    P.ssp_unbind(st, 5)
    g = _get(P, st)
    assert (g["flags"], g["has_loop"], g["playhead"], g["W"], g["C"]) == (0, 0, 0, 0, 0)
    P.ssp_msg(st, 1000, 0, 0)
    assert _get(P, st)["W"] == 0                                           # a sampler that holds no stream ignores the message


def test_state_machine_a_late_end_finishes_at_the_message():
    """an end that arrives when every frame has been played (E <= C) finishes the sampler where the message is applied: no block of
    padding is played behind it, C stays at E"""
    P = _peek_lib()
    st = C.create_string_buffer(128)
    P.ssp_init(st)
    P.ssp_bind(st, 3, 256, 64, 0)
    P.ssp_transport(st, 0)
    assert P.ssp_block(st, 64, 0) == (2 | (64 << 8)) and _get(P, st)["C"] == 64
    assert P.ssp_block(st, 64, 0) == 1 and _get(P, st)["U"] == 1          # all played, no end yet: starved
    P.ssp_msg(st, 64 + 64, 1, 64)                                          # the end, late: W covers the padding
    g = _get(P, st)
    assert (g["C"], g["U"], g["playing"], g["flags"] & 4, g["playhead"]) == (64, 1, False, 4, 64)
    assert P.ssp_block(st, 64, 0) == 0 and _get(P, st)["C"] == 64          # not a rendered block
    P.ssp_transport(st, 0)
    assert not _get(P, st)["playing"]
    # ... and in the model
    e, s = _model_voice(64)
    node = e.nodes[s]
    ring = e.new_stream(P_F32, 2, 256)
    ring.write(np.ones((64, 2), dtype=F32))
    e.sampler_set_stream(s, ring)
    e.sampler_play(s)
    e.process_blocks(2)
    assert (node.C, node.U, node.finished) == (64, 1, False)
    assert ring.end()
    e.process_blocks(1)
    assert (node.C, node.U, node.finished, bool(node.playing)) == (64, 1, True, False)


# ================================================================================================ CPU tier 2: the host half
def _host(F=64, update=True, **kw):
    e = HostOnlyEngine(max_block_frames=F, **kw)
    s = e.sampler(100.0)
    e.connect_stereo(s, e.graph_out_node)
    if update:
        e.update()
    return e, s


def _rc(e, fn, *a):
    return getattr(e.cx.L, fn)(e.cx.c, *a)


def _status(e, sid):
    w, c, u, f = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    assert _rc(e, "fwgpu_sample_stream_status", sid, C.byref(w), C.byref(c), C.byref(u), C.byref(f)) == 0
    return w.value, c.value, u.value, f.value


def _write(e, sid, fmt, rows):
    a = sm.layout(fmt, rows.shape[1], rows)
    return _rc(e, "fwgpu_sample_stream_write", sid, a.ctypes.data_as(C.c_void_p), rows.shape[0])


def test_host_refusals():
    e, s = _host()
    L = e.cx.L
    assert _rc(e, "fwgpu_sample_create_stream", P_F32, 2, 4 * 64 - 1) == INVALID          # R too small
    assert _rc(e, "fwgpu_sample_create_stream", P_F32, 2, (1 << 30) + 1) == INVALID       # ... too large
    assert _rc(e, "fwgpu_sample_create_stream", 6, 2, 1024) == INVALID and _rc(e, "fwgpu_sample_create_stream", P_F32, 0, 1024) == INVALID
    sid = _rc(e, "fwgpu_sample_create_stream", P_F32, 2, 4 * 64)
    assert sid >= 0
    plain = e.new_sample(P_F32, 2, np.zeros((2, 100), dtype=F32))
    assert _rc(e, "fwgpu_sample_stream_write", plain, None, 0) == INVALID                   # not a stream
    assert _rc(e, "fwgpu_sample_stream_end", plain) == INVALID
    # a FIR or resampler node on a stream
    for kind in (fwapi.FIR, fwapi.RESAMPLER):
        p = (C.c_float * 4)(float(sid), 1.0, 0.0, 1.0)
        assert L.fwgpu_add_node(e.cx.c, kind, 0 if kind == fwapi.RESAMPLER else 2, 2, p, 4) == INVALID
    # bound once, to one sampler
    s2 = e.sampler(100.0)
    assert _rc(e, "fwgpu_sampler_set_sample", s, sid, 0, 0) == 0
    assert _rc(e, "fwgpu_sampler_set_sample", s, sid, 0, 0) == INVALID
    assert _rc(e, "fwgpu_sampler_set_sample", s2, sid, 0, 0) == INVALID
    # seek and loop messages on the bound sampler (and not on another one)
    assert _rc(e, "fwgpu_sampler_set_playhead_secs", s, 0.5, 0) == INVALID
    assert _rc(e, "fwgpu_sampler_set_loop_range", s, 1, 0.0, 0.0, 0) == INVALID
    assert _rc(e, "fwgpu_sampler_set_playhead_secs", s2, 0.5, 0) == 0
    # end without room, then with; a write and a second end after it
    rows = rows_for(P_F32, 2, 4 * 64 - 10, 1)
    assert _write(e, sid, P_F32, rows) == 4 * 64 - 10
    assert _rc(e, "fwgpu_sample_stream_end", sid) == QUEUE_FULL
    sid2 = _rc(e, "fwgpu_sample_create_stream", P_F32, 2, 4 * 64)
    assert _write(e, sid2, P_F32, rows[:100]) == 100
    assert _rc(e, "fwgpu_sample_stream_end", sid2) == 0
    assert _write(e, sid2, P_F32, rows[:10]) == INVALID and _rc(e, "fwgpu_sample_stream_end", sid2) == INVALID
    assert _status(e, sid2) == (100, 0, 0, 0)
    # setting another sample on the sampler leaves the stream finished; then seek is accepted again
    assert _rc(e, "fwgpu_sampler_set_sample", s, plain, 0, 0) == 0
    assert _status(e, sid)[3] == 1 and _write(e, sid, P_F32, rows[:1]) == INVALID
    assert _rc(e, "fwgpu_sampler_set_playhead_secs", s, 0.5, 0) == 0
    # removing the node does the same
    sid3 = _rc(e, "fwgpu_sample_create_stream", I_I16, 2, 4 * 64)
    assert _rc(e, "fwgpu_sampler_set_sample", s2, sid3, 0, 0) == 0 and _status(e, sid3)[3] == 0
    e.remove_node(s2)
    assert _status(e, sid3)[3] == 1
    assert e.violation() == ""


def test_host_what_a_write_queues():
    """a sampler no plan holds yet keeps its messages on the control side, where the helper can read them: the binding carries R and
    the W of that moment, every write one CMD_SMP_STREAM with the new W (at_block 0, behind the data: the ring's bytes are there when
    the call returns), the end one more with E"""
    P = _peek_lib()
    e, s = _host(update=False)
    assert P.fwp_layout_check(e.cx.c, 48000, 64, 0, 2, 0) == 0
    sid = _rc(e, "fwgpu_sample_create_stream", I_I16, 2, 300)
    rows = rows_for(I_I16, 2, 500, 2)
    assert _write(e, sid, I_I16, rows[:70]) == 70 and P.fwp_early_count(e.cx.c) == 0       # before a sampler holds it: the ring alone
    assert _rc(e, "fwgpu_sampler_set_sample", s, sid, 1, 0) == 0

    def msg(i, eng=e):
        """[type, block, i0, i1, d0 bits, d1 bits]"""
        w = fwapi.early_msgs(P, eng.cx.c)[i]
        return [w[0], w[1], w[3], w[4], w[5] | (w[6] << 32), w[7] | (w[8] << 32)]

    assert P.fwp_early_count(e.cx.c) == 1
    assert msg(0)[:6] == [10, 0, sid, 1, 300, 70]                                          # CMD_SMP_SET_SAMPLE: stop flag, R, W
    assert _write(e, sid, I_I16, rows[70:170]) == 100
    assert P.fwp_early_count(e.cx.c) == 2 and msg(1)[:6] == [sm.CMD_SMP_STREAM, 0, 0, 0, 170, 0]
    got = C.create_string_buffer(170 * 4)
    assert P.ssp_ring_bytes(e.cx.c, sid, 0, 170 * 4, got)
    assert got.raw == rows[:170].tobytes()
    assert _rc(e, "fwgpu_sample_stream_end", sid) == 0
    assert P.fwp_early_count(e.cx.c) == 3 and msg(2)[:6] == [sm.CMD_SMP_STREAM, 0, 1, 0, 170 + 64, 170]
    assert _status(e, sid) == (170, 0, 0, 0)
    # a plain sample's binding carries no stream payload
    e2, s2 = _host(update=False)
    plain = e2.new_sample(P_F32, 2, np.zeros((2, 100), dtype=F32))
    assert _rc(e2, "fwgpu_sampler_set_sample", s2, plain, 0, 0) == 0
    assert msg(0, e2)[:6] == [10, 0, plain, 0, 0, 0]


@pytest.mark.parametrize("fmt", [I_I16, P_U16])
def test_host_write_splits_at_the_rings_end(fmt):
    """the ring's bytes, for an interleaved and a planar 16-bit format: a write that crosses the ring's end lands in two pieces (per
    channel for the planar format), a write larger than the free space is cut to it, and — planar — the source's channel c is read
    from c * frames whatever is accepted; free space never exceeds R - (written - consumed as published)"""
    P = _peek_lib()
    e, s = _host()
    R, ch = 4 * 64 + 24, 2
    sid = _rc(e, "fwgpu_sample_create_stream", fmt, ch, R)
    assert _rc(e, "fwgpu_sampler_set_sample", s, sid, 0, 0) == 0 and _rc(e, "fwgpu_sampler_play", s, 0) == 0
    rows = rows_for(fmt, ch, 3 * R, 3)
    assert _write(e, sid, fmt, rows[:200]) == 200
    assert _write(e, sid, fmt, rows[200:500]) == R - 200                                   # cut to the free space
    assert _write(e, sid, fmt, rows[:10]) == 0

    def ring():
        b = C.create_string_buffer(R * ch * 2)
        assert P.ssp_ring_bytes(e.cx.c, sid, 0, R * ch * 2, b)
        a = np.frombuffer(b.raw, dtype=sm.DTYPE[fmt])
        return a.reshape(R, ch) if fmt <= 2 else a.reshape(ch, R).T

    assert np.array_equal(ring(), rows[:R])
    # the harness renders nothing, so nothing is consumed: the published count stays 0 and so does the free space
    e.process_blocks(2)
    assert _status(e, sid) == (R, 0, 0, 0) and _write(e, sid, fmt, rows[:10]) == 0
    rec = (C.c_ulonglong * 9)()
    assert P.ssp_stream_rec(e.cx.c, sid, rec) and rec[7] >= 1 and P.ssp_stream_pub_n(e.cx.c) == 1
    assert e.violation() == ""


def test_host_write_wraps_with_a_consumed_count(tmp_path):
    """... and with a consumed count: the stand-alone program plays the sampler itself (CPU tier 3 below runs it under the
    sanitizers; here one seed without them is enough to see the wrap in the ring's bytes checked frame by frame)"""
    exe = str(tmp_path / "stream_driver")
    _build_driver(exe, [])
    r = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stream-driver ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_host_full_message_ring():
    """the sampler's message ring holds 128 messages between two drains: the write that finds it full returns FWGPU_ERR_QUEUE_FULL
    and leaves `written` where it was; after a process call the same call succeeds"""
    e, s = _host()
    sid = _rc(e, "fwgpu_sample_create_stream", P_F32, 2, 1 << 12)
    assert _rc(e, "fwgpu_sampler_set_sample", s, sid, 0, 0) == 0
    rows = rows_for(P_F32, 2, 300, 4)
    for i in range(127):
        assert _write(e, sid, P_F32, rows[i:i + 1]) == 1
    assert _write(e, sid, P_F32, rows[127:140]) == QUEUE_FULL
    assert _status(e, sid)[0] == 127
    assert _rc(e, "fwgpu_sample_stream_end", sid) == QUEUE_FULL and _status(e, sid)[0] == 127
    e.process_blocks(1)
    assert _write(e, sid, P_F32, rows[127:140]) == 13 and _status(e, sid)[0] == 140
    assert _rc(e, "fwgpu_sample_stream_end", sid) == 0


def test_host_an_end_that_found_the_message_ring_full_at_the_binding_can_be_sent_again():
    """a stream ended before it is bound sends its end behind the binding; where the sampler's ring has room for the binding alone the
    binding stands, the call returns FWGPU_ERR_QUEUE_FULL, and fwgpu_sample_stream_end — refused on an ended stream otherwise — delivers
    the end once there is room"""
    e, s = _host()
    sid = _rc(e, "fwgpu_sample_create_stream", P_F32, 2, 4 * 64)
    assert _write(e, sid, P_F32, rows_for(P_F32, 2, 30, 5)) == 30
    assert _rc(e, "fwgpu_sample_stream_end", sid) == 0
    assert _rc(e, "fwgpu_sample_stream_end", sid) == INVALID                # ended, not bound: nothing to repeat
    for _ in range(127):
        assert _rc(e, "fwgpu_sampler_play", s, 0) == 0
    assert _rc(e, "fwgpu_sampler_set_sample", s, sid, 0, 0) == QUEUE_FULL    # the 128th message is the binding; the end found no room
    assert _rc(e, "fwgpu_sampler_set_sample", s, sid, 0, 0) == INVALID       # ... and the binding stands
    assert _rc(e, "fwgpu_sampler_set_playhead_secs", s, 0.5, 0) == INVALID
    assert _rc(e, "fwgpu_sample_stream_end", sid) == QUEUE_FULL              # still full
    e.process_blocks(1)
    assert _rc(e, "fwgpu_sample_stream_end", sid) == 0                       # delivered
    assert _rc(e, "fwgpu_sample_stream_end", sid) == INVALID                 # once
    assert _status(e, sid)[0] == 30
    assert e.violation() == ""


def test_host_destroying_a_bound_stream_frees_its_sampler():
    """fwgpu_sample_destroy of a bound stream: the sampler holds a stream no longer, seek and loop messages are accepted again"""
    e, s = _host()
    sid = _rc(e, "fwgpu_sample_create_stream", P_F32, 2, 4 * 64)
    assert _rc(e, "fwgpu_sampler_set_sample", s, sid, 0, 0) == 0
    assert _rc(e, "fwgpu_sampler_set_playhead_secs", s, 0.5, 0) == INVALID
    e.process_blocks(1)
    assert _rc(e, "fwgpu_sample_destroy", sid) == 0
    assert _rc(e, "fwgpu_sampler_set_playhead_secs", s, 0.5, 0) == 0
    assert _rc(e, "fwgpu_sampler_set_loop_range", s, 1, 0.0, 0.0, 0) == 0
    e.process_blocks(1)
    assert e.violation() == ""


def test_host_plans_keep_their_kind_and_a_bound_stream_keeps_the_resident_kernel_out():
    """a stream changes no plan: the bank stays the voice-bank plan, the chain the chain plan; one-block callbacks with a stream bound
    never ring the resident kernel's doorbell"""
    for variant, kind in (("bank", 1), ("chain", 2), ("hybrid", 3)):
        e = HostOnlyEngine(max_block_frames=B, max_batch=4)
        _build(e, variant, PLANS[variant][1], PLANS[variant][2], P_F32, 2, 300, None)
        assert e.cx.plan_kind() == kind, variant
    e = HostOnlyEngine(max_block_frames=B)
    v = _build(e, "bank", 6, [1], P_F32, 2, 300, None)
    for _ in range(6):
        e.process_interleaved(B)
    assert e.cx.rt_resident_stats() == (0, 0)
    assert e.violation() == ""


def test_names_and_ids_agree():
    """header, fwgpu_types.h, _lib.py and ffi.rs"""
    import firewheel_amd._lib as flib

    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    types = open(os.path.join(ROOT, "firewheel_amd", "csrc", "fwgpu_types.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "ffi.rs")).read()
    names = ["fwgpu_sample_create_stream", "fwgpu_sample_stream_write", "fwgpu_sample_stream_write_device", "fwgpu_sample_stream_end",
             "fwgpu_sample_stream_status"]
    for n in names:
        assert re.search(r"\bint %s\(fwgpu_ctx\* ctx" % n, hdr), n
        assert n in flib.SIGNATURES and re.search(r"pub fn %s\(" % n, ffi), n
    assert re.search(r"CMD_SMP_STREAM = 17\b", types) and re.search(r"CMD_SMP_FADE = 16\b", types) and "CMD_SMP_STREAM = 17" in hdr
    assert sm.CMD_SMP_STREAM == 17
    assert re.search(r"#define FWGPU_STREAM_RING_FRAMES_MAX 1073741824ull", hdr) and re.search(r"#define SMP_STREAM_RING_MAX \(1ull << 30\)", types)
    assert sm.RING_MAX == 1 << 30 and sm.RING_MIN_BLOCKS == 4
    assert re.search(r"#define FWGPU_STREAM_RING_MIN_BLOCKS 4\b", hdr) and re.search(r"#define SMP_STREAM_RING_MIN_BLOCKS 4u", types)
    assert len(flib.SIGNATURES["fwgpu_sample_stream_status"][1]) == 6


# ================================================================================================ CPU tier 3: the sanitizer program
def _build_driver(out, extra):
    srcs = [os.path.join(HARNESS, "stream_driver.cpp"), os.path.join(HARNESS, "launch_stubs.cpp")] + fwapi.host_sources()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wno-unused-function", "-I", os.path.join(HARNESS, "fakehip"),
                           "-I", os.path.join(ROOT, "include"), "-o", out] + extra + srcs)


def test_accounting_under_address_and_ub_sanitizers(tmp_path):
    """tests/host_harness/stream_driver.cpp: a program with its own main that drives the write / free-space / publish accounting over
    seeded schedules, built with -fsanitize=address,undefined and run as a child process (CPU only; nothing loaded into Python)"""
    exe = str(tmp_path / "stream_driver_asan")
    _build_driver(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "stream-driver ok: 6 seeds" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (
        r.stdout[-2000:], r.stderr[-6000:])


# ================================================================================================ graphs (GpuEngine / HostOnlyEngine / the model)
class Feed(object):
    """one streamed voice of an engine: the stream (the product's StreamSource, or the model's Ring), its data, how far it is written"""

    def __init__(self, e, sampler, fmt, ch, R, rows):
        self.e, self.sampler, self.fmt, self.ch, self.R, self.rows = e, sampler, fmt, ch, R, rows
        self.pos = 0
        self.ended = False
        self.model = hasattr(e, "new_stream")  # (the model, bare or tagged; the product's engines keep theirs on .cx)
        if self.model:
            self.src = e.new_stream(fmt, ch, R)
            e.sampler_set_stream(sampler, self.src)
        else:
            self.src = e.cx.new_stream(fmt, ch, R)
            e.sampler_set_sample(sampler, self.src.id)

    def write(self, n):
        """up to n frames of what is left -> frames accepted"""
        rows = self.rows[self.pos:self.pos + n]
        if len(rows) == 0:
            return 0
        got = self.src.write(rows) if self.model else self.src.write(sm.layout(self.fmt, self.ch, rows))
        self.pos += got
        return got

    def end(self):
        if self.model:
            self.ended = self.src.end()
        else:
            try:
                self.src.end()
                self.ended = True
            except Exception as ex:  # FWGPU_ERR_QUEUE_FULL: no room for the padding yet
                assert getattr(ex, "code", None) == QUEUE_FULL, ex
        return self.ended

    def feed_ahead(self):
        """write all that fits; behind the last frame, the end"""
        self.write(len(self.rows))
        if self.pos == len(self.rows) and not self.ended:
            self.end()

    def status(self):
        if self.model:
            n = self.src.node
            return (self.pos, n.C, n.U, n.finished)
        return self.src.status()


def _build(e, variant, n_voices, streamed, fmt, ch, R, rows_of, pv=80.0, other_frames=None):
    """`n_voices` voices under one SumNode ("level" / "bank": sampler -> volume [-> pan]; "chain": sampler -> biquad -> delay;
    "hybrid": the bank's bus is consumed twice, dry and through a delay, which no fused plan takes as a whole; "level" / "bank": two
    leaf SumNodes under a root SumNode, the tree the one-launch realtime kernels take).  Voices in `streamed`
    play a stream of ring R (rows_of(v) = their data; None: the stream is only bound), or — on a twin, streamed == "twin" — the same
    frames as a whole one-shot sample; the others loop a plain sample.  Returns {voice: Feed or sampler id}."""
    rng = np.random.default_rng(31)
    twin = streamed == "twin"
    ends, smps = [], []
    for v in range(n_voices):
        s = e.sampler(pv)
        if variant == "chain":
            bq = e.biquad(int(rng.integers(0, 3)), float(rng.uniform(300, 6000)), 0.707)
            e.connect_stereo(s, bq)
            cur = e.delay([64, 129, 300][v % 3] / 48000.0, feedback=float(rng.choice([0.0, 0.4])), mix=0.5)
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
    if variant in ("level", "bank"):
        half = (n_voices + 1) // 2
        m = e.sum(2)
        for i, part in enumerate((ends[:half], ends[half:])):
            leaf = e.sum(max(2, len(part)))
            for p, n in enumerate(part):
                e.connect_stereo(n, leaf, 2 * p)
            e.connect_stereo(leaf, m, 2 * i)
    else:
        m = e.sum(max(2, n_voices))
        for p, n in enumerate(ends):
            e.connect_stereo(n, m, 2 * p)
    if variant == "hybrid":
        dl = e.delay(0.004, 0.3, 1.0)
        e.connect_stereo(m, dl)
        top = e.sum(2)
        e.connect_stereo(m, top, 0)
        e.connect_stereo(dl, top, 2)
        e.connect_stereo(top, e.graph_out_node)
    else:
        e.connect_stereo(m, e.graph_out_node)
    e.update()
    out = {}
    for v in range(n_voices):
        if not twin and v in streamed:
            out[v] = Feed(e, smps[v], fmt, ch, R, rows_of(v) if rows_of else rows_for(fmt, ch, 0, 0))
        elif twin and v in rows_of.voices:
            rows = rows_of(v)
            e.sampler_set_sample(smps[v], e.new_sample(fmt, ch, sm.layout(fmt, ch, rows)))
            out[v] = smps[v]
        else:
            rows = rows_for(P_F32, 2, other_frames or 700 + 13 * v, 77 + v)
            e.sampler_set_sample(smps[v], e.new_sample(P_F32, 2, sm.layout(P_F32, 2, rows)))
            e.sampler_set_loop_range(smps[v], fwapi.LOOP_FULL)
            out[v] = smps[v]
        e.sampler_play(smps[v])
    return out


class RowsOf(object):
    def __init__(self, fmt, ch, frames, voices):
        self.fmt, self.ch, self.frames, self.voices = fmt, ch, frames, list(voices)

    def __call__(self, v):
        return rows_for(self.fmt, self.ch, self.frames, 11 * v + self.frames)


PLANS = {  # name -> (variant, voices, streamed voices, engine arguments, blocks per call or None: the case's K)
    "level": ("level", 3, [1], dict(force_generic=True), None),
    "bank": ("bank", 20, [2, 9, 17], dict(), None),
    "chain": ("chain", 6, [1, 4], dict(), None),
    "hybrid": ("hybrid", 8, [0, 5], dict(), None),
    "one_block": ("bank", 20, [2, 9, 17], dict(), 1),
}


def _fed_cases():
    cases = []
    for plan in PLANS:
        fmts = [(f, 2) for f in range(6)] + [(P_F32, 1), (I_I16, 1), (P_U16, 1)] if plan in ("bank", "level") else [(P_F32, 2), (I_I16, 2), (P_F32, 1)]
        for fmt, ch in fmts:
            for K in ((1, 3) if plan != "one_block" else (1,)):
                for extra in (24, 0):
                    for frames in (10 * B + 17, 10 * B):
                        cases.append(pytest.param(plan, fmt, ch, K, extra, frames, id="%s-%s-%dch-K%d-R+%d-%d" % (plan, FMT_NAMES[fmt], ch, K, extra, frames)))
    return cases


def _engines(plan, K):
    variant, n, streamed, kw, _ = PLANS[plan]
    mk = lambda: GpuEngine(max_block_frames=B, max_batch=max(K, 1), **kw)
    return variant, n, streamed, mk


@pytest.mark.gpu
@pytest.mark.parametrize("plan,fmt,ch,K,extra,frames", _fed_cases())
def test_fed_ahead_equals_a_one_shot(plan, fmt, ch, K, extra, frames):
    """a stream written ahead of the playhead between calls and then ended equals, bit for bit and flag for flag, a second context that
    holds the same frames as a whole sample played as a one-shot, the blocks behind the end included.  R = (K + 2) * 64 + 24 (the wrap
    falls inside a block) and (K + 2) * 64 (on an edge), at least the ABI's 4 * 64; 10 * 64 + 17 and 10 * 64 frames."""
    variant, n, streamed, mk = _engines(plan, K)
    R = max(K + 2, sm.RING_MIN_BLOCKS) * B + extra
    rows_of = RowsOf(fmt, ch, frames, streamed)
    s, t = mk(), mk()
    feeds = _build(s, variant, n, streamed, fmt, ch, R, rows_of)
    _build(t, variant, n, "twin", fmt, ch, R, rows_of)
    assert s.cx.plan_kind() == t.cx.plan_kind()
    calls = (frames // B + 4 + K - 1) // K
    for call in range(calls):
        for v in streamed:
            feeds[v].feed_ahead()
        a, fa = _run(s, K, plan)
        b, fb = _run(t, K, plan)
        assert np.array_equal(fwapi.bits(a), fwapi.bits(b)), (call, _first_diff(a, b))
        assert np.array_equal(fa, fb), call
    for v in streamed:
        w, c, u, fin = feeds[v].status()
        assert (w, u, fin) == (frames, 0, True) and frames <= c < frames + B, (v, w, c, u, fin)


def _run(e, K, plan):
    """K blocks -> (interleaved output, silence flags or None).  The one-block plan goes through the host-buffer call, which is what
    takes the one-launch realtime kernel (the flags variant of the device call does not)"""
    if plan == "one_block":
        return np.asarray(e.process_interleaved(K * B)), None
    a, f = e.process_blocks_flags(K)
    return a, np.asarray(f, dtype=bool)


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    d = np.nonzero(fwapi.bits(a) != fwapi.bits(b))[0]
    return None if len(d) == 0 else dict(first=int(d[0]), block=int(d[0]) // (2 * B), count=int(len(d)), got=float(a[d[0]]), want=float(b[d[0]]),
                                         max_abs=float(np.max(np.abs(a[d].astype(np.float64) - b[d].astype(np.float64)))))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("fmt", [I_I16, P_U16])
@pytest.mark.parametrize("plan", ["level", "bank"])
def test_end_block_with_the_wrap_in_front_of_the_end(plan, fmt, K):
    """the one place where the end block is not a one-shot's last block (include/fwgpu.h, rule 4): R = 4 * 64 + 24 and 4 * 64 + 41
    frames, so the end block starts at ring frame 256, the ring wraps 24 frames in and the end falls 41 frames in.  The 23 frames
    behind the end are read from the padding: 0.0 in a signed format, 0x8000 = 1.5e-5 in an unsigned one.  Against the model, which
    restates exactly that, on the level executor and the bank."""
    R, frames = 4 * B + 24, 4 * B + 41
    first = R - (frames // B) * B % R
    assert first < frames % B < B  # the wrap, then the end, inside the end block
    g, m, fg, fmod, streamed = _pair(plan, K, fmt, 2, R, frames)
    for call in range((frames // B + 3 + K - 1) // K):
        for feeds in (fg, fmod):
            for v in streamed:
                feeds[v].feed_ahead()
        _both(g, m, K, plan, call)
        for v in streamed:
            assert fg[v].status()[1:] == fmod[v].status()[1:], (call, v, fg[v].status(), fmod[v].status())
    for v in streamed:
        assert fg[v].status() == (frames, 5 * B, 0, True), (v, fg[v].status())


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["level", "bank", "one_block"])
def test_a_late_end_finishes_without_a_block_of_padding(plan):
    """the writer calls `end` two calls after the last frame was played: the blocks in between are starved (silent, counted), and the
    end finishes the sampler where it arrives — C stays at E, no block of padding is rendered.  Bit for bit and flag for flag the
    one-shot twin, which ended with its last frame."""
    K = PLANS[plan][4] or 3
    variant, n, streamed, mk = _engines(plan, K)
    frames = 10 * B
    R = max(K + 2, sm.RING_MIN_BLOCKS) * B + 24
    rows_of = RowsOf(P_I16, 2, frames, streamed)
    s, t = mk(), mk()
    feeds = _build(s, variant, n, streamed, P_I16, 2, R, rows_of)
    _build(t, variant, n, "twin", P_I16, 2, R, rows_of)
    calls_data = -(-(frames // B) // K)  # the call in which the last frame is played
    for call in range(calls_data + 4):
        for v in streamed:
            feeds[v].write(frames)
            if call == calls_data + 1:
                assert feeds[v].end()
        a, fa = _run(s, K, plan)
        b, fb = _run(t, K, plan)
        assert np.array_equal(fwapi.bits(a), fwapi.bits(b)), (call, _first_diff(a, b))
        assert np.array_equal(fa, fb), call
    for v in streamed:
        assert feeds[v].status() == (frames, frames, (calls_data + 1) * K - frames // B, True), (v, feeds[v].status())


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [P_F32, I_I16])
def test_queued_calls_without_a_sync_against_a_full_ring(fmt):
    """calls of K = 3 blocks queued with no host sync between them (fwgpu_process_blocks_device), the writer filling the ring to the
    last frame it is given before each: the free space it is given must never reach frames a queued call still has to read.  Every
    write makes the next call one with messages, which on this plan would otherwise take the control-ahead mode.  R = 3 * K * 64 + 24:
    a call waits for the publication of two calls back, so the count the writer sees lags by at most two calls and a ring of three
    calls is never starved.  Bit for bit the one-shot twin."""
    import torch

    K, calls = 3, 14
    frames = 36 * B + 17
    R = 3 * K * B + 24
    variant, n, streamed, mk = _engines("bank", K)
    rows_of = RowsOf(fmt, 2, frames, streamed)
    s, t = mk(), mk()
    feeds = _build(s, variant, n, streamed, fmt, 2, R, rows_of)
    _build(t, variant, n, "twin", fmt, 2, R, rows_of)
    per = K * B * 2
    buf = torch.full((calls * per,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    want = []
    for call in range(calls):
        for v in streamed:
            feeds[v].feed_ahead()
        s.cx.process_blocks_device(K, buf[call * per:].data_ptr(), 2)
        want.append(np.asarray(t.process_blocks(K)))
    s.cx.synchronize()
    got = buf.cpu().numpy()
    for call in range(calls):
        a = got[call * per:(call + 1) * per]
        assert np.array_equal(fwapi.bits(a), fwapi.bits(want[call])), (call, _first_diff(a, want[call]))
    for v in streamed:
        w, c, u, fin = feeds[v].status()
        assert (w, u, fin) == (frames, 0, True) and frames <= c < frames + B, (v, w, c, u, fin)


@pytest.mark.gpu
@pytest.mark.parametrize("plan,fmt,seed", [("level", P_F32, 0), ("bank", P_F32, 1), ("bank", I_I16, 2), ("chain", P_F32, 3), ("hybrid", I_I16, 4),
                                           ("one_block", P_F32, 5), ("level", P_U16, 6), ("bank", I_F32, 7)])
def test_starved_equals_a_twin_that_is_paused(plan, fmt, seed):
    """the writer falls behind for blocks chosen by a seed — a call of K = 3 in which only the first block's frames are there among
    them.  The twin holds the whole data as a one-shot, gets `pause` at each starved block and `play` at the block where the data
    arrives; no fades (a pause resets an envelope).  status reports exactly the starved block count and C."""
    rng = np.random.default_rng(500 + seed)
    K = PLANS[plan][4] or 3
    variant, n, streamed, mk = _engines(plan, K)
    streamed = streamed[:1]
    R, frames = 8 * B + 24, 14 * B
    rows_of = RowsOf(fmt, 2, frames, streamed)
    s, t = mk(), mk()
    feeds = _build(s, variant, n, streamed, fmt, 2, R, rows_of)
    twin = _build(t, variant, n, "twin", fmt, 2, R, rows_of)
    v = streamed[0]
    f = feeds[v]
    C = U = 0
    starved_now = False
    call = 0
    opening = [3] + [0] * (3 if K == 1 else 1) + [1]  # one call's worth, nothing (every block starved), one block alone
    while C < frames and call < 60:
        # what the writer delivers before this call: nothing, one block (the K = 3 call that runs dry after its first block), or plenty
        mode = opening[call] if call < len(opening) else int(rng.choice([0, 1, 3], p=[0.3, 0.3, 0.4]))
        have = f.pos - C
        room = R - B - have  # (the writer leaves room for the end's padding: the end is never late)
        if mode == 1 and have < B:
            f.write(B - have)
        elif mode == 3:
            f.write(max(0, min(K * B if call == 0 else int(rng.integers(2, 6)) * B, room)))
        if f.pos == frames and not f.ended:
            f.end()
        avail = f.pos - C + (B if f.ended else 0)
        for b in range(K):  # the twin's transport, block by block, from what the stream's sampler will find
            ok = avail >= B and C < frames
            if C >= frames:
                break
            if not ok and not starved_now:
                t.sampler_pause(twin[v], at_block=b)
                starved_now = True
            elif ok and starved_now:
                t.sampler_play(twin[v], at_block=b)
                starved_now = False
            if ok:
                avail -= B
                C += B
            else:
                U += 1
        a, fa = _run(s, K, plan)
        bb, fb = _run(t, K, plan)
        assert np.array_equal(fwapi.bits(a), fwapi.bits(bb)), (call, _first_diff(a, bb))
        assert np.array_equal(fa, fb), call
        w, c, u, fin = f.status()
        assert (c, u) == (C, U), (call, c, u, C, U)
        call += 1
    assert C >= frames and U >= 3 and f.status()[3], (C, frames, U, f.status(), f.pos, f.ended, call)


# ------------------------------------------------------------------------------------------------ against the model
def _pair(plan, K, fmt, ch, R, frames, streamed=None):
    variant, n, st, mk = _engines(plan, K)
    streamed = streamed or st
    rows_of = RowsOf(fmt, ch, frames, streamed)
    g = fm.GpuFade(mk())
    m = fm.Tagged(sm.StreamRefEngine(max_block_frames=B))
    fg = _build(g, variant, n, streamed, fmt, ch, R, rows_of)
    fmod = _build(m, variant, n, streamed, fmt, ch, R, rows_of)
    return g, m, fg, fmod, streamed


def _both(g, m, K, plan, note=None):
    a, fa = _run(g, K, plan)
    b, fb = m.process_blocks_flags(K)
    assert np.array_equal(fwapi.bits(a), fwapi.bits(b)), (note, _first_diff(a, b))
    assert fa is None or np.array_equal(fa, np.asarray(fb, dtype=bool)), note


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["level", "bank", "chain", "one_block"])
def test_with_the_other_voice_features(plan):
    """against the numpy model: a volume glide down to 0 and back (a volume of 0 sent later renders x * 0 through the ordinary path:
    the mute test needs an Inactive smoother, see test_a_muted_voice_holds_c), pause / play, stop (which acts as pause), and a fade
    out with then = STOP on a streaming voice — which leaves the stream where it stands, not finished"""
    K = PLANS[plan][4] or 3
    g, m, fg, fmod, streamed = _pair(plan, K, P_F32, 2, 12 * B + 24, 70 * B)
    v = streamed[0]
    script = {1: [("pv", 35.0, 1 % K)], 3: [("pv", 0.0, 0)], 8: [("pv", 90.0, 2 % K)], 9: [("pause", None, 1 % K)], 10: [("play", None, 0)],
              11: [("stop", None, 2 % K)], 12: [("play", None, 1 % K)], 13: [("fade", (0.0, 150, fm.STOP), 0)]}
    for call in range(18):
        for e, feeds in ((g, fg), (m, fmod)):
            f = feeds[v]
            f.write(min(3 * K * B, f.R - (f.pos - (f.status()[1]))))
            for what, arg, at in script.get(call, []):
                smp = f.sampler
                if what == "pv":
                    e.set_param(smp, 0, arg, at_block=at)
                elif what == "fade":
                    e.fade(smp, arg[0], arg[1], arg[2], at_block=at)
                else:
                    getattr(e, "sampler_" + what)(smp, at_block=at)
        _both(g, m, K, plan, call)
        sg, smod = fg[v].status(), fmod[v].status()
        assert sg[1:] == smod[1:], (call, sg, smod)
    assert not fg[v].status()[3]


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["level", "bank", "one_block"])
def test_a_muted_voice_holds_c(plan):
    """a muted stretch: a voice created at volume 0 is muted by the sampler's own test (an Inactive smoother below 1e-5) — its playhead
    holds, and so does C, with the frames there and no block starved; with the volume up C moves.  Against the model."""
    K = PLANS[plan][4] or 3
    variant, n, streamed, mk = _engines(plan, K)
    rows_of = RowsOf(P_I16, 2, 30 * B, streamed)
    g, m = fm.GpuFade(mk()), fm.Tagged(sm.StreamRefEngine(max_block_frames=B))
    fg = _build(g, variant, n, streamed, P_I16, 2, 8 * B, rows_of, pv=0.0)
    fmod = _build(m, variant, n, streamed, P_I16, 2, 8 * B, rows_of, pv=0.0)
    v = streamed[0]
    for call in range(8):
        for e, feeds in ((g, fg), (m, fmod)):
            feeds[v].write(2 * K * B)
            if call == 3:
                e.set_param(feeds[v].sampler, 0, 70.0, at_block=K - 1)
        _both(g, m, K, plan, call)
        sg, smod = fg[v].status(), fmod[v].status()
        assert sg[1:] == smod[1:], (call, sg, smod)
        if call < 3:
            assert sg[1:3] == (0, 0), (call, sg)
    assert fg[v].status()[1] > 0 and fg[v].status()[2] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["level", "bank"])
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_seeded_fuzz_against_the_model(plan, seed):
    """writes, starvation, transport, volumes and ends — late ones among them — on the level executor and the bank (FWGPU_FUZZ_SEEDS
    sets how many seeds)"""
    rng = np.random.default_rng(7000 + seed)
    K = int(rng.choice([1, 2, 4]))
    fmt = int(rng.integers(0, 6))
    ch = int(rng.choice([1, 2]))
    R = int(rng.choice([(K + 3) * B, max(K + 2, 4) * B + 24, 5 * B + 1])) if K <= 2 else (K + 2) * B + 24
    frames = int(rng.integers(9, 16)) * B + int(rng.choice([0, 17, 63]))
    g, m, fg, fmod, streamed = _pair(plan, K, fmt, ch, R, frames)
    for call in range(24):
        for v in streamed:
            n = int(rng.choice([0, 0, B // 2, B, 2 * B, 4 * B]))
            want_end = rng.random() < 0.5
            acts = []
            r = rng.random()
            if r < 0.12:
                acts.append(("pause", None))
            elif r < 0.3:
                acts.append(("play", None))
            elif r < 0.36:
                acts.append(("stop", None))
            elif r < 0.5:
                acts.append(("pv", float(rng.choice([0.0, 20.0, 100.0]))))
            at = int(rng.integers(0, K))
            for e, feeds in ((g, fg), (m, fmod)):
                f = feeds[v]
                f.write(n)
                if f.pos == frames and not f.ended and want_end:
                    f.end()
                for what, arg in acts:
                    if what == "pv":
                        e.set_param(f.sampler, 0, arg, at_block=at)
                    else:
                        getattr(e, "sampler_" + what)(f.sampler, at_block=at)
            assert fg[v].pos == fmod[v].pos and fg[v].ended == fmod[v].ended, (call, v)
        _both(g, m, K, plan, (seed, call))
        for v in streamed:
            assert fg[v].status()[1:] == fmod[v].status()[1:], (seed, call, v, fg[v].status(), fmod[v].status())


# ------------------------------------------------------------------------------------------------ around it
@pytest.mark.gpu
def test_lazy_calls_stop_while_a_stream_plays_and_come_back_behind_its_end():
    """calls of two blocks (a one-block call of this tree belongs to the one-launch realtime kernel, which runs its own control and
    counts in neither column of fwgpu_lazy_stats)"""
    e = GpuEngine(max_block_frames=B, max_batch=4)
    frames = 20 * B
    feeds = _build(e, "bank", 20, [3], P_F32, 2, 8 * B, RowsOf(P_F32, 2, frames, [3]), other_frames=10 * B)  # (whole-block loops: lazy-capable)
    f = feeds[3]
    f.write(8 * B)
    for _ in range(3):
        e.process_blocks(2)
    lazy0, ctl0 = e.cx.lazy_stats()
    for _ in range(4):  # message-free calls with the stream bound: the control kernel runs every time
        e.process_blocks(2)
    lazy1, ctl1 = e.cx.lazy_stats()
    assert lazy1 == lazy0 and ctl1 == ctl0 + 4, (lazy0, ctl0, lazy1, ctl1)
    assert f.status()[1:3] == (8 * B, 6)  # 8 blocks written, 14 asked for: the last 6 starved
    for _ in range(12):
        f.feed_ahead()
        e.process_blocks(2)
    assert f.status()[3]
    lazy2, ctl2 = e.cx.lazy_stats()
    for _ in range(4):
        e.process_blocks(2)
    lazy3, ctl3 = e.cx.lazy_stats()
    assert lazy3 >= lazy2 + 3 and ctl3 <= ctl2 + 1, (lazy2, ctl2, lazy3, ctl3)


@pytest.mark.gpu
def test_resident_kernel_stays_out_while_a_stream_is_bound():
    e = GpuEngine(max_block_frames=B)
    frames = 6 * B
    feeds = _build(e, "bank", 20, [3], P_F32, 2, 8 * B, RowsOf(P_F32, 2, frames, [3]), other_frames=10 * B)
    f = feeds[3]
    f.feed_ahead()
    for _ in range(8):
        e.process_interleaved(B)
    assert e.cx.rt_resident_stats() == (0, 0)
    assert e.cx.rt_path_stats()[1] >= 7, e.cx.rt_path_stats()  # the callbacks took the one-launch kernel, one launch each
    assert f.status()[3]  # the control side has seen the end: the table entry is gone
    for _ in range(8):
        e.process_interleaved(B)
    launches, doorbells = e.cx.rt_resident_stats()
    assert launches >= 1 and doorbells >= 1, (launches, doorbells)


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
def test_graph_edit_in_mid_stream_carries_w_c_and_e(force_generic):
    """a graph edit with a plan install in mid-stream: the twin context is edited the same way and plays the whole sample"""
    mk = lambda: GpuEngine(max_block_frames=B, max_batch=2, force_generic=force_generic)
    frames = 9 * B + 17
    rows_of = RowsOf(P_I16, 2, frames, [1])
    s, t = mk(), mk()
    feeds = _build(s, "bank", 4, [1], P_I16, 2, 4 * B + 24, rows_of)
    _build(t, "bank", 4, "twin", P_I16, 2, 0, rows_of)
    f = feeds[1]
    for call in range(8):
        f.feed_ahead()
        if call == 2:
            for e in (s, t):  # a new voice into the graph: a new plan, installed by the next call
                smp = e.sampler(60.0)
                top = e.sum(2)
                e.connect_stereo(smp, top, 0)
                e.update()
        a, fa = s.process_blocks_flags(2)
        b, fb = t.process_blocks_flags(2)
        assert np.array_equal(fwapi.bits(a), fwapi.bits(b)), (call, _first_diff(a, b))
        assert np.array_equal(fa, fb)
    w, c, u, fin = f.status()
    assert (w, u, fin) == (frames, 0, True)


@pytest.mark.gpu
def test_write_device_from_a_torch_tensor_equals_write_from_numpy():
    import torch

    outs = []
    for dev in (False, True):
        e = GpuEngine(max_block_frames=B, max_batch=2)
        rows_of = RowsOf(P_F32, 2, 7 * B + 5, [0])
        feeds = _build(e, "bank", 3, [0], P_F32, 2, 5 * B, rows_of)
        f = feeds[0]
        got = []
        for call in range(6):
            rows = f.rows[f.pos:f.pos + (f.R - (f.pos - f.status()[1]))]
            if len(rows):
                a = sm.layout(P_F32, 2, rows)
                f.pos += f.src.write(torch.from_numpy(a).cuda() if dev else a)
            if f.pos == len(f.rows) and not f.ended:
                f.end()
            got.append(np.asarray(e.process_blocks(2)))
        assert f.status()[3]
        outs.append(np.concatenate(got))
    assert np.array_equal(fwapi.bits(outs[0]), fwapi.bits(outs[1])) and np.any(outs[0] != 0)


@pytest.mark.gpu
def test_a_bank_without_a_stream_renders_as_before():
    """the benched bank (1024 voices, block 256, 4096-frame sources) with no stream in it, in short calls: bit-identical to the oracle,
    which the parent's output equals, and its message-free calls still go lazy — which one bound stream would keep them from.  A guard:
    it holds on the parent too (the whole benched call is tests/test_gpu_benched_shapes.py's)"""
    import scenarios

    g = GpuEngine(max_block_frames=256, max_batch=4)
    o = scenarios.TaggedOracle(fwapi.OracleEngine(max_block_frames=256))
    a = scenarios.scenario_voice_bank_steady(g, 1024, 4, src_frames=4096)
    b = scenarios.scenario_voice_bank_steady(o, 1024, 4, src_frames=4096)
    assert g.cx.plan_kind() == 1 and np.array_equal(fwapi.bits(a), fwapi.bits(b))
    for _ in range(2):  # (the call behind the messages still runs the control kernel)
        g.process_blocks(4), o.process_blocks(4)
    lazy0, ctl0 = g.cx.lazy_stats()
    for _ in range(4):
        a, b = g.process_blocks(4), o.process_blocks(4)
        assert np.array_equal(fwapi.bits(a), fwapi.bits(b))
    lazy1, ctl1 = g.cx.lazy_stats()
    assert lazy1 >= lazy0 + 3 and ctl1 <= ctl0 + 1, (lazy0, ctl0, lazy1, ctl1)
