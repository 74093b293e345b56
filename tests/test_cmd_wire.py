"""The wire format of control messages (fwgpu_types.h: struct Cmd, 40 bytes, and its makers): every bit of every message the C ABI
queues, pinned.

On a host-only context, with nodes that no plan holds yet, one call per message-queuing entry point and per branch of it; the ABI
keeps such messages on the control side (fwgpu_ctx::early_msgs), where tests/host_harness/early_peek.h reads them.  The nine words of
every message — type, block, the bits of f0, i0, i1, d0 (low, high), d1 (low, high) — are compared, in order, with
tests/golden/cmd_wire.json: this project's own recorded output, written once (`python tests/test_cmd_wire.py --write`) by the code
as it stood before the makers and readers existed.  A change to how a message is packed shows up here as a changed word, not as a
wrong coefficient in a kernel.  A new message type adds its calls to `calls()` and its lines to the golden file.

The values exercise the packing: negative and -0.0 floats, an infinite cutoff, steps and frames with bits set above 2^32 (a ring is at
most 2^30 frames and the harness consumes nothing, so a stream's R and W stay below 2^32 here; the compile-time round trips beside the
makers cover the full 64 bits).
"""
import json
import os
import sys

import numpy as np

import fwapi
from fwapi import HostOnlyEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cmd_wire.json")
CROSSFADE = 20
P_F32, I_I16 = 5, 0
LINEAR, BEZIER = 0, 1
FADE_NONE, FADE_PAUSE, FADE_STOP = 0, 1, 2
INF = float("inf")


def calls():
    """[(label, the nine words of each message the call queued)], in call order"""
    P = fwapi.peek_lib("rs_glide_peek")
    e = HostOnlyEngine(sample_rate=44100, max_block_frames=64)
    L, c = e.cx.L, e.cx.c
    assert P.fwp_layout_check(c, 44100, 64, 0, 2, 0) == 0
    plain = e.new_sample(P_F32, 2, np.zeros((2, 100), dtype=np.float32))
    vol, smp, beep, pan, width = e.volume(50.0), e.sampler(100.0), e.beep(), e.pan(0.0), e.width(1.0)
    bq, dl, rs, sp = e.biquad(0, 800.0, 2.0), e.delay(0.01), e.resampler(plain, 1.0, loop=True), e.spatial(1.0, 0.0, 1.0, n_in=2)
    xf = e.add_node(CROSSFADE, 4, 2, [])
    smp2 = e.sampler(100.0)
    out, seen = [], [0]

    def call(label, fn, *a):
        assert getattr(L, fn)(c, *a) == 0, (label, L.fwgpu_last_error(c).decode())
        msgs = fwapi.early_msgs(P, c)
        out.append((label, [list(w) for w in msgs[seen[0]:]]))
        seen[0] = len(msgs)

    sp_ = "fwgpu_node_set_param"
    call("volume", sp_, vol, 0, 37.5, 1)
    call("sampler gain", sp_, smp, 0, 80.0, 0)
    call("beep off", sp_, beep, 0, 0.0, 2)
    call("beep on", sp_, beep, 0, 1.0, 0xfffffffe)
    call("pan -0.6", sp_, pan, 0, -0.6, 3)
    call("width 1.7", sp_, width, 0, 1.7, 0)
    call("width -2 (clamped)", sp_, width, 0, -2.0, 4)
    call("biquad cutoff inf", sp_, bq, 1, INF, 0)
    call("biquad q", sp_, bq, 2, 3.0, 5)
    call("biquad cutoff", sp_, bq, 1, 1234.5, 0)
    call("delay feedback", sp_, dl, 1, 0.4, 6)
    call("delay mix", sp_, dl, 2, 0.3, 7)
    call("resampler ratio 200", sp_, rs, 1, 200.0, 0)
    call("resampler ratio 0.37", sp_, rs, 1, 0.37, 8)
    call("resampler pause", sp_, rs, 3, 0.0, 0)
    call("resampler play", sp_, rs, 3, 1.0, 9)
    call("resampler seek 3e9", sp_, rs, 4, 3e9, 0)
    call("resampler seek -1 (clamped)", sp_, rs, 4, -1.0, 10)
    call("spatial x", sp_, sp, 0, -3.0, 0)
    call("spatial y", sp_, sp, 1, 0.5, 11)
    call("spatial z", sp_, sp, 2, -0.25, 0)
    call("crossfade position", sp_, xf, 0, 0.25, 12)
    call("crossfade_to linear", "fwgpu_crossfade_to", xf, 0.75, 1000, LINEAR, 0.0, 0.0, 1.0, 1.0, 2)
    call("crossfade_to bezier", "fwgpu_crossfade_to", xf, 0.1, 1 << 24, BEZIER, 0.25, -1.0, 0.75, 2.0, 5)
    call("crossfade_to bezier -0.0", "fwgpu_crossfade_to", xf, -0.0, 7, BEZIER, -0.0, -0.0, 1.0, 1.5, 0)
    call("glide frames 0", "fwgpu_resampler_glide", rs, 0.37, 0, 13)
    call("glide", "fwgpu_resampler_glide", rs, 2.5, 1 << 24, 0)
    call("glide ratio 1e9 (clamped)", "fwgpu_resampler_glide", rs, 1e9, 1, 14)
    call("glide ratio -inf (clamped)", "fwgpu_resampler_glide", rs, -INF, 5, 0)
    call("sweep frames 0", "fwgpu_biquad_sweep", bq, 240.0, 0.9, 0, 15)
    call("sweep", "fwgpu_biquad_sweep", bq, 5000.0, 3.0, 1 << 24, 0)
    call("sweep cutoff inf", "fwgpu_biquad_sweep", bq, INF, 1.0, 4800, 16)
    call("set_sample plain", "fwgpu_sampler_set_sample", smp, plain, 0, 0)
    call("set_sample plain, stop", "fwgpu_sampler_set_sample", smp, plain, 1, 17)
    call("play", "fwgpu_sampler_play", smp, 18)
    call("pause", "fwgpu_sampler_pause", smp, 0)
    call("stop", "fwgpu_sampler_stop", smp, 19)
    call("fade", "fwgpu_sampler_fade", smp, 0.37, 480, FADE_PAUSE, 20)
    call("fade longest, stop", "fwgpu_sampler_fade", smp, 1.0, 1 << 24, FADE_STOP, 0)
    call("fade -0.0 step", "fwgpu_sampler_fade", smp, -0.0, 0, FADE_NONE, 21)
    call("playhead", "fwgpu_sampler_set_playhead_secs", smp, 1.25, 0)
    call("playhead negative", "fwgpu_sampler_set_playhead_secs", smp, -3.5, 22)
    call("playhead inf", "fwgpu_sampler_set_playhead_secs", smp, INF, 0)
    call("loop off", "fwgpu_sampler_set_loop_range", smp, 0, 0.0, 0.0, 23)
    call("loop full", "fwgpu_sampler_set_loop_range", smp, 1, 0.0, 0.0, 0)
    call("loop range", "fwgpu_sampler_set_loop_range", smp, 2, 0.5, 1.75, 24)
    sid = L.fwgpu_sample_create_stream(c, I_I16, 2, 300)
    assert sid >= 0
    rows = np.arange(340, dtype=np.int16).reshape(170, 2)
    assert L.fwgpu_sample_stream_write(c, sid, rows.ctypes.data_as(fwapi.C.c_void_p), 70) == 70
    call("set_sample stream", "fwgpu_sampler_set_sample", smp2, sid, 1, 0)
    assert L.fwgpu_sample_stream_write(c, sid, rows.ctypes.data_as(fwapi.C.c_void_p), 100) == 100
    out.append(("stream write", [list(w) for w in fwapi.early_msgs(P, c)[seen[0]:]]))
    seen[0] += len(out[-1][1])
    call("stream end", "fwgpu_sample_stream_end", sid)
    assert e.violation() == ""
    return out


def test_every_message_the_abi_queues_is_bit_for_bit_the_recorded_one():
    want = json.load(open(GOLDEN))
    got = calls()
    assert [g[0] for g in got] == [w["call"] for w in want]
    for (label, msgs), w in zip(got, want):
        assert msgs == w["msgs"], (label, [[hex(x) for x in m] for m in msgs], [[hex(x) for x in m] for m in w["msgs"]])
    # every entry point queued what it is documented to queue: no call without a message, the two- and three-message params in full
    n = {label: len(msgs) for label, msgs in got}
    assert min(n.values()) == 1 and n["pan -0.6"] == 2 and n["delay mix"] == 2 and n["spatial x"] == n["spatial y"] == n["spatial z"] == 3
    assert {m[0] for _, msgs in got for m in msgs} == {0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22, 23, 24, 25}   # every CMD_*


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", ".."))  # (the package, as the suite's conftest finds it)
        with open(GOLDEN, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps({"call": label, "msgs": msgs}) for label, msgs in calls()) + "\n]\n")
        print("wrote", GOLDEN)
