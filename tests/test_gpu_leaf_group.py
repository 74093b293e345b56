"""GPU tier (-m gpu): grouped calls — a steady (message-free) call of a voice-bank plan whose tree is leaves -> root -> stereo graph_out is
rendered by ONE kernel, k_leaf_group_lazy: a workgroup per (block, 256-frame piece) renders every leaf of the root, adds
them in the reference's order and writes the interleaved output; the leaf sums never go to memory and k_root_out does not run.

Every scenario builds its graph with fwapi on the oracle and on the product, runs a first call that carries the start messages and then
message-free calls (the second call still runs the control kernel: the call before it had messages), and compares EVERY block of EVERY
call with the oracle bit for bit (uint32 view).  It also asserts fwgpu_plan_group_stats: the number of launch batches the one-pass kernel
rendered is the number the scenario expects, so a dead path cannot pass.  The whole list runs a second time in a context created under
FWGPU_LEAF_GROUP=0: group_stats() == 0 and the same bits.  (FWGPU_LEAF_GROUP_MIN=1 in both: the size rule — fwgpu_ctx.h
group_min_items — would keep calls of 2, 5 and 16 blocks on the two-kernel path; test_leaf_group_host.py holds the rule's own test.)

The oracle's result of a scenario is computed once and shared by its two cases."""
import contextlib
import os

import numpy as np
import pytest

from fwapi import (INTERLEAVED_I16, LOOP_FULL, MONO_TO_STEREO, PLANAR_F32, GpuEngine, OracleEngine, bits)
from scenarios import voice_source

pytestmark = pytest.mark.gpu

LAZY_ON = os.environ.get("FWGPU_LAZY") != "0"


@contextlib.contextmanager
def group_env(on):
    """the environment a context is CREATED under (the switch is read there, like FWGPU_LAZY)"""
    keys = {"FWGPU_LEAF_GROUP": "1" if on else "0", "FWGPU_LEAF_GROUP_MIN": "1"}
    saved = {k: os.environ.get(k) for k in keys}
    os.environ.update(keys)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build(e, leaf_ports, mbf, src_blocks=4, fmts=None, m2s=(), prog=(), one_shot=None, neg_zero=False, idle=()):
    """leaf_ports[l] voices (sampler -> [mono to stereo] -> volume -> [width -> hard clip] -> pan) under leaf mixer l, the leaves under
    one root mixer, the root at graph_out.  fmts: {voice: sample format}; m2s: voices that are a one-output sampler behind MonoToStereo;
    prog: voices with a width and a hard-clip stage; one_shot: {voice: frames} (every other voice loops over src_blocks whole blocks);
    neg_zero: every source sample is -0.0; idle: voices that are never started."""
    fmts, one_shot = fmts or {}, one_shot or {}
    rig = dict(samplers=[], volumes=[], pans=[], leaves=[], mbf=mbf)
    v = 0
    for ports in leaf_ports:
        leaf = e.sum(ports)
        for p in range(ports):
            mono = v in m2s
            s = e.sampler(100.0 - (v % 7), n_out=1 if mono else 2)
            cur = s
            if mono:
                a = e.add_node(MONO_TO_STEREO, 1, 2)
                e.connect(s, 0, a, 0)
                cur = a
            vol = e.volume(35.0 + (v * 13) % 60)
            e.connect_stereo(cur, vol)
            cur = vol
            if v in prog:
                w = e.width(0.25 + 0.1 * (v % 5))
                h = e.hard_clip(-9.0 - (v % 3))
                e.connect_stereo(cur, w)
                e.connect_stereo(w, h)
                cur = h
            pan = e.pan(((v * 7) % 11 - 5) / 6.0)
            e.connect_stereo(cur, pan)
            e.connect_stereo(pan, leaf, 2 * p)
            rig["samplers"].append(s)
            rig["volumes"].append(vol)
            rig["pans"].append(pan)
            v += 1
        rig["leaves"].append(leaf)
    root = e.sum(len(leaf_ports))
    for l, leaf in enumerate(rig["leaves"]):
        e.connect_stereo(leaf, root, 2 * l)
    e.connect_stereo(root, e.graph_out_node)
    rig["root"] = root
    e.update()
    for v, s in enumerate(rig["samplers"]):
        frames = one_shot.get(v, src_blocks * mbf)
        ch = 1 if v in m2s else 2
        data = voice_source(7000 + v, frames, ch)
        if neg_zero:
            data = np.full_like(data, -0.0)
        fmt = fmts.get(v, PLANAR_F32)
        if fmt == INTERLEAVED_I16:
            raw = np.round(data * 32767).astype(np.int16).T.copy()
        else:
            raw = data
        e.sampler_set_sample(s, e.new_sample(fmt, ch, raw))
        if v not in one_shot:
            e.sampler_set_loop_range(s, LOOP_FULL)
        if v not in idle:
            e.sampler_play(s)
    return rig


def voices_of_leaf(leaf_ports, l):
    a = sum(leaf_ports[:l])
    return range(a, a + leaf_ports[l])


# ---- what happens between two calls (run alike on both engines)
def s_gain_and_pause(e, rig, i):
    if i == 4:
        e.set_param(rig["volumes"][1], 0, 33.0)
    if i == 14:
        e.sampler_pause(rig["samplers"][2])
    if i == 24:
        e.sampler_play(rig["samplers"][2])


def s_second_level(e, rig, i):
    """a plan install: a mixer between leaf 0 and the root — the tree is no longer leaves -> root"""
    if i == 4:
        mid = e.sum(2)
        e.disconnect(rig["leaves"][0], 0, rig["root"], 0)
        e.disconnect(rig["leaves"][0], 1, rig["root"], 1)
        e.connect_stereo(rig["leaves"][0], mid, 0)
        e.connect_stereo(mid, rig["root"], 0)
        e.update()


def lazy_calls(n_calls, msg_calls=(0,)):
    """the calls rendered without a control kernel: not one with messages, not the one behind it"""
    return [i for i in range(n_calls) if not any(i in (m, m + 1) for m in msg_calls)]


def batches(K, max_batch):
    return -(-K // max_batch) if max_batch else 1


# name -> dict(leaf_ports, mbf, K, calls, max_batch, flags, script, msg_calls, grouped (calls expected to be grouped), build kwargs)
def _scenarios():
    S = {}

    def add(name, leaf_ports, mbf, K, calls=5, max_batch=None, flags=False, script=None, msg_calls=(0,), grouped=None, **kw):
        g = lazy_calls(calls, msg_calls) if grouped is None else grouped
        S[name] = dict(leaf_ports=leaf_ports, mbf=mbf, K=K, calls=calls, max_batch=max_batch, flags=flags, script=script, grouped=g, kw=kw)

    # root and leaf widths; block lengths; batch sizes
    add("root1_copy", [3], 64, 2)
    add("root2_leaf32_leaf1", [32, 1], 256, 5)
    add("root3_last_leaf_narrow", [19, 3, 2], 64, 2)
    add("root4_unmasked", [3, 3, 3, 1], 256, 2)
    add("root5_two_pieces", [3, 1, 19, 2, 1], 512, 5)
    add("root32_four_pieces", [2] * 31 + [1], 1024, 2, calls=4)
    add("root5_K16", [3, 1, 19, 2, 1], 256, 16, calls=4)
    # (batches of 6, 6 and 4 blocks: a last batch of ONE block would be the realtime kernels', which leave no lazy records)
    add("root3_call_of_several_batches", [19, 3, 2], 64, 16, max_batch=6)
    # frames % 4 != 0: no port is VB_SIMPLE, and a SOUNDING voice leaves no lazy record at such a length (k_control.hip.h make_lazy: its
    # compact record needs frames % 4 == 0) — such calls keep their control kernel and are never grouped: the bits must match all the same.
    add("frames_not_a_multiple_of_4", [3, 2, 2, 2, 3], 250, 5, grouped=[])
    # ... a voice that is never started does (the silent branch), so a bank of them IS grouped at 250 frames: the kernel's last quad of a
    # block holds two frames (250 = 62 x 4 + 2: the frame-by-frame store of the output), and the result is +0.0 with both channels flagged
    add("every_voice_idle_frames_not_a_multiple_of_4", [3, 2, 2, 2, 3], 250, 5, flags=True, idle=tuple(range(12)))
    # silence and zeros (process_blocks_device_flags: the graph-output flags are compared too)
    add("one_voice_idle", [3, 3, 3, 3, 3], 64, 5, flags=True, idle=(4,))
    add("idle_leaf_added_root3_negzero", [2, 2, 2], 64, 5, flags=True, neg_zero=True, idle=(2, 3))
    add("idle_leaf_skipped_root5_negzero", [2, 2, 2, 2, 2], 64, 5, flags=True, neg_zero=True, idle=(2, 3))
    add("every_voice_idle", [3, 3, 3], 64, 5, flags=True, idle=tuple(range(9)))
    add("negzero_partials", [3, 2], 256, 2, flags=True, neg_zero=True)
    # sources and stages
    add("i16_interleaved", [4, 3, 5], 256, 5, fmts=dict([(v, INTERLEAVED_I16) for v in range(4)] + [(5, INTERLEAVED_I16), (8, INTERLEAVED_I16)]))
    add("mono_to_stereo_voice", [3, 3, 3, 3, 3], 64, 5, m2s=(1, 7))
    add("width_and_hard_clip", [5, 3, 19], 256, 5, prog=tuple(range(0, 27, 2)))
    # loops (4 blocks long: every call of 5 blocks crosses the wrap), one-shots and state
    add("one_shot_ends_in_third_call", [3, 3, 3, 3, 3], 64, 4, calls=7, one_shot={4: 2 * 4 * 64 + 64 + 17}, grouped="lazy")
    # (how many calls a message keeps the control kernel running depends on the smoothers: grouped == lazy call by call, and grouped calls
    #  come back behind each message)
    add("gain_then_pause_then_play", [3, 3, 3, 3, 3], 64, 8, calls=34, script=s_gain_and_pause, grouped="lazy")
    add("second_mixer_level_installed", [3, 3, 3, 3, 3], 64, 4, calls=8, script=s_second_level, msg_calls=(0,), grouped=[2, 3])
    # hand-off under uneven load: the waves of a workgroup finish at different times; every word of the output is checked
    lp = [32] * 32
    add("handoff_32x32_uneven", lp, 256, 64, calls=4, fmts={v: INTERLEAVED_I16 for l in range(32) for v in list(voices_of_leaf(lp, l))[:l % 4]})
    return S


SCENARIOS = _scenarios()
_oracle = {}


def run(e, sc):
    rig = build(e, sc["leaf_ports"], sc["mbf"], **sc["kw"])
    outs, marks = [], []
    for i in range(sc["calls"]):
        if sc["script"] is not None:
            sc["script"](e, rig, i)
        if sc["flags"]:
            o, f = e.process_blocks_flags(sc["K"])
            outs.append((np.asarray(o), np.asarray(f)))
        else:
            outs.append((np.asarray(e.process_blocks(sc["K"])), None))
        if hasattr(e, "cx"):
            marks.append((e.cx.group_stats(), e.cx.lazy_stats()[0]))
    return outs, marks


def oracle_of(name):
    if name not in _oracle:
        sc = SCENARIOS[name]
        _oracle[name] = run(OracleEngine(max_block_frames=sc["mbf"]), sc)[0]
    return _oracle[name]


@pytest.mark.parametrize("switch", [1, 0])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_grouped_calls_match_the_oracle_bit_for_bit(name, switch):
    sc = SCENARIOS[name]
    want = oracle_of(name)
    with group_env(switch):
        g = GpuEngine(max_block_frames=sc["mbf"], max_batch=sc["max_batch"])
    got, marks = run(g, sc)
    assert g.cx.plan_kind() == 1
    mbf = sc["mbf"]
    for i, ((w, wf), (o, of)) in enumerate(zip(want, got)):
        wb, ob = bits(w).reshape(sc["K"], -1), bits(o).reshape(sc["K"], -1)
        bad = [k for k in range(sc["K"]) if not np.array_equal(wb[k], ob[k])]
        assert not bad, "%s switch %d: call %d blocks %s differ (first word %d of block %d)" % (
            name, switch, i, bad, int(np.flatnonzero(wb[bad[0]] != ob[bad[0]])[0]), bad[0])
        if wf is not None:
            assert np.array_equal(wf, of), "%s switch %d: call %d graph-output flags %s, oracle %s" % (name, switch, i, of.tolist(), wf.tolist())
    if name.startswith("every_voice_idle"):
        assert all(not bits(o).any() for o, _ in got)  # +0.0, not -0.0
    per_call = [marks[0][0]] + [marks[i][0] - marks[i - 1][0] for i in range(1, len(marks))]
    lazy_per_call = [marks[0][1]] + [marks[i][1] - marks[i - 1][1] for i in range(1, len(marks))]
    if not switch or not LAZY_ON:
        assert g.cx.group_stats() == 0, per_call
        return
    nb = batches(sc["K"], sc["max_batch"])
    if sc["grouped"] == "lazy":
        assert per_call == lazy_per_call, (per_call, lazy_per_call)
        if name == "one_shot_ends_in_third_call":
            # the records hold up to the block the one-shot ends in: the third call (the first that could be lazy) is not, so it is not
            # grouped; what follows the end is grouped again as soon as it is lazy again
            assert per_call[2] == 0 and sum(per_call) > 0, (per_call, lazy_per_call)
        if name == "gain_then_pause_then_play":
            assert per_call[4] == per_call[14] == per_call[24] == 0, per_call
            # grouped calls before the gain message, and again behind the pause (a voice paused after it has played) and behind the play
            assert per_call[2] and per_call[3] and any(per_call[15:24]) and any(per_call[25:34]), "grouped batches per call: %s" % (per_call,)
        return
    assert per_call == [nb if i in sc["grouped"] else 0 for i in range(sc["calls"])], (name, per_call, lazy_per_call)
    if sc["grouped"] and name != "second_mixer_level_installed":
        assert per_call == lazy_per_call, (per_call, lazy_per_call)  # every lazy batch of an eligible plan is a grouped one
    assert mbf == g.max_block_frames
