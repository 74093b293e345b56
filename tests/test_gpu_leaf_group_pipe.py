"""GPU tier (-m gpu): how a wave of the grouped kernel (k_leaf_group_lazy) streams a run of plain ports — whole batches
of U ports in straight-line code, the guarded body for what is left of a run, and port 0's copy decided once per run (k_leaf.hip.h
leaf_fast_pipe, LEAF_GROUP_PIPE).

Every scenario is built with fwapi on the oracle and twice on the product — a context created under FWGPU_LEAF_GROUP=1 and one under
FWGPU_LEAF_GROUP=0, FWGPU_LEAF_GROUP_MIN=1 in both so that calls of a few blocks are grouped — and runs a first call with the start
messages and then message-free calls: the loops are four blocks long, so lazy_blk0 advances and every loop wraps.  EVERY block of EVERY
call is compared bit for bit (uint32 view) with the oracle and between the two contexts, and group_stats() says the one-pass kernel
rendered calls of the first context (> 0) and none of the second (== 0).

The shapes are those at which the port loop takes another path: U = LEAF_GROUP_U = 8 ports in flight per wave."""
import numpy as np
import pytest

from fwapi import INTERLEAVED_I16, LOOP_FULL, PLANAR_F32, GpuEngine, OracleEngine, bits
from scenarios import voice_source
from test_gpu_leaf_group import LAZY_ON, group_env

pytestmark = pytest.mark.gpu

U = 8  # LEAF_GROUP_U (k_leaf.hip.h)


def build(e, leaf_ports, mbf, src_blocks=4, i16=(), prog=(), neg_zero=(), idle=()):
    """leaf_ports[l] voices (sampler -> volume -> [width -> hard clip] -> pan) under leaf mixer l, the leaves under one root mixer at
    graph_out.  i16: voices with an interleaved 16-bit source; prog: voices with a width and a hard-clip stage; neg_zero: voices whose
    source samples are all -0.0; idle: voices that are never started.  Every voice loops over src_blocks whole blocks."""
    rig = dict(samplers=[], volumes=[], leaves=[])
    v = 0
    for ports in leaf_ports:
        leaf = e.sum(ports)
        for p in range(ports):
            s = e.sampler(100.0 - (v % 7), n_out=2)
            vol = e.volume(35.0 + (v * 13) % 60)
            e.connect_stereo(s, vol)
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
            v += 1
        rig["leaves"].append(leaf)
    root = e.sum(len(leaf_ports))
    for l, leaf in enumerate(rig["leaves"]):
        e.connect_stereo(leaf, root, 2 * l)
    e.connect_stereo(root, e.graph_out_node)
    e.update()
    for v, s in enumerate(rig["samplers"]):
        data = voice_source(9000 + v, src_blocks * mbf, 2)
        if v in neg_zero:
            data = np.full_like(data, -0.0)
        if v in i16:
            e.sampler_set_sample(s, e.new_sample(INTERLEAVED_I16, 2, np.round(data * 32767).astype(np.int16).T.copy()))
        else:
            e.sampler_set_sample(s, e.new_sample(PLANAR_F32, 2, data))
        e.sampler_set_loop_range(s, LOOP_FULL)
        if v not in idle:
            e.sampler_play(s)
    return rig


def first_voice(leaf_ports, l):
    return sum(leaf_ports[:l])


def pause_at(call, voice):
    def script(e, rig, i):
        if i == call:
            e.sampler_pause(rig["samplers"][voice])
    return script


def ramp_at(call, voice):
    def script(e, rig, i):
        if i == call:
            e.set_param(rig["volumes"][voice], 0, 33.0)
    return script


MIXED = [1, U - 1, U, U + 1, 2 * U - 1, 2 * U, 31, 32]  # the guard-free body once, twice and four times over, with and without a guarded tail


def _scenarios():
    S = {}

    def add(name, leaf_ports, mbf=64, K=3, calls=4, script=None, after=None, **kw):
        # after: the first call from which a grouped call is expected again behind the script's message (None: calls 2 .. are grouped)
        S[name] = dict(leaf_ports=leaf_ports, mbf=mbf, K=K, calls=calls, script=script, after=after, kw=kw)

    # leaf sizes, in one tree
    add("sizes_block256", MIXED, mbf=256)
    add("sizes_block64", MIXED, mbf=64, K=4)
    add("sizes_reversed_block64", MIXED[::-1], mbf=64, K=2, calls=3)
    # leaf counts: uneven runs of the two waves, wave 1 empty, 2/3/4-port roots on the unmasked sum path
    add("leaves_1", [U + 1])
    add("leaves_2", [32, 2 * U + 1])
    add("leaves_3", [U, 2 * U, U + 1])
    add("leaves_4", [U, U + 1, 2 * U, U - 1])
    add("leaves_5", [2 * U, 1, 32, U, 2 * U + 1])
    add("leaves_32", [(1, U, 2 * U + 1, 32, U - 1)[l % 5] for l in range(32)], K=2, calls=3)
    # port 0 of a leaf: the copy (sum.rs:117) against an add — -0.0 samples, silent, paused while port 1 plays
    # (every source is -0.0, so the sign of each leaf's zero reaches the output: -0.0 + -0.0 = -0.0, anything + +0.0 = +0.0)
    lp = [U + 1, U]
    add("port0_negzero", lp, neg_zero=tuple(range(2 * U + 1)))
    add("port0_idle_rest_negzero", lp, neg_zero=tuple(range(2 * U + 1)), idle=(0,))
    add("port0_idle_two_port_leaf_negzero", [2, U], neg_zero=tuple(range(U + 2)), idle=(0,))
    add("port0_paused_port1_plays", lp, K=8, calls=14, script=pause_at(3, 0), after=4)
    # silent leaves: between two whole leaves; the first and the last leaf of a wave's run (8 leaves: wave 0 has 0-3, wave 1 has 4-7)
    lp = [2 * U, U, 32, U + 1, U, 2 * U, U, U + 1]
    sil = [v for l in (1, 3, 4, 6) for v in range(first_voice(lp, l), first_voice(lp, l) + lp[l])]
    add("silent_leaves_inside_and_at_run_ends", lp, idle=tuple(sil))
    lp = [U, 2 * U, U, U + 1, U, 2 * U]
    sil = [v for l in (0, 5) for v in range(first_voice(lp, l), first_voice(lp, l) + lp[l])]
    add("silent_first_and_last_leaf", lp, idle=tuple(sil))
    # broken runs: port 3 and port U of a 32-port leaf in front of a whole leaf
    lp = [32, 2 * U]
    for at in (3, U):
        add("paused_port%d" % at, lp, K=8, calls=14, script=pause_at(3, at), after=4)
        # (the gain smoother settles over some 5 500 frames, and the records come back behind that: 16 blocks of 64 frames per call)
        add("ramp_port%d" % at, lp, K=16, calls=14, script=ramp_at(3, at), after=4)
        add("i16_port%d" % at, lp, i16=(at,))
    # block sizes: four pieces; a last piece with idle lanes (260 = 256 + 4: one lane owns frames, the v_readlane operands were
    # pinned under the full exec mask); 64
    lp = [32, U + 1, 2 * U + 1, U, 1]
    add("block1024", lp, mbf=1024, K=2, calls=3)
    add("block260", lp, mbf=260, K=3)
    add("block64", lp, mbf=64, K=4)
    # stage programs: the PROG instantiation keeps its own path
    add("prog_sizes", MIXED, mbf=256, K=2, calls=3, prog=tuple(range(0, sum(MIXED), 2)))
    add("prog_block260", lp, mbf=260, K=2, calls=3, prog=tuple(range(0, sum(lp), 3)))
    return S


SCENARIOS = _scenarios()


def run(e, sc):
    rig = build(e, sc["leaf_ports"], sc["mbf"], **sc["kw"])
    outs, marks = [], []
    for i in range(sc["calls"]):
        if sc["script"] is not None:
            sc["script"](e, rig, i)
        o, f = e.process_blocks_flags(sc["K"])
        outs.append((np.asarray(o), np.asarray(f)))
        if hasattr(e, "cx"):
            marks.append(e.cx.group_stats())
    return outs, marks


def same(name, what, want, got, K):
    for i, ((w, wf), (o, of)) in enumerate(zip(want, got)):
        wb, ob = bits(w).reshape(K, -1), bits(o).reshape(K, -1)
        bad = [k for k in range(K) if not np.array_equal(wb[k], ob[k])]
        assert not bad, "%s, %s: call %d blocks %s differ (first word %d of block %d)" % (
            name, what, i, bad, int(np.flatnonzero(wb[bad[0]] != ob[bad[0]])[0]), bad[0])
        assert np.array_equal(wf, of), "%s, %s: call %d graph-output flags %s against %s" % (name, what, i, of.tolist(), wf.tolist())


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_grouped_port_runs_match_the_oracle_and_the_two_kernel_path(name):
    sc = SCENARIOS[name]
    want = run(OracleEngine(max_block_frames=sc["mbf"]), sc)[0]
    with group_env(1):
        g_on = GpuEngine(max_block_frames=sc["mbf"])
    with group_env(0):
        g_off = GpuEngine(max_block_frames=sc["mbf"])
    on, marks = run(g_on, sc)
    off, marks_off = run(g_off, sc)
    assert g_on.cx.plan_kind() == 1 and g_off.cx.plan_kind() == 1
    same(name, "grouped against the oracle", want, on, sc["K"])
    same(name, "switch off against the oracle", want, off, sc["K"])
    same(name, "grouped against switch off", off, on, sc["K"])
    assert marks_off[-1] == 0, marks_off
    if not LAZY_ON:
        return
    per_call = [marks[0]] + [marks[i] - marks[i - 1] for i in range(1, len(marks))]
    assert g_on.cx.group_stats() > 0, per_call
    if sc["after"] is None:
        assert all(per_call[2:]), per_call  # every message-free call behind the first two is a grouped one
    else:
        assert per_call[2] and any(per_call[sc["after"]:]), per_call  # ... and grouped calls come back behind the message
