"""The biquad's coefficient sweep (fwgpu_biquad_sweep, CMD_BQ_SWEEP = 25; SPEC): "move the cutoff over N frames" in
ONE message — the five coefficients travel linearly and per frame, inside the kernels that run the recurrence.

The reference is tests/bq_sweep_model.py: the SPEC's state machine, c(j) in numpy f32 — one separately rounded operation after the
other — and tests/refmodel.py's Direct Form I with each frame's own five values, inside a RefEngine.  Every comparison is `fwapi.bits`
equality: the arithmetic is a handful of f32 operations over exact integers, so there is no tolerance to choose.

CPU tier: the model's properties (c(0) = A, c(j) = T behind the end, monotone and inside, every (a1, a2) of a sweep inside the stability
triangle, finite output); the functions the kernels compile (fwgpu_types.h bq_sweep_*, built on the host) against the model; the ABI on
the host-only harness; the header, fwgpu_types.h, ffi.rs, nodes.rs and _lib.py agree; the typed mirror.

GPU tier (block 256, five calls of K = 3 blocks, the first and the last message-free): sweep lengths and start blocks, the interplay
with set_cutoff_hz / set_q and with other sweeps, the three filter types, bus biquads of 1, 2, 3 and 6 channels through the level
executor (a call that ends in a short block; force_generic; fwgpu_node_process), the batch walkers around a sweep, chain-plan voices of
five shapes, lazy calls around a sweep.  Every GPU case calls fwgpu_biquad_sweep.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bq_sweep_model as bm
import fwapi
import refmodel
from busnodes import assert_bits
from fwapi import LOOP_FULL, PLANAR_F32, PLANAR_I16, GpuEngine, HostOnlyEngine
from scenarios import voice_source

INVALID = -20
F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SR = 48000
LP, HP, BP = 0, 1, 2
F, K, N_CALLS = 256, 3, 5          # block, blocks per call, calls: call 0 and call 4 carry no message


def fbits(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def bits5(co):
    return [fbits(x) for x in co]


# ================================================================================================ CPU tier: the model's properties
def _extreme_sweeps():
    """(type, from, to) between the extremes the clamps allow (1 Hz and 0.49 fs) at Q = 4, both ways, and to a middle"""
    out = []
    for t in (LP, HP, BP):
        for a, b in ((1.0, 0.49 * SR), (0.49 * SR, 1.0), (1.0, 1000.0), (0.49 * SR, 300.0), (20000.0, 20.0)):
            out.append((t, a, b))
    return out


@pytest.mark.parametrize("N", [1, 2, 7, 1000])
def test_model_values_start_on_a_end_on_t_are_monotone_inside_and_stable(N):
    for t, f_from, f_to in _extreme_sweeps():
        A = np.array(refmodel.rbj_coefs(t, f_from, 4.0, SR), dtype=F32)
        T = np.array(refmodel.rbj_coefs(t, f_to, 4.0, SR), dtype=F32)
        sw = bm.Sweep(A)
        sw.start(T, N)
        assert bits5(sw.A) == bits5(A)                                       # the message takes A = c(0) under the old state: the head
        C5 = sw.values(N + 3)
        assert bits5(C5[0]) == bits5(A), (t, f_from, f_to)                   # c(0) equals A
        for j in (N, N + 1, N + 2):
            assert bits5(C5[j]) == bits5(T)                                  # c(j) == T bit for bit for k + j >= N
        lo, hi = np.minimum(A, T), np.maximum(A, T)
        assert np.all(C5 >= lo) and np.all(C5 <= hi)                         # every coordinate stays between its ends
        d = np.diff(C5.astype(np.float64), axis=0)
        for i in range(5):
            assert np.all(d[:, i] >= 0) if T[i] >= A[i] else np.all(d[:, i] <= 0), (t, i)   # ... and is monotone in j
        a1, a2 = C5[:, 3].astype(np.float64), C5[:, 4].astype(np.float64)
        assert np.all(np.abs(a2) < 1.0) and np.all(np.abs(a1) < 1.0 + a2), (t, f_from, f_to)   # the stability triangle
        # a function of k + j: the state moved on by 3 frames gives the same values
        if N > 3:
            sw2 = bm.Sweep(A)
            sw2.start(T, N)
            sw2.advance(3)
            assert fwapi.bits(sw2.values(N)).tolist() == fwapi.bits(C5[3:]).tolist()
        # the model's output stays finite (and is not silence) on a full-scale input
        x = voice_source(77, N + 300, 1)
        st = np.zeros((1, 4), dtype=F32)
        Call = np.concatenate([C5[:N], np.repeat(T[None, :], 300, axis=0)])
        y = bm.filter_rows(x, Call[None, :, :], st)
        assert np.all(np.isfinite(y)) and np.abs(y).max() < 1e3 and np.any(y != 0)


def test_model_retarget_set_coefs_and_the_end():
    A = np.array(refmodel.rbj_coefs(LP, 500.0, 2.0, SR), dtype=F32)
    T = np.array(refmodel.rbj_coefs(LP, 9000.0, 2.0, SR), dtype=F32)
    U = np.array(refmodel.rbj_coefs(LP, 60.0, 0.7, SR), dtype=F32)
    sw = bm.Sweep(A)
    sw.start(T, 700)
    sw.advance(256)
    mid = sw.values(1)[0]
    assert sw.k == 256 and np.all(mid != A) and np.all(mid != T)
    sw.start(U, 300)                                   # a retarget continues from where the sweep stands
    assert bits5(sw.A) == bits5(mid) and (sw.N, sw.k) == (300, 0) and bits5(sw.values(1)[0]) == bits5(mid)
    sw.advance(256)
    assert (sw.N, sw.k) == (300, 256)
    sw.advance(256)                                    # over: at rest, the head holds the target
    assert sw.at_rest() and bits5(sw.head) == bits5(U) and bits5(sw.values(2)[1]) == bits5(U)
    sw.start(T, 5000)
    sw.advance(100)
    sw.set_coefs(A)                                    # CMD_SET_COEFS during a sweep ends it and sets the coefficients
    assert sw.at_rest() and bits5(sw.values(1)[0]) == bits5(A)
    sw.start(T, 0)                                     # frames == 0: a step
    assert sw.at_rest() and bits5(sw.head) == bits5(T)


def _bus(e, nch, ftype=LP, cutoff=700.0, q=4.0, src_len=2048):
    """nch one-channel samplers (looping noise) -> an nch-channel biquad -> graph_out (an engine with nch graph outputs)"""
    b = e.biquad(ftype, cutoff, q, ch=nch)
    smps = []
    for c in range(nch):
        s = e.sampler(90.0, n_out=1)
        e.connect(s, 0, b, c)
        e.connect(b, c, e.graph_out_node, c)
        smps.append(s)
    e.update()
    for c, s in enumerate(smps):
        e.sampler_set_sample(s, e.new_sample(PLANAR_F32, 1, voice_source(900 + c, src_len + 37 * c, 1)))
        e.sampler_set_loop_range(s, LOOP_FULL)
        e.sampler_play(s)
    return b


def test_model_at_rest_is_the_biquad_of_refmodel_and_block_splits_do_not_matter():
    outs = {}
    for name, eng in (("ref", refmodel.RefEngine(max_block_frames=64, num_graph_outputs=2, short_blocks=True)), ("sweep", bm.SweepRefEngine(max_block_frames=64, num_graph_outputs=2, short_blocks=True))):
        b = _bus(eng, 2)
        eng.set_param(b, 1, 3000.0)
        outs[name] = eng.process_interleaved(500)
    assert_bits(outs["sweep"], outs["ref"], "no sweep: refmodel's biquad")
    runs = {}
    for name, blocks in (("one", [448]), ("64", [64] * 7), ("mixed", [1, 63, 100, 28, 256])):
        eng = bm.SweepRefEngine(max_block_frames=512, num_graph_outputs=2, short_blocks=True)
        b = _bus(eng, 2)
        eng.sweep(b, 9000.0, 1.0, 300)
        runs[name] = np.concatenate([eng.process_interleaved(n) for n in blocks])
    for name in runs:
        assert_bits(runs[name], runs["one"], name)     # c(j) depends on k + j alone
    assert np.any(runs["one"] != 0)


# ================================================================================================ CPU tier: the kernels' own statement
def _peek_lib():
    """tests/host_harness/bq_sweep_peek.cpp beside the harness library: the messages a ctx keeps for nodes no plan holds yet, the host's
    sweep book, and the sweep functions of fwgpu_types.h — the ones the kernels compile — built for the host"""
    up = C.POINTER(C.c_uint)
    return fwapi.peek_lib("bq_sweep_peek", {"bsp_sweep_book": (None, [C.c_void_p, C.POINTER(C.c_ulonglong)]), "bsp_values": (None, [up, up, C.c_uint, up]),
                                            "bsp_start": (C.c_int, [up, up, up, C.c_uint]), "bsp_advance": (C.c_int, [up, C.c_uint]),
                                            "bsp_unpack": (None, [up, up])})


def _st(sw):
    return (C.c_uint * 12)(*(bits5(sw.A) + bits5(sw.T) + [sw.N, sw.k]))


def _u5(co):
    return (C.c_uint * 5)(*bits5(co))


def test_the_kernels_own_statement_equals_the_model():
    """fwgpu_types.h bq_sweep_of / _put / _coef / _start / _advance, compiled for the host, against Sweep: values, the message (a retarget
    and a step included), the advance and the end — on the states a random run of messages and blocks passes through"""
    P = _peek_lib()
    rng = np.random.default_rng(31)
    ended = retargets = 0
    for case in range(40):
        rnd = lambda: refmodel.rbj_coefs(int(rng.integers(0, 3)), float(np.exp(rng.uniform(0, np.log(0.49 * SR)))), float(rng.choice([0.3, 0.707, 4.0, 12.0])), SR)
        sw = bm.Sweep(rnd())
        for step in range(25):
            if rng.random() < 0.4:
                N = int(rng.choice([0, 1, 2, 7, 255, 256, 257, 300, 700, 5000, 1 << 24]))
                T = np.array(rnd(), dtype=F32)
                st = _st(sw)
                retargets += sw.N != 0 and N != 0
                step_head = P.bsp_start(st, _u5(sw.head), _u5(T), N)
                sw.start(T, N)
                assert step_head == (N == 0)
                if N:
                    assert list(st) == bits5(sw.A) + bits5(sw.T) + [sw.N, sw.k], (case, step)
                else:
                    assert list(st)[10:] == [0, 0] and list(st)[5:10] == bits5(T)
            Fr = int(rng.choice([1, 37, 64, 100, 256]))
            st = _st(sw)
            got = (C.c_uint * (5 * Fr))()
            P.bsp_values(st, _u5(sw.head), Fr, got)
            assert list(got) == fwapi.bits(sw.values(Fr)).reshape(-1).tolist(), (case, step)
            was = sw.N
            over = P.bsp_advance(st, Fr)
            sw.advance(Fr)
            assert over == (was != 0 and sw.N == 0) and list(st)[10:] == [sw.N, sw.k], (case, step)
            if over:
                assert list(st)[5:10] == bits5(sw.head)            # the target the caller writes to the head
                ended += 1
    assert ended >= 20 and retargets >= 10


# ================================================================================================ CPU tier: the ABI on the harness
_early = fwapi.early_msgs


def test_abi_what_a_call_queues_and_what_it_refuses():
    """one Cmd per call: CMD_BQ_SWEEP with the target packed as CMD_SET_COEFS packs it and the frames in the bits of d1; frames == 0
    queues a plain CMD_SET_COEFS; the cutoff and Q stay with the node, so that a later set_param of Q alone starts from them"""
    P = _peek_lib()
    e = HostOnlyEngine(sample_rate=44100, max_block_frames=96, num_graph_inputs=3, num_graph_outputs=2)
    L, c = e.cx.L, e.cx.c
    assert P.fwp_layout_check(c, 44100, 96, 3, 2, 0) == 0
    assert P.fwp_layout_check(c, 44100, 64, 3, 2, 0) == 2       # (and it does look)
    b = e.biquad(HP, 800.0, 2.0)
    vol = e.volume(50.0)
    assert L.fwgpu_biquad_sweep(c, b, 5000.0, 3.0, bm.FRAMES_MAX, 0) == 0            # the longest sweep
    assert L.fwgpu_biquad_sweep(c, b, 120.0, 0.5, 1, 3) == 0
    assert L.fwgpu_biquad_sweep(c, b, 240.0, 0.9, 0, 2) == 0                        # a step
    assert L.fwgpu_node_set_param(c, b, 2, 6.0, 1) == 0                             # Q alone: the cutoff is the last sweep's, 240 Hz
    for bad, word in ((lambda: L.fwgpu_biquad_sweep(c, vol, 500.0, 1.0, 10, 0), "not a BiquadNode"),
                      (lambda: L.fwgpu_biquad_sweep(c, b, float("nan"), 1.0, 10, 0), "NaN"),
                      (lambda: L.fwgpu_biquad_sweep(c, b, 500.0, float("nan"), 10, 0), "NaN"),
                      (lambda: L.fwgpu_biquad_sweep(c, b, 500.0, 1.0, bm.FRAMES_MAX + 1, 0), "2^24"),
                      (lambda: L.fwgpu_biquad_sweep(c, 12345, 500.0, 1.0, 10, 0), "unknown node")):
        assert bad() == INVALID                                                     # a refused call queues nothing
        assert word in L.fwgpu_last_error(c).decode(), (word, L.fwgpu_last_error(c).decode())
    got = _early(P, c)
    want = [(bm.CMD_BQ_SWEEP, 0, refmodel.rbj_coefs(HP, 5000.0, 3.0, 44100), bm.FRAMES_MAX), (bm.CMD_BQ_SWEEP, 3, refmodel.rbj_coefs(HP, 120.0, 0.5, 44100), 1),
            (bm.CMD_SET_COEFS, 2, refmodel.rbj_coefs(HP, 240.0, 0.9, 44100), 0), (bm.CMD_SET_COEFS, 1, refmodel.rbj_coefs(HP, 240.0, 6.0, 44100), 0)]
    assert len(got) == len(want)
    for g, (typ, blk, co, frames) in zip(got, want):
        assert g[:2] == (typ, blk) and list(g[2:7]) == bits5(co) and g[7:] == (frames, 0), (g, typ, blk)
        un = (C.c_uint * 6)()
        P.bsp_unpack((C.c_uint * 9)(*g), un)                                        # ... and the kernels' unpacking gives them back
        assert list(un) == bits5(co) + [frames]
    # an infinity is a value like any other: the clamps of biquad_coefs take it
    assert L.fwgpu_biquad_sweep(c, b, float("inf"), 1.0, 10, 0) == 0
    assert list(_early(P, c)[-1][2:7]) == bits5(refmodel.rbj_coefs(HP, 0.49 * 44100, 1.0, 44100))
    e.connect_stereo(b, e.graph_out_node)
    e.update()                                                                      # the plan that activates the node releases them
    assert _early(P, c) == []
    e.process_blocks(4)
    assert e.violation() == ""


def _chain_bank(e, V, shapes, fmt=PLANAR_F32, leaf=20, src_len=2048):
    """V voices sampler -> filters -> volume under SumNodes of `leaf` ports -> graph_out; voice v has shape shapes[v % len]: a string of
    B (biquad) and D (delay).  Returns [(sampler, [the voice's biquads])]."""
    rng = np.random.default_rng(5)
    voices, ends = [], []
    for v in range(V):
        s = e.sampler(85.0)
        cur, bqs = s, []
        for ch in shapes[v % len(shapes)]:
            if ch == "B":
                n = e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 6000)), float(rng.choice([0.707, 2.0, 5.0])))
                bqs.append(n)
            else:
                n = e.delay([64, 129, 300][v % 3] / float(SR), feedback=float(rng.choice([0.0, 0.45])), mix=0.5)
            e.connect_stereo(cur, n)
            cur = n
        vol = e.volume(float(rng.uniform(40, 100)))
        e.connect_stereo(cur, vol)
        voices.append((s, bqs))
        ends.append(vol)
    mixers = []
    for i in range(0, V, leaf):
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
    for v, (s, _) in enumerate(voices):
        data = voice_source(4200 + v, src_len, 2)
        smp = e.new_sample(fmt, 2, np.round(data * 32767).astype(np.int16) if fmt == PLANAR_I16 else data)
        e.sampler_set_sample(s, smp)
        e.sampler_set_loop_range(s, LOOP_FULL)
        e.sampler_play(s)
    return voices


def test_harness_a_sweep_keeps_every_launch_in_order_and_the_host_counts_its_frames():
    """the host half on the harness: a chain plan with a sweep in flight launches its control kernel and nothing the launch stubs object to;
    the host's book (frames rendered, the frame behind which no sweep is in flight) follows the SPEC's count; lazy calls come back"""
    P = _peek_lib()
    e = bm.GpuSweep(HostOnlyEngine(max_block_frames=64, max_batch=4))
    voices = _chain_bank(e, 6, ["B", "BD"], leaf=8, src_len=64 * 8)
    assert e.cx.plan_kind() == 2
    book = (C.c_ulonglong * 3)()
    marks = []
    for call in range(10):
        if call == 3:
            e.sweep(voices[1][1][0], 5000.0, 2.0, 64 * 6 + 5, at_block=2)       # from frame 3*256 + 128 over 389 frames: into call 5
        e.process_blocks(4)
        P.bsp_sweep_book(e.cx.c, book)
        marks.append((e.cx.lazy_stats(), tuple(book)))
    assert e.violation() == ""
    end = 3 * 256 + 2 * 64 + 64 * 6 + 5
    assert [m[1][0] for m in marks] == [256 * (i + 1) for i in range(10)]
    assert [m[1][1] for m in marks] == [0] * 3 + [end] * 7
    assert [m[1][2] for m in marks] == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0], marks    # calls 3, 4, 5 may meet the sweep (it ends inside call 5)
    lazy, ctl = [m[0][0] for m in marks], [m[0][1] for m in marks]
    if os.environ.get("FWGPU_LAZY") != "0":
        assert lazy[2] > lazy[0], marks                                          # quiet calls in front of the sweep are lazy
        assert lazy[5] == lazy[2] and ctl[5] - ctl[2] == 3, marks                # a sweep in flight: the control kernel
        assert lazy[9] - lazy[6] == 3, marks                                     # ... and lazy again behind it


def test_header_types_ffi_and_lib_agree():
    import firewheel_amd._lib as flib

    rd = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr, types = rd("include", "fwgpu.h"), rd("firewheel_amd", "csrc", "fwgpu_types.h")
    ffi, nodes = rd("rust", "firewheel-gpu", "src", "ffi.rs"), rd("rust", "firewheel-gpu", "src", "nodes.rs")
    assert re.search(r"#define FWGPU_BIQUAD_SWEEP_FRAMES_MAX 16777216\b", hdr)
    assert "int fwgpu_biquad_sweep(fwgpu_ctx* ctx, int64_t node, float cutoff_hz, float q, uint32_t frames, uint32_t at_block);" in hdr
    assert re.search(r"CMD_BQ_SWEEP = 25\b", types) and re.search(r"CMD_SET_COEFS = 4\b", types) and re.search(r"#define BQ_SWEEP_FRAMES_MAX 16777216u", types)
    assert re.search(r"K_LAST = K_CROSSFADE\b", types)           # no new node kind
    for line in ("static_assert(sizeof(NodeState) == 128", "static_assert(sizeof(ChainStart) == 64", "static_assert(sizeof(Cmd) == 40"):
        assert line in types
    for name in ("bq_sweep_start", "bq_sweep_coef", "bq_sweep_advance"):
        assert re.search(r"FW_TYPES_HD inline \w+ %s\(" % name, types), name
    assert "pub const FWGPU_BIQUAD_SWEEP_FRAMES_MAX: u32 = 16777216;" in ffi
    assert "pub fn fwgpu_biquad_sweep(ctx: *mut fwgpu_ctx, node: i64, cutoff_hz: f32, q: f32, frames: u32, at_block: u32) -> c_int;" in ffi
    assert "pub fn sweep_to" in nodes and "ffi::fwgpu_biquad_sweep" in nodes
    res, args = flib.SIGNATURES["fwgpu_biquad_sweep"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_uint32, C.c_uint32]


def test_typed_mirror_sweep_to():
    import firewheel_amd as fa

    P = _peek_lib()
    cx = fwapi.hostonly_ctx(sample_rate=SR, max_block_frames=64)
    n = fa.BiquadNode(fa.BiquadNode.LOWPASS, 900.0, 3.0)
    cx.add_node(2, 2, n)
    n.sweep_to(200.0, 4800)                                  # q None: the Q it has
    n.sweep_to_secs(7000.0, 0.25, q=1.5, at_block=2)
    assert (n.cutoff_hz, n.q) == (7000.0, 1.5) and fa.BiquadNode.SWEEP_FRAMES_MAX == bm.FRAMES_MAX
    got = _early(P, cx.c)
    assert [(g[0], g[1], g[7]) for g in got] == [(bm.CMD_BQ_SWEEP, 0, 4800), (bm.CMD_BQ_SWEEP, 2, 12000)]
    assert list(got[0][2:7]) == bits5(refmodel.rbj_coefs(LP, 200.0, 3.0, SR)) and list(got[1][2:7]) == bits5(refmodel.rbj_coefs(LP, 7000.0, 1.5, SR))
    with pytest.raises(fa.FwgpuError):
        n.sweep_to(500.0, bm.FRAMES_MAX + 1)


# ================================================================================================ GPU tier
def _at(call, where, plus=0):
    """(call, at_block) of block `where` ('first' / 'mid' / 'last') of `call`, `plus` blocks further on"""
    g = call * K + {"first": 0, "mid": K // 2, "last": K - 1}[where] + plus
    return g // K, g % K


def _send(e, node, what, args, at):
    if what == "sweep":
        e.sweep(node, args[0], args[1], args[2], at_block=at)
    elif what == "cutoff":
        e.set_param(node, 1, args[0], at_block=at)
    elif what == "q":
        e.set_param(node, 2, args[0], at_block=at)
    else:
        raise ValueError(what)


def run_bus(e, nch, msgs, ftype=LP, tail_frames=0, n_calls=N_CALLS):
    """the bus graph through n_calls calls of K blocks (+ one call that ends in a short block); msgs: [(call, at_block, what, args)]"""
    b = _bus(e, nch, ftype)
    outs = []
    for call in range(n_calls):
        for (cl, at, what, args) in msgs:
            if cl == call:
                _send(e, b, what, args, at)
        outs.append(np.asarray(e.process_blocks(K, n_out_ch=nch)))
    if tail_frames:                                              # a sweep from the second block of a call whose third block is short
        if isinstance(e, bm.Tagged):
            outs.append(np.asarray(e.process_blocks(1, n_out_ch=nch)))
            _send(e, b, "sweep", (300.0, 2.0, 450), 0)
            outs.append(np.asarray(e.e.process_interleaved(F + tail_frames, n_out_ch=nch)))
        else:
            _send(e, b, "sweep", (300.0, 2.0, 450), 1)
            outs.append(np.asarray(e.process_interleaved(2 * F + tail_frames, n_out_ch=nch)))
    return np.concatenate(outs)


_REF = {}


def ref_bus(nch, msgs, **kw):
    """the model's output of a bus case, computed once per case and never changed"""
    key = (nch, repr(msgs), repr(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = run_bus(bm.Tagged(bm.SweepRefEngine(max_block_frames=F, num_graph_outputs=nch, short_blocks=True)), nch, msgs, **kw)
        _REF[key].setflags(write=False)
        assert np.any(_REF[key] != 0)
    return _REF[key]


def gpu_bus(nch, msgs, force_generic=False, **kw):
    g = GpuEngine(max_block_frames=F, max_batch=K, num_graph_outputs=nch, force_generic=force_generic)
    got = run_bus(bm.GpuSweep(g), nch, msgs, **kw)
    return g, got


def S(pos, cutoff, q, N):
    return pos + ("sweep", (cutoff, q, N))


LENGTHS = [1, 255, 256, 257, 300, 700, 5000]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "mid", "last"])
@pytest.mark.parametrize("N", LENGTHS)
def test_g1_sweep_lengths_and_start_blocks(N, where):
    """a stereo bus biquad, K = 3 whole 256-frame chunks: the batch walkers take the calls in front of the sweep and behind it, the node
    kernel the calls with it — the filter state hands over between the two without a seam"""
    msgs = [S(_at(1, where), 6000.0, 4.0, N)]
    g, got = gpu_bus(2, msgs)
    assert_bits(got, ref_bus(2, msgs), "N = %d from the %s block" % (N, where))


INTERPLAY = {
    "retarget in mid-sweep": [S(_at(1, "first"), 9000.0, 4.0, 700), S(_at(1, "last"), 150.0, 1.0, 300)],
    "set_cutoff_hz during a sweep": [S(_at(1, "mid"), 9000.0, 4.0, 5000), _at(2, "mid") + ("cutoff", (2500.0,))],
    "set_q during a sweep": [S(_at(1, "mid"), 9000.0, 4.0, 5000), _at(2, "first") + ("q", (0.8,)), S(_at(3, "first"), 100.0, 0.8, 257)],
    "two sweeps for one block": [S(_at(1, "mid"), 9000.0, 4.0, 700), S(_at(1, "mid"), 200.0, 2.0, 300)],
    "a sweep, then set_cutoff_hz, for one block": [S(_at(2, "first"), 9000.0, 4.0, 700), _at(2, "first") + ("cutoff", (1200.0,))],
    "set_cutoff_hz, then a sweep, for one block": [_at(2, "last") + ("cutoff", (1200.0,)), S(_at(2, "last"), 9000.0, 4.0, 300)],
    "a step (frames 0) in mid-sweep": [S(_at(1, "first"), 9000.0, 4.0, 5000), S(_at(2, "mid"), 400.0, 3.0, 0)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INTERPLAY))
def test_g2_message_interplay(name):
    g, got = gpu_bus(2, INTERPLAY[name])
    assert_bits(got, ref_bus(2, INTERPLAY[name]), name)


@pytest.mark.gpu
@pytest.mark.parametrize("ftype", [LP, HP, BP])
def test_g3_filter_types(ftype):
    msgs = [S(_at(1, "mid"), 11000.0, 4.0, 700), S(_at(3, "first"), 40.0, 9.0, 300)]
    g, got = gpu_bus(2, msgs, ftype=ftype)
    assert_bits(got, ref_bus(2, msgs, ftype=ftype), "filter type %d" % ftype)


@pytest.mark.gpu
@pytest.mark.parametrize("force_generic", [False, True])
@pytest.mark.parametrize("nch", [1, 2, 3, 6])
def test_g4_level_executor_channel_counts_and_a_short_block(nch, force_generic):
    """1 - 4 channels go through the LDS rows, 6 through the lane-per-channel loop; the last call ends in a block of 100 frames"""
    msgs = [S(_at(1, "first"), 5000.0, 4.0, 700), S(_at(2, "last"), 90.0, 1.0, 300)]
    g, got = gpu_bus(nch, msgs, force_generic=force_generic, tail_frames=100)
    if force_generic:
        assert g.cx.plan_kind() == 0
    assert_bits(got, ref_bus(nch, msgs, tail_frames=100), "%d channels" % nch)


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [2, 6])
def test_g5_node_process(nch):
    """fwgpu_node_process: ONE node, a block per call on the caller's buffers"""
    g = GpuEngine(max_block_frames=F, num_graph_outputs=nch)
    gg = bm.GpuSweep(g)
    m = bm.SweepRefEngine(max_block_frames=F, num_graph_outputs=nch)
    nodes = []
    for e in (gg, m):
        b = e.biquad(BP, 1500.0, 3.0, ch=nch)
        for c in range(nch):
            e.connect(b, c, e.graph_out_node, c)
        e.update()
        nodes.append(b)
    x = voice_source(321, 9 * F, nch)
    got, want = [], []
    for blk, frames in enumerate([F, F, 100, F, 37, F, F, 1, F]):
        if blk == 1:
            gg.sweep(nodes[0], 9000.0, 1.0, 600)
            m.sweep(nodes[1], 9000.0, 1.0, 600)
        if blk == 5:
            gg.sweep(nodes[0], 300.0, 6.0, 257)
            m.sweep(nodes[1], 300.0, 6.0, 257)
        ins = [x[c, blk * F:blk * F + frames] for c in range(nch)]
        y, _ = g.node_process(nodes[0], frames, ins, nch)
        got.append(y)
        want.append(m.node_process(nodes[1], frames, ins, nch))
    assert_bits(np.concatenate(got, axis=1), np.concatenate(want, axis=1), "node_process, %d channels" % nch)


# ------------------------------------------------------------------------------------------------ the chain plan
V_CHAIN = 40
CHAIN_SHAPES = {
    "B": (["B"], PLANAR_F32), "BB second": (["BB"], PLANAR_F32), "BB both": (["BB"], PLANAR_I16), "BD": (["BD"], PLANAR_F32), "DB": (["DB"], PLANAR_F32),
}


def run_chain(e, name):
    shapes, fmt = CHAIN_SHAPES[name]
    voices = _chain_bank(e, V_CHAIN, shapes, fmt=fmt)
    outs = []
    for call in range(N_CALLS):
        if call == 1:                                        # sweeps on a few voices only, the others steady in the same leaves
            for v, (N, where) in ((0, (700, "first")), (7, (300, "mid")), (25, (5000, "last"))):
                bqs = voices[v][1]
                cl, at = _at(1, where)
                if name == "BB second":
                    e.sweep(bqs[1], 7000.0, 3.0, N, at_block=at)
                elif name == "BB both":
                    e.sweep(bqs[0], 7000.0, 3.0, N, at_block=at)
                    e.sweep(bqs[1], 250.0, 1.0, N // 2 + 1, at_block=at)
                else:
                    e.sweep(bqs[0], 7000.0, 3.0, N, at_block=at)
        if call == 2:
            e.sweep(voices[0][1][-1], 100.0, 6.0, 257, at_block=1)       # a second sweep of the same filter, behind the first
            e.set_param(voices[25][1][0], 1, 900.0, at_block=2)          # set_cutoff_hz ends voice 25's long one
        outs.append(np.asarray(e.process_blocks(K)))
    return np.concatenate(outs)


_REF_CHAIN = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CHAIN_SHAPES))
def test_g6_chain_plan(name):
    if name not in _REF_CHAIN:
        _REF_CHAIN[name] = run_chain(bm.Tagged(bm.SweepRefEngine(max_block_frames=F)), name)
        _REF_CHAIN[name].setflags(write=False)
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got = run_chain(bm.GpuSweep(g), name)
    assert g.cx.plan_kind() == 2 and g.cx.plan_fused_voices() == V_CHAIN
    assert np.any(_REF_CHAIN[name] != 0)
    assert_bits(got, _REF_CHAIN[name], "chain plan, voices " + name)


# ------------------------------------------------------------------------------------------------ lazy calls around a sweep
def _lazy_run(e, build):
    node = build(e)
    outs, marks = [], []
    for call in range(10):
        if call == 4:
            e.sweep(node, 6000.0, 3.0, 5 * F + 3, at_block=1)             # through call 5 and 3 frames into call 6; at rest from call 7 on
        outs.append(np.asarray(e.process_blocks(K)))
        if hasattr(e, "cx"):
            marks.append(e.cx.lazy_stats())
    return np.concatenate(outs), marks


def _bank_with_master_biquad(e):
    """twelve dry voices -> SumNode -> a master biquad on the mix bus -> graph_out"""
    rng = np.random.default_rng(9)
    ends, smps = [], []
    for v in range(12):
        s = e.sampler(80.0)
        vol = e.volume(float(rng.uniform(30, 100)))
        e.connect_stereo(s, vol)
        smps.append(s)
        ends.append(vol)
    m = e.sum(12)
    for p, n in enumerate(ends):
        e.connect_stereo(n, m, 2 * p)
    b = e.biquad(LP, 900.0, 2.0)
    e.connect_stereo(m, b)
    e.connect_stereo(b, e.graph_out_node)
    e.update()
    for v, s in enumerate(smps):
        e.sampler_set_sample(s, e.new_sample(PLANAR_F32, 2, voice_source(7700 + v, 8 * F, 2)))     # a loop of 8 whole blocks: lazy-capable
        e.sampler_set_loop_range(s, LOOP_FULL)
        e.sampler_play(s)
    return b


def _chain_for_lazy(e):
    voices = _chain_bank(e, 12, ["BD"], leaf=12, src_len=8 * F)
    return voices[3][1][0]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["bus biquad", "chain voice"])
def test_g7_a_call_inside_a_sweep_runs_the_control_kernel_and_lazy_calls_resume_behind_it(which):
    build = _bank_with_master_biquad if which == "bus biquad" else _chain_for_lazy
    want, _ = _lazy_run(bm.Tagged(bm.SweepRefEngine(max_block_frames=F)), build)
    g = GpuEngine(max_block_frames=F, max_batch=K)
    got, marks = _lazy_run(bm.GpuSweep(g), build)
    assert g.cx.plan_kind() == (1 if which == "bus biquad" else 2)
    assert_bits(got, want, "ten calls, " + which)
    if os.environ.get("FWGPU_LAZY") == "0":
        return
    lazy, ctl = [m[0] for m in marks], [m[1] for m in marks]
    assert lazy[3] > lazy[1], marks                               # quiet calls in front of the sweep are lazy
    assert lazy[6] == lazy[3] and ctl[6] - ctl[3] == 3, marks     # calls 4, 5, 6: a sweep in flight (or ending): the control kernel, no lazy batch
    assert lazy[9] - lazy[6] == 3, marks                          # ... and lazy again from the first call wholly behind it, bit-exact (above)
