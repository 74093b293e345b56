"""FIR reverb morphs (SPEC; include/fwgpu.h "FIR reverb morph"): a FirReverbNode with two impulse-response slots over one
history, blended along the crossfader's curve by one message (fwgpu_fir_morph), the silent slot's impulse response exchanged by a
graph edit (fwgpu_fir_set_ir).  Everything is bit-exact against tests/fir_morph_model.py: the two slot sums are plain FIR nodes on the
impulse responses padded to T (refmodel.FirNode, or the oracle for the larger T), the blend is numpy.

CPU tier: the model's own properties, the g++ build of fwgpu_types.h fir_morph_* against it, and the host half on the harness
(tests/host_harness, companion fir_morph_peek.cpp).  GPU tier: tests g1 .. g6."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fir_morph_model as M
import fwapi
import scenarios
from busnodes import assert_bits, harness_run
from fwapi import FIR, PLANAR_F32, PLANAR_I16, GpuEngine, HostOnlyEngine

INVALID = -20
F32 = np.float32
U, ULL, LL = C.c_uint, C.c_ulonglong, C.c_longlong
LINEAR_LAW, EQUAL_POWER = M.LINEAR_LAW, M.EQUAL_POWER
EASE = (0.42, 0.0, 0.58, 1.0)
OVERSHOOT = (0.3, -0.5, 0.7, 1.5)
FRAMES_MAX = 1 << 24
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PLAN_KIND = {"hybrid": 3, "generic": 0}


def fbits(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def peek():
    p, UP, LP = C.c_void_p, C.POINTER(U), C.POINTER(LL)
    return fwapi.peek_lib("fir_morph_peek", {
        "fmp_state_bytes": (U, []), "fmp_init": (None, [p, U, C.c_int, U, U]), "fmp_state_ok": (C.c_int, [p, C.c_int, C.c_int]),
        "fmp_msg": (None, [p, U, U, C.c_int, UP]), "fmp_block": (C.c_int, [p, U, UP]), "fmp_out": (None, [UP, U, UP, UP, UP]),
        "fmp_times": (None, [p, C.POINTER(ULL)]), "fmp_node": (C.c_int, [p, LL, LP, C.POINTER(ULL)]), "fmp_ctx": (None, [p, C.POINTER(ULL)]),
        "fmp_cached": (C.c_int, [p, U, LP]), "fmp_group": (C.c_int, [p, U, LP]), "fmp_group_partners_ok": (C.c_int, [p, U]),
        "fmp_pins": (None, [UP])})


def _ctl(curve):
    x1, y1, x2, y2 = (0.0, 0.0, 1.0, 1.0) if curve is None else curve
    return (U * 4)(fbits(x1), fbits(y1), fbits(x2), fbits(y2))


def noise(seed, n, ch):
    """noise with -0.0 and subnormals sprinkled in (the ends copy bit for bit)"""
    x = fwapi.xorshift_uniform(seed, n * ch).reshape(n, ch).astype(F32)
    u = fwapi.bits(x).copy()
    words = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x00400000], dtype=np.uint32)
    idx = np.arange(7, n, 61)
    u[idx, 0] = words[np.arange(len(idx)) % 4]
    return u.view(F32)


# ================================================================================================ CPU tier: the model's own properties
@pytest.mark.parametrize("law", [LINEAR_LAW, EQUAL_POWER])
def test_model_the_ends_are_copies(law):
    sa, sb = noise(1, 300, 2), noise(2, 300, 2)
    ya, ma = M.render(M.Morph(0.0, law), sa, sb, [100, 200])
    yb, mb = M.render(M.Morph(1.0, law), sa, sb, [100, 200])
    assert_bits(ya, sa, "at rest at 0")
    assert_bits(yb, sb, "at rest at 1")
    assert ma == [M.MODE_A] * 2 and mb == [M.MODE_B] * 2
    # a fade that ends inside a block: the frames behind its end copy slot B, and the block still runs both slots
    y, modes = M.render(M.Morph(0.0, law), sa, sb, [100, 200], {0: [(1.0, 150, EASE)]})
    assert_bits(y[150:], sb[150:], "behind the segment's end")
    assert_bits(y[:1], sa[:1], "the first frame of a segment from 0 stands at 0")
    assert modes == [M.MODE_BOTH, M.MODE_BOTH]
    assert np.any(fwapi.bits(y[1:150]) != fwapi.bits(sa[1:150])) and np.any(fwapi.bits(y[1:150]) != fwapi.bits(sb[1:150]))
    # an empty slot B is a wet fader: its sum is +0.0
    y, _ = M.render(M.Morph(0.0, law), sa, None, [300], {0: [(1.0, 0, None)]})
    assert not fwapi.bits(y).any()


@pytest.mark.parametrize("curve", [None, EASE, OVERSHOOT])
def test_model_is_independent_of_how_the_blocks_are_split(curve):
    sa, sb = noise(3, 512, 2), noise(4, 512, 2)
    one, _ = M.render(M.Morph(0.25, EQUAL_POWER), sa, sb, [512], {0: [(0.9, 400, curve)]})
    many, _ = M.render(M.Morph(0.25, EQUAL_POWER), sa, sb, [64, 37, 155, 256], {0: [(0.9, 400, curve)]})
    assert_bits(many, one, "split blocks")
    # a message lands at a block's first frame wherever the blocks were cut before it
    a, _ = M.render(M.Morph(0.0, LINEAR_LAW), sa, sb, [128, 384], {0: [(1.0, 300, curve)], 1: [(0.2, 100, curve)]})
    b, _ = M.render(M.Morph(0.0, LINEAR_LAW), sa, sb, [64, 64, 100, 284], {0: [(1.0, 300, curve)], 2: [(0.2, 100, curve)]})
    assert_bits(b, a, "a retarget at frame 128")


def test_model_slot_sums_refmodel_and_oracle_agree_on_a_padded_impulse_response():
    """the two sources of slot sums the tests use are the same function: FirNode on a padded h == the oracle's plain FIR node on it"""
    h = scenarios.reverb_ir(5, 70, 2)
    x = noise(6, 64 * 6 + 21, 2)
    calls = [128, 64 + 21, 192]
    ref = M.slot_sum_ref(h, 300, x, M.blocks_of(calls, 64))
    orc = M.slot_sum_oracle(h, 300, x, calls, 64)
    assert_bits(orc, ref, "padded to 300")
    assert_bits(M.slot_sum_oracle(h, 70, x, calls, 64), ref, "padding changes no bit of a sum that has one segment")


# ================================================================================================ CPU tier: fwgpu_types.h fir_morph_* in g++
SCRIPTS = [
    # (position, law, blocks, {block: [(position, frames, curve)]})
    (0.0, EQUAL_POWER, [64] * 12, {1: [(1.0, 150, None)], 5: [(0.0, 200, EASE)], 7: [(0.3, 81, None)], 10: [(1.0, 0, None)]}),
    (1.0, LINEAR_LAW, [256, 256, 37, 256, 256, 256], {0: [(0.0, 300, OVERSHOOT)], 2: [(0.5, 10, None), (1.0, 400, EASE)], 5: [(0.0, 0, None)]}),
    (0.3, EQUAL_POWER, [100] * 6, {2: [(0.3, 50, EASE)], 3: [(1.0, 1, None)], 4: [(0.0, 100, None)]}),
]


@pytest.mark.parametrize("position,law,blocks,msgs", SCRIPTS)
def test_gpp_build_of_the_helpers_matches_the_model(position, law, blocks, msgs):
    P = peek()
    st = (C.c_ubyte * P.fmp_state_bytes())()
    P.fmp_init(st, fbits(position), law, 300, 299 + 4 * 256)
    assert P.fmp_state_ok(st, 1, 1) == 1
    n = sum(blocks)
    sa, sb = noise(11, n, 1), noise(12, n, 1)
    want, modes = M.render(M.Morph(position, law), sa, sb, blocks, msgs)
    got, pos, t = np.zeros(n, dtype=np.uint32), 0, 0
    for i, f in enumerate(blocks):
        for (p1, frames, curve) in msgs.get(i, ()):
            P.fmp_msg(st, fbits(p1), frames, 0 if curve is None else 1, _ctl(curve))
        rec = (U * 16)()
        assert P.fmp_block(st, f, rec) == modes[i], (i, modes[i])
        a = np.ascontiguousarray(fwapi.bits(sa[pos:pos + f, 0]))
        b = np.ascontiguousarray(fwapi.bits(sb[pos:pos + f, 0]))
        out = (U * f)()
        P.fmp_out(rec, f, a.ctypes.data_as(C.POINTER(U)), b.ctypes.data_as(C.POINTER(U)), out)
        got[pos:pos + f] = np.frombuffer(out, dtype=np.uint32)
        pos += f
        t += f
        times = (ULL * 2)()
        P.fmp_times(st, times)
        assert times[0] == t and times[1] <= t
        assert P.fmp_state_ok(st, 1, 1) == 1
    assert_bits(got.view(F32), want[:, 0], "fir_morph_block / fir_morph_out")


def test_gpp_state_predicate_and_layout_pins():
    P = peek()
    pins = (U * 7)()
    P.fmp_pins(pins)
    assert list(pins) == [23, FIR, 128, 16, 64, 168, 4096]
    st = (C.c_ubyte * P.fmp_state_bytes())()
    P.fmp_init(st, fbits(0.5), EQUAL_POWER, 300, 555)
    assert P.fmp_state_ok(st, 1, 1) == 1
    assert P.fmp_state_ok(st, 2, 2) == 0          # (two rings do not fit the slice of one)
    for bad in (fbits(1.5), fbits(-0.1), fbits(float("nan"))):
        P.fmp_init(st, bad, EQUAL_POWER, 300, 555)
        assert P.fmp_state_ok(st, 1, 1) == 0
    P.fmp_init(st, fbits(0.5), 2, 300, 555)
    assert P.fmp_state_ok(st, 1, 1) == 0
    P.fmp_init(st, fbits(0.5), 0, 300, 200)       # a ring shorter than the taps
    assert P.fmp_state_ok(st, 1, 1) == 0


# ================================================================================================ CPU tier: the host half on the harness
def _fir_host(mbf=64, ch=2, **kw):
    e = HostOnlyEngine(max_block_frames=mbf, num_graph_inputs=ch, num_graph_outputs=ch, **kw)
    return e


def _ir(e, taps, channels=2, seed=7):
    return e.new_sample(PLANAR_F32, channels, scenarios.reverb_ir(seed, taps, channels))


def _wire(e, f, ch=2):
    for c in range(ch):
        e.connect(e.graph_in_node, c, f, c)
        e.connect(f, c, e.graph_out_node, c)


def _morph(e, node, position, frames, curve=None, at_block=0):
    shape, (x1, y1, x2, y2) = (0, (0.0, 0.0, 1.0, 1.0)) if curve is None else (1, curve)
    return e.cx.L.fwgpu_fir_morph(e.cx.c, node, position, frames, shape, x1, y1, x2, y2, at_block)


def _set_ir(e, node, slot, sample):
    return e.cx.L.fwgpu_fir_set_ir(e.cx.c, node, slot, sample)


def _node(P, e, node):
    out, end = (LL * 15)(), ULL(0)
    assert P.fmp_node(e.cx.c, node, out, C.byref(end)) == 1
    keys = ("morph", "ir_a", "ir_b", "max_taps", "target", "hold", "activated", "T", "R", "ext_off", "ext_len", "enabled", "tab", "tab_n", "held")
    d = dict(zip(keys, list(out)))
    d["target_end"] = end.value
    return d


def _ctx(P, e):
    out = (ULL * 6)()
    P.fmp_ctx(e.cx.c, out)
    return dict(zip(("frames_done", "frames_ctl", "cached", "ext_used", "limbo", "free"), list(out)))


def _groups(P, e):
    out, i, got = (LL * 7)(), 0, []
    while P.fmp_group(e.cx.c, i, out) == 1:
        got.append(dict(zip(("level", "T", "morph", "rows", "a", "b", "pad"), list(out))))
        assert P.fmp_group_partners_ok(e.cx.c, i) == 1
        i += 1
    return got


def _cached(P, e):
    out, i, got = (LL * 4)(), 0, []
    while P.fmp_cached(e.cx.c, i, out) == 1:
        got.append(tuple(out)[:3])
        i += 1
    return sorted(got)


def _layout_ok(P, e, mbf=64, ch=2):
    assert P.fwp_layout_check(e.cx.c, 48000, mbf, ch, ch, 0) == 0


def test_one_parameter_is_the_plain_node_and_sets_no_morph_flag():
    P = peek()
    e = _fir_host()
    _layout_ok(P, e)
    a, b = _ir(e, 300), _ir(e, 300, seed=8)
    nodes = [e.fir(a), e.fir(b), e.fir(a)]
    for f in nodes:
        for c in range(2):
            e.connect(e.graph_in_node, c, f, c)
    m = e.sum(3)
    for i, f in enumerate(nodes):
        e.connect_stereo(f, m, 2 * i)
    e.connect_stereo(m, e.graph_out_node)
    e.update()
    g = _groups(P, e)
    assert len(g) == 1 and g[0]["morph"] == 0 and (g[0]["T"], g[0]["a"], g[0]["b"], g[0]["rows"]) == (300, 6, 0, 128), g
    for f in nodes:
        d = _node(P, e, f)
        assert (d["morph"], d["enabled"], d["T"], d["ext_len"]) == (0, 0, 300, 2 * 2 * d["R"])
        assert _morph(e, f, 1.0, 10) == INVALID and "morph-capable" in e.cx.L.fwgpu_last_error(e.cx.c).decode()
        assert _set_ir(e, f, 1, b) == INVALID and "morph-capable" in e.cx.L.fwgpu_last_error(e.cx.c).decode()
    assert _cached(P, e) == [(a, 0, 300), (a, 1, 300), (b, 0, 300), (b, 1, 300)]
    launches, _ = harness_run(e)
    assert launches["fir"] > 0


@pytest.mark.parametrize("params,T", [((-1,), 300), ((-1, 0, 1.0), 300), ((-1, 512, 0.25, 0), 512), (("b",), 700), (("b", 0, 0.0, 1), 700),
                                      (("b", 1 << 12), 4096), (("a", 300), 300)])
def test_creation_parameters_accepted(params, T):
    P = peek()
    e = _fir_host()
    a, b = _ir(e, 300), _ir(e, 700, seed=8)
    params = [a] + [{"a": a, "b": b}.get(x, x) for x in params]
    f = e.add_node(FIR, 2, 2, [float(x) for x in params])
    _wire(e, f)
    d = _node(P, e, f)
    assert d["morph"] == 1 and d["activated"] == 0 and d["ir_a"] == a and d["ir_b"] == params[1]
    e.update()
    d = _node(P, e, f)
    R = T - 1 + d["tab_n"] * 64
    assert (d["T"], d["R"], d["enabled"], d["activated"]) == (T, R, 1, 1)
    assert d["tab"] % 16 == 0 and d["tab"] >= d["ext_off"] + 4 * R and d["tab"] + 16 * d["tab_n"] == d["ext_off"] + d["ext_len"]
    g = _groups(P, e)
    assert len(g) == 1 and (g[0]["morph"], g[0]["T"], g[0]["a"]) == (1, T, 2) and g[0]["b"] == (0 if params[1] == -1 else 2)
    # a tile per impulse-response CHANNEL; the rows of two slots that hold the same sample share their tiles
    assert g[0]["rows"] == (64 if params[1] in (-1, a) else 128)
    launches, _ = harness_run(e)      # the launch_fir stub's checks hold for a morph group as written
    assert launches["fir"] > 0


NAN = float("nan")


@pytest.mark.parametrize("params", [(-2,), (0.5,), (NAN,), (99,), ("b", 699), ("b", -1), ("b", (1 << 24) + 2), ("b", 0.5), (-1, 299),
                                    (-1, 0, -0.1), (-1, 0, 1.1), (-1, 0, NAN), (-1, 0, 0.5, 2), (-1, 0, 0.5, 0.5), (-1, 0, 0.5, NAN)])
def test_creation_parameters_refused_at_update(params):
    e = _fir_host()
    a, b = _ir(e, 300), _ir(e, 700, seed=8)
    f = e.add_node(FIR, 2, 2, [float(a)] + [float({"b": b}.get(x, x)) for x in params])
    _wire(e, f)
    for _ in range(2):      # (still there, still refused)
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.update()
        assert ei.value.code == INVALID and "FirReverbNode" in str(ei.value)
    e.remove_node(f)
    good = e.add_node(FIR, 2, 2, [float(a), float(b)])
    _wire(e, good)
    e.update()      # the graph is usable


def test_a_bad_slot_a_is_refused_at_add_node_as_today():
    e = _fir_host()
    b = _ir(e, 300)
    for bad in (-1.0, 57.0):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.add_node(FIR, 2, 2, [bad, float(b)])
        assert ei.value.code == INVALID and "FIR node" in str(ei.value)
    st = e.cx.new_stream(PLANAR_F32, 2, 4096)
    with pytest.raises(e.fa.FwgpuError):
        e.add_node(FIR, 2, 2, [float(st.id), float(b)])
    f = e.add_node(FIR, 2, 2, [float(b), float(st.id)])      # a stream in slot B: a parameter, refused by the update
    _wire(e, f)
    with pytest.raises(e.fa.FwgpuError):
        e.update()


REFUSED = [
    ("position", dict(position=-0.001)), ("position", dict(position=1.001)), ("position", dict(position=NAN)),
    ("frames", dict(frames=FRAMES_MAX + 1)), ("shape", dict(shape=2)), ("shape", dict(shape=-1)),
    ("x1", dict(x1=-0.1)), ("x1", dict(x1=1.1)), ("x1", dict(x1=NAN)), ("x2", dict(x2=-0.1)), ("x2", dict(x2=1.1)), ("x2", dict(x2=NAN)),
    ("y1", dict(y1=-1.1)), ("y1", dict(y1=2.1)), ("y1", dict(y1=NAN)), ("y2", dict(y2=-1.1)), ("y2", dict(y2=2.1)), ("y2", dict(y2=NAN)),
]


@pytest.mark.parametrize("what,bad", REFUSED)
def test_fir_morph_has_the_refusals_of_crossfade_to(what, bad):
    e = _fir_host()
    f = e.add_node(FIR, 2, 2, [float(_ir(e, 300)), -1.0])
    _wire(e, f)
    e.update()
    a = dict(position=0.5, frames=100, shape=1, x1=0.42, y1=0.0, x2=0.58, y2=1.0)
    call = lambda d: e.cx.L.fwgpu_fir_morph(e.cx.c, f, d["position"], d["frames"], d["shape"], d["x1"], d["y1"], d["x2"], d["y2"], 0)
    assert call(a) == 0
    assert call(dict(a, **bad)) == INVALID, what
    assert "fwgpu_fir_morph" in e.cx.L.fwgpu_last_error(e.cx.c).decode()


def test_fir_morph_accepts_the_borders_and_refuses_other_nodes():
    P = peek()
    e = _fir_host()
    f = e.add_node(FIR, 2, 2, [float(_ir(e, 300)), -1.0])
    v = e.volume(50.0)
    _wire(e, f)
    L, c = e.cx.L, e.cx.c
    assert L.fwgpu_fir_morph(c, f, 1.0, FRAMES_MAX, 1, 0.0, -1.0, 1.0, 2.0, 7) == 0      # before the first update, too: held like every early message
    assert P.fwp_early_count(c) == 1
    e.update()
    assert P.fwp_early_count(c) == 0
    assert L.fwgpu_fir_morph(c, f, 0.0, 0, 0, 0.0, 0.0, 1.0, 1.0, 0) == 0
    for other in (v, e.graph_out_node, 12345 << 32):
        assert L.fwgpu_fir_morph(c, other, 0.5, 10, 0, 0.0, 0.0, 1.0, 1.0, 0) == INVALID
        assert L.fwgpu_fir_set_ir(c, other, 1, 0) == INVALID
    assert L.fwgpu_fir_morph(None, f, 0.5, 10, 0, 0.0, 0.0, 1.0, 1.0, 0) == INVALID
    assert L.fwgpu_fir_set_ir(None, f, 1, 0) == INVALID
    assert L.fwgpu_fir_morph_stats(None, None, None) == INVALID
    assert e.cx.fir_morph_stats() == (0, 0)      # (the harness runs no kernel)
    with pytest.raises(e.fa.FwgpuError):         # fwgpu_node_process goes on refusing the kind
        e.node_process(f, 64, [np.zeros(64, F32)] * 2, 2)


def test_set_ir_refusals_and_the_inaudible_rule():
    P = peek()
    e = _fir_host(max_batch=4)
    a, b, third, long_one = _ir(e, 300), _ir(e, 200, seed=8), _ir(e, 250, 1, seed=9), _ir(e, 301, seed=10)
    st = e.cx.new_stream(PLANAR_F32, 2, 4096)
    f = e.add_node(FIR, 2, 2, [float(a), float(b)])      # T = 300, at rest at A
    _wire(e, f)
    e.update()
    err = lambda: e.cx.L.fwgpu_last_error(e.cx.c).decode()
    assert _set_ir(e, f, 2, third) == INVALID and "slot" in err()
    assert _set_ir(e, f, -1, third) == INVALID
    assert _set_ir(e, f, 1, long_one) == INVALID and "capacity" in err()
    assert _set_ir(e, f, 1, st.id) == INVALID and "stream" in err()
    assert _set_ir(e, f, 1, 77) == INVALID and _set_ir(e, f, 1, -2) == INVALID
    assert _set_ir(e, f, 0, -1) == INVALID
    assert _set_ir(e, f, 0, third) == INVALID and "audible" in err()      # at rest at A: slot A is what one hears
    assert _node(P, e, f)["hold"] == 0
    # slot B is silent: exchanged, emptied and filled again — each a graph edit the next update builds
    assert _set_ir(e, f, 1, third) == 0
    d = _node(P, e, f)
    assert (d["ir_b"], d["hold"]) == (third, 1)
    e.update()
    assert _node(P, e, f)["hold"] == 0 and _groups(P, e)[0]["b"] == 2
    assert (third, 0, 300) in _cached(P, e) and (b, 0, 300) not in _cached(P, e)
    assert _set_ir(e, f, 1, -1) == 0
    e.update()
    assert _groups(P, e)[0]["b"] == 0 and _groups(P, e)[0]["rows"] == 64
    assert _set_ir(e, f, 1, b) == 0
    e.update()
    # a morph to B: slot A stays audible until the fade's last frame has been rendered by a call that has returned
    assert _morph(e, f, 1.0, 100, EASE, at_block=1) == 0
    d = _node(P, e, f)
    assert d["target"] == fbits(1.0) and d["target_end"] == 0 + 64 + 100
    assert _set_ir(e, f, 0, third) == INVALID and "audible" in err()
    assert _set_ir(e, f, 1, third) == INVALID      # ... and slot B is what the morph is heading for
    e.process_blocks(2, n_out_ch=2)                # 128 frames: the fade ends at 164
    assert _set_ir(e, f, 0, third) == INVALID
    e.process_blocks(1, n_out_ch=2)                # 192
    assert _ctx(P, e)["frames_ctl"] == 192
    assert _set_ir(e, f, 0, third) == 0
    assert _node(P, e, f)["ir_a"] == third
    # a morph to somewhere in between leaves both slots audible for good
    e.update()
    assert _morph(e, f, 0.5, 0) == 0
    e.process_blocks(1, n_out_ch=2)
    assert _set_ir(e, f, 0, a) == INVALID and _set_ir(e, f, 1, a) == INVALID
    assert e.violation() == ""


def test_a_morph_behind_a_set_ir_is_held_and_released_by_the_update():
    P = peek()
    e = _fir_host(max_batch=4)
    _layout_ok(P, e)
    a, b, third = _ir(e, 300), _ir(e, 300, seed=8), _ir(e, 120, seed=9)
    f = e.add_node(FIR, 2, 2, [float(a), float(b), 0.0, 1.0])      # at rest at B
    _wire(e, f)
    e.update()
    assert _morph(e, f, 1.0, 0) == 0 and P.fwp_early_count(e.cx.c) == 0      # no edit pending: straight to the ring
    e.process_blocks(1, n_out_ch=2)
    assert _set_ir(e, f, 0, third) == 0
    assert _morph(e, f, 0.0, 480, EASE, at_block=2) == 0
    assert _morph(e, f, 0.5, 10) == 0
    msgs = fwapi.early_msgs(P, e.cx.c)
    assert [(m[0], m[1], m[2], m[3], m[4]) for m in msgs] == [(23, 2, fbits(0.0), 480, 1), (23, 0, fbits(0.5), 10, 0)]
    e.process_blocks(2, n_out_ch=2)      # the calls between the edit and the update run the old plan and see no message
    assert P.fwp_early_count(e.cx.c) == 2 and _node(P, e, f)["hold"] == 1
    e.update()
    assert P.fwp_early_count(e.cx.c) == 0 and _node(P, e, f)["hold"] == 0
    assert _morph(e, f, 0.0, 10) == 0 and P.fwp_early_count(e.cx.c) == 0
    launches, _ = harness_run(e)
    assert launches["fir"] > 0


def test_a_held_morph_counts_from_its_release_not_from_when_it_was_sent():
    """a morph that waits in early_msgs starts behind the update that releases it, however many frames the old plan renders before:
    until then both slots count as audible, and its end is reckoned from the release"""
    P = peek()
    e = _fir_host(max_batch=4)
    a, b, third, fourth = _ir(e, 300), _ir(e, 300, seed=8), _ir(e, 120, seed=9), _ir(e, 90, seed=10)
    f = e.add_node(FIR, 2, 2, [float(a), float(b), 0.0, 1.0])      # at rest at B
    _wire(e, f)
    e.update()
    assert _set_ir(e, f, 0, third) == 0
    assert _morph(e, f, 0.0, 100) == 0                             # held behind the edit
    assert _node(P, e, f)["held"] == 1
    e.process_blocks(4, n_out_ch=2)                                # 256 frames on the old plan: the node still rests at p = 1
    assert _ctx(P, e)["frames_ctl"] == 256
    err = lambda: e.cx.L.fwgpu_last_error(e.cx.c).decode()
    assert _set_ir(e, f, 1, fourth) == INVALID and "audible" in err()      # slot B is all one hears
    assert _set_ir(e, f, 0, a) == INVALID                                  # ... and slot A is where the held morph is heading
    e.update()
    d = _node(P, e, f)
    assert (d["held"], d["target"], d["target_end"]) == (0, fbits(0.0), 256 + 100)
    assert _set_ir(e, f, 1, fourth) == INVALID and "audible" in err()      # released, not rendered yet
    e.process_blocks(1, n_out_ch=2)                                # 320
    assert _set_ir(e, f, 1, fourth) == INVALID
    e.process_blocks(1, n_out_ch=2)                                # 384 >= 356
    assert _set_ir(e, f, 1, fourth) == 0
    assert e.violation() == ""
    # the same for a morph sent before the node's first plan
    g = e.add_node(FIR, 2, 2, [float(a), float(b)])
    for c in range(2):
        e.connect(e.graph_in_node, c, g, c)
    assert _morph(e, g, 1.0, 100, EASE, at_block=1) == 0
    assert _node(P, e, g)["held"] == 1
    assert _set_ir(e, g, 0, third) == INVALID and _set_ir(e, g, 1, third) == INVALID
    e.process_blocks(8, n_out_ch=2)                                # 512 more frames on the plan without the node: 896
    e.update()
    d = _node(P, e, g)
    assert (d["held"], d["target"], d["target_end"]) == (0, fbits(1.0), 896 + 64 + 100)
    assert _set_ir(e, g, 0, third) == INVALID and "audible" in err()       # the fade from A has not rendered a frame
    e.process_blocks(2, n_out_ch=2)                                # 1024
    assert _set_ir(e, g, 0, third) == INVALID
    e.process_blocks(1, n_out_ch=2)                                # 1088 >= 1060
    assert _set_ir(e, g, 0, third) == 0
    # a failed update releases nothing: the morph stays held, the slots audible
    assert _morph(e, g, 0.0, 10) == 0 and _node(P, e, g)["held"] == 1
    bad = e.add_node(FIR, 2, 2, [float(a), float(b), 0.0, 1.5])
    with pytest.raises(e.fa.FwgpuError):
        e.update()
    assert _node(P, e, g)["held"] == 1 and _set_ir(e, g, 1, fourth) == INVALID
    e.remove_node(bad)
    e.update()
    assert _node(P, e, g)["held"] == 0


def test_the_morph_that_applies_last_sets_the_target_whatever_the_send_order():
    P = peek()
    e = _fir_host(max_batch=4)
    a, b, third = _ir(e, 300), _ir(e, 300, seed=8), _ir(e, 120, seed=9)
    f = e.add_node(FIR, 2, 2, [float(a), float(b)])
    _wire(e, f)
    e.update()
    assert _morph(e, f, 1.0, 10, at_block=3) == 0       # applies at block 3 ...
    assert _morph(e, f, 0.0, 10, at_block=1) == 0       # ... behind this one, which was sent later
    d = _node(P, e, f)
    assert (d["target"], d["target_end"]) == (fbits(1.0), 3 * 64 + 10)
    e.process_blocks(4, n_out_ch=2)
    assert _set_ir(e, f, 1, third) == INVALID and _set_ir(e, f, 0, third) == 0
    assert e.violation() == ""


def test_a_sample_in_either_slot_cannot_be_destroyed():
    e = _fir_host()
    a, b, third = _ir(e, 300), _ir(e, 300, seed=8), _ir(e, 300, seed=9)
    f = e.add_node(FIR, 2, 2, [float(a), float(b), 0.0, 1.0])
    _wire(e, f)
    L, c = e.cx.L, e.cx.c
    for when in ("before", "after"):
        for s in (a, b):
            assert L.fwgpu_sample_destroy(c, s) == INVALID and "in use" in L.fwgpu_last_error(c).decode()
            assert L.fwgpu_sample_retired(c, s) == 0
        e.update()
    assert _set_ir(e, f, 0, third) == 0      # at rest at B: slot A is silent
    assert L.fwgpu_sample_destroy(c, third) == INVALID
    assert L.fwgpu_sample_destroy(c, a) == 0      # its last user let go of it
    e.update()
    e.remove_node(f)
    e.update()
    assert L.fwgpu_sample_destroy(c, b) == 0 and L.fwgpu_sample_destroy(c, third) == 0


def test_removal_returns_the_ext_slice_and_both_converted_copies():
    P = peek()
    e = _fir_host()
    a, b = _ir(e, 300), _ir(e, 200, 1, seed=8)      # B is mono: one copy serves both channels
    keep = e.fir(a)                                 # a plain node on A, padded to its own 300: the same copies
    f = e.add_node(FIR, 2, 2, [float(a), float(b)])
    g = e.add_node(FIR, 2, 2, [float(a), float(b), 512.0])
    for n in (keep, f, g):
        for c in range(2):
            e.connect(e.graph_in_node, c, n, c)
    m = e.sum(3)
    for i, n in enumerate((keep, f, g)):
        e.connect_stereo(n, m, 2 * i)
    e.connect_stereo(m, e.graph_out_node)
    e.update()
    assert _cached(P, e) == [(a, 0, 300), (a, 0, 512), (a, 1, 300), (a, 1, 512), (b, 0, 300), (b, 0, 512)]
    used = _ctx(P, e)["ext_used"]
    free0 = _ctx(P, e)["free"]
    e.remove_node(g)
    e.update()
    e.update()
    e.process_blocks(1, n_out_ch=2)
    e.update()
    assert _cached(P, e) == [(a, 0, 300), (a, 1, 300), (b, 0, 300)]      # the 512 copies went with their one user; B's 300 stays for f
    assert _ctx(P, e)["free"] == free0 + 1 + 3 and _ctx(P, e)["limbo"] == 0
    e.remove_node(f)
    e.update()
    e.update()
    assert _cached(P, e) == [(a, 0, 300), (a, 1, 300)]                   # A's copies stay for the plain node
    assert _ctx(P, e)["free"] == free0 + 2 + 4
    # a node of the same shape takes the ring's slice back; its three copies are new ones at the pool's end (as a plain node's are:
    # the slices of copies that went wait on the free lists for a ring of their size)
    g2 = e.add_node(FIR, 2, 2, [float(a), float(b), 512.0])
    for c in range(2):
        e.connect(e.graph_in_node, c, g2, c)
    e.connect_stereo(g2, m, 2)
    e.update()
    assert _ctx(P, e)["ext_used"] == used + 3 * 512
    assert _cached(P, e) == [(a, 0, 300), (a, 0, 512), (a, 1, 300), (a, 1, 512), (b, 0, 512)]
    launches, _ = harness_run(e)
    assert launches["fir"] > 0


def test_a_node_that_waits_for_its_activation_keeps_its_samples_copies():
    """the last-user scan counts every alive FIR node on the sample, activated or not, as it did for plain nodes before"""
    P = peek()
    e = _fir_host()
    a = _ir(e, 300)
    first = e.fir(a)
    _wire(e, first)
    e.update()
    waiting = e.fir(a)
    e.remove_node(first)
    assert _cached(P, e) == [(a, 0, 300), (a, 1, 300)]      # (the removed node's ring went to limbo, the copies did not)
    _wire(e, waiting)
    e.update()
    assert _cached(P, e) == [(a, 0, 300), (a, 1, 300)]


@pytest.mark.parametrize("max_batch,force_generic", [(1, False), (4, False), (4, True)])
def test_process_calls_of_a_morph_bank_pass_the_launch_stub(max_batch, force_generic):
    """40 morph nodes on two impulse-response pairs beside 3 plain nodes of the same T: two groups on one level, whole tiles per
    impulse response, partners linked both ways; short blocks and imported schedules plan the same way"""
    P = peek()
    e = HostOnlyEngine(max_block_frames=64, num_graph_inputs=2, num_graph_outputs=2, max_batch=max_batch, force_generic=force_generic)
    irs = [_ir(e, 300, seed=20 + i) for i in range(4)]
    nodes = [e.add_node(FIR, 2, 2, [float(irs[i % 2]), float(irs[2 + i % 2]), 0.0, (0.0, 1.0, 0.3)[i % 3]]) for i in range(40)]
    nodes += [e.fir(irs[0]) for _ in range(3)]
    outs = []
    for i in range(0, len(nodes), 8):
        grp = nodes[i:i + 8]
        m = e.sum(len(grp))
        for p, n in enumerate(grp):
            for c in range(2):
                e.connect(e.graph_in_node, c, n, c)
            e.connect_stereo(n, m, 2 * p)
        outs.append(m)
    top = e.sum(len(outs))
    for p, m in enumerate(outs):
        e.connect_stereo(m, top, 2 * p)
    e.connect_stereo(top, e.graph_out_node)
    e.update()
    g = sorted(_groups(P, e), key=lambda d: d["morph"])
    assert [d["morph"] for d in g] == [0, 1] and g[0]["level"] == g[1]["level"] and g[0]["T"] == g[1]["T"] == 300
    assert (g[0]["a"], g[0]["b"], g[0]["rows"]) == (6, 0, 64)
    assert (g[1]["a"], g[1]["b"], g[1]["rows"]) == (80, 80, 8 * 32)      # 20 rows per impulse-response channel and slot: eight padded tiles
    for i, n in enumerate(nodes[:40:7]):
        assert _morph(e, n, (i % 2) * 1.0, 100 + i, EASE if i % 2 else None, at_block=i % 3) == 0
    launches, _ = harness_run(e)
    assert launches["fir"] > 0
    e.process_interleaved(64 * 2 + 19, 2, inp=np.zeros((64 * 2 + 19) * 2, F32), n_in_ch=2)      # a call that ends in a short block
    assert e.violation() == ""


# ================================================================================================ CPU tier: mirrors, header, ffi
def test_typed_mirror_header_and_generated_ffi():
    import firewheel_amd as fa
    from firewheel_amd import _lib as flib

    P = peek()
    plain = fa.FirReverbNode(3)
    assert (plain.KIND, plain.params(), plain.morph) == (FIR, [3.0], False)      # the one-argument constructor sends one parameter, as before
    node = fa.FirReverbNode(3, ir_b=4, max_taps=512, position=0.25, law=0)
    assert node.morph and node.params() == [3.0, 4.0, 512.0, 0.25, 0.0]
    assert fa.FirReverbNode(3, max_taps=64).params() == [3.0, -1.0, 64.0, 0.0, 1.0]
    wet = fa.FirReverbNode(3, morph=True)      # the wet fader: an empty slot B with every other argument at its default
    assert wet.morph and wet.params() == [3.0, -1.0, 0.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        fa.FirReverbNode(3, ir_b=4, morph=False)
    for name in ("fwgpu_fir_morph", "fwgpu_fir_set_ir", "fwgpu_fir_morph_stats"):
        assert name in flib.SIGNATURES
    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=2, num_graph_outputs=2)
    a = cx.new_sample(PLANAR_F32, 2, scenarios.reverb_ir(1, 300, 2))
    b = cx.new_sample(PLANAR_F32, 2, scenarios.reverb_ir(2, 200, 2))
    third = cx.new_sample(PLANAR_F32, 1, scenarios.reverb_ir(3, 100, 1))
    node = fa.FirReverbNode(a, ir_b=b)
    m = cx.add_node(2, 2, node)
    for c in range(2):
        cx.connect(cx.graph_in_node(), c, m, c)
        cx.connect(m, c, cx.graph_out_node(), c)
    node.morph_to(1.0, 96, fa.CrossfadeNode.EASE_IN)      # before the first update
    cx.update()
    out, end = (LL * 15)(), ULL(0)
    assert P.fmp_node(cx.c, m, out, C.byref(end)) == 1 and (out[0], out[1], out[2], out[7]) == (1, a, b, 300)
    cx.process_interleaved(np.zeros(256, F32), 2, 2, 128)
    node.set_ir(0, third)
    assert node.ir == third
    node.morph_to_secs(0.0, 0.01, at_block=1)
    assert node.position == 0.0 and P.fwp_early_count(cx.c) == 1
    cx.update()
    assert cx.fir_morph_stats() == (0, 0)
    for bad in (lambda: node.morph_to(1.5, 10), lambda: node.morph_to(0.5, FRAMES_MAX + 1), lambda: node.morph_to(0.5, 10, (2.0, 0, 1, 1)),
                lambda: node.set_ir(2, a), lambda: node.set_ir(1, None)):      # (the last: slot B is where the morph came from: audible)
        with pytest.raises(fa.FwgpuError):
            bad()
    plain = fa.FirReverbNode(a)
    cx.add_node(2, 2, plain)
    with pytest.raises(fa.FwgpuError):
        plain.morph_to(1.0, 10)
    cx.close()
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    for decl in ("int fwgpu_fir_morph(fwgpu_ctx* ctx, int64_t node, float position, uint32_t frames, int shape, float x1, float y1, float x2, "
                 "float y2,\n                    uint32_t at_block);",
                 "int fwgpu_fir_set_ir(fwgpu_ctx* ctx, int64_t node, int slot, int sample);",
                 "int fwgpu_fir_morph_stats(fwgpu_ctx* ctx, uint64_t* tiles_run, uint64_t* tiles_skipped);"):
        assert decl in hdr, decl
    assert re.search(r"FWGPU_FIR = 12\b", hdr)
    ffi = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "ffi.rs")).read()
    assert ("pub fn fwgpu_fir_morph(ctx: *mut fwgpu_ctx, node: i64, position: f32, frames: u32, shape: c_int, x1: f32, y1: f32, x2: f32, "
            "y2: f32, at_block: u32) -> c_int;") in ffi
    assert "pub fn fwgpu_fir_set_ir(ctx: *mut fwgpu_ctx, node: i64, slot: c_int, sample: c_int) -> c_int;" in ffi
    assert "pub fn fwgpu_fir_morph_stats(ctx: *mut fwgpu_ctx, tiles_run: *mut u64, tiles_skipped: *mut u64) -> c_int;" in ffi
    nodes = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "nodes.rs")).read()
    assert "pub fn morph_to(" in nodes and "pub fn set_ir(" in nodes and "ffi::fwgpu_fir_morph" in nodes and "ffi::fwgpu_fir_set_ir" in nodes
    types = open(os.path.join(ROOT, "firewheel_amd", "csrc", "fwgpu_types.h")).read()
    assert "fir_morph_state_ok" in types and re.search(r"#define FIR_MORPH_BLK_FLOATS 16\b", types)


# ================================================================================================ GPU tier
gpu = pytest.mark.gpu


class Rig(object):
    """graph input (ch channels) -> one morph-capable FIR node -> graph output, on the GPU; `dry` (the hybrid plan): eight silent
    sampler voices on a SumNode of their own, as tests/test_gpu_fir.py stream_rig"""

    def __init__(self, mbf, K, plan, ha, hb, T=0, position=0.0, law=EQUAL_POWER, ch=2, fmt_a=PLANAR_F32, fmt_b=PLANAR_F32):
        g = GpuEngine(max_block_frames=mbf, max_batch=K, num_graph_inputs=ch, num_graph_outputs=ch, force_generic=plan == "generic")
        self.g, self.ch, self.mbf = g, ch, mbf
        self.ira = g.new_sample(fmt_a, np.atleast_2d(ha).shape[0], ha)
        self.irb = -1 if hb is None else g.new_sample(fmt_b, np.atleast_2d(hb).shape[0], hb)
        self.f = g.add_node(FIR, ch, ch, [float(self.ira), float(self.irb), float(T), position, float(law)])
        _wire(g, self.f, ch)
        if plan == "hybrid":
            m = g.sum(8)
            for v in range(8):
                g.connect_stereo(g.sampler(100.0), m, 2 * v)
        g.update()
        assert g.cx.plan_kind() == PLAN_KIND[plan]

    def to(self, position, frames, curve=None, at_block=0):
        assert _morph(self.g, self.f, position, frames, curve, at_block) == 0

    def call(self, x):
        y = self.g.process_interleaved(len(x), self.ch, inp=np.ascontiguousarray(x).reshape(-1), n_in_ch=self.ch)
        return np.asarray(y, F32).reshape(-1, self.ch)

    def run(self, x, calls, msgs=()):
        """msgs: {call index: [(at_block, position, frames, curve), ...]} sent, in order, in front of that call"""
        msgs, out, pos = dict(msgs), [], 0
        for i, n in enumerate(calls):
            for (at_block, position, frames, curve) in msgs.get(i, ()):
                self.to(position, frames, curve, at_block)
            out.append(self.call(x[pos:pos + n]))
            pos += n
        return np.concatenate(out)


def model_messages(calls, mbf, msgs):
    """the Rig's per-call messages keyed by the run's block index, as fir_morph_model.render takes them"""
    out, blk = {}, 0
    for i, n in enumerate(calls):
        for (at_block, position, frames, curve) in dict(msgs).get(i, ()):
            out.setdefault(blk + at_block, []).append((position, frames, curve))
        blk += (n + mbf - 1) // mbf
    return out


def slot_sums(h, T, x, calls, mbf, fmt=PLANAR_F32):
    """refmodel.FirNode for the small T, the oracle for the larger ones (the CPU tier holds the two against each other)"""
    if h is None:
        return None
    if T <= 2:
        return M.slot_sum_ref(h, T, x, M.blocks_of(calls, mbf))
    return M.slot_sum_oracle(h, T, x, calls, mbf, fmt)


def plain_gpu(h, T, x, calls, mbf, K, plan):
    """the plain one-parameter node on the padded impulse response, on the GPU"""
    hp = M.pad_ir(h, T)
    g = GpuEngine(max_block_frames=mbf, max_batch=K, num_graph_inputs=2, num_graph_outputs=2, force_generic=plan == "generic")
    f = g.fir(g.new_sample(PLANAR_F32, hp.shape[0], hp))
    _wire(g, f)
    g.update()
    out, pos = [], 0
    for n in calls:
        y = g.process_interleaved(n, 2, inp=np.ascontiguousarray(x[pos:pos + n]).reshape(-1), n_in_ch=2)
        out.append(np.asarray(y, F32).reshape(-1, 2))
        pos += n
    return np.concatenate(out)


# ------------------------------------------------------------------ g1. at rest
@gpu
@pytest.mark.parametrize("position,plan", [(0.0, "hybrid"), (1.0, "generic"), (0.0, "generic"), (1.0, "hybrid")])
def test_g1_at_rest_is_the_plain_node_and_the_idle_slot_costs_no_matrix_work(position, plan):
    T, mbf, K = 4097, 256, 4
    ha, hb = scenarios.reverb_ir(31, 4097, 2), scenarios.reverb_ir(32, 300, 2)
    calls = [4 * mbf, 3 * mbf, 4 * mbf]
    x = noise(33, sum(calls), 2)
    r = Rig(mbf, K, plan, ha, hb, position=position)
    run0, skip0 = r.g.cx.fir_morph_stats()
    y = r.run(x, calls)
    run1, skip1 = r.g.cx.fir_morph_stats()
    h = ha if position == 0.0 else hb
    assert_bits(y, M.slot_sum_oracle(h, T, x, calls, mbf), "the slot sum of the audible slot (oracle)")
    assert_bits(y, plain_gpu(h, T, x, calls, mbf, K, plan), "the plain node on the padded impulse response (GPU)")
    per_slot = 2 * M.gemm_workgroups(1, T, mbf) * 11      # a tile per channel of the slot's impulse response, two segments, 11 blocks
    assert per_slot == 44
    assert (run1 - run0, skip1 - skip0) == (per_slot, per_slot)


# ------------------------------------------------------------------ g2. fades in flight
def fade_script(mbf):
    """calls (frames) and per-call messages: a message at at_block > 0 inside a batch, a segment that ends inside a block, a call
    that ends in a short block, a retarget in mid-fade, rest in between, frames = 0, two messages for one block"""
    calls = [4 * mbf, 4 * mbf, 3 * mbf + 37, 4 * mbf, 2 * mbf, 4 * mbf, 3 * mbf]
    msgs = {
        1: [(1, 1.0, 2 * mbf + mbf // 2, None)],             # linear, from block 1 of a batch; ends in the middle of block 3
        2: [(2, 0.0, 3 * mbf, EASE)],                        # Bezier, across the short block and into the next call
        3: [(1, 0.3, mbf + 17, None)],                       # a retarget in mid-fade; then at rest in between
        5: [(0, 1.0, 0, None), (2, 0.5, 10, None), (2, 0.0, 2 * mbf, OVERSHOOT)],   # a jump; two messages for one block, in send order
    }
    return calls, msgs


G2 = [(T, mbf, K) for T in (1, 2, 300, 4097) for mbf in (64, 256, 512) for K in (1, 4)]


@gpu
@pytest.mark.parametrize("T,mbf,K", G2)
def test_g2_fades_in_flight(T, mbf, K):
    i = G2.index((T, mbf, K))
    law, plan = (LINEAR_LAW, EQUAL_POWER)[i % 2], ("hybrid", "generic")[(i // 2 + i // 6) % 2]
    la, lb = T, max(1, T - T // 3)
    ha, hb = scenarios.reverb_ir(40 + T, la, 2), scenarios.reverb_ir(41 + T, lb, 2)
    calls, msgs = fade_script(mbf)
    x = noise(42 + T + mbf, sum(calls), 2)
    y = Rig(mbf, K, plan, ha, hb, law=law).run(x, calls, msgs)
    sa, sb = slot_sums(ha, T, x, calls, mbf), slot_sums(hb, T, x, calls, mbf)
    want, modes = M.render(M.Morph(0.0, law), sa, sb, M.blocks_of(calls, mbf), model_messages(calls, mbf, msgs))
    assert {M.MODE_A, M.MODE_B, M.MODE_BOTH} <= set(modes)
    assert_bits(y, want, "T=%d mbf=%d K=%d law=%d %s" % (T, mbf, K, law, plan))


# ------------------------------------------------------------------ g3. unequal lengths and formats
@gpu
@pytest.mark.parametrize("what", ["300_4097", "4097_300", "mono_ir", "i16_ir", "empty_b"])
def test_g3_unequal_lengths_and_formats(what):
    mbf, K = 256, 4
    calls, msgs = fade_script(mbf)
    x = noise(50, sum(calls), 2)
    fa = fb = PLANAR_F32
    if what == "300_4097":
        ha, hb, T = scenarios.reverb_ir(51, 300, 2), scenarios.reverb_ir(52, 4097, 2), 4097
    elif what == "4097_300":
        ha, hb, T = scenarios.reverb_ir(53, 4097, 2), scenarios.reverb_ir(54, 300, 2), 4097
    elif what == "mono_ir":
        ha, hb, T = scenarios.reverb_ir(55, 300, 1), scenarios.reverb_ir(56, 190, 2), 300
    elif what == "i16_ir":
        ha, T = scenarios.reverb_ir(57, 300, 2), 300
        hb = np.round(scenarios.reverb_ir(58, 211, 2) * 32767.0 * 20.0).clip(-32768, 32767).astype(np.int16)
        fb = PLANAR_I16
    else:
        ha, hb, T = scenarios.reverb_ir(59, 300, 2), None, 300
    plan = "hybrid" if what in ("300_4097", "i16_ir") else "generic"
    y = Rig(mbf, K, plan, ha, hb, law=EQUAL_POWER, fmt_a=fa, fmt_b=fb).run(x, calls, msgs)
    sa, sb = slot_sums(ha, T, x, calls, mbf, fa), slot_sums(hb, T, x, calls, mbf, fb)
    want, _ = M.render(M.Morph(0.0, EQUAL_POWER), sa, sb, M.blocks_of(calls, mbf), model_messages(calls, mbf, msgs))
    assert_bits(y, want, what)
    if what == "empty_b":      # the wet fader: all of "slot B" is silence
        blocks = M.blocks_of(calls, mbf)
        at_b = [i for i, m in enumerate(M.render(M.Morph(0.0, EQUAL_POWER), sa, None, blocks, model_messages(calls, mbf, msgs))[1]) if m == M.MODE_B]
        assert at_b
        start = sum(blocks[:at_b[0]])
        assert not fwapi.bits(y[start:start + blocks[at_b[0]]]).any()


# ------------------------------------------------------------------ g4. a bank
@gpu
def test_g4_a_bank_of_morph_nodes_beside_plain_nodes():
    T, mbf, K, N = 300, 256, 4, 40
    g = GpuEngine(max_block_frames=mbf, max_batch=K, num_graph_inputs=2, num_graph_outputs=44, force_generic=True)
    hs = [scenarios.reverb_ir(60 + i, (300, 220, 300, 170)[i], 2) for i in range(4)]      # pair p: A = hs[p], B = hs[2 + p]
    irs = [g.new_sample(PLANAR_F32, 2, h) for h in hs]
    start = lambda i: (0.0, 1.0, 0.0, 0.3)[i % 4]      # rests at A, rests at B, will be in flight, rests in between
    pair = lambda i: (i // 4) % 2
    nodes = [g.add_node(FIR, 2, 2, [float(irs[pair(i)]), float(irs[2 + pair(i)]), 300.0, start(i), float(i % 2)]) for i in range(N)]
    nodes += [g.fir(irs[0]), g.fir(irs[2]), g.fir(irs[0])]      # plain nodes of the same T on the same level
    for n in nodes:
        for c in range(2):
            g.connect(g.graph_in_node, c, n, c)
    for q in range(21):      # pairs of nodes through a SumNode (a + b, one f32 addition), the last node on its own
        m = g.sum(2)
        g.connect_stereo(nodes[2 * q], m, 0)
        g.connect_stereo(nodes[2 * q + 1], m, 2)
        for c in range(2):
            g.connect(m, c, g.graph_out_node, 2 * q + c)
    for c in range(2):
        g.connect(nodes[42], c, g.graph_out_node, 42 + c)
    g.update()
    calls = [4 * mbf, 4 * mbf, 2 * mbf + 100]
    x = noise(64, sum(calls), 2)
    flights = {i: (1, 1.0 if i % 8 == 2 else 0.65, 1500 + 10 * i, EASE if i % 8 == 2 else None) for i in range(N) if i % 4 == 2}
    run0, skip0 = g.cx.fir_morph_stats()
    out, pos = [], 0
    for ci, n in enumerate(calls):
        if ci == 0:
            for i, (at_block, position, frames, curve) in flights.items():
                assert _morph(g, nodes[i], position, frames, curve, at_block) == 0
        y = g.process_interleaved(n, 44, inp=np.ascontiguousarray(x[pos:pos + n]).reshape(-1), n_in_ch=2)
        out.append(np.asarray(y, F32).reshape(-1, 44))
        pos += n
    y = np.concatenate(out)
    run1, skip1 = g.cx.fir_morph_stats()
    sums = [M.slot_sum_oracle(h, T, x, calls, mbf) for h in hs]      # computed once, shared by the 43 nodes
    blocks = M.blocks_of(calls, mbf)
    want = []
    for i in range(N):
        msgs = {flights[i][0]: [flights[i][1:]]} if i in flights else {}
        want.append(M.render(M.Morph(start(i), i % 2), sums[pair(i)], sums[2 + pair(i)], blocks, msgs)[0])
    want += [sums[0], sums[2], sums[0]]
    for q in range(21):
        assert_bits(y[:, 2 * q:2 * q + 2], (want[2 * q] + want[2 * q + 1]).astype(F32), "nodes %d + %d" % (2 * q, 2 * q + 1))
    assert_bits(y[:, 42:44], want[42], "the last plain node")
    # 80 rows per slot = 20 per impulse-response channel: four padded tiles per slot; every tile holds a node that runs both slots
    total = sum(2 * 4 * M.gemm_workgroups(32, T, mbf, f) for f in blocks)
    assert (run1 - run0) + (skip1 - skip0) == total and skip1 == skip0


# ------------------------------------------------------------------ g5. set_ir
@gpu
@pytest.mark.parametrize("plan,held", [("hybrid", False), ("generic", True)])
def test_g5_set_ir_swaps_a_silent_slot_and_the_new_tail_is_complete(plan, held):
    T, mbf, K = 300, 64, 2      # R = 299 + 128 = 427
    h1, h2, h3 = scenarios.reverb_ir(70, 300, 2), scenarios.reverb_ir(71, 300, 2), scenarios.reverb_ir(72, 260, 1)
    r = Rig(mbf, K, plan, h1, h2, law=EQUAL_POWER)
    third = r.g.new_sample(PLANAR_F32, 1, h3)
    calls = [2 * mbf, 4 * mbf, 2 * mbf, 2 * mbf, 2 * mbf, 6 * mbf, 4 * mbf]      # 1408 frames: more than three ring lengths
    x = noise(73, sum(calls), 2)
    bounds = np.cumsum([0] + calls)
    out = [r.call(x[bounds[0]:bounds[1]])]                       # at rest at A
    r.to(1.0, 100, EASE, at_block=1)
    out.append(r.call(x[bounds[1]:bounds[2]]))                   # the fade ends 164 frames into this call
    assert _set_ir(r.g, r.f, 0, third) == 0                      # slot A is silent now
    if held:
        r.to(0.0, 200, None, at_block=1)                         # held until the update below
    out.append(r.call(x[bounds[2]:bounds[3]]))                   # between the edit and the adoption: unchanged, all of B
    r.g.update()
    if held:
        out.append(r.call(x[bounds[3]:bounds[4]]))               # the released morph starts at block 1 of this call
        out.append(r.call(x[bounds[4]:bounds[5]]))
    else:
        out.append(r.call(x[bounds[3]:bounds[4]]))               # adopted, still all of B: when the swap lands cannot be observed
        r.to(0.0, 200, None, at_block=1)
        out.append(r.call(x[bounds[4]:bounds[5]]))
    out.append(r.call(x[bounds[5]:bounds[6]]))
    out.append(r.call(x[bounds[6]:bounds[7]]))
    y = np.concatenate(out)
    # the model: slot A is h1 until it fell silent and h3 — convolved with the WHOLE input history — from then on
    s1, s2, s3 = (M.slot_sum_oracle(h, T, x, calls, mbf) for h in (h1, h2, h3))
    swap = bounds[2]
    sa = np.where((np.arange(len(x)) < swap)[:, None], s1, s3)
    back_call = 3 if held else 4
    msgs = {1: [(1, 1.0, 100, EASE)], back_call: [(1, 0.0, 200, None)]}
    want, modes = M.render(M.Morph(0.0, EQUAL_POWER), sa, s2, M.blocks_of(calls, mbf), model_messages(calls, mbf, msgs))
    assert_bits(y, want, "set_ir")
    first = bounds[back_call] + mbf      # the first faded-in frames carry the full tail of the third impulse response
    assert np.any(fwapi.bits(y[first + 1:first + 64]) != fwapi.bits(s2[first + 1:first + 64]))
    assert_bits(y[-mbf:], s3[-mbf:], "at rest at the new slot A")
    assert modes[-1] == M.MODE_A and modes[bounds[3] // mbf - 1] == M.MODE_B


# ------------------------------------------------------------------ g6. one-block callbacks
@gpu
@pytest.mark.parametrize("plan", ["hybrid", "generic"])
def test_g6_one_block_callbacks_through_two_ring_wraps(plan):
    T, mbf, K = 300, 64, 4      # R = 555
    ha, hb = scenarios.reverb_ir(80, 300, 2), scenarios.reverb_ir(81, 141, 2)
    calls = [mbf] * 20          # 1280 frames > 2 R
    x = noise(82, sum(calls), 2)
    msgs = {2: [(0, 1.0, 900, EASE)], 17: [(0, 0.25, 100, None)]}
    y = Rig(mbf, K, plan, ha, hb, law=LINEAR_LAW).run(x, calls, msgs)
    sa, sb = M.slot_sum_oracle(ha, T, x, calls, mbf), M.slot_sum_oracle(hb, T, x, calls, mbf)
    want, _ = M.render(M.Morph(0.0, LINEAR_LAW), sa, sb, M.blocks_of(calls, mbf), model_messages(calls, mbf, msgs))
    assert_bits(y, want, "one-block calls, %s" % plan)
