"""The level meter node (FWGPU_METER = 16; SPEC): per block and input channel the peak, the f32 sum of squares in
a fixed order and the number of samples over 1.0, measured on the device; the audio passes through bit for bit.

Reference for the readings: `model_block` below, a numpy restatement of the SPEC's text (not of the kernel), applied to a signal that
was obtained without the meter —
  * a master meter: the OracleEngine's output of the same graph built WITHOUT meters (a meter in front of graph_out sees exactly that);
  * a meter on a leaf bus, inside a voice chain, or a tap: the output of another oracle graph whose graph_out is wired to the metered
    bus (for a tap the oracle graph simply lacks the node);
  * a graph fed from stream inputs: the input itself.
peak, over, frames and sum_squares are compared bit for bit (two NaNs compare equal); the GPU tier has no tolerance anywhere.

CPU tier: shapes and creation parameters, the planner (plans, launches and lazy calls unchanged by master meters) and the
fwgpu_meter_read contract on the host-only harness, and the model's own error bound.

One figure of the issue is restated: it counts "3 + 5 + a 100-frame partial call" at max_block_frames 64 as 9 blocks, but 100 frames
at 64 are TWO blocks (64 + 36) under its own rule "every block it processes, full or partial": the count is 10, and a 36-frame call
on its own then adds 1.
"""
import os

import numpy as np
import pytest

import fwapi
import scenarios
from fwapi import LOOP_FULL, GpuEngine, HostOnlyEngine, OracleEngine

METER = 16
INVALID = -20
FUZZ_SEEDS = int(os.environ.get("FWGPU_FUZZ_SEEDS", "20"))


# ------------------------------------------------------------------------------------------------ the SPEC in numpy
def model_block(x):
    """one block of one channel -> (peak, sum_squares, over, frames), from DESIGN.md section 6 / include/fwgpu.h"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.size
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(x)
        ok = a[~np.isnan(a)]
        peak = np.float32(ok.max()) if ok.size else np.float32(0.0)  # NaN samples ignored; never negative: |-0.0| = +0.0
        over = int(np.count_nonzero(a > np.float32(1.0)))            # NaN > 1 is false
        sq = (x * x).astype(np.float32)                              # one f32 product per sample
        rows = np.concatenate([sq, np.zeros((-n) % 256, dtype=np.float32)]).reshape(-1, 256)  # (+0.0 added to a sum >= 0 changes no bit)
        acc = np.zeros(256, dtype=np.float32)
        for r in rows:                                               # acc[j] += x[i] * x[i] for i = j, j + 256, ... ascending
            acc = (acc + r).astype(np.float32)
        t = (((acc[0::4] + acc[1::4]).astype(np.float32) + acc[2::4]).astype(np.float32) + acc[3::4]).astype(np.float32)
        h = 32
        while h >= 1:                                                # t[l] = t[l] + t[l + h] for l < h
            t = (t[:h] + t[h:2 * h]).astype(np.float32)
            h //= 2
    return peak, np.float32(t[0]), over, n


def model(signal, mbf):
    """signal [channels][frames] -> structured [blocks][channels]; the last block may be short"""
    from firewheel_amd.graph import METER_DTYPE

    signal = np.atleast_2d(np.asarray(signal, dtype=np.float32))
    nb = (signal.shape[1] + mbf - 1) // mbf
    out = np.zeros((nb, signal.shape[0]), dtype=METER_DTYPE)
    for b in range(nb):
        for c in range(signal.shape[0]):
            out[b, c] = model_block(signal[c, b * mbf:(b + 1) * mbf])
    return out


def assert_readings(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("peak", "sum_squares"):
        g, w = got[f].view(np.uint32), want[f].view(np.uint32)
        same = (g == w) | (np.isnan(got[f]) & np.isnan(want[f]))
        bad = np.argwhere(~same)
        assert bad.size == 0, "%s: %s differs in %d of %d records, first (block, channel) %s: %r vs %r" % (
            what, f, len(bad), same.size, tuple(bad[0]), got[f][tuple(bad[0])], want[f][tuple(bad[0])])
    for f in ("over", "frames"):
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, "%s: %s differs, first (block, channel) %s: %d vs %d" % (what, f, tuple(bad[0]), got[f][tuple(bad[0])], want[f][tuple(bad[0])])


def assert_bits(a, b, what, sounding=True):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    bad = np.nonzero(fwapi.bits(a) != fwapi.bits(b))[0]
    assert bad.size == 0, "%s: %d of %d samples differ, first at %d: %r vs %r" % (what, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]])
    if sounding:
        assert np.any(a != 0), what + ": nothing sounded"


def planar(interleaved, ch=2):
    return np.asarray(interleaved, dtype=np.float32).reshape(-1, ch).T


# ------------------------------------------------------------------------------------------------ graphs with places for meters
# places: ("src", i) behind voice i's sampler, ("voice", i) at the end of its chain, ("leaf", j) behind leaf sum j, ("master", k)
# behind the k-th node of the master chain (0 = behind the root sum).  `meters` maps a place to (n_out, ring_blocks): 2 = a pass-through
# in the signal path, 0 = a tap beside it.  `probe`: the place graph_out is wired to (oracle graphs that produce a meter's input).
def _stage(e, tok, rng, delay_frames):
    if tok == "v":
        return e.volume(float(rng.uniform(30, 100)))
    if tok == "p":
        return e.pan(float(rng.uniform(-1, 1)))
    if tok == "c":
        return e.hard_clip(-3.0)
    if tok == "C":
        return e.hard_clip(0.0)  # 0 dB: the threshold is 1.0
    if tok == "w":
        return e.width(1.3)
    if tok == "B":
        return e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 8000)), float(rng.choice([0.707, 1.8])))
    if tok == "D":
        return e.delay(delay_frames / float(e.sample_rate), feedback=float(rng.choice([0.0, 0.45])), mix=0.5)
    raise ValueError(tok)


class Bank(object):
    pass


def build(e, shapes, master=("v",), meters=None, probe=None, radix=4, seed=0, send=False, src_blocks=6, master_volume=90.0, dangling=False):
    meters = meters or {}
    b = Bank()
    b.e, b.meter, b.probe_node = e, {}, None
    rng = np.random.default_rng(4200 + seed)

    def place(node, key):
        if key == probe:
            b.probe_node = node
        if key in meters:
            n_out, ring = meters[key]
            m = e.add_node(METER, 2, n_out, [ring] if ring is not None else [])
            e.connect_stereo(node, m)
            b.meter[key] = m
            if n_out:
                return m
        return node

    b.samplers, b.vols, ends = [], [], []
    for i, sh in enumerate(shapes):
        s = e.sampler(100.0)
        b.samplers.append(s)
        cur = place(s, ("src", i))
        vols = []
        for t in sh:
            n = _stage(e, t, rng, (64, 129, 300, 384)[i % 4])
            if t == "v":
                vols.append(n)
            e.connect_stereo(cur, n)
            cur = n
        b.vols.append(vols)
        ends.append(place(cur, ("voice", i)))
    leaves = []
    for j, i in enumerate(range(0, len(ends), radix)):
        grp = ends[i:i + radix]
        m = e.sum(max(2, len(grp)))
        for p, n in enumerate(grp):
            e.connect_stereo(n, m, 2 * p)
        leaves.append(place(m, ("leaf", j)))
    root = e.sum(max(2, len(leaves) + (1 if send else 0)))
    for p, m in enumerate(leaves):
        e.connect_stereo(m, root, 2 * p)
    if send:  # leaf 0's bus is consumed twice: dry into the root and through a send delay (not a fused shape as a whole: plan 3)
        d = e.delay(300 / float(e.sample_rate), feedback=0.3, mix=1.0)
        e.connect_stereo(leaves[0], d)
        e.connect_stereo(d, root, 2 * len(leaves))
    cur = place(root, ("master", 0))
    b.master, b.master_toks = [], list(master)
    for k, t in enumerate(master, 1):
        n = e.volume(master_volume) if t == "v" else _stage(e, t, rng, 200)
        b.master.append(n)
        e.connect_stereo(cur, n)
        cur = place(n, ("master", k))
    if probe is not None:
        assert b.probe_node is not None, probe
        cur = b.probe_node
    e.connect_stereo(cur, e.graph_out_node)
    if dangling:
        b.dangling = e.add_node(fwapi.DUMMY, 1, 1)
    e.update()
    mbf = e.max_block_frames
    for i, s in enumerate(b.samplers):
        e.sampler_set_sample(s, e.new_sample(fwapi.PLANAR_F32, 2, scenarios.voice_source(seed * 1000 + 31 + i, src_blocks * mbf, 2)))
    return b


def script(e, b, calls=(3, 5, 2, 4, 6, 3, 5)):
    """steady calls, glides in the voices and on the master, a source pause and a resume, message-free calls in between"""
    for s in b.samplers:
        e.sampler_set_loop_range(s, LOOP_FULL)
        e.sampler_play(s)
    out = [e.process_blocks(calls[0]), e.process_blocks(calls[1])]
    for i, vols in enumerate(b.vols):
        for j, n in enumerate(vols):
            if (i + j) % 2 == 0:
                e.set_param(n, 0, 20.0 + 7.0 * ((i + j) % 5), at_block=1 + (i % 2))
    if b.master and b.master_toks[0] == "v":
        e.set_param(b.master[0], 0, 60.0, at_block=1)
    out.append(e.process_blocks(calls[2]))
    out.append(e.process_blocks(calls[3]))
    for i, s in enumerate(b.samplers):
        if i % 3 == 0:
            e.sampler_pause(s, at_block=1)
    out.append(e.process_blocks(calls[4]))
    for i, s in enumerate(b.samplers):
        if i % 3 == 0:
            e.sampler_play(s, at_block=0)
    out.append(e.process_blocks(calls[5]))
    out.append(e.process_blocks(calls[6]))
    return np.concatenate([np.asarray(o) for o in out])


def oracle(mbf):
    return scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf))


DRY = ["v", "vp", "", "pv", "vc", "v", "vp", "p", "v"]
CHAIN = ["vB", "BD", "v", "vBD", "vp", "DBv", "BB", "cB", "v"]
PLANS = {1: dict(shapes=DRY), 2: dict(shapes=CHAIN), 3: dict(shapes=DRY, send=True)}


# ================================================================================================ CPU tier
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (2, 2), (5, 5), (64, 64), (2, 0), (7, 0)])
@pytest.mark.parametrize("ring", [1, 8, 1024, 65536])
def test_shapes_and_rings_that_activate(n_in, n_out, ring):
    e = HostOnlyEngine(max_block_frames=64)
    m = e.add_node(METER, n_in, n_out, [ring])
    e.update()
    e.process_blocks(2)
    rd, done = e.cx.meter_read(m, max(0, 2 - ring), 2)
    assert done == 2 and rd.shape == (min(ring, 2), n_in) and e.violation() == ""


def test_default_ring_is_1024_blocks():
    e = HostOnlyEngine(max_block_frames=64, max_batch=64)
    m = e.add_node(METER, 2, 0)
    e.update()
    for _ in range(17):
        e.process_blocks(64)
    assert e.cx.meter_read(m, 1088 - 1024, 4)[0].shape == (4, 2)
    with pytest.raises(e.fa.FwgpuError) as ei:
        e.cx.meter_read(m, 1088 - 1025, 4)
    assert ei.value.code == INVALID


@pytest.mark.parametrize("n_in,n_out", [(2, 1), (0, 0), (3, 2), (65, 65)])
def test_shapes_that_do_not_activate(n_in, n_out):
    e = HostOnlyEngine(max_block_frames=64)
    v = e.volume(50.0)
    e.connect_stereo(v, e.graph_out_node)
    try:
        m = e.add_node(METER, n_in, n_out, [8])
    except e.fa.FwgpuError as err:  # (more than 64 ports per side: refused where every kind is, at add_node)
        assert n_in > 64 and err.code == INVALID
    else:
        with pytest.raises(fwapi.CompileGraphError) as ei:
            e.update()
        assert ei.value.name == "NodeActivationFailed", ei.value
        e.remove_node(m)
    e.update()  # the graph is usable
    e.process_blocks(2)
    assert e.violation() == ""


@pytest.mark.parametrize("ring", [0.0, -3.0, 65537.0, float("nan"), 1e30])
def test_rings_that_do_not_activate(ring):
    e = HostOnlyEngine(max_block_frames=64)
    v = e.volume(50.0)
    e.connect_stereo(v, e.graph_out_node)
    m = e.add_node(METER, 2, 2, [ring])
    with pytest.raises(fwapi.CompileGraphError) as ei:
        e.update()
    assert ei.value.name == "NodeActivationFailed", ei.value
    with pytest.raises(fwapi.CompileGraphError):
        e.update()  # (still there, still refused)
    e.remove_node(m)
    good = e.add_node(METER, 2, 2, [8])
    e.connect_stereo(v, good)
    e.update()
    e.process_blocks(3)
    assert e.cx.meter_read(good, 0, 3)[1] == 3 and e.violation() == ""


def _harness_run(plan, meters, max_batch, master=("v", "c")):
    e = HostOnlyEngine(max_block_frames=128, max_batch=max_batch)
    b = build(e, master=master, meters=meters, **PLANS[plan])
    e.reset_launches()
    calls = (3, 5, 2, 4, 6, 3, 5)
    script(e, b, calls)
    la = e.launches()
    for _ in range(6):
        e.process_blocks(4)  # message-free calls, the glides long settled on the fake device
    return e, b, la, sum((k + max_batch - 1) // max_batch for k in calls)


@pytest.mark.parametrize("plan", [1, 2, 3])
@pytest.mark.parametrize("max_batch", [64, 3])
def test_master_meters_leave_the_plan_its_launches_and_its_lazy_calls_alone(plan, max_batch):
    e0, _, la0, batches = _harness_run(plan, {}, max_batch)
    assert e0.cx.plan_kind() == plan and e0.violation() == ""
    for meters in ({("master", 2): (2, 16)}, {("master", 0): (2, 16), ("master", 1): (2, 1024), ("master", 2): (2, 4)}):
        e, b, la, _ = _harness_run(plan, meters, max_batch)
        assert e.violation() == "", e.violation()
        assert e.cx.plan_kind() == e0.cx.plan_kind() and e.cx.plan_fused_voices() == e0.cx.plan_fused_voices()
        want = dict(la0, level=la0["level"] + len(meters) * batches)
        assert la == want, (la, want)
        assert e.cx.lazy_stats()[0] == e0.cx.lazy_stats()[0], (e.cx.lazy_stats(), e0.cx.lazy_stats())
        if plan != 3:
            assert e.cx.lazy_stats()[0] > 0  # (lazy calls do happen on the fused plans)
        for m in b.meter.values():
            assert e.cx.meter_read(m, 0, 0)[1] == 28 + 24


@pytest.mark.parametrize("plan", [1, 2])
def test_a_master_chain_of_nothing_but_a_meter_keeps_the_plan_kind(plan):
    e = HostOnlyEngine(max_block_frames=128, max_batch=8)
    build(e, master=(), meters={("master", 0): (2, 8)}, **PLANS[plan])
    assert e.cx.plan_kind() == plan
    e.process_blocks(5)
    assert e.violation() == ""


def test_meter_read_contract_on_the_harness():
    e = HostOnlyEngine(max_block_frames=64, max_batch=4)
    v = e.volume(50.0)
    m = e.add_node(METER, 2, 2, [8])
    other = e.add_node(METER, 3, 0, [2])
    e.connect_stereo(v, m)
    e.connect_stereo(m, e.graph_out_node)
    e.update()
    assert e.cx.meter_read(m, 0, 4)[0].shape == (0, 2) and e.cx.meter_read(m, 0, 0)[1] == 0
    e.process_blocks(3)
    e.process_blocks(5)
    e.process_interleaved(100)   # 64 + 36 frames: two blocks (see the module's docstring)
    rd, done = e.cx.meter_read(m, 0, 0)
    assert done == 10 and rd.shape[0] == 0
    e.process_interleaved(36)    # a short block on its own is one block
    assert e.cx.meter_read(m, 0, 0)[1] == 11
    # n clips to what exists; the harness' kernels are no-ops: the records are the ring's zeros
    rd, done = e.cx.meter_read(m, 9, 5)
    assert done == 11 and rd.shape == (2, 2) and not rd["peak"].any() and not rd["frames"].any()
    assert e.cx.meter_read(m, 11, 3)[0].shape == (0, 2) and e.cx.meter_read(m, 400, 3)[0].shape == (0, 2)
    assert e.cx.meter_read(other, 9, 2)[0].shape == (2, 3)
    # just inside the ring / one block further back
    assert e.cx.meter_read(m, 3, 8)[0].shape == (8, 2)

    def refused(node, first, n, out_null=False):
        import ctypes as C

        from firewheel_amd import _lib

        done = C.c_uint64(777)
        buf = (_lib.MeterReading * 64)()
        rc = e.cx.L.fwgpu_meter_read(e.cx.c, node, first, n, None if out_null else buf, C.byref(done))
        assert rc == INVALID and done.value == 11, (rc, done.value)

    refused(m, 2, 8)
    refused(m, 0, 1)
    refused(other, 8, 1)              # (a ring of 2)
    refused(v, 9, 1)                  # not a meter
    refused(e.graph_out_node, 9, 1)
    refused(12345 << 32, 9, 1)        # no such node
    refused(m, 9, 1, out_null=True)   # blocks requested, nowhere to put them
    # a meter added later: blocks before its first plan are refused, the block count goes on
    late = e.add_node(METER, 2, 0, [64])
    e.connect_stereo(v, late)
    e.update()
    refused(late, 10, 1)
    e.process_blocks(2)
    assert e.cx.meter_read(late, 11, 4)[0].shape == (2, 2) and e.cx.meter_read(m, 11, 4)[1] == 13
    # a removed meter is no meter of the plan any more
    e.remove_node(late)
    e.update()
    with pytest.raises(e.fa.FwgpuError):
        e.cx.meter_read(late, 11, 1)
    assert e.violation() == ""
    assert e.cx.L.fwgpu_meter_read(None, m, 0, 0, None, None) == INVALID


def test_typed_mirror_node_and_db_helpers():
    import firewheel_amd as fa
    from firewheel_amd import graph as G

    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=0, num_graph_outputs=2)
    v = cx.add_node(2, 2, G.VolumeNode(50.0))
    node = fa.MeterNode(ring_blocks=16)
    m = cx.add_node(2, 2, node)
    for c in range(2):
        cx.connect(v, c, m, c)
        cx.connect(m, c, cx.graph_out_node(), c)
    cx.update()
    cx.process_interleaved(None, 0, 2, 64 * 3)
    rd, done = node.read(0, 8)
    assert done == 3 and rd.shape == (3, 2) and rd.dtype == G.METER_DTYPE
    r = np.zeros(3, dtype=G.METER_DTYPE)
    r["peak"], r["sum_squares"], r["frames"] = [1.0, 0.5, 0.0], [64.0, 16.0, 0.0], 64
    assert_bits(G.MeterNode.peak_db(r), np.array([0.0, 20.0 * np.log10(np.float32(0.5)), -np.inf], dtype=np.float32), "peak_db", sounding=False)
    assert_bits(G.MeterNode.rms_db(r), np.array([0.0, 20.0 * np.log10(np.float32(0.5)), -np.inf], dtype=np.float32), "rms_db", sounding=False)
    cx.close()


@pytest.mark.parametrize("frames", [1, 63, 64, 100, 256, 1000, 1024])
def test_model_sum_of_squares_is_within_the_summation_bound(frames):
    """every term is >= 0, so the textbook bound holds: |fl(sum) - sum| <= gamma_n * sum with n = the roundings on the longest path —
    one product, ceil(frames / 256) sequential adds, three in-lane adds, six tree adds (n = ceil(frames / 256) + 10), u = 2^-24"""
    u = 2.0 ** -24
    n = (frames + 255) // 256 + 10
    gamma = n * u / (1.0 - n * u)
    rng = np.random.default_rng(frames)
    for trial in range(20):
        x = (rng.standard_normal(frames) * rng.choice([1e-3, 0.3, 1.0, 40.0])).astype(np.float32)
        _, ss, _, fr = model_block(x)
        exact = float(np.sum(x.astype(np.float64) ** 2))
        assert fr == frames and abs(float(ss) - exact) <= gamma * exact, (frames, trial, float(ss), exact)


def test_model_on_the_specs_corner_values():
    one_up = np.nextafter(np.float32(1.0), np.float32(2.0))
    p, ss, ov, fr = model_block(np.array([-0.0] * 7, dtype=np.float32))
    assert (fr, ov) == (7, 0) and p.view(np.uint32) == 0 and ss.view(np.uint32) == 0
    p, ss, ov, fr = model_block(np.array([np.nan] * 300, dtype=np.float32))
    assert ov == 0 and p.view(np.uint32) == 0 and np.isnan(ss)
    p, ss, ov, fr = model_block(np.array([1.0, -1.0, one_up, -one_up, np.nan, 0.25], dtype=np.float32))
    assert ov == 2 and p == one_up and np.isnan(ss)
    p, ss, ov, fr = model_block(np.array([np.inf, -3.0], dtype=np.float32))
    assert ov == 2 and np.isinf(p) and np.isinf(ss)


# ================================================================================================ GPU tier
def _read_all(g, m, blocks):
    rd, done = g.cx.meter_read(m, 0, blocks)
    assert done == blocks and rd.shape[0] == blocks, (done, rd.shape, blocks)
    return rd


@pytest.mark.gpu
@pytest.mark.parametrize("plan", [1, 2, 3, 0])
@pytest.mark.parametrize("max_batch,mbf", [(64, 256), (3, 128), (1, 64)])
def test_master_meter_is_bit_exact_on_every_plan(plan, max_batch, mbf):
    cfg = PLANS[plan or 1]
    o = oracle(mbf)
    ro = script(o, build(o, master=("v", "c"), **cfg))
    g = GpuEngine(max_block_frames=mbf, max_batch=max_batch, force_generic=plan == 0)
    meters = {("master", 0): (2, None), ("master", 2): (2, 64)}
    b = build(g, master=("v", "c"), meters=meters, **cfg)
    rg = script(g, b)
    assert g.cx.plan_kind() == plan
    assert_bits(ro, rg, "plan %d K<=%d mbf %d" % (plan, max_batch, mbf))
    assert_readings(_read_all(g, b.meter[("master", 2)], 28), model(planar(ro), mbf), "meter in front of graph_out, plan %d" % plan)
    # ... and the one right behind the root sum: the oracle graph wired out there
    o2 = oracle(mbf)
    r2 = script(o2, build(o2, master=("v", "c"), probe=("master", 0), **cfg))
    assert_readings(_read_all(g, b.meter[("master", 0)], 28), model(planar(r2), mbf), "meter behind the root sum, plan %d" % plan)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", [1, 2, 0])
def test_silence_flags_pass_through_and_read_zero(plan):
    mbf = 128
    cfg = PLANS[plan or 1]

    def run(e, meters):
        b = build(e, master=("c",), meters=meters, **cfg)
        for s in b.samplers:
            e.sampler_set_loop_range(s, LOOP_FULL)
            e.sampler_play(s)
        outs = [e.process_blocks_flags(4)]
        for s in b.samplers:
            e.sampler_pause(s, at_block=0)
        outs += [e.process_blocks_flags(6), e.process_blocks_flags(5)]
        return b, np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])

    _, ro, fo = run(OracleEngine(max_block_frames=mbf), {})
    g = GpuEngine(max_block_frames=mbf, max_batch=4, force_generic=plan == 0)
    b, rg, fg = run(g, {("master", 1): (2, None)})
    assert g.cx.plan_kind() == plan
    assert_bits(ro, rg, "pause")
    assert np.array_equal(fo, fg), (fo.T, fg.T)
    rd = _read_all(g, b.meter[("master", 1)], 15)
    assert_readings(rd, model(planar(ro), mbf), "paused bank")
    if plan == 2:
        return  # (filters and delay lines never report silence: their tails ring on)
    assert fg[-5:].all() and not fg[:4].any()  # a dry bank falls silent with its sources
    tail = rd[-5:]
    assert not tail["peak"].view(np.uint32).any() and not tail["sum_squares"].view(np.uint32).any() and not tail["over"].any()
    assert (tail["frames"] == mbf).all()


@pytest.mark.gpu
def test_overs_in_front_of_and_behind_a_hard_clip():
    mbf = 256

    def run(e, meters, probe=None):
        b = build(e, shapes=["", "", "", "v"], master=("v", "C"), master_volume=130.0, meters=meters, probe=probe, radix=4)
        for s in b.samplers:
            e.sampler_set_loop_range(s, LOOP_FULL)
            e.sampler_play(s)
        return b, np.concatenate([np.asarray(e.process_blocks(k)) for k in (4, 5)])

    _, ro = run(OracleEngine(max_block_frames=mbf), {})
    _, rhot = run(OracleEngine(max_block_frames=mbf), {}, probe=("master", 1))
    g = GpuEngine(max_block_frames=mbf)
    b, rg = run(g, {("master", 1): (2, None), ("master", 2): (2, None)})
    assert g.cx.plan_kind() == 1
    assert_bits(ro, rg, "130 % master")
    hot, clipped = _read_all(g, b.meter[("master", 1)], 9), _read_all(g, b.meter[("master", 2)], 9)
    assert_readings(hot, model(planar(rhot), mbf), "in front of the clip")
    assert_readings(clipped, model(planar(ro), mbf), "behind the clip")
    assert hot["over"].sum() > 0 and hot["peak"].max() > 1.0
    assert clipped["over"].sum() == 0 and clipped["peak"].max() <= 1.0


def _exact_input(n, mbf, blocks, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.2, 1.2, size=(n, blocks * mbf)).astype(np.float32)
    one_up = np.nextafter(np.float32(1.0), np.float32(2.0))
    special = np.array([-0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, one_up, -one_up, 0.0], dtype=np.float32)
    for c in range(n):
        x[c, 0:mbf] = -0.0                                   # block 0: all -0.0
        x[c, mbf:2 * mbf] = np.nan                           # block 1: all NaN
        idx = rng.integers(2 * mbf, 4 * mbf, size=40)        # blocks 2, 3: specials scattered in ordinary audio
        x[c, idx] = special[rng.integers(0, special.size, size=40)]
        x[c, 4 * mbf:5 * mbf] = rng.choice([1.0, -1.0, one_up, -one_up], size=mbf).astype(np.float32)  # block 4: the threshold itself
        x[c, 5 * mbf + 3] = np.nan                           # block 5: one NaN among finite samples
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("mbf", [100, 256])
def test_exact_inputs_through_the_device_call(n, mbf):
    import torch

    blocks = 8
    x = _exact_input(n, mbf, blocks, seed=n * 1000 + mbf)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=n, num_graph_outputs=n, max_batch=3)
    m = g.add_node(METER, n, n, [16])
    for c in range(n):
        g.connect(g.graph_in_node, c, m, c)
        g.connect(m, c, g.graph_out_node, c)
    g.update()
    assert g.cx.plan_kind() == 0
    d_in = torch.from_numpy(np.ascontiguousarray(x.T)).to("cuda")
    d_out = torch.full((blocks * mbf * n,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g.cx.process_blocks_device_io(blocks, d_in.data_ptr(), n, d_out.data_ptr(), n)
    g.cx.synchronize()
    y = d_out.cpu().numpy().reshape(-1, n).T
    same = (fwapi.bits(y) == fwapi.bits(x)) | (np.isnan(y) & np.isnan(x))  # (NaN payloads excepted)
    assert same.all(), np.argwhere(~same)[:5]
    rd = _read_all(g, m, blocks)
    assert_readings(rd, model(x, mbf), "exact inputs n %d mbf %d" % (n, mbf))
    assert not rd["peak"][0].view(np.uint32).any() and not rd["sum_squares"][0].view(np.uint32).any()   # -0.0 reads +0.0
    assert not rd["peak"][1].view(np.uint32).any() and not rd["over"][1].any() and np.isnan(rd["sum_squares"][1]).all()  # all NaN
    assert (rd["over"][4] > 0).all() and (rd["over"][4] < mbf).all()


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [1, 63, 100])
def test_partial_blocks(tail):
    """(a stream-input graph: the reference's sampler panics on a block shorter than max_block_frames — oracle Q5 — so the short blocks
    come from graph_in; the signal behind the stateless hard clip is the oracle's output of the graph without the meter)"""
    mbf = 256
    frames = 2 * mbf + tail
    rng = np.random.default_rng(tail)
    calls = [rng.uniform(-1.5, 1.5, size=f * 2).astype(np.float32) for f in (frames, tail, mbf)]

    def run(e, metered):
        c = e.hard_clip(-3.0)
        e.connect_stereo(e.graph_in_node, c)
        m = None
        if metered:
            m = e.add_node(METER, 2, 2, [64])
            e.connect_stereo(c, m)
        e.connect_stereo(m if metered else c, e.graph_out_node)
        e.update()
        return m, [np.asarray(e.process_interleaved(x.size // 2, inp=x, n_in_ch=2)) for x in calls]

    _, ro = run(OracleEngine(max_block_frames=mbf, num_graph_inputs=2), False)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=2)
    m, rg = run(g, True)
    assert_bits(np.concatenate(ro), np.concatenate(rg), "tail %d" % tail)
    rd = _read_all(g, m, 5)
    assert list(rd["frames"][:, 0]) == [mbf, mbf, tail, tail, mbf]
    assert_readings(rd, np.concatenate([model(planar(x), mbf) for x in ro]), "tail %d" % tail)
    assert rd["over"].sum() == 0 and rd["peak"].max() <= 1.0 and rd["peak"].min() > 0.0


MID = {("leaf", 0): (2, None), ("leaf", 1): (0, 32), ("src", 1): (2, 64), ("voice", 5): (0, None)}


@pytest.mark.gpu
@pytest.mark.parametrize("shapes", [DRY, CHAIN], ids=["dry", "chain"])
@pytest.mark.parametrize("max_batch", [64, 3])
def test_meters_on_a_leaf_bus_in_a_voice_chain_and_taps(shapes, max_batch):
    mbf = 128
    o = oracle(mbf)
    ro = script(o, build(o, shapes=shapes, master=("v",)))
    g = GpuEngine(max_block_frames=mbf, max_batch=max_batch)
    b = build(g, shapes=shapes, master=("v",), meters=MID)
    rg = script(g, b)
    assert_bits(ro, rg, "mid-graph meters")
    for key in MID:
        op = oracle(mbf)
        sig = script(op, build(op, shapes=shapes, master=("v",), probe=key))
        assert_readings(_read_all(g, b.meter[key], 28), model(planar(sig), mbf), "meter at %r (plan %d)" % (key, g.cx.plan_kind()))


@pytest.mark.gpu
def test_ring_of_8_keeps_the_last_8_blocks():
    mbf = 128
    calls = (3, 5, 20)

    def start(e, meters):
        b = build(e, shapes=DRY[:6], master=("v",), meters=meters)
        for s in b.samplers:
            e.sampler_set_loop_range(s, LOOP_FULL)
            e.sampler_play(s)
        return b

    o = OracleEngine(max_block_frames=mbf)
    start(o, {})
    ref = model(planar(np.concatenate([o.process_blocks(k) for k in calls + (20,)])), mbf)
    g = GpuEngine(max_block_frames=mbf, max_batch=64)
    b = start(g, {("master", 1): (2, 8), ("leaf", 0): (0, 8)})
    m = b.meter[("master", 1)]
    done = 0
    for k in calls:
        g.process_blocks(k)
        done += k
        lo = max(0, done - 8)
        rd, d = g.cx.meter_read(m, lo, 64)
        assert d == done and rd.shape[0] == done - lo
        assert_readings(rd, ref[lo:done], "after %d blocks" % done)
        if lo:
            with pytest.raises(g.fa.FwgpuError) as ei:
                g.cx.meter_read(m, lo - 1, 1)
            assert ei.value.code == INVALID and ei.value.blocks_done == done
    g.process_blocks_flags(20)  # ONE device call, one launch of 20 blocks over a ring of 8
    done += 20
    for first, n in ((done - 8, 8), (done - 8, 64), (done - 3, 2), (done - 1, 1)):
        rd, d = g.cx.meter_read(m, first, n)
        assert d == done and rd.shape[0] == min(n, done - first)
        assert_readings(rd, ref[first:first + rd.shape[0]], "blocks %d.." % first)
    for old in (done - 9, done - 20, 0):
        with pytest.raises(g.fa.FwgpuError):
            g.cx.meter_read(m, old, 1)
    assert g.cx.meter_read(b.meter[("leaf", 0)], done - 8, 8)[0].shape == (8, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", [1, 2])
def test_plan_switches_keep_the_block_index_and_the_ring(plan):
    mbf = 128
    cfg = PLANS[plan]

    def run(e, gpu):
        b = build(e, master=("v",), meters={("master", 1): (2, 256)} if gpu else {}, **cfg)
        for s in b.samplers:
            e.sampler_set_loop_range(s, LOOP_FULL)
            e.sampler_play(s)
        kinds, outs, late = [], [e.process_blocks(5)], None
        d = e.add_node(fwapi.DUMMY, 1, 1)   # a dangling node: the level executor
        e.update()
        kinds.append(e.cx.plan_kind() if gpu else None)
        outs.append(e.process_blocks(4))
        if gpu:  # a meter added mid-stream, as a tap on the master volume
            late = e.add_node(METER, 2, 0, [256])
            e.connect_stereo(b.master[0], late)
            e.update()
        outs.append(e.process_blocks(3))
        e.remove_node(d)
        e.update()
        kinds.append(e.cx.plan_kind() if gpu else None)
        outs.append(e.process_blocks(6))
        return b, np.concatenate([np.asarray(x) for x in outs]), kinds, late

    _, ro, _, _ = run(OracleEngine(max_block_frames=mbf), False)
    g = GpuEngine(max_block_frames=mbf, max_batch=4)
    b, rg, kinds, late = run(g, True)
    assert kinds[0] in (0, 3) and g.cx.plan_kind() in (0, 3)   # (the tap keeps the last plan off the fused grammar as a whole)
    assert_bits(ro, rg, "plan switches")
    ref = model(planar(ro), mbf)
    assert_readings(_read_all(g, b.meter[("master", 1)], 18), ref, "across the switches")
    rd, done = g.cx.meter_read(late, 9, 64)
    assert done == 18
    assert_readings(rd, ref[9:], "the late tap")
    with pytest.raises(g.fa.FwgpuError) as ei:
        g.cx.meter_read(late, 8, 1)
    assert ei.value.code == INVALID
    # ... and back on the fused plan once the tap is gone: indices continue, everything metered before is still there
    g.remove_node(late)
    g.update()
    assert g.cx.plan_kind() == plan
    g.process_blocks(2)
    rd, done = g.cx.meter_read(b.meter[("master", 1)], 0, 64)
    assert done == 20 and rd.shape[0] == 20
    assert_readings(rd[:18], ref, "after the way back")


@pytest.mark.gpu
def test_b1_node_process_passes_audio_and_mask_through():
    mbf = 256
    g = GpuEngine(max_block_frames=mbf)
    m2, m64, tap = g.add_node(METER, 2, 2, [4]), g.add_node(METER, 64, 64, [4]), g.add_node(METER, 2, 0, [4])
    g.connect_stereo(m2, g.graph_out_node)
    g.update()
    rng = np.random.default_rng(5)
    x = rng.uniform(-2, 2, size=(2, mbf)).astype(np.float32)
    y, om = g.node_process(m2, mbf, list(x), 2)
    assert_bits(y, x, "2 -> 2")
    assert om == 0
    y, om = g.node_process(m2, 100, list(x[:, :100]), 2, in_mask=0b10)   # a silent channel: zero-filled and flagged
    assert om == 0b10 and not fwapi.bits(y[1]).any()
    assert_bits(y[0], x[0, :100], "the live channel")
    x64 = rng.uniform(-1, 1, size=(64, mbf)).astype(np.float32)
    mask = (1 << 63) | (1 << 17) | 1
    y, om = g.node_process(m64, mbf, list(x64), 64, in_mask=mask)
    assert om == mask
    for c in range(64):
        if (mask >> c) & 1:
            assert not fwapi.bits(y[c]).any(), c
        else:
            assert_bits(y[c], x64[c], "channel %d" % c)
    y, om = g.node_process(tap, mbf, list(x), 0)
    assert y.shape[0] == 0 and om == 0
    assert g.cx.meter_read(m2, 0, 4)[1] == 0  # (B1 calls are not recorded: no block was counted)


def _fuzz(seed):
    rng = np.random.default_rng(77000 + seed)
    mbf = int(rng.choice([64, 128, 256]))
    max_batch = int(rng.choice([1, 3, 8, 64]))
    toks = ["", "v", "vp", "pv", "vc", "p", "vw"] + (["vB", "BD", "vBD", "DBv", "cB"] if rng.random() < 0.5 else [])
    shapes = [str(rng.choice(toks)) for _ in range(int(rng.integers(3, 11)))]
    radix = int(rng.choice([2, 4, 8]))
    master = tuple(rng.choice(["v", "c", "p"], size=int(rng.integers(0, 3))))
    n_leaves = (len(shapes) + radix - 1) // radix
    places = [("master", k) for k in range(len(master) + 1)] + [("leaf", j) for j in range(n_leaves)]
    places += [("voice", i) for i in range(len(shapes))] + [("src", i) for i in range(len(shapes))]
    meters = {}
    for i in rng.choice(len(places), size=int(rng.integers(1, 5)), replace=False):
        key = places[int(i)]
        meters[key] = (int(rng.choice([2, 2, 0])), int(rng.choice([1, 3, 8, 40, 1024])))
    calls = [int(rng.choice([1, 2, 3, 5, 9, 20])) for _ in range(7)]
    kw = dict(shapes=shapes, master=master, radix=radix, seed=seed, send=bool(rng.random() < 0.25), master_volume=float(rng.choice([90.0, 140.0])))
    return mbf, max_batch, meters, calls, kw


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_meters_anywhere(seed):
    mbf, max_batch, meters, calls, kw = _fuzz(seed)
    o = oracle(mbf)
    ro = script(o, build(o, **kw), calls)
    g = GpuEngine(max_block_frames=mbf, max_batch=max_batch)
    b = build(g, meters=meters, **kw)
    rg = script(g, b, calls)
    what = "seed %d (plan %d, mbf %d, K<=%d, meters %r)" % (seed, g.cx.plan_kind(), mbf, max_batch, meters)
    assert_bits(ro, rg, what)
    total = sum(calls)
    for key, (n_out, ring) in meters.items():
        op = oracle(mbf)
        ref = model(planar(script(op, build(op, probe=key, **kw), calls)), mbf)
        # what a reader that polls after every call would still find: the last min(ring, total) blocks
        lo = max(0, total - ring)
        rd, done = g.cx.meter_read(b.meter[key], lo, total)
        assert done == total and rd.shape[0] == total - lo, what
        assert_readings(rd, ref[lo:], "%s at %r" % (what, key))
        if lo:
            with pytest.raises(g.fa.FwgpuError):
                g.cx.meter_read(b.meter[key], lo - 1, 1)


def test_fuzz_meters_anywhere_on_the_host_harness():
    """the same graphs and calls through the host half on the fake runtime: every table the kernels would read is validated"""
    for seed in range(FUZZ_SEEDS):
        mbf, max_batch, meters, calls, kw = _fuzz(seed)
        e = HostOnlyEngine(max_block_frames=mbf, max_batch=max_batch)
        b = build(e, meters=meters, **kw)
        script(e, b, calls)
        assert e.violation() == "", (seed, e.violation())
        for key in meters:
            assert e.cx.meter_read(b.meter[key], sum(calls), 0)[1] == sum(calls)
