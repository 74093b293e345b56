"""The spectrum meter (SPEC; include/fwgpu.h): a FWGPU_METER created with two or more parameters — ring_blocks,
fft_size, bands — also records, per block and input channel, the band powers of a Hann-windowed radix-2 FFT over the channel's last
fft_size frames.  Created with none or one parameter it is the level meter it was.

Reference for the records: tests/spectrum_model.py, a numpy restatement of the SPEC's text, applied to a signal obtained without the
node (the stream input itself; the oracle's output of the same graph built without the meter).  The GPU tier compares bit for bit.

CPU tier: the model against numpy's own FFT in f64, the sine and zero readings, the band edges, creation parameters / slice layout /
tables / read contract on the host-only harness, the planner, the typed mirror, the header and the generated ffi.rs."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import busnodes
import fwapi
import spectrum_model as sm
from busnodes import PLANS, assert_bits, planar
from fwapi import GpuEngine, HostOnlyEngine, OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METER = 16
INVALID = -20
F32 = np.float32
U = C.c_uint


def peek():
    p, UP = C.c_void_p, C.POINTER(U)
    return fwapi.peek_lib("spectrum_peek", {"spk_state": (C.c_int, [p, C.c_longlong, UP]), "spk_layout": (None, [UP, C.c_int, C.c_int, UP]),
                                            "spk_ext": (C.c_int, [p, U, U, UP])})


# ================================================================================================ CPU tier: the model
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_model_against_an_independent_transform(N):
    """P against numpy's rfft of the f64-windowed signal: the error of 12 stages of f32 butterflies, far below a display's needs.
    (Measured 1.9e-7 .. 2.5e-7 of the peak for these three N; the bound is the issue's.)"""
    x = np.random.default_rng(N).uniform(-1, 1, N).astype(F32)
    w = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / N) for i in range(N)])
    R = np.fft.rfft(x.astype(np.float64) * w)
    ref = (R.real ** 2 + R.imag ** 2) * (16.0 / (N * N))
    P = sm.powers(x, N)
    err = np.abs(P.astype(np.float64) - ref).max() / ref.max()
    print("N %d: max |P - ref| / max ref = %.3g" % (N, err))
    assert err < 1e-6


@pytest.mark.parametrize("N", sm.FFT_SIZES)
def test_model_sine_on_a_bin_centre_and_zeros(N):
    for k in (3, N // 8, N // 2 - 2):
        P = sm.powers(np.sin(2.0 * np.pi * k * np.arange(N) / N).astype(F32), N)
        print("N %d bin %d: %r" % (N, k, P[k - 1:k + 2]))
        assert abs(float(P[k]) - 1.0) <= 2e-7 and abs(float(P[k - 1]) - 0.25) <= 2e-7 and abs(float(P[k + 1]) - 0.25) <= 2e-7
        assert np.delete(P, [k - 1, k, k + 1]).max() < 1e-12
    assert not fwapi.bits(sm.powers(np.zeros(N, dtype=F32), N)).any()
    assert not fwapi.bits(sm.model(np.zeros((2, 300), dtype=F32), [100, 200], N, 7)).any()


@pytest.mark.parametrize("N", sm.FFT_SIZES)
def test_edges_are_strictly_increasing_for_every_band_count(N):
    from firewheel_amd.graph import MeterNode

    for B in range(1, N // 2 + 1):
        e = sm.edges(N, B)
        assert e.size == B + 1 and e[0] == 1 and e[-1] == N // 2 + 1 and (np.diff(e) > 0).all(), (N, B)
    assert np.array_equal(sm.edges(N, 0), np.arange(N // 2 + 2))
    assert np.array_equal(sm.edges(N, N // 2), np.arange(1, N // 2 + 2))  # one bin per band, DC left out
    for B in (0, 1, 32, N // 2):
        assert np.array_equal(MeterNode.band_edges(N, B), sm.edges(N, B))


def test_model_windows_blocks_and_bands():
    """the hop is the block, a flagged block counts as zeros, band sums are the powers' chains"""
    N, mbf = 256, 100
    x = np.random.default_rng(1).uniform(-1, 1, (1, 3 * mbf + 37)).astype(F32)
    blocks = [mbf, mbf, mbf, 37]
    r = sm.model(x, blocks, N, 0)
    assert r.shape == (4, 1, N // 2 + 1)
    padded = np.concatenate([np.zeros(N, dtype=F32), x[0]])
    for g, end in enumerate(np.cumsum(blocks)):
        assert_bits(r[g, 0], sm.powers(padded[end:end + N], N), "block %d" % g)
    silent = np.zeros((4, 1), dtype=bool)
    silent[1, 0] = True
    y = x.copy()
    y[0, mbf:2 * mbf] = 0
    assert_bits(sm.model(x, blocks, N, 0, silent=silent), sm.model(y, blocks, N, 0), "a flagged block")
    e = sm.edges(N, 5)
    banded = sm.model(x, blocks, N, 5)
    for b in range(5):
        acc = r[2, 0, e[b]]
        for k in range(e[b] + 1, e[b + 1]):
            acc = F32(acc + r[2, 0, k])
        assert fwapi.bits(banded[2, 0, b]) == fwapi.bits(acc)


# ================================================================================================ CPU tier: the host harness
def _host(mbf=64, **kw):
    e = HostOnlyEngine(max_block_frames=mbf, **kw)
    v = e.volume(50.0)
    e.connect_stereo(v, e.graph_out_node)
    return e, v


nan, inf = float("nan"), float("inf")
BAD = [[nan, 1024, 32], [8, nan, 32], [8, 1024, nan], [inf, 1024, 32], [8, inf, 32], [8, 1024, inf], [8, -inf, 32], [8, 1024, -inf],
       [8.5, 1024, 32], [8, 1024.5, 32], [8, 1024, 31.5], [0, 1024, 32], [65537, 1024, 32], [8, 128, 32], [8, 8192, 32], [8, 1000, 32], [8, 768, 32],
       [8, 0, 0], [8, 1024, 513], [8, 256, 129], [8, 1024, -1], [8, 300], [nan, 1024]]


@pytest.mark.parametrize("params", BAD, ids=[repr(p) for p in BAD])
def test_parameters_refused_at_update(params):
    e, v = _host()
    m = e.add_node(METER, 2, 2, params)
    for _ in range(2):  # (still there, still refused)
        with pytest.raises(fwapi.CompileGraphError) as ei:   # (node activation failed, as for a bad ring_blocks)
            e.update()
        assert "MeterNode" in str(ei.value)
    e.remove_node(m)
    good = e.add_node(METER, 2, 2, [8, 1024, 32])
    e.connect_stereo(v, good)
    e.update()  # the graph is usable
    assert e.cx.spectrum_layout(good)[0] == 1024


@pytest.mark.parametrize("n_in,n_out,params", [(9, 9, [8, 256, 8]), (9, 0, [8, 256, 8]), (64, 64, [8, 256]), (8, 8, [65536, 256, 33]),
                                               (2, 2, [65536, 4096, 0]), (1, 1, [8193, 4096, 2048])])
def test_shapes_and_ring_sizes_refused_at_update(n_in, n_out, params):
    """more than 8 channels; ring_blocks * n_in * B > 2^24 floats"""
    e, v = _host()
    m = e.add_node(METER, n_in, n_out, params)
    with pytest.raises(fwapi.CompileGraphError) as ei:
        e.update()
    assert "MeterNode" in str(ei.value)
    e.remove_node(m)
    e.update()
    assert e.add_node(METER, n_in, n_out, params[:1]) >= 0  # the plain meter of that shape and ring is fine
    e.update()


ACCEPTED = [[8, 256], [1, 256, 0], [8, 512, 256], [1024, 1024, 32], [4, 2048, 1], [2, 4096, 2048], [65536, 256, 32], [8192, 4096, 2048], [3, 4096, 0]]
# (every shape the ring cap lets through: [8192, 4096, 2048] is at the cap with one channel)
ACCEPTED_CASES = [(p_, n, tap) for p_ in ACCEPTED for n, tap in ((1, False), (2, False), (8, False), (2, True))
                  if p_[0] * n * sm.record_len(p_[1], p_[2] if len(p_) > 2 else 32) <= 1 << 24]


@pytest.mark.parametrize("params,n,tap", ACCEPTED_CASES, ids=["%r-%d%s" % (p_, n, "-tap" if tap else "") for p_, n, tap in ACCEPTED_CASES])
def test_parameters_and_shapes_accepted_layout_and_set_param_refused(params, n, tap):
    R, N = params[0], params[1]
    bands = params[2] if len(params) > 2 else 32
    B = sm.record_len(N, bands)
    e, _ = _host()
    m = e.add_node(METER, n, 0 if tap else n, params)
    e.update()
    assert e.cx.plan_node_level(m) >= 0
    for slot in range(3):
        with pytest.raises(e.fa.FwgpuError) as ei:
            e.set_param(m, slot, 16.0)
        assert ei.value.code == INVALID
    fft, b, edges = e.cx.spectrum_layout(m)
    assert (fft, b) == (N, bands) and np.array_equal(edges, sm.edges(N, bands))
    P = peek()
    st, lay = (U * 32)(), (U * 15)()
    assert P.spk_state(e.cx.c, m, st) == 1
    P.spk_layout(st, n, 0 if tap else n, lay)
    on, ok, win, tw, ed, head, hist, ring, ext_len, r_, n_, bands_, b_, off, length = list(lay)
    assert (on, ok, r_, n_, bands_, b_) == (1, 1, R, N, bands, B)
    assert win >= R * n * 4 and win % 64 == 0 and tw == win + N and ed == win + 2 * N and head == 2 * N + (B + 1 + 63) // 64 * 64
    assert hist == win + head and ring == hist + n * N and ext_len == ring + R * n * B and length == ext_len and off % 64 == 0


def test_a_plain_meter_is_the_node_it_was():
    """state and slice of a meter created with no or one parameter: loop_end = R and nothing else, 4 floats per (slot, channel) — and
    the same for the twin that stands beside a spectrum meter"""
    P = peek()
    for with_spectrum in (False, True):
        e, v = _host()
        if with_spectrum:
            e.connect_stereo(v, e.add_node(METER, 2, 2, [8, 256, 16]))
        a, b = e.add_node(METER, 3, 3, []), e.add_node(METER, 2, 0, [40])
        e.update()
        for node, n, R in ((a, 3, 1024), (b, 2, 40)):
            st, lay = (U * 32)(), (U * 15)()
            assert P.spk_state(e.cx.c, node, st) == 1
            P.spk_layout(st, n, n, lay)
            assert lay[0] == 0 and lay[9] == R and lay[10] == 0 and lay[11] == 0 and lay[12] == 0 and lay[14] == R * n * 4
            s = np.frombuffer(st, dtype=np.uint32).copy()
            ref = np.zeros(32, dtype=np.uint32)   # NodeState of make_state's zeros: sample = -1, the sample rate, two smoothers at rest at 0
            fresh = (U * 32)()
            e2, _ = _host()
            assert P.spk_state(e2.cx.c, e2.add_node(METER, n, n, [R]), fresh) == 1   # (not activated: ext_off = ext_len = 0)
            ref[:] = np.frombuffer(fresh, dtype=np.uint32)
            s[29] = s[30] = 0   # ext_off, ext_len
            assert np.array_equal(s, ref)
            with pytest.raises(e.fa.FwgpuError) as ei:
                e.cx.spectrum_read(node, 0, 1)
            assert ei.value.code == INVALID
            with pytest.raises(e.fa.FwgpuError):
                e.cx.spectrum_layout(node)


@pytest.mark.parametrize("N,bands", [(256, 0), (1024, 32), (4096, 2048), (2048, 5)])
def test_tables_in_the_slice_are_the_models(N, bands):
    P = peek()
    e, v = _host()
    m = e.add_node(METER, 2, 2, [3, N, bands])
    e.connect_stereo(v, m)
    e.update()
    e.process_blocks(1)   # adoption: the launch stub writes the slices' heads and zeros
    st, lay = (U * 32)(), (U * 15)()
    assert P.spk_state(e.cx.c, m, st) == 1
    P.spk_layout(st, 2, 2, lay)
    words = (U * lay[14])()
    assert P.spk_ext(e.cx.c, lay[13], lay[14], words) == 1
    s = np.frombuffer(words, dtype=np.uint32)
    B = sm.record_len(N, bands)
    wr, wi = sm.twiddles(N)
    assert np.array_equal(s[lay[2]:lay[2] + N], fwapi.bits(sm.window(N)))
    assert np.array_equal(s[lay[3]:lay[3] + N // 2], fwapi.bits(wr)) and np.array_equal(s[lay[3] + N // 2:lay[3] + N], fwapi.bits(wi))
    assert np.array_equal(s[lay[4]:lay[4] + B + 1], sm.edges(N, bands).astype(np.uint32))
    assert not s[:lay[2]].any() and not s[lay[4] + B + 1:].any()   # level ring, history and spectrum ring: zeros
    assert e.violation() == ""


def test_spectrum_read_contract_on_the_harness():
    e = HostOnlyEngine(max_block_frames=64, max_batch=4)
    v = e.volume(50.0)
    m = e.add_node(METER, 2, 2, [8, 256, 16])
    plain = e.add_node(METER, 2, 0, [8])
    e.connect_stereo(v, m)
    e.connect_stereo(v, plain)
    e.connect_stereo(m, e.graph_out_node)
    e.update()
    assert e.cx.spectrum_read(m, 0, 4)[0].shape == (0, 2, 16) and e.cx.spectrum_read(m, 0, 0)[1] == 0
    e.process_blocks(3)
    e.process_blocks(5)
    e.process_interleaved(100)   # 64 + 36 frames: two blocks
    rd, done = e.cx.spectrum_read(m, 9, 5)
    assert done == 10 and rd.shape == (1, 2, 16) and not fwapi.bits(rd).any()   # (the harness' kernels are no-ops: the ring's zeros)
    assert e.cx.spectrum_read(m, 2, 8)[0].shape == (8, 2, 16) and e.cx.spectrum_read(m, 10, 3)[0].shape == (0, 2, 16)
    assert e.cx.meter_read(m, 2, 8)[0].shape == (8, 2)   # the level ring of the same node

    def refused(node, first, n, out_null=False):
        done = C.c_uint64(777)
        buf = (C.c_float * 4096)()
        rc = e.cx.L.fwgpu_spectrum_read(e.cx.c, node, first, n, None if out_null else buf, C.byref(done))
        assert rc == INVALID and done.value == 10, (rc, done.value)

    refused(m, 1, 8)                  # older than the ring retains
    refused(plain, 9, 1)              # a plain meter
    refused(v, 9, 1)
    refused(12345 << 32, 9, 1)
    refused(m, 9, 1, out_null=True)
    late = e.add_node(METER, 2, 0, [64, 512])
    e.connect_stereo(v, late)
    e.update()
    refused(late, 9, 1)               # before its first plan
    e.process_blocks(2)
    assert e.cx.spectrum_read(late, 10, 4)[0].shape == (2, 2, 32)   # (two parameters: 32 bands)
    e.remove_node(late)
    e.update()
    with pytest.raises(e.fa.FwgpuError):
        e.cx.spectrum_read(late, 10, 1)
    assert e.violation() == ""
    assert e.cx.L.fwgpu_spectrum_read(None, m, 0, 0, None, None) == INVALID
    assert e.cx.L.fwgpu_spectrum_layout(None, m, None, None, None, 0) == INVALID
    few = (C.c_uint32 * 4)(9, 9, 9, 9)
    assert e.cx.L.fwgpu_spectrum_layout(e.cx.c, m, None, None, few, 3) == 16 and list(few) == list(sm.edges(256, 16)[:3]) + [9]


@pytest.mark.parametrize("seed", range(4))
def test_random_ragged_calls_leave_no_violation(seed):
    rng = np.random.default_rng(900 + seed)
    mbf = int(rng.choice([64, 96, 256]))
    n = int(rng.choice([1, 2, 8]))
    e = HostOnlyEngine(max_block_frames=mbf, num_graph_inputs=n, num_graph_outputs=n, max_batch=int(rng.choice([1, 3, 64])))
    N = int(rng.choice(sm.FFT_SIZES))
    m = e.add_node(METER, n, n, [int(rng.choice([1, 4, 100])), N, int(rng.choice([0, 1, 32, N // 2]))])
    tap = e.add_node(METER, n, 0, [5, 256, 3])
    for c in range(n):
        e.connect(e.graph_in_node, c, m, c)
        e.connect(e.graph_in_node, c, tap, c)
        e.connect(m, c, e.graph_out_node, c)
    e.update()
    for f in busnodes.ragged_calls(mbf, at_least=2000) + [int(x) for x in rng.integers(1, 4 * mbf, size=6)]:
        e.process_interleaved(f, n_out_ch=n, inp=np.zeros(f * n, dtype=F32), n_in_ch=n)
    assert e.violation() == "", e.violation()
    blocks = e.cx.spectrum_read(m, 0, 0)[1]
    assert blocks > 0 and e.cx.meter_read(tap, 0, 0)[1] == blocks


# ================================================================================================ CPU tier: the planner
def spectrum_bank(e, spec, **kw):
    """busnodes.bank with a master chain of a volume and a 2 -> 2 meter of parameters `spec` (its "M" entry takes ring_blocks alone)"""
    add = e.add_node

    def add_node(kind, n_in, n_out, params=()):
        return add(kind, n_in, n_out, list(spec) if kind == METER else params)

    e.add_node = add_node
    try:
        return busnodes.bank(e, master=[("v", 90.0), ("M", spec[0])], salt=83, **kw)
    finally:
        del e.add_node


@pytest.mark.parametrize("plan", [1, 2, 3])
def test_a_master_spectrum_meter_changes_no_planner_decision(plan):
    def run(spec):
        e = HostOnlyEngine(max_block_frames=128, max_batch=4)
        b = spectrum_bank(e, spec, **PLANS[plan])
        la, kinds = busnodes.harness_run(e)
        return e, b, la, kinds

    e0, b0, la0, kinds0 = run([16])
    e, b, la, kinds = run([16, 1024, 32])
    assert e0.cx.plan_kind() == e.cx.plan_kind() == plan
    assert e.cx.plan_fused_voices() == e0.cx.plan_fused_voices() and e.cx.lazy_stats() == e0.cx.lazy_stats()
    assert la == la0 and kinds == kinds0
    assert e.cx.spectrum_read(b.node["M"], 0, 0)[1] == sum(busnodes.HARNESS_CALLS)
    with pytest.raises(e0.fa.FwgpuError):
        e0.cx.spectrum_layout(b0.node["M"])


# ================================================================================================ CPU tier: mirror, header, ffi.rs
def test_typed_mirror_header_types_and_generated_ffi():
    import firewheel_amd as fa
    from firewheel_amd import graph as G

    assert fa.MeterNode().params() == [1024.0] and fa.MeterNode(7).params() == [7.0]
    assert fa.MeterNode(16, 1024).params() == [16.0, 1024.0, 32.0] and fa.MeterNode(16, 4096, 0).params() == [16.0, 4096.0, 0.0]
    hz = G.MeterNode.band_hz(1024, 32, 48000)
    e = sm.edges(1024, 32)
    assert hz.shape == (32, 2) and hz[0, 0] == 46.875 and hz[-1, 1] == 24000.0 and np.array_equal(hz[:, 0], e[:-1] * 46.875)
    db = G.MeterNode.power_db(np.array([1.0, 0.1, 0.0], dtype=F32))
    assert db.dtype == F32 and db[0] == 0.0 and abs(db[1] + 10.0) < 1e-5 and db[2] == -np.inf
    cx = fwapi.hostonly_ctx(sample_rate=48000, max_block_frames=64, num_graph_inputs=0, num_graph_outputs=2)
    v = cx.add_node(2, 2, G.VolumeNode(50.0))
    node = fa.MeterNode(16, 512, 0)
    m = cx.add_node(2, 2, node)
    for c in range(2):
        cx.connect(v, c, m, c)
        cx.connect(m, c, cx.graph_out_node(), c)
    cx.update()
    fft, bands, edges = cx.spectrum_layout(m)
    assert (fft, bands) == (512, 0) and np.array_equal(edges, np.arange(258))
    rd, done = node.spectrum(0, 4)
    assert rd.shape == (0, 2, 257) and done == 0
    bad = cx.add_node(2, 2, fa.MeterNode(16, 1000))
    with pytest.raises(fa.CompileGraphError):
        cx.update()
    cx.remove_node(bad)
    cx.update()
    cx.close()
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    assert re.search(r"int64_t fwgpu_spectrum_read\(fwgpu_ctx\* ctx, int64_t node, uint64_t first_block, uint32_t num_blocks, float\* out, uint64_t\* blocks_done\);", hdr)
    assert re.search(r"int fwgpu_spectrum_layout\(fwgpu_ctx\* ctx, int64_t node, uint32_t\* fft_size, uint32_t\* bands, uint32_t\* edges, uint32_t edges_cap\);", hdr)
    for name, val in (("FFT_MIN", 256), ("FFT_MAX", 4096), ("CH_MAX", 8), ("BANDS_DEFAULT", 32)):
        assert re.search(r"#define FWGPU_SPECTRUM_%s %d\b" % (name, val), hdr)
    types = open(os.path.join(ROOT, "firewheel_amd", "csrc", "fwgpu_types.h")).read()
    assert re.search(r"K_KIND_MAX = K_COMPRESSOR\b", types)   # no new kind, no new launch bit
    assert "enum : int { LB_SET0 = 1, LB_SET1 = 2, LB_SET2 = 4, LB_WALKERS = 8, LB_LIMITER = 16, LB_DUCKER = 32, LB_DELAY_COMP = 64, LB_COMPRESSOR = 128 };" in types
    assert re.search(r"#define SPEC_FFT_MIN 256u", types) and re.search(r"#define SPEC_FFT_MAX 4096u", types) and re.search(r"#define SPEC_CH_MAX 8\b", types)
    assert "spec_state_ok" in types and "spec_ext_len" in types
    ffi = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "ffi.rs")).read()
    assert "pub fn fwgpu_spectrum_read(" in ffi and "pub fn fwgpu_spectrum_layout(" in ffi
    assert "pub const FWGPU_SPECTRUM_FFT_MAX: u32 = 4096;" in ffi and "pub const FWGPU_SPECTRUM_CH_MAX: u32 = 8;" in ffi
    nodes = open(os.path.join(ROOT, "rust", "firewheel-gpu", "src", "nodes.rs")).read()
    assert "pub fn with_spectrum(" in nodes and "ffi::fwgpu_spectrum_read" in nodes


# ================================================================================================ GPU tier
def stream(n, frames, seed):
    """finite, seeded: a loud stretch, a quiet one (1e-4), and a sine on top of noise behind them"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(n, frames))
    env = np.full(frames, 0.3)
    env[:frames // 4] = 0.9
    env[frames // 4:frames // 2] = 1e-4
    x = x * env + 0.5 * np.sin(2.0 * np.pi * 0.03 * np.arange(frames))[None, :] * (np.arange(frames) > frames // 2)
    return x.astype(F32)


# ---- G1: graph_in(n) -> plain meter -> spectrum meter -> graph_out(n) on the level executor
G1 = [  # (max_block_frames, max_batch, n, N, B, tap)
    (64, 1, 1, 256, 0, False),       # hop shorter than the window, one block per launch
    (64, 3, 2, 256, 16, False),      # bands
    (64, 3, 2, 256, 16, True),       # ... and as a tap
    (96, 64, 2, 512, 32, False),     # a block length that is no multiple of 64; windows across several blocks of a launch and into the history
    (256, 3, 8, 256, 8, False),      # block equal to the window; one input left unconnected: its records are zero bits
    (512, 2, 2, 256, 0, False),      # block longer than the window
    (64, 64, 1, 4096, 64, False),    # the window at its cap, 64 blocks long
    (256, 4, 2, 4096, 2048, False),  # one bin per band at the cap
]
RING = 4   # (the five-block launches of the max_batch 64 cases are longer than the ring: they keep their last four blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,max_batch,n,N,B,tap", G1)
def test_g1_stream_graphs(mbf, max_batch, n, N, B, tap):
    calls = busnodes.ragged_calls(mbf)
    x = stream(n, sum(calls), 100 * n + mbf + N)
    dead = 5 if n == 8 else -1
    blocks = sm.blocks_of(calls, mbf)
    silent = np.zeros((len(blocks), n), dtype=bool)
    if dead >= 0:
        silent[:, dead] = True
    want = sm.model(x, blocks, N, B, silent=silent)
    assert want.max() > 1e-3
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=n, num_graph_outputs=n, max_batch=max_batch)
    p = g.add_node(METER, n, n, [RING])
    m = g.add_node(METER, n, 0 if tap else n, [RING, N, B])
    for c in range(n):
        if c != dead:
            g.connect(g.graph_in_node, c, p, c)
            g.connect(p, c, m, c)
        g.connect(p if tap else m, c, g.graph_out_node, c)
    g.update()
    assert g.cx.plan_kind() == 0
    assert g.cx.spectrum_layout(m)[0] == N
    a = done = 0
    for i, f in enumerate(calls):
        what = "n %d mbf %d N %d B %d call %d (%d frames at %d)" % (n, mbf, N, B, i, f, a)
        inp = np.ascontiguousarray(x[:, a:a + f].T).ravel()
        y = planar(g.process_interleaved(f, n_out_ch=n, inp=inp, n_in_ch=n), n)
        ref = x[:, a:a + f].copy()
        if dead >= 0:
            ref[dead] = 0
        assert_bits(y, ref, what + ": the audio")
        nb = (f + mbf - 1) // mbf
        first = done + nb - min(nb, RING)
        rd, d = g.cx.spectrum_read(m, first, nb)
        assert d == done + nb and rd.shape == (done + nb - first, n, sm.record_len(N, B))
        assert_bits(rd, want[first:done + nb], what + ": the spectrum records")
        lv, _ = g.cx.meter_read(m, first, nb)
        lp, _ = g.cx.meter_read(p, first, nb)
        assert lv.tobytes() == lp.tobytes() and lv["frames"][-1, 0] == (f - 1) % mbf + 1, what + ": the level records"
        if dead >= 0:
            assert not fwapi.bits(rd[:, dead]).any()
        a += f
        done += nb


# ---- G2: the master chain of a voice bank
@pytest.mark.gpu
@pytest.mark.parametrize("plan", [1, 2, 3])
def test_g2_master_chain_of_a_voice_bank(plan):
    mbf, N, B, ring = 128, 256, 16, 4
    calls = [4, 2, 4, 9, 1, 4]   # blocks; max_batch 4
    o = OracleEngine(max_block_frames=mbf)
    busnodes.bank(o, master=[("v", 90.0), ("M", ring)], leave_out="M", salt=83, **PLANS[plan])
    mix = planar(np.concatenate([np.asarray(o.process_blocks(k)) for k in calls]))
    want = sm.model(mix, [mbf] * sum(calls), N, B)
    t = GpuEngine(max_block_frames=mbf, max_batch=4)
    tm = spectrum_bank(t, [ring], **PLANS[plan]).node["M"]   # the twin: a plain meter in its place
    g = GpuEngine(max_block_frames=mbf, max_batch=4)
    b = spectrum_bank(g, [ring, N, B], **PLANS[plan])
    m = b.node["M"]
    done, outs = 0, []
    for k in calls:
        outs.append(np.asarray(g.process_blocks(k)))
        t.process_blocks(k)
        done += k
        lo = max(0, done - ring)
        rd, d = g.cx.spectrum_read(m, lo, 64)
        assert d == done and rd.shape == (done - lo, 2, B)
        assert_bits(rd, want[lo:done], "plan %d after %d blocks" % (plan, done))
        assert g.cx.meter_read(m, lo, 64)[0].tobytes() == t.cx.meter_read(tm, lo, 64)[0].tobytes()
        if lo:
            with pytest.raises(g.fa.FwgpuError) as ei:
                g.cx.spectrum_read(m, lo - 1, 1)
            assert ei.value.code == INVALID and ei.value.blocks_done == done
    assert g.cx.plan_kind() == t.cx.plan_kind() == plan and g.cx.plan_fused_voices() == t.cx.plan_fused_voices()
    assert g.cx.lazy_stats() == t.cx.lazy_stats(), (g.cx.lazy_stats(), t.cx.lazy_stats())
    assert_bits(planar(np.concatenate(outs)), mix, "the mix")
    assert np.any(mix != 0) and want.max() > 1e-6


# ---- G3: connected into a sounding graph; an unrelated edit carries the history and the ring
@pytest.mark.gpu
def test_g3_connected_into_a_sounding_graph_and_carried_across_an_edit():
    mbf, N, B, ring = 128, 512, 0, 64
    phases = [[3 * mbf, 2 * mbf], [4 * mbf, 2 * mbf + 5, 3 * mbf], [2 * mbf, 37, 4 * mbf]]
    total = sum(sum(p_) for p_ in phases)
    x = stream(2, total, 31)
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=2, num_graph_outputs=4, max_batch=4)
    v = g.volume(100.0)
    for c in range(2):
        g.connect(g.graph_in_node, c, v, c)
        g.connect(v, c, g.graph_out_node, c)
    g.update()
    pos = [0]

    def run(fs):
        outs = []
        for f in fs:
            inp = np.ascontiguousarray(x[:, pos[0]:pos[0] + f].T).ravel()
            outs.append(np.asarray(g.process_interleaved(f, n_out_ch=4, inp=inp, n_in_ch=2)))
            pos[0] += f
        return planar(np.concatenate(outs), 4)

    outs = [run(phases[0])]
    joined = len(sm.blocks_of(phases[0], mbf))   # the block the meter joins at
    for c in range(2):
        g.disconnect(v, c, g.graph_out_node, c)
    m = g.add_node(METER, 2, 2, [ring, N, B])
    g.connect_stereo(v, m)
    g.connect_stereo(m, g.graph_out_node)
    g.update()
    outs.append(run(phases[1]))
    n1 = sum(phases[0])
    blocks = sm.blocks_of(phases[1] + phases[2], mbf)
    want = sm.model(x[:, n1:], blocks, N, B)    # x[n < 0] = +0.0: nothing of what sounded before the activation
    nb1 = len(sm.blocks_of(phases[1], mbf))
    rd, done = g.cx.spectrum_read(m, joined, 64)
    assert done == joined + nb1
    assert_bits(rd, want[:nb1], "from the activation on")
    with pytest.raises(g.fa.FwgpuError) as ei:
        g.cx.spectrum_read(m, joined - 1, 1)
    assert ei.value.code == INVALID
    w = g.volume(50.0)          # an unrelated edit
    for c in range(2):
        g.connect(g.graph_in_node, c, w, c)
        g.connect(w, c, g.graph_out_node, 2 + c)
    g.update()
    outs.append(run(phases[2]))
    rd, done = g.cx.spectrum_read(m, joined, 64)
    assert done == joined + len(blocks)
    assert_bits(rd, want, "across the edit: the ring's earlier records and windows that reach back over it")
    got = np.concatenate(outs, axis=1)
    assert_bits(got[:2], x, "the audio")
    n2 = n1 + sum(phases[1])
    assert_bits(got[2:, n2:], (x[:, n2:] * F32(0.25)).astype(F32), "the other bus")   # (a volume of 50 %)


# ---- G4: fwgpu_node_process
@pytest.mark.gpu
def test_g4_node_process_records_nothing_and_leaves_the_history():
    mbf, N, B = 128, 256, 4
    g = GpuEngine(max_block_frames=mbf, num_graph_inputs=2, max_batch=4)
    m = g.add_node(METER, 2, 2, [16, N, B])
    g.connect_stereo(g.graph_in_node, m)
    g.connect_stereo(m, g.graph_out_node)
    g.update()
    x = stream(2, 7 * mbf + 50, 8)
    other = np.random.default_rng(9).uniform(-2, 2, size=(2, 100)).astype(F32)
    calls = [3 * mbf, mbf + 50, 3 * mbf]
    want = sm.model(x, sm.blocks_of(calls, mbf), N, B)
    a = done = 0
    for i, f in enumerate(calls):
        y = planar(g.process_interleaved(f, inp=np.ascontiguousarray(x[:, a:a + f].T).ravel(), n_in_ch=2))
        assert_bits(y, x[:, a:a + f], "call %d" % i)
        nb = (f + mbf - 1) // mbf
        rd, d = g.cx.spectrum_read(m, done, nb)
        assert d == done + nb
        assert_bits(rd, want[done:done + nb], "call %d: the window continues from the stream, not from node_process" % i)
        a += f
        done += nb
        y, om = g.node_process(m, 100, list(other), 2, in_mask=0b10 if i == 1 else 0)
        assert om == (0b10 if i == 1 else 0)
        assert_bits(y[0], other[0], "node_process passes the audio")
        if i == 1:
            assert not fwapi.bits(y[1]).any()
        assert g.cx.spectrum_read(m, 0, 0)[1] == done   # no block was counted
        assert_bits(g.cx.spectrum_read(m, done - nb, nb)[0], want[done - nb:done], "... and no record was touched")
