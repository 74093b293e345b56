"""GPU tier: the FIR convolution bank (k_fir_append / k_fir_gemm / k_fir_reduce, launched by launch_fir) where it can go wrong:
every split-K segment carrying data, the mirrored history ring wrapping inside a K-batch, many 32-row tiles on one impulse
response, several impulse responses in one launch, cascades, formats and node lifecycle.

Two independent references: the oracle (a linear history, fw_oracle.cpp FirProcessor; the same SPEC summation order, so the
bar is bit-exact) and an f64 convolution, which also catches what both f32 restatements could share.  Window
position m of a block that starts at frame n0 holds x[n0-(T-1)+m]: only runs longer than T put data into the early segments,
and only runs longer than R = T-1 + max_batch*max_block_frames wrap the ring — every test here runs at least that far."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fwapi
import scenarios
from fwapi import (INTERLEAVED_F32, INTERLEAVED_I16, INTERLEAVED_U16, LOOP_FULL, PLANAR_F32, PLANAR_I16, PLANAR_U16, GpuEngine,
                   OracleEngine, bits)
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24
PLAN_KIND = {"hybrid": 3, "generic": 0}


# ------------------------------------------------------------------ references
def conv64(x, h):
    """the first len(x) outputs of the f64 linear convolution x * h (FFT padded to at least len(x) + len(h))"""
    n = len(x)
    L = 1 << int(np.ceil(np.log2(n + len(h))))
    return np.fft.irfft(np.fft.rfft(np.asarray(x, np.float64), L) * np.fft.rfft(np.asarray(h, np.float64), L), L)[:n]


def check_f64(y, ref, bound, i0, what, extra=0.0):
    """|y - ref| <= 64u bound + 1e-12 max(bound) (+ extra) from sample i0 on; exactly +0.0 before it"""
    y = np.asarray(y, f32)
    assert not np.any(bits(y[:i0])), "%s: output before the first nonzero input is not +0.0" % what
    tol = 64 * U * bound + 1e-12 * np.max(bound) + extra
    err = np.abs(y.astype(np.float64) - ref)
    bad = np.flatnonzero(err[i0:] > np.broadcast_to(tol, err.shape)[i0:])
    assert bad.size == 0, "%s: %d/%d samples outside the f64 bound, first at %d: %r vs %r (tol %g)" % (
        what, bad.size, len(y) - i0, i0 + bad[0], y[i0 + bad[0]], ref[i0 + bad[0]], np.broadcast_to(tol, err.shape)[i0 + bad[0]])


def assert_f64(y, x, h, what):
    """y against conv64(x, h), bound conv64(|x|, |h|), from the first nonzero input on"""
    x = np.asarray(x, np.float64)
    nz = np.flatnonzero(x)
    check_f64(y, conv64(x, h), conv64(np.abs(x), np.abs(h)), int(nz[0]) if nz.size else len(x), what)


def flat_ir(seed, taps, channels):
    """noise with a flat envelope (every tap matters at the f64 tolerance), L1-normalised per channel"""
    return scenarios.reverb_ir(seed, taps, channels, decay=1e9)


# ------------------------------------------------------------------ call schedules
def call_schedule(rng, n_frames, mbf, K, odd=True):
    """call lengths (frames) covering at least n_frames: whole blocks drawn over 1..K, and (odd) one call early on whose length
    is no multiple of mbf (the generic executor runs its trailing partial block on its own, shifting the ring phase)"""
    calls, done = [], 0
    while done < n_frames:
        f = (mbf + 37 if mbf > 37 else mbf + 1) if (odd and len(calls) == 2) else int(rng.integers(1, K + 1)) * mbf
        calls.append(f)
        done += f
    return calls


def launches(calls, mbf, Kg):
    """(first frame, blocks, frames per block) of every FIR launch the executor makes for these calls (fwgpu_run.cpp: whole blocks
    in batches of generic_k, a trailing partial block on its own)"""
    out, pos = [], 0
    for f in calls:
        left = f
        while left:
            bf = min(left, mbf)
            k = min(left // mbf, Kg) if bf == mbf else 1
            out.append((pos, k, bf))
            pos += k * bf
            left -= k * bf
    return out


def assert_straddles(calls, mbf, Kg, R, wraps=2):
    hits = [s for s, k, bf in launches(calls, mbf, Kg) if (s % R) + k * bf > R]
    assert hits, "no K-batch straddles the ring's wrap (R = %d)" % R
    assert sum(calls) >= wraps * R, (sum(calls), R)


# ------------------------------------------------------------------ graphs
def mix_tree(e, outs, ports=16):
    """stereo nodes -> SumNodes of <= `ports` ports (a tree) -> the graph output"""
    while len(outs) > 1:
        nxt = []
        for i in range(0, len(outs), ports):
            grp = outs[i:i + ports]
            m = e.sum(len(grp))
            for p, n in enumerate(grp):
                e.connect_stereo(n, m, 2 * p)
            nxt.append(m)
        outs = nxt
    e.connect_stereo(outs[0], e.graph_out_node)


def stream_rig(e, h, fir_ch, dry):
    """graph input (fir_ch channels) -> FIR(h) -> graph output; dry: eight silent sampler voices on a SumNode of their own, which
    makes the plan a hybrid one (voice banks on the fused kernels, the FIR on the levels) without touching the output"""
    ir = e.new_sample(PLANAR_F32, h.shape[0], h)
    f = e.fir(ir, ch=fir_ch)
    for c in range(fir_ch):
        e.connect(e.graph_in_node, c, f, c)
        e.connect(f, c, e.graph_out_node, c)
    if dry:
        m = e.sum(8)
        for v in range(8):
            e.connect_stereo(e.sampler(100.0), m, 2 * v)
    e.update()
    return f


def stream_engine(T, mbf, K, ch, plan, h):
    g = GpuEngine(max_block_frames=mbf, max_batch=K, num_graph_inputs=ch, num_graph_outputs=ch, force_generic=plan == "generic")
    stream_rig(g, h, ch, dry=True)
    assert g.cx.plan_kind() == PLAN_KIND[plan]
    return g


def stream_oracle(mbf, ch, h):
    o = OracleEngine(max_block_frames=mbf, num_graph_inputs=ch, num_graph_outputs=ch)
    stream_rig(o, h, ch, dry=False)  # (the reference's sampler takes whole blocks only, Q5; the silent voices change no output)
    return o


def run_stream(e, x, calls):
    """x: (frames, ch) graph input, fed call by call; returns the (frames, ch) output"""
    ch = x.shape[1]
    out, pos = [], 0
    for f in calls:
        y = e.process_interleaved(f, ch, inp=np.ascontiguousarray(x[pos:pos + f]).reshape(-1), n_in_ch=ch)
        out.append(np.asarray(y, f32).reshape(-1, ch))
        pos += f
    return np.concatenate(out)


def noise_input(seed, n, ch, lead=37):
    x = fwapi.xorshift_uniform(seed, n * ch).reshape(n, ch)
    x[:lead] = 0.0  # the output must stay exactly +0.0 until the first nonzero input
    return x


# ------------------------------------------------------------------ 1. segment / ring matrix
# T: one tap; two; one segment; W = T-1+256 exactly FIR_SEG; a last segment of one position; FIR_SEG +- 0/1; 3 and 4 segments.
# mbf 100: a partial 256-column group and frames that are no multiple of 4; 1024: four column groups.  Pairwise over T x mbf x K.
MATRIX = [
    (1, 256, 16, "hybrid"), (2, 100, 5, "generic"), (255, 64, 1, "hybrid"), (255, 1024, 16, "generic"),
    (3841, 256, 5, "generic"), (3841, 64, 16, "hybrid"), (3842, 256, 16, "hybrid"), (3842, 100, 1, "generic"),
    (4096, 100, 16, "generic"), (4096, 1024, 5, "hybrid"), (4097, 256, 1, "hybrid"), (4097, 64, 5, "generic"),
    (8193, 64, 16, "generic"), (8193, 1024, 1, "hybrid"), (12289, 100, 5, "hybrid"), (12289, 256, 16, "generic"),
]


@pytest.mark.parametrize("T,mbf,K,plan", MATRIX)
def test_fir_segments_and_ring_wrap_match_oracle_and_f64(T, mbf, K, plan):
    R = T - 1 + K * mbf
    rng = np.random.default_rng(T * 131 + mbf * 7 + K)
    calls = call_schedule(rng, 2 * R + T, mbf, K)
    assert_straddles(calls, mbf, K, R)
    h = flat_ir(900 + T, T, 2)
    x = noise_input(T + mbf, sum(calls), 2)
    yg = run_stream(stream_engine(T, mbf, K, 2, plan, h), x, calls)
    yo = run_stream(stream_oracle(mbf, 2, h), x, calls)
    assert_bits_equal(yo, yg, "T=%d mbf=%d K=%d %s" % (T, mbf, K, plan))
    for c in range(2):
        assert_f64(yg[:, c], x[:, c], h[c], "T=%d mbf=%d K=%d %s ch%d" % (T, mbf, K, plan, c))


# ------------------------------------------------------------------ 2. config 4's length
def _impulse_across_wrap(T, ch, plan, mbf=256, K=16, seed=1):
    R = T - 1 + K * mbf
    n_imp = R - 1000  # its taps come out through the ring's wrap
    rng = np.random.default_rng(seed)
    calls = call_schedule(rng, n_imp + T + 1, mbf, K)
    assert_straddles(calls, mbf, K, R, wraps=1)
    h = flat_ir(70 + T, T, ch)
    x = np.zeros((sum(calls), ch), f32)
    amp = (1.0, 0.5)[:ch]
    x[n_imp] = amp
    y = run_stream(stream_engine(T, mbf, K, ch, plan, h), x, calls)
    # one nonzero product per output: y[n_imp + k] = h[k] * amp exactly, for every tap of every segment
    assert not np.any(bits(y[:n_imp])), "output before the impulse"
    for c in range(ch):
        want = (h[c] * f32(amp[c])).astype(f32)
        assert_bits_equal(want, y[n_imp:n_imp + T, c], "impulse response through the wrap, T=%d ch%d %s" % (T, c, plan))
    assert not np.any(bits(y[n_imp + T:])), "output after the last tap"


@pytest.mark.parametrize("plan", ["hybrid", "generic"])
def test_config4_length_impulse_across_the_ring_wrap_is_every_tap(plan):
    _impulse_across_wrap(65536, 2, plan)


@pytest.mark.parametrize("plan", ["hybrid", "generic"])
def test_config4_length_random_input_past_the_wrap_matches_oracle_f64_and_scales(plan):
    # 300+ blocks of 256 frames (the wrap is at block 272); one mono row: ~13 ms of oracle time per block
    T, mbf, K = 65536, 256, 16
    R = T - 1 + K * mbf
    calls = call_schedule(np.random.default_rng(4), 300 * mbf, mbf, K)
    assert_straddles(calls, mbf, K, R, wraps=1)
    h = flat_ir(4242, T, 1)
    x = noise_input(99, sum(calls), 1)
    yg = run_stream(stream_engine(T, mbf, K, 1, plan, h), x, calls)
    yo = run_stream(stream_oracle(mbf, 1, h), x, calls)
    assert_bits_equal(yo, yg, "65536 taps, mono row, %s" % plan)
    assert_f64(yg[:, 0], x[:, 0], h[0], "65536 taps vs f64, %s" % plan)
    y4 = run_stream(stream_engine(T, mbf, K, 1, plan, h), (x * f32(0.25)).astype(f32), calls)
    assert_bits_equal((yg * f32(0.25)).astype(f32), y4, "input x 0.25 -> output x 0.25, %s" % plan)


# ------------------------------------------------------------------ 3. beyond config 4 (no oracle: ~60 ms per block)
def test_fir_2pow18_taps_impulse_across_the_wrap():
    _impulse_across_wrap(1 << 18, 1, "hybrid", seed=2)


def test_fir_2pow18_taps_random_input_matches_f64():
    T, mbf, K = 1 << 18, 256, 16
    R = T - 1 + K * mbf
    calls = call_schedule(np.random.default_rng(3), R + 4096, mbf, K)
    assert any((s % R) + k * bf > R for s, k, bf in launches(calls, mbf, K))
    h = flat_ir(2018, T, 1)
    x = noise_input(2019, sum(calls), 1)
    y = run_stream(stream_engine(T, mbf, K, 1, "hybrid", h), x, calls)
    assert_f64(y[:, 0], x[:, 0], h[0], "2^18 taps vs f64")


# ------------------------------------------------------------------ sampler-driven banks
def voice_bank(e, fir_of, n_voices, src_seed=0, src_frames=1531):
    """n_voices x (stereo sampler at a voice-specific gain, looping -> the FIR node fir_of(e, v) makes) -> sum tree -> out.
    fir_of returns (first node, last node) of the voice's FIR stage, or (node, node, "mono") for a ch=1 FIR fed by channel 0."""
    outs, samplers = [], []
    for v in range(n_voices):
        s = e.sampler(70.0 + (v * 7) % 31)
        spec = fir_of(e, v)
        if len(spec) == 3:
            e.connect(s, 0, spec[0], 0)
            m2s = e.sum(1)  # a mono FIR node's one channel onto the left of a stereo port (right unconnected)
            e.connect(spec[1], 0, m2s, 0)
            outs.append(m2s)
        else:
            e.connect_stereo(s, spec[0])
            outs.append(spec[1])
        samplers.append(s)
    mix_tree(e, outs)
    e.update()
    for v, s in enumerate(samplers):
        e.sampler_set_sample(s, e.new_sample(PLANAR_F32, 2, scenarios.voice_source(src_seed + v, src_frames + 17 * v)))
        e.sampler_set_loop_range(s, LOOP_FULL)
        e.sampler_play(s)
    return samplers


def drive(e, calls, n_out=2):
    return np.concatenate([np.asarray(e.process_interleaved(f, n_out), f32) for f in calls])


def both_banks(build, mbf, K, calls, plan="hybrid"):
    g = GpuEngine(max_block_frames=mbf, max_batch=K, force_generic=plan == "generic")
    build(g)
    assert g.cx.plan_kind() == PLAN_KIND[plan]
    yg = drive(g, calls)
    o = OracleEngine(max_block_frames=mbf)
    build(o)
    return drive(o, calls), yg


# 4a. one stereo impulse response shared by many FIR voices: more than 32 rows (several tiles) on one h, through two wraps
@pytest.mark.parametrize("V,T,mbf,K", [(33, 4097, 128, 4), (64, 300, 256, 16), (256, 300, 256, 16)])
def test_fir_bank_of_many_tiles_on_one_impulse_response_matches_oracle(V, T, mbf, K):
    R = T - 1 + K * mbf
    calls = call_schedule(np.random.default_rng(V), 2 * R + T, mbf, K, odd=False)
    assert_straddles(calls, mbf, K, R)
    h = scenarios.reverb_ir(500 + V, T, 2)

    def build(e):
        ir = e.new_sample(PLANAR_F32, 2, h)
        voice_bank(e, lambda e, v: (lambda f: (f, f))(e.fir(ir)), V, src_seed=300)

    yo, yg = both_banks(build, mbf, K, calls)
    assert_bits_equal(yo, yg, "%d voices on one h, T=%d" % (V, T))


# 4b. one level with several impulse responses of one T (a different h per tile, padding between the groups), a mono impulse
# response on stereo nodes, ch=1 FIR nodes, two T values — and a FIR -> FIR cascade (two launches sharing d_fir_partials)
def test_fir_mixed_level_and_cascade_match_oracle():
    mbf, K, TA, TD = 128, 4, 1000, 4500
    irs = {"A": scenarios.reverb_ir(11, TA, 2), "B": scenarios.reverb_ir(12, TA, 2), "C": scenarios.reverb_ir(13, TA, 1),
           "D": scenarios.reverb_ir(14, TD, 2)}
    plan = ["A"] * 12 + ["B"] * 10 + ["C"] * 5 + ["A1"] * 3 + ["D"] * 6 + ["AD"] * 2
    R = TD - 1 + K * mbf
    calls = call_schedule(np.random.default_rng(8), 2 * R + TD, mbf, K, odd=False)
    assert_straddles(calls, mbf, K, R)

    def build(e):
        smp = {k: e.new_sample(PLANAR_F32, v.shape[0], v) for k, v in irs.items()}

        def fir_of(e, v):
            p = plan[v]
            if p == "A1":
                f = e.fir(smp["A"], ch=1)
                return (f, f, "mono")
            if p == "AD":
                a, d = e.fir(smp["A"]), e.fir(smp["D"])
                e.connect_stereo(a, d)
                return (a, d)
            f = e.fir(smp[p])
            return (f, f)

        voice_bank(e, fir_of, len(plan), src_seed=700)

    yo, yg = both_banks(build, mbf, K, calls)
    assert_bits_equal(yo, yg, "mixed FIR level + cascade")


# 4c. the benched shape: 256 voices, 65 536 taps, K 16.  The oracle would take ~10 s per block here: f64 only.
def test_fir_benched_shape_256_voices_65536_taps_matches_f64():
    V, T, mbf, K, n_src = 256, 65536, 256, 16, 16
    R = T - 1 + K * mbf
    calls = call_schedule(np.random.default_rng(256), 300 * mbf, mbf, K, odd=False)
    assert_straddles(calls, mbf, K, R, wraps=1)
    n = sum(calls)
    h = flat_ir(65536, T, 2)
    srcs = [scenarios.voice_source(4400 + j, 1500 + 61 * j) for j in range(n_src)]

    g = GpuEngine(max_block_frames=mbf, max_batch=K)
    ir = g.new_sample(PLANAR_F32, 2, h)
    ss = []
    outs = []
    for v in range(V):
        s = g.sampler(100.0)  # unity gain: voice v's input is source v % 16 exactly (checked below on the oracle)
        f = g.fir(ir)
        g.connect_stereo(s, f)
        outs.append(f)
        ss.append(s)
    mix_tree(g, outs)
    g.update()
    assert g.cx.plan_kind() == 3
    for v, s in enumerate(ss):
        g.sampler_set_sample(s, g.new_sample(PLANAR_F32, 2, srcs[v % n_src]))
        g.sampler_set_loop_range(s, LOOP_FULL)
        g.sampler_play(s)
    y = drive(g, calls).reshape(n, 2)
    # the samplers' output (the FIR inputs), from the oracle: n_src samplers straight to 2 * n_src graph outputs
    o = OracleEngine(max_block_frames=mbf, num_graph_outputs=2 * n_src)
    os_ = [o.sampler(100.0) for _ in range(n_src)]
    for j, s in enumerate(os_):
        o.connect_stereo(s, o.graph_out_node, 2 * j)
    o.update()
    for j, s in enumerate(os_):
        o.sampler_set_sample(s, o.new_sample(PLANAR_F32, 2, srcs[j]))
        o.sampler_set_loop_range(s, LOOP_FULL)
        o.sampler_play(s)
    xs = drive(o, calls, 2 * n_src).reshape(n, n_src, 2)
    assert np.array_equal(xs[:srcs[0].shape[1], 0, 0], srcs[0][0])  # (unity gain, from frame 0)
    per = V // n_src
    for c in range(2):  # sums over the voices as sums over the sources (each feeds `per` voices)
        ref = conv64(per * xs[:, :, c].astype(np.float64).sum(axis=1), h[c])
        bound = per * conv64(np.abs(xs[:, :, c]).astype(np.float64).sum(axis=1), np.abs(h[c]))
        sum_abs_ref = per * sum(np.abs(conv64(xs[:, j, c], h[c])) for j in range(n_src))
        # + 256u sum_v |ref_v|: the Sum nodes' roundings
        check_f64(y[:, c], ref, bound, 0, "256 x 65536 taps ch%d" % c, extra=256 * U * sum_abs_ref)


# ------------------------------------------------------------------ 5. formats and lifecycle
def _ir_in_format(fmt, h):
    """h (channels, T) in [-1, 1) as sample data of format fmt"""
    ch, T = h.shape
    if fmt in (INTERLEAVED_F32, PLANAR_F32):
        d = h.astype(f32)
    else:
        d = np.round(h * 32767.0).astype(np.int16)
        if fmt in (INTERLEAVED_U16, PLANAR_U16):
            d = (d.astype(np.int32) + 32768).astype(np.uint16)
    return d if fmt >= PLANAR_I16 else np.ascontiguousarray(d.T)


def test_fir_impulse_responses_in_every_sample_format_match_oracle():
    mbf, K, T = 128, 4, 777  # T no multiple of 64: the f32 copy is padded
    fmts = [INTERLEAVED_I16, INTERLEAVED_U16, INTERLEAVED_F32, PLANAR_I16, PLANAR_U16, PLANAR_F32]
    R = T - 1 + K * mbf
    calls = call_schedule(np.random.default_rng(6), 2 * R + T, mbf, K, odd=False)
    assert_straddles(calls, mbf, K, R)

    def build(e):
        irs = []
        for i, fmt in enumerate(fmts):
            for ch in (1, 2):
                h = (fwapi.xorshift_uniform(60 + 2 * i + ch, ch * T).reshape(ch, T) * f32(0.05)).astype(f32)
                irs.append(e.new_sample(fmt, ch, _ir_in_format(fmt, h)))
        voice_bank(e, lambda e, v: (lambda f: (f, f))(e.fir(irs[v])), len(irs), src_seed=800)

    yo, yg = both_banks(build, mbf, K, calls)
    assert_bits_equal(yo, yg, "impulse responses in six formats, mono and stereo")


def _reuse_slices(mbf=128, K=4):
    """a FIR node that has seen loud input is removed; a new node with the same T, then one with a smaller T, takes over its ext
    slice (same 64-rounded length): their first blocks must be a fresh node's (the oracle's new processor starts from zeros)"""
    T1, T2 = 1001, 995  # stereo rings: 4R = 6048 and 6024 floats, both 6080 once rounded to 64
    h1, h2 = flat_ir(31, T1, 2), flat_ir(32, T2, 2)
    x = (noise_input(33, 200 * mbf, 2, lead=0) * f32(8.0)).astype(f32)
    res = []
    for e in (GpuEngine(max_block_frames=mbf, max_batch=K, num_graph_inputs=2),
              OracleEngine(max_block_frames=mbf, num_graph_inputs=2)):
        f = stream_rig(e, h1, 2, dry=True)
        s2 = e.new_sample(PLANAR_F32, 2, h2)
        pos, out = 0, []

        def run(blocks):
            nonlocal pos
            out.append(run_stream(e, x[pos:pos + blocks * mbf], [mbf] * blocks))
            pos += blocks * mbf

        run(30)
        used = []
        for smp in (None, s2):
            e.remove_node(f)
            e.update()
            run(1)
            if e.backend != "oracle":
                used.append(e.cx.ext_pool_floats()[0])
            f = e.fir(smp if smp is not None else e.new_sample(PLANAR_F32, 2, h1), ch=2)
            e.connect_stereo(e.graph_in_node, f)
            e.connect_stereo(f, e.graph_out_node)
            e.update()
            if e.backend != "oracle":
                assert e.cx.plan_kind() == 3
                used.append(e.cx.ext_pool_floats()[0])
            run(12)
        res.append((np.concatenate(out), used))
    (yg, used), (yo, _) = res
    assert_bits_equal(yo, yg, "FIR nodes on recycled ext slices")
    # the new nodes' rings took the removed node's slice: only the new impulse responses' f32 copies (one per channel) were added
    assert used[1] - used[0] == 2 * ((T1 + 63) // 64 * 64) and used[3] - used[2] == 2 * ((T2 + 63) // 64 * 64), used


def test_fir_node_replaced_on_a_recycled_ext_slice_starts_fresh():
    _reuse_slices()


def test_fir_node_replaced_on_a_recycled_ext_slice_starts_fresh_with_poisoned_memory():
    env = dict(os.environ, FWGPU_POISON="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "reuse"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "reuse ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("plan", ["hybrid", "generic"])
def test_fir_ring_after_max_batch_grows_past_two_wraps(plan):
    # the ring was sized for max_batch 2 at activation; max_batch 16 afterwards must not outrun it (generic_k stays 2)
    T, mbf, K0 = 4097, 128, 2
    R = T - 1 + K0 * mbf
    calls = call_schedule(np.random.default_rng(5), 2 * R + T, mbf, 16)
    assert_straddles(calls, mbf, K0, R)
    h = flat_ir(41, T, 2)
    x = noise_input(42, sum(calls), 2)
    g = stream_engine(T, mbf, K0, 2, plan, h)
    g.cx.set_max_batch(16)
    g.update()
    assert g.cx.plan_kind() == PLAN_KIND[plan]
    yg = run_stream(g, x, calls)
    yo = run_stream(stream_oracle(mbf, 2, h), x, calls)
    assert_bits_equal(yo, yg, "FIR ring vs a later max_batch, %s" % plan)
    for c in range(2):
        assert_f64(yg[:, c], x[:, c], h[c], "later max_batch ch%d" % c)


def test_fir_two_nodes_share_an_impulse_response_one_is_removed():
    T, mbf, K = 3000, 128, 4
    R = T - 1 + K * mbf
    h = scenarios.reverb_ir(51, T, 2)
    calls1 = call_schedule(np.random.default_rng(53), 30 * mbf, mbf, K, odd=False)
    calls2 = call_schedule(np.random.default_rng(54), 2 * R + T, mbf, K)
    assert_straddles(calls1 + calls2, mbf, K, R)
    x = noise_input(52, sum(calls1) + sum(calls2), 2, lead=0)
    outs = []
    for e in (GpuEngine(max_block_frames=mbf, max_batch=K, num_graph_inputs=2),
              OracleEngine(max_block_frames=mbf, num_graph_inputs=2)):
        ir = e.new_sample(PLANAR_F32, 2, h)
        fa, fb = e.fir(ir), e.fir(ir)
        m = e.sum(2)
        for p, f in enumerate((fa, fb)):
            e.connect_stereo(e.graph_in_node, f)
            e.connect_stereo(f, m, 2 * p)
        e.connect_stereo(m, e.graph_out_node)
        d = e.sum(8)
        for v in range(8):
            e.connect_stereo(e.sampler(100.0), d, 2 * v)
        e.update()
        y1 = run_stream(e, x, calls1)
        e.remove_node(fb)
        e.update()
        if e.backend != "oracle":
            assert e.cx.plan_kind() == 3
        outs.append(np.concatenate([y1, run_stream(e, x[sum(calls1):], calls2)]))
    assert_bits_equal(outs[1], outs[0], "shared impulse response, one node removed")


@pytest.mark.parametrize("graph", ["1", "0"])
def test_fir_one_block_realtime_callbacks_through_two_wraps(graph, monkeypatch):
    monkeypatch.setenv("FWGPU_RT_GRAPH", graph)
    T, mbf, K, V = 4097, 128, 4, 8
    R = T - 1 + K * mbf
    h = scenarios.reverb_ir(61, T, 2)
    n_calls = (2 * R + T) // mbf + 2

    def build(e):
        ir = e.new_sample(PLANAR_F32, 2, h)
        voice_bank(e, lambda e, v: (lambda f: (f, f))(e.fir(ir)), V, src_seed=900)

    g = GpuEngine(max_block_frames=mbf, max_batch=K)
    build(g)
    assert g.cx.plan_kind() == 3
    yg = np.concatenate([np.asarray(g.process_blocks(1), f32) for _ in range(n_calls)])
    o = OracleEngine(max_block_frames=mbf)
    build(o)
    yo = np.concatenate([o.process_blocks(1) for _ in range(n_calls)])
    assert_bits_equal(yo, yg, "one-block callbacks, FWGPU_RT_GRAPH=%s" % graph)


def test_fir_tail_after_a_long_pause_decays_to_exact_zeros_with_oracle_flags():
    T, mbf, K, V = 1500, 128, 4, 8
    h = scenarios.reverb_ir(71, T, 2)
    pause = (T + mbf - 1) // mbf + 8  # blocks: longer than the impulse response (and a sampler's pause)
    res = []
    for e in (GpuEngine(max_block_frames=mbf, max_batch=K), OracleEngine(max_block_frames=mbf)):
        ir = e.new_sample(PLANAR_F32, 2, h)
        ss = voice_bank(e, lambda e, v: (lambda f: (f, f))(e.fir(ir)), V, src_seed=950)
        if e.backend != "oracle":
            assert e.cx.plan_kind() == 3
        parts = [e.process_blocks_flags(4), e.process_blocks_flags(3)]
        for s in ss:
            e.sampler_pause(s)
        parts += [e.process_blocks_flags(4) for _ in range(pause // 4 + 1)]
        for s in ss:
            e.sampler_play(s)
        parts += [e.process_blocks_flags(3), e.process_blocks_flags(4)]
        res.append((np.concatenate([np.asarray(p[0], f32) for p in parts]), np.concatenate([p[1] for p in parts])))
    (yg, fg), (yo, fo) = res
    assert_bits_equal(yo, yg, "FIR tail across a pause")
    assert np.array_equal(fo, fg), "silence flags differ from the oracle's"
    y = yg.reshape(-1, 2)
    p0, p1 = 7 * mbf, (7 + 4 * (pause // 4 + 1)) * mbf
    assert np.any(y[p0:p0 + T] != 0), "no tail after the pause began"
    assert not np.any(bits(y[p1 - 4 * mbf:p1])), "the tail does not end in exact +0.0"
    assert np.any(y[p1:] != 0)


if __name__ == "__main__":  # (the poisoned-memory run of the slice-reuse test: a child process of its own)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["reuse"]:
        _reuse_slices()
        print("reuse ok")
