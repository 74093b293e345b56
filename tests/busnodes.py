"""What the tests of the bus nodes with a kernel of their own share (tests/test_limiter.py, test_ducker.py, test_delay_comp.py,
test_bus_nodes.py): the bit comparison, the ragged calls, voices and banks of them, and the planner tests' calls on the host harness."""
import numpy as np

import fwapi
import scenarios
from fwapi import LOOP_FULL, HostOnlyEngine

METER, LIMITER, DUCKER, DELAY_COMP = 16, 17, 18, 19
# launch_level's bits (firewheel_amd/csrc/fwgpu_types.h kind_launch_bits): k_level's three instantiations and the batch walkers together,
# and a bit per kernel of its own
LB_LEVEL, LB_LIMITER, LB_DUCKER, LB_DELAY_COMP = 15, 16, 32, 64
F32 = np.float32


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(fwapi.bits(got) != fwapi.bits(want))
    assert bad.size == 0, "%s: %d of %d samples differ, first at %s: %r vs %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def planar(interleaved, ch=2):
    return np.asarray(interleaved, dtype=F32).reshape(-1, ch).T


def ragged_calls(mbf, at_least=6000):
    """several K-block calls with K in {1, 2, 5}, a call of 3 blocks plus a 37-frame tail, a 1-frame call"""
    pattern = [2 * mbf, 5 * mbf, mbf, 3 * mbf + 37, 1, 5 * mbf, 2 * mbf, mbf]
    calls = []
    while len(calls) < 5 or sum(calls) < at_least:
        calls.append(pattern[len(calls) % len(pattern)])
    return calls


def _host(mbf=64, **kw):
    e = HostOnlyEngine(max_block_frames=mbf, **kw)
    v = e.volume(50.0)
    e.connect_stereo(v, e.graph_out_node)
    return e, v


# ------------------------------------------------------------------------------------------------ voices and banks
class Bank(object):
    pass


def _stage(e, tok, rng, i):
    if isinstance(tok, float):
        return e.volume(tok)
    if tok == "v":
        return e.volume(float(rng.uniform(30, 100)))
    if tok == "p":
        return e.pan(float(rng.uniform(-1, 1)))
    if tok == "c":
        return e.hard_clip(-3.0)
    if tok == "B":
        return e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 8000)), float(rng.choice([0.707, 1.8])))
    if tok == "D":
        return e.delay((64, 129, 300, 384)[i % 4] / float(e.sample_rate), feedback=float(rng.choice([0.0, 0.45])), mix=0.5)
    raise ValueError(tok)


def _voice(e, b, shape, i=0, rng=None):
    """a sampler and the stages of `shape` behind it: letters (parameters drawn from rng) or floats (a volume of that percent)"""
    s = e.sampler(100.0)
    b.samplers.append(s)
    cur = s
    for t in shape:
        n = _stage(e, t, rng, i)
        e.connect_stereo(cur, n)
        cur = n
    return cur


def _start(e, s, seed, i, salt, src_blocks=6):
    """salt: what tells the sources of one test file from another's (31 limiter, 57 ducker, 71 delay-comp)"""
    e.sampler_set_sample(s, e.new_sample(fwapi.PLANAR_F32, 2, scenarios.voice_source(seed * 1000 + salt + i, src_blocks * e.max_block_frames, 2)))
    e.sampler_set_loop_range(s, LOOP_FULL)
    e.sampler_play(s)


DRY = ["v", "vp", "", "pv", "vc", "v", "vp", "p", "v"]
CHAIN = ["vB", "BD", "v", "vBD", "vp", "DBv", "BB", "cB", "v"]
# fused plan kind -> a bank that gets it: voice-bank, chain, hybrid (a send)
PLANS = {1: dict(shapes=DRY), 2: dict(shapes=CHAIN), 3: dict(shapes=DRY, send=True)}


def bank(e, shapes, master, send=False, spatial=False, submix=False, middle=None, seed=0, leave_out="", rng_base=4200, salt=31):
    """voices -> leaf sums of four (the last one with a free port pair) -> root sum -> master chain -> graph_out 0,1.
    master: a list of ("v", percent) | ("L", C, H) | ("M", ring_blocks) | ("C", threshold_db); kinds named in `leave_out` are not built
    (the oracle's graph).  send: leaf 0's bus is consumed twice, dry and through a send delay — not a fused shape as a whole (plan 3).
    spatial: a spatialiser behind the root, which no fused plan takes.  submix: beside the bank a sub-mix S of two more voices ->
    `middle` -> graph_out 2,3; middle: ("dcomp", D), "volume" (the twin: a 2 -> 2 volume of 100 % in its place) or None (S itself)"""
    b = Bank()
    b.e, b.samplers, b.node, b.middle, b.seed, b.salt = e, [], {}, None, seed, salt
    rng = np.random.default_rng(rng_base + seed)
    ends = [_voice(e, b, sh, i, rng) for i, sh in enumerate(shapes)]
    leaves = []
    for i in range(0, len(ends), 4):
        grp = ends[i:i + 4]
        m = e.sum(max(2, len(grp)) + (1 if i + 4 >= len(ends) else 0))
        for p, n in enumerate(grp):
            e.connect_stereo(n, m, 2 * p)
        leaves.append(m)
        b.spare = (m, 2 * len(grp))
    root = e.sum(max(2, len(leaves) + (1 if send else 0)))
    for p, m in enumerate(leaves):
        e.connect_stereo(m, root, 2 * p)
    if send:
        d = e.delay(300 / float(e.sample_rate), feedback=0.3, mix=1.0)
        e.connect_stereo(leaves[0], d)
        e.connect_stereo(d, root, 2 * len(leaves))
    cur = root
    if spatial:
        sp = e.spatial(1.0, 0.5, -2.0, n_in=2)
        e.connect_stereo(cur, sp)
        cur = sp
    for spec in master:
        if spec[0] in leave_out:
            continue
        if spec[0] == "v":
            n = e.volume(spec[1])
        elif spec[0] == "L":
            n = e.add_node(LIMITER, 2, 2, [spec[1], spec[2]])
        elif spec[0] == "M":
            n = e.add_node(METER, 2, 2, [spec[1]])
        else:
            n = e.hard_clip(spec[1])
        b.node[spec[0]] = n
        e.connect_stereo(cur, n)
        cur = n
    b.last = cur
    e.connect_stereo(cur, e.graph_out_node)
    if submix:
        b.S = e.sum(2)
        for p in range(2):
            e.connect_stereo(_voice(e, b, "v", len(shapes) + p, rng), b.S, 2 * p)
        if middle == "volume":
            b.middle = e.volume(100.0)
        elif middle is not None:
            b.middle = e.add_node(DELAY_COMP, 2, 2, [float(middle[1])])
        if b.middle is not None:
            e.connect_stereo(b.S, b.middle)
            e.connect_stereo(b.middle, e.graph_out_node, 2)
        else:
            e.connect_stereo(b.S, e.graph_out_node, 2)
    e.update()
    for i, s in enumerate(b.samplers):
        _start(e, s, seed, i, salt)
    return b


# ------------------------------------------------------------------------------------------------ the planner tests' calls
HARNESS_CALLS = (3, 5, 2, 4, 6, 3, 5, 4, 4)   # blocks


def harness_run(e, n_out_ch=2):
    """HARNESS_CALLS through a HostOnlyEngine whose graph is built -> (launches by kind, OR of the level launches' bits).  The launch
    stubs must have found every descriptor invariant kept."""
    e.reset_launches()
    for k in HARNESS_CALLS:
        e.process_blocks(k, n_out_ch=n_out_ch)
    report = e.violation()
    fwapi.hostonly_lib().fwh_violation_reset()   # (a report must not spill into the tests behind this one)
    assert report == "", report
    return e.launches(), e.level_kinds_seen()


def harness_batches(max_batch):
    return sum((k + max_batch - 1) // max_batch for k in HARNESS_CALLS)
