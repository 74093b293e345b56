"""Resampler voice banks at every window and loop-length gate.

A resampling source in a fused voice bank is not rendered by one kernel: a (leaf, block) goes to one of four pieces of code by gates the
device computes from the ratio, the block length, the sample length, the loop flag and the format (firewheel_amd/csrc/k_leaf.hip.h):

  tier P  k_leaf_rs (rs_pure_lane): every port silent or "pure" — planar f32, no ramp, no glide, w_max <= RS2_WIN, a loop >= RS2_WIN + RS_TAPS
  tier S  leaf_rs_piece (k_leaf_sum_wl, the work list): planar f32, no glide, w_max <= RS_WIN, (step >> 32) < 8, a loop >= RS_WIN + RS_TAPS
  tier F  voice_eval's frame-by-frame fetch: everything else — other formats, short loops, large ratios, glides, a spatialiser's upstream
  tier G  K_RESAMPLER of the level executor (k_generic.hip.h)

with w_max = ceil(min(frames, 256) * step) + 1 + RS_TAPS.  `rs_tier` below restates the gates on the test's side; TABLE holds one voice
on each side of each of them, one f32 ratio or one frame apart, the short loops whose taps wrap several times, the ratios at both ends
of the legal range, one-shots that end inside a piece, and leaves whose ports sit on different tiers.

CPU tier: the table is not vacuous (every line listed with the voices on each side of it); OracleEngine and refmodel.RefEngine agree on
it bit for bit and every voice sounds; the planner takes it as ONE fused voice bank (host-only harness).
GPU tier: the table on the fused bank at block lengths 64 / 100 / 256 / 512 with control calls, lazy calls and a ragged tail; leaves
that change tier from block to block inside one launch (ratio steps, seeks, pause / resume); the level executor; 16-bit and interleaved
sources; a spatialiser's upstream; one-block calls; a ratio glide across the gates.  Every comparison is `bits` equality.

Out of scope: the gates `i_end < 2^30` and `len < 2^30` need samples of gigabytes.
"""
import collections
import os
import re

import numpy as np
import pytest

import fwapi
import rs_glide_model as gm
import scenarios
from fwapi import INTERLEAVED_F32, INTERLEAVED_I16, PLANAR_F32, PLANAR_I16, GpuEngine, HostOnlyEngine, OracleEngine, bits
from refmodel import RefEngine, resampler_step

F32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _define(path, name):
    text = open(os.path.join(ROOT, "firewheel_amd", "csrc", path)).read()
    return int(re.search(r"^#define %s (\d+)\b" % name, text, flags=re.M).group(1))


RS_TAPS = _define("fwgpu_types.h", "RS_TAPS")     # (the tap count lives beside RS_PHASES; the two windows in the leaf kernels' header)
RS2_WIN = _define("k_leaf.hip.h", "RS2_WIN")
RS_WIN = _define("k_leaf.hip.h", "RS_WIN")


# ================================================================================================ the gates, restated
def w_max(frames, step):
    """window frames of any 256-frame piece of a block — k_leaf.hip.h rs_pure_lane and k_leaf_sum_wl's `w_max`"""
    return ((min(frames, 256) * step + 0xFFFFFFFF) >> 32) + 1 + RS_TAPS


# Mirrors, in k_leaf.hip.h:
#   P  rs_pure_lane: `(df & VB_RESAMPLE) && !(df & (VB_RAMP_MASK | VB_RS_GLIDE)) && format == FMT_P_F32` and
#      `w_max <= RS2_WIN && ... len >= 1u && (!loop || len >= RS2_WIN + RS_TAPS)`
#   S  the work-list kernel's resampler ports: `el = !(df & VB_RS_GLIDE) && format == FMT_P_F32 && w_max <= RS_WIN && (step >> 32) < 8 && ...
#      len >= 1u && (!loop || len >= RS_WIN + RS_TAPS)` (a ramp does not keep a port off the staged path)
#   F  whatever `el` refuses: voice_eval's frame-by-frame fetch
# (the clauses on 2^30 are left out: see the docstring).  "P" is the voice's OWN eligibility: its leaf is rendered by k_leaf_rs only if
# every sounding port says "P"; beside another tier the leaf goes to the work list, where a "P" voice runs staged like an "S" one.
def rs_tier(frames, step, length, loop, fmt, ramping=False, glide=False):
    if fmt != PLANAR_F32 or glide or length < 1:
        return "F"
    w = w_max(frames, step)
    if not ramping and w <= RS2_WIN and (not loop or length >= RS2_WIN + RS_TAPS):
        return "P"
    if w <= RS_WIN and (step >> 32) < 8 and (not loop or length >= RS_WIN + RS_TAPS):
        return "S"
    return "F"


def lazy_capable(frames, step, length, loop, fmt):
    """k_control.hip.h make_lazy, mode 3: a steady voice leaves a lazy record when k_leaf_rs renders every block of it and its step is
    below 2^33 — ONE voice that is not keeps the control kernel in every call of the plan"""
    return rs_tier(frames, step, length, loop, fmt) == "P" and step < (1 << 33)


def edge_ratios(nfr, win):
    """(the largest f32 ratio whose window of `nfr` frames still fits `win`, the next f32 above it)"""
    up = lambda x: np.nextafter(F32(x), F32(np.inf))
    r = F32((win - 1 - RS_TAPS) / float(nfr))
    while w_max(nfr, resampler_step(r)) > win:
        r = np.nextafter(r, F32(0))
    while w_max(nfr, resampler_step(up(r))) <= win:
        r = up(r)
    return float(r), float(up(r))


# ================================================================================================ the case table
V = collections.namedtuple("V", "length ratio loop ch fmt leaf paused role")


def voice(length, ratio, loop, leaf, ch=2, fmt=PLANAR_F32, paused=False, role=""):
    return V(int(length), float(F32(ratio)), bool(loop), ch, fmt, leaf, paused, role)


MBFS = (64, 100, 256, 512)
LENGTHS = (1, 2, 15, 16, 17, 255, 527, 528, 529, 1055, 1056, 1057)
RATIOS = (1.0 / 256.0, 0.0371, 1.0, 1.93, 1.94, 3.99, 4.0, 4.01, 7.99, 8.0, 15.9, 100.0, 256.0)
BELOW_8 = float(np.nextafter(F32(8.0), F32(0)))
S_RATIOS = {64: (7.9, BELOW_8), 100: (6.0, 7.5), 256: (2.5, 3.9)}     # tier S (on a long sample) at that piece length


def _full_table():
    t = []
    # lengths x ratios x loop / one-shot, a leaf per (length, loop): short loops make all-F leaves, long ones span P, S and F
    for n in LENGTHS:
        for loop in (True, False):
            for r in RATIOS:
                t.append(voice(n, r, loop, "x%d%s" % (n, "L" if loop else "1"), ch=1 if len(t) % 5 == 4 else 2))
    # both sides of each window line, one f32 apart, for every piece length in use; both sides of step >> 32 == 8
    edges = [r for nfr in (64, 100, 256) for win in (RS2_WIN, RS_WIN) for r in edge_ratios(nfr, win)] + [BELOW_8, 8.0]
    for n, loop in ((529, True), (1057, True), (6000, False)):
        for r in edges:
            t.append(voice(n, r, loop, "e%d" % n))
    # a leaf of nothing but P voices at every block length; a one-shot that ends in the last piece of a 512-frame block (frame 408)
    for i, r in enumerate((0.5, 1.0, 1.5, 1.9, 1.0 / 256.0, 0.0371, 1.25, 0.75)):
        t.append(voice(5000 if i == 3 else 1500 + 7 * i, r, i != 3, "pure", ch=1 if i == 5 else 2))
    t.append(voice(400, 1.0, False, "pure"))
    # P-eligible voices beside S voices (the work list renders both staged), S beside F — for each piece length its own S ratios
    for nfr, (a, b) in sorted(S_RATIOS.items()):
        t += [voice(3000, 1.0, True, "ps%d" % nfr), voice(3100, a, True, "ps%d" % nfr), voice(2900, 1.5, False, "ps%d" % nfr), voice(3200, b, True, "ps%d" % nfr)]
        t += [voice(3100, a, True, "sf%d" % nfr), voice(17, 1.0, True, "sf%d" % nfr), voice(3200, b, True, "sf%d" % nfr), voice(300, 1.3, True, "sf%d" % nfr)]
    # silent ports at port 0 and elsewhere, under a 3-port mixer (sum.rs spells its path out) and under an n-port one; pure and F leaves
    t += [voice(2000, 1.1, True, "q3a", paused=True), voice(2100, 0.9, True, "q3a"), voice(2200, 1.3, True, "q3a")]
    t += [voice(2000, 1.1, True, "q3b"), voice(2100, 0.9, True, "q3b", paused=True), voice(2200, 1.3, True, "q3b")]
    t += [voice(2000, 1.1, True, "q5a", paused=True)] + [voice(2100 + 50 * i, 0.8 + 0.2 * i, True, "q5a") for i in range(4)]
    t += [voice(2100 + 50 * i, 0.8 + 0.2 * i, True, "q5b", paused=i in (2, 4)) for i in range(5)]
    t += [voice(17, 1.1, True, "f3", paused=True), voice(300, 0.9, True, "f3"), voice(16, 5.0, True, "f3")]
    t += [voice(300, 0.9 + 0.7 * i, True, "f5", paused=i in (0, 3)) for i in range(5)]
    t.append(voice(300, 256.0, True, "f5"))      # (a block of 256 frames advances it 218 loop lengths: the per-block `mod` is the whole story)
    return t


R_LENGTHS = (1, 15, 17, 527, 529, 1057)
R_RATIOS = (1.0 / 256.0, 1.93, 4.01, 256.0)


def _reduced_table(fmt=PLANAR_F32):
    """48 voices (+ 12 planar-f32 ones beside them when `fmt` is another format): a leaf per length"""
    t = []
    for n in R_LENGTHS:
        for loop in (True, False):
            for r in R_RATIOS:
                t.append(voice(n, r, loop, "r%d" % n, ch=1 if len(t) % 5 == 4 else 2, fmt=fmt))
        if fmt != PLANAR_F32:
            t += [voice(2000 + n, 1.0, True, "r%d" % n), voice(1900 + n, 1.5, False, "r%d" % n)]
    return t


def _spatial_table():
    """the reduced table with two sampler -> spatialiser voices in every leaf: the leaf kernel's spatialiser stage in its resampler
    instantiation, beside resampler ports of every tier"""
    t = _reduced_table()
    for n in R_LENGTHS:
        t += [voice(1500 + n, 1.0, True, "r%d" % n, role="sp_sampler"), voice(1400 + n, 1.0, n % 2 == 1, "r%d" % n, ch=1, role="sp_sampler")]
    return sorted(t, key=lambda v: R_LENGTHS.index(int(v.leaf[1:])))     # (stable: the spatialiser voices are each leaf's last two ports)


def _ordinary_table():
    """the reduced table's topology on 3000-frame samples at ratios 0.9 .. 1.3: what an ordinary resampler bank is"""
    return [v._replace(length=3000, ratio=float(F32(0.9 + 0.4 * (i % 9) / 8.0))) for i, v in enumerate(_reduced_table())]


def _walk_table():
    """test 3's leaves: ONE voice per leaf is moved across the gates by messages (its role says how), the other ports stay P-eligible"""
    t = []
    for leaf, (n, loop, role) in enumerate([(3000, True, "walk"), (700, True, "walk"), (90000, False, "walk"), (17, True, "seek_loop"), (600, True, "seek_loop"),
                                            (2000, False, "seek_end"), (17, True, "pause"), (3000, True, "pause16")]):
        name = "w%d" % leaf
        for p in range(4):
            if p == leaf % 4:      # (the moved voice sits at another port from leaf to leaf, port 0 among them)
                t.append(voice(n, 1.0, loop, name, role=role, fmt=PLANAR_I16 if role == "pause16" else PLANAR_F32))
            else:
                t.append(voice(2500 + 100 * p, 0.8 + 0.3 * p, p != 1, name, ch=1 if p == 3 else 2))
    return t


WALK = (1.5, 1.94, 3.99, 4.01, 7.9, 9.0, 256.0, 1.0 / 256.0, 1.0)     # (7.9: tier S at 64-frame blocks, where 1.94 .. 4.01 are still P)
TABLE = _full_table()
TABLES = {"full": TABLE, "reduced": _reduced_table(), "ordinary": _ordinary_table(), "walk": _walk_table(), "spatial": _spatial_table(),
          "i16": _reduced_table(PLANAR_I16), "i16i": _reduced_table(INTERLEAVED_I16), "f32i": _reduced_table(INTERLEAVED_F32)}


def leaves_of(table):
    out = collections.OrderedDict()
    for i, v in enumerate(table):
        out.setdefault(v.leaf, []).append(i)
    return out


def tier_of(v, mbf):
    return rs_tier(mbf, resampler_step(v.ratio), v.length, v.loop, v.fmt)


def describe(table, ids, mbf):
    return ", ".join("#%d %s len %d ratio %.9g %s tier %s" % (i, table[i].leaf, table[i].length, table[i].ratio, "loop" if table[i].loop else "one-shot",
                                                              tier_of(table[i], mbf)) for i in ids)


# ================================================================================================ graphs (any fwapi.Engine)
class Rig(object):
    def __init__(self, table):
        self.table, self.src, self.vol, self.mixers = table, [], [], []

    def where(self, pred):
        return [i for i, v in enumerate(self.table) if pred(v)]


def _sample(e, seed, v):
    data = scenarios.voice_source(7300 + seed, v.length, v.ch)
    if v.fmt in (PLANAR_I16, INTERLEAVED_I16):
        data = np.round(data * 32767).astype(np.int16)
    return e.new_sample(v.fmt, v.ch, data.T.copy() if v.fmt in (INTERLEAVED_I16, INTERLEAVED_F32) else data)


def build(e, table, spatial=False):
    """voices resampler -> volume -> pan (or resampler -> spatialiser), a SumNode per leaf, SumNodes of 16 leaves, a root"""
    rng = np.random.default_rng(4242)
    rig = Rig(table)
    ends = []
    samplers = []
    for i, v in enumerate(table):
        gain, pan, xyz = float(rng.uniform(30, 100)), float(rng.uniform(-1, 1)), [float(x) for x in rng.uniform(-4, 4, 3)]
        if v.role == "sp_sampler":
            s = e.sampler(gain)
            samplers.append((s, _sample(e, i, v), v.loop))
        else:
            s = e.resampler(_sample(e, i, v), v.ratio, loop=v.loop, playing=not v.paused, n_out=2)
        if spatial or v.role == "sp_sampler":
            cur = e.spatial(xyz[0], xyz[1] / 4.0, xyz[2], n_in=2)
            e.connect_stereo(s, cur)
            rig.vol.append(None)
        else:
            vol = e.volume(gain)
            cur = e.pan(pan)
            e.connect_stereo(s, vol)
            e.connect_stereo(vol, cur)
            rig.vol.append(vol)
        rig.src.append(s)
        ends.append(cur)

    def mix(nodes):
        m = e.sum(max(len(nodes), 2))
        for p, n in enumerate(nodes):
            e.connect_stereo(n, m, 2 * p)
        return m

    rig.mixers = [mix([ends[i] for i in ids]) for ids in leaves_of(table).values()]
    level = rig.mixers
    while len(level) > 1:
        level = [mix(level[i:i + 16]) for i in range(0, len(level), 16)]
    e.connect_stereo(level[0], e.graph_out_node)
    e.update()
    for s, smp, loop in samplers:
        e.sampler_set_sample(s, smp)
        if loop:
            e.sampler_set_loop_range(s, fwapi.LOOP_FULL)
        e.sampler_play(s)
    return rig


# ================================================================================================ the runs (any engine) -> [output per call]
TAIL = {64: 37, 100: 37, 256: 100, 512: 257}
QUIET0, QUIET = 9, 7      # run_bank: the message-free calls are blocks [QUIET0 + 2 i, QUIET0 + 2 i + 2), i < QUIET


def _call(e, outs, marks, frames):
    outs.append(np.asarray(e.process_interleaved(frames)))
    if marks is not None:
        marks.append(e.cx.lazy_stats()[0])


def run_bank(e, table, mbf, marks=None, **kw):
    """test 2: calls of a few blocks; the voices that leave no lazy record pause (call 2); SEVEN message-free calls (calls 3 .. 9: the
    first follows the messages and runs the control kernel, and so does a call a one-shot ends in — quiet_calls_without_an_end says which
    do not); everything resumes, the voices paused from the start too; a block + a short block; a block.  QUIET0 + 2 * QUIET + 4 blocks + the tail."""
    rig = build(e, table, **kw)
    outs = []
    busy = rig.where(lambda v: not v.paused and v.role != "sp_sampler" and not lazy_capable(mbf, resampler_step(v.ratio), v.length, v.loop, v.fmt))
    _call(e, outs, marks, 2 * mbf)
    _call(e, outs, marks, (QUIET0 - 4) * mbf)
    for i in busy:
        e.set_param(rig.src[i], 3, 0.0, at_block=1)
    for _ in range(1 + QUIET):
        _call(e, outs, marks, 2 * mbf)
    for i in busy:
        e.set_param(rig.src[i], 3, 1.0, at_block=1)
    for i in rig.where(lambda v: v.paused):
        e.set_param(rig.src[i], 3, 1.0, at_block=0)
    _call(e, outs, marks, 2 * mbf)
    _call(e, outs, marks, mbf + TAIL[mbf])
    _call(e, outs, marks, mbf)
    return outs


def run_long(e, table, mbf, marks=None, **kw):
    """ONE call of 70 blocks (the control kernel's second round of 64 blocks: `inc %= M`, one conditional subtraction), two short ones"""
    build(e, table, **kw)
    outs = []
    for frames in (70 * mbf, 3 * mbf, 2 * mbf + TAIL[mbf]):
        _call(e, outs, marks, frames)
    return outs


def run_walk(e, table, mbf, marks=None, **kw):
    """test 3: ONE call of 11 blocks in which a voice per leaf changes tier from block to block"""
    rig = build(e, table, **kw)
    outs = []
    _call(e, outs, marks, 2 * mbf)
    for i, v in enumerate(table):
        s = rig.src[i]
        if v.role == "walk":
            for b, r in enumerate(WALK):
                e.set_param(s, 1, r, at_block=b + 1)
        elif v.role == "seek_loop":       # to the last frame of the loop, to 0, to the last frame again at ratios that wrap it at once
            e.set_param(s, 4, float(v.length - 1), at_block=1)
            e.set_param(s, 4, 0.0, at_block=3)
            e.set_param(s, 1, 4.01, at_block=4)
            e.set_param(s, 4, float(v.length - 1), at_block=5)
            e.set_param(s, 1, 0.7, at_block=7)
        elif v.role == "seek_end":        # just in front of a one-shot's end: it runs out inside the block; back to 0 and started again
            e.set_param(s, 4, float(v.length - 5), at_block=2)
            e.set_param(s, 4, 0.0, at_block=5)
            e.set_param(s, 3, 1.0, at_block=5)
            e.set_param(s, 4, float(v.length - mbf // 2), at_block=7)
        elif v.role in ("pause", "pause16"):  # the leaf's one port that is not pure: paused, the leaf is k_leaf_rs's; resumed, the work list's
            for b in (1, 4, 7):
                e.set_param(s, 3, 0.0, at_block=b)
            for b in (3, 5, 9):
                e.set_param(s, 3, 1.0, at_block=b)
    _call(e, outs, marks, 11 * mbf)
    _call(e, outs, marks, 3 * mbf)
    return outs


def run_singles(e, table, mbf, marks=None, **kw):
    build(e, table, **kw)
    outs = []
    for _ in range(30):
        _call(e, outs, marks, mbf)
    return outs


def new_oracle(mbf):
    return scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf, short_blocks=True))


_oracle_cache = {}


def oracle_run(run, name, mbf, **kw):
    """the oracle's calls for (run, table, block length): computed once, shared, never written to"""
    key = (run.__name__, name, mbf, tuple(sorted(kw.items())))
    if key not in _oracle_cache:
        outs = run(new_oracle(mbf), TABLES[name], mbf, **kw)
        for o in outs:
            o.setflags(write=False)
        assert all(np.all(np.isfinite(o)) for o in outs) and any(np.any(o != 0) for o in outs)
        _oracle_cache[key] = outs
    return _oracle_cache[key]


def first_mismatch(want, got):
    for c, (a, b) in enumerate(zip(want, got)):
        if a.shape != b.shape or not np.array_equal(bits(a), bits(b)):
            return c
    return None if len(want) == len(got) else min(len(want), len(got))


def explain(run, name, mbf, call, make_gpu, **kw):
    """a failure's message: each leaf rendered alone on both sides, the first one that differs named with its voices and their tiers"""
    table = TABLES[name]
    for leaf, ids in leaves_of(table).items():
        sub = [table[i] for i in ids]
        c = first_mismatch(run(new_oracle(mbf), sub, mbf, **kw), run(make_gpu(), sub, mbf, **kw))
        if c is not None:
            return "call %d differs; leaf %r alone differs from call %d on: %s" % (call, leaf, c, describe(table, ids, mbf))
    return "call %d differs; no leaf differs when rendered alone" % call


def check(run, name, mbf, make_gpu, plan=1, marks=None, **kw):
    want = oracle_run(run, name, mbf, **kw)
    g = make_gpu()
    got = run(g, TABLES[name], mbf, marks=marks, **kw)
    assert g.cx.plan_kind() == plan
    if plan == 1:
        assert g.cx.plan_fused_voices() == len(TABLES[name])
    c = first_mismatch(want, got)
    if c is not None:
        raise AssertionError("%s table, %d-frame blocks: %s" % (name, mbf, explain(run, name, mbf, c, make_gpu, **kw)))
    return g


# ================================================================================================ CPU tier
def _blocks(v, mbf, n):
    """[(32.32 position at the block's start, at its end before the wrap)] of the blocks a voice started at 0 plays"""
    step, pos, out = resampler_step(v.ratio), 0, []
    for _ in range(n):
        end = pos + mbf * step
        out.append((pos, end))
        if v.loop:
            pos = end % (v.length << 32)
        elif (end >> 32) >= v.length + RS_TAPS // 2:
            break
        else:
            pos = end
    return out


def quiet_calls_without_an_end(table, mbf):
    """run_bank's message-free calls behind the first in which no playing one-shot runs out: the horizon the control kernel reports
    (k_control.hip.h make_lazy) lets the host render exactly these from the lazy records"""
    ends = set()
    for v in table:
        if not v.loop and not v.paused and lazy_capable(mbf, resampler_step(v.ratio), v.length, v.loop, v.fmt):
            b = _blocks(v, mbf, QUIET0 + 2 * QUIET + 1)      # (one block more than the calls hold: a voice that plays them all has it)
            if len(b) <= QUIET0 + 2 * QUIET:
                ends.add(len(b) - 1)
    return [i for i in range(1, QUIET) if not ends & {QUIET0 + 2 * i, QUIET0 + 2 * i + 1}]


def _contiguous(v, mbf, pos):
    """rs_pure_lane's `contig`: the block's whole window lies inside the sample"""
    step = resampler_step(v.ratio)
    span = ((mbf * step + 0xFFFFFFFF) >> 32) + 1 + RS_TAPS + 4
    i0 = (pos >> 32) % v.length if v.loop else pos >> 32
    qb0 = i0 - (RS_TAPS // 2 - 1)
    return qb0 >= 0 and qb0 + span <= v.length


@pytest.mark.parametrize("mbf", MBFS)
def test_the_table_has_a_voice_on_each_side_of_every_gate(mbf):
    T, nfr = TABLE, min(mbf, 256)
    step = lambda v: resampler_step(v.ratio)
    sounding = lambda v: v.fmt == PLANAR_F32 and not v.paused
    lines = []

    def line(what, **sides):
        found = {k: [i for i, v in enumerate(T) if sounding(v) and pred(v)] for k, pred in sides.items()}
        lines.append((what, found))
        for k, ids in found.items():
            print("%-52s %-14s %s" % (what, k, describe(T, ids[:2], mbf) or "-"))
            assert ids, "mbf %d: no voice for %r, side %r" % (mbf, what, k)

    for name, win in (("RS2_WIN", RS2_WIN), ("RS_WIN", RS_WIN)):
        lo, hi = edge_ratios(nfr, win)
        assert (w_max(mbf, resampler_step(lo)), w_max(mbf, resampler_step(hi))) == (win, win + 1)     # adjacent f32 ratios, adjacent windows
        line("w_max against %s" % name, at=lambda v: w_max(mbf, step(v)) == win and v.length >= RS_WIN + RS_TAPS,
             above=lambda v: w_max(mbf, step(v)) == win + 1 and v.length >= RS_WIN + RS_TAPS)
    assert tier_of(voice(4000, edge_ratios(nfr, RS2_WIN)[0], True, ""), mbf) == "P" and tier_of(voice(4000, edge_ratios(nfr, RS2_WIN)[1], True, ""), mbf) != "P"
    # (step >> 32) < 8 decides only where eight source frames per output frame still fit RS_WIN: pieces of up to (RS_WIN - 1 - RS_TAPS) / 8
    # = 127 frames.  Of the block lengths used here that is 64 and 100; at 256 and 512 w_max has sent such a ratio to tier F long before.
    if w_max(mbf, 8 << 32) <= RS_WIN:
        assert mbf in (64, 100)
        line("step >> 32 against 8", seven=lambda v: step(v) >> 32 == 7 and v.length >= RS_WIN + RS_TAPS and tier_of(v, mbf) == "S",
             eight=lambda v: step(v) >> 32 == 8 and w_max(mbf, step(v)) <= RS_WIN and v.length >= RS_WIN + RS_TAPS and tier_of(v, mbf) == "F")
    else:
        assert mbf in (256, 512)
    wraps = lambda v: any(not _contiguous(v, mbf, p) for p, _ in _blocks(v, mbf, 6))
    for gate in (RS2_WIN + RS_TAPS, RS_WIN + RS_TAPS):
        assert gate in (528, 1056)                        # (the table's lengths are written out: a change of the windows must change them)
        # (... at a ratio where this gate decides: P against F for the first, S against F for the second)
        decides = (lambda v: tier_of(v._replace(length=4000), mbf) == "P") if gate == 528 else (lambda v: tier_of(v._replace(length=4000), mbf) == "S")
        for n in (gate - 1, gate, gate + 1):
            line("loop of %d frames whose window wraps" % n, here=lambda v, n=n: v.loop and v.length == n and decides(v) and wraps(v))
    assert tier_of(voice(527, 1.93, True, ""), 256) == "F" and tier_of(voice(528, 1.93, True, ""), 256) == "P"
    assert tier_of(voice(1055, 2.5, True, ""), 256) == "F" and tier_of(voice(1056, 2.5, True, ""), 256) == "S"
    for n in (1, 2, 15, 16, 17):
        line("%d-frame sample" % n, loop=lambda v, n=n: v.loop and v.length == n, one_shot=lambda v, n=n: not v.loop and v.length == n)
    line("ratio 1/256: a piece inside one source frame", loop=lambda v: step(v) == 1 << 24 and v.loop, one_shot=lambda v: step(v) == 1 << 24 and not v.loop)
    line("ratio 256", short_loop=lambda v: step(v) == 1 << 40 and v.loop and v.length < 528, long_loop=lambda v: step(v) == 1 << 40 and v.loop and v.length >= 1056)
    line("one-shot shorter than its window", here=lambda v: not v.loop and v.length < w_max(mbf, step(v)) - RS_TAPS and tier_of(v, mbf) == "P")
    line("one-shot that ends inside block 0", P=lambda v: not v.loop and len(_blocks(v, mbf, 2)) == 1 and tier_of(v, mbf) == "P",
         other=lambda v: not v.loop and len(_blocks(v, mbf, 2)) == 1 and tier_of(v, mbf) != "P")
    if mbf == 512:
        def in_last_piece(v):
            b = _blocks(v, mbf, 12)
            return not v.loop and len(b) < 12 and ((b[-1][0] + 256 * step(v)) >> 32) < v.length + RS_TAPS // 2
        line("one-shot that ends in the last piece of a block", here=in_last_piece)
    both = lambda v: len({_contiguous(v, mbf, p) for p, _ in _blocks(v, mbf, 6)}) == 2 and tier_of(v, mbf) == "P"
    line("contiguous in one block, wrapping in another", loop=lambda v: v.loop and both(v), one_shot=lambda v: not v.loop and both(v))

    # per leaf: the tiers of its ports
    kinds = {}
    for leaf, ids in leaves_of(T).items():
        tiers = frozenset(tier_of(T[i], mbf) for i in ids if not T[i].paused)
        silent = [p for p, i in enumerate(ids) if T[i].paused]
        kinds.setdefault((tiers, len(ids) == 3, bool(silent and silent[0] == 0), bool(silent and silent[-1] > 0)), []).append(leaf)
    have = lambda tiers, **kw: [l for (t, three, at0, later), ls in kinds.items() for l in ls if t == frozenset(tiers) and
                                all({"three": three, "at0": at0, "later": later}[k] == want for k, want in kw.items())]
    for what, leaves in (("all P", have("P", at0=False, later=False)), ("all F", have("F", at0=False, later=False)), ("P beside S", have("PS")), ("S beside F", have("SF")),
                         ("pure, 3 ports, port 0 silent", have("P", three=True, at0=True)), ("pure, 3 ports, a later port silent", have("P", three=True, later=True)),
                         ("pure, n ports, port 0 silent", have("P", three=False, at0=True)), ("pure, n ports, later ports silent", have("P", three=False, later=True)),
                         ("F, 3 ports, port 0 silent", have("F", three=True, at0=True)), ("F, n ports, silent ports", have("F", three=False, at0=True, later=True))):
        print("%-52s %s" % ("leaf: " + what, leaves[:4]))
        assert leaves, "mbf %d: no leaf that is %s" % (mbf, what)
    quiet = quiet_calls_without_an_end(T, mbf)
    print("%-52s %s" % ("message-free calls no one-shot ends in", quiet))
    assert any(a + 1 == b and b + 1 == c for a, b, c in zip(quiet, quiet[1:], quiet[2:])), quiet      # three in a row
    assert len(TABLE) <= 420, len(TABLE) and len(TABLES["reduced"]) == 48 and all(len(TABLES[k]) <= 60 for k in ("i16", "i16i", "f32i", "ordinary", "walk", "spatial"))


def test_the_walked_ratios_cross_the_gates_and_the_other_ports_stay_pure():
    for mbf in (64, 256):
        for ids in leaves_of(TABLES["walk"]).values():
            moved = [i for i in ids if TABLES["walk"][i].role]
            assert len(moved) == 1 and all(tier_of(TABLES["walk"][i], mbf) == "P" for i in ids if i not in moved)
        long_loop = [rs_tier(mbf, resampler_step(r), 3000, True, PLANAR_F32) for r in WALK]
        assert long_loop == {64: list("PPPPSFFPP"), 256: list("PSSFFFFPP")}[mbf], long_loop
        assert [rs_tier(mbf, resampler_step(r), 700, True, PLANAR_F32) for r in WALK] == {64: list("PPPPFFFPP"), 256: list("PFFFFFFPP")}[mbf]
    assert rs_tier(256, resampler_step(1.0), 3000, True, PLANAR_F32, ramping=True) == "S" and rs_tier(256, resampler_step(1.0), 3000, True, PLANAR_F32, glide=True) == "F"
    assert rs_tier(256, resampler_step(1.0), 3000, True, PLANAR_I16) == "F" and rs_tier(64, 1 << 40, 300, True, PLANAR_F32) == "F"


def _model_run(table, mbf, spatial=False):
    """3 blocks, the voices paused from the start resumed, 3 more — on both CPU restatements; per voice, whether the model's own output
    buffer of it (behind its pan / spatialiser: what its leaf's SumNode reads) held a nonzero frame in some block"""
    o, m = OracleEngine(max_block_frames=mbf), RefEngine(max_block_frames=mbf)
    ro, rm = build(o, table, spatial), build(m, table, spatial)
    ends = [m.in_edge[mx][2 * p][0] for mx, ids in zip(rm.mixers, leaves_of(table).values()) for p in range(len(ids))]
    order = [i for ids in leaves_of(table).values() for i in ids]
    bufs = {n: out_bufs for n, _, _, out_bufs in m.plan}
    heard = np.zeros(len(table), dtype=bool)
    outs_o, outs_m = [], []
    for b in range(6):
        if b == 3:
            for i, v in enumerate(table):
                if v.paused:
                    o.set_param(ro.src[i], 3, 1.0)
                    m.set_param(rm.src[i], 3, 1.0)
        outs_o.append(o.process_blocks(1))
        outs_m.append(m.process_blocks(1))
        for i, n in zip(order, ends):
            heard[i] |= any(not m.flags[buf] and np.any(m.pool[buf][:mbf] != 0) for buf in bufs[n])
    return np.concatenate(outs_o), np.concatenate(outs_m), heard


@pytest.mark.parametrize("name,mbf", [("full", 64), ("full", 256), ("reduced", 100), ("i16", 64), ("i16i", 256), ("f32i", 100), ("walk", 64), ("spatial", 64)])
def test_both_cpu_references_agree_on_the_table_and_every_voice_sounds(name, mbf):
    out_o, out_m, heard = _model_run(TABLES[name], mbf)
    assert np.array_equal(bits(out_o), bits(out_m))
    assert np.all(np.isfinite(out_o)) and np.any(out_o != 0)
    assert heard.all(), "voices that never sound: " + describe(TABLES[name], list(np.flatnonzero(~heard)), mbf)


@pytest.mark.parametrize("name,mbf,spatial", [("full", 64, False), ("full", 100, False), ("full", 256, False), ("full", 512, False), ("reduced", 64, False),
                                              ("spatial", 64, False), ("spatial", 256, False), ("ordinary", 64, False), ("walk", 64, False), ("walk", 256, False), ("i16", 100, False),
                                              ("i16i", 100, False), ("f32i", 100, False)])
def test_the_planner_takes_every_table_as_one_fused_voice_bank(name, mbf, spatial):
    """on the host-only harness: a refusal by the planner shows here and not as a puzzling GPU result"""
    e = HostOnlyEngine(max_block_frames=mbf, max_batch=4)
    build(e, TABLES[name], spatial)
    assert e.cx.plan_kind() == 1
    assert e.cx.plan_fused_voices() == len(TABLES[name])
    e.process_blocks(2)
    assert e.violation() == ""


def test_the_planner_keeps_a_resampler_in_front_of_a_spatialiser_off_the_bank():
    """fwgpu_plan_detect.cpp walk_voice_chain: "a spatialiser voice is a dry sampler voice" — resampler -> spatialiser is no voice of the
    bank: the plan is the hybrid one, the pair is rendered by the level executor (tier G in front of K_SPATIAL).  The GPU tier renders it
    that way (test_g4_in_front_of_a_spatialiser_on_the_levels) and, on the bank, the spatialiser stage beside resampler ports."""
    e = HostOnlyEngine(max_block_frames=64, max_batch=4)
    build(e, TABLES["reduced"], True)
    assert e.cx.plan_kind() == 3


# ================================================================================================ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("mbf,max_batch", [(64, 4), (100, 3), (256, 3), (512, 4), (256, 32)])
def test_g2_the_table_on_the_fused_bank(mbf, max_batch):
    marks = []      # marks[i] = lazy batches counted behind call i
    check(run_bank, "full", mbf, lambda: GpuEngine(max_block_frames=mbf, max_batch=max_batch), marks=marks)
    quiet = [3 + i for i in quiet_calls_without_an_end(TABLE, mbf)]
    print("lazy batches behind each call:", marks, "message-free calls no one-shot ends in:", quiet)
    if os.environ.get("FWGPU_LAZY") == "0":
        assert marks[-1] == 0, marks
        return
    # calls 0 .. 2 (sounding voices that leave no record; the pauses) and 3 (the call behind the messages) run the control kernel, and so
    # does a call a one-shot ends in (the horizon); every other message-free call is ONE batch rendered from the lazy records — three
    # in a row among them (the table test) — and nothing behind the resume messages is
    assert marks[3] == 0 and marks[3 + QUIET - 1] > 0, marks
    assert [c for c in range(1, len(marks)) if marks[c] > marks[c - 1]] == quiet, (marks, quiet)


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,max_batch", [(64, 128), (64, 3)])
def test_g2_seventy_blocks_in_one_call(mbf, max_batch):
    """the reduced table (48 voices; ratio 256 on loops of 1, 15, 17, 527 and 529 frames among them): with max_batch 128 the control kernel
    fills blocks 64..69 from blocks 0..5 by its 64-block stride; with max_batch 3 the same 70 blocks are 24 launches"""
    check(run_long, "reduced", mbf, lambda: GpuEngine(max_block_frames=mbf, max_batch=max_batch))


@pytest.mark.gpu
@pytest.mark.parametrize("mbf", [64, 256])
def test_g3_a_leaf_changes_tier_from_block_to_block_inside_one_launch(mbf):
    check(run_walk, "walk", mbf, lambda: GpuEngine(max_block_frames=mbf, max_batch=16))


@pytest.mark.gpu
def test_g4_the_level_executor_renders_the_table():
    check(run_bank, "full", 100, lambda: GpuEngine(max_block_frames=100, max_batch=3, force_generic=True), plan=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["i16", "i16i", "f32i"])
@pytest.mark.parametrize("mbf,max_batch", [(64, 4), (256, 3)])
def test_g4_sixteen_bit_and_interleaved_sources_beside_f32_voices(name, mbf, max_batch):
    check(run_bank, name, mbf, lambda: GpuEngine(max_block_frames=mbf, max_batch=max_batch))


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,max_batch", [(64, 4), (256, 3)])
def test_g4_in_front_of_a_spatialiser_on_the_levels(mbf, max_batch):
    check(run_bank, "reduced", mbf, lambda: GpuEngine(max_block_frames=mbf, max_batch=max_batch), plan=3, spatial=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mbf,max_batch", [(64, 4), (256, 3)])
def test_g4_beside_spatialiser_voices_in_the_bank(mbf, max_batch):
    check(run_bank, "spatial", mbf, lambda: GpuEngine(max_block_frames=mbf, max_batch=max_batch))


@pytest.mark.gpu
@pytest.mark.parametrize("mbf", [64, 256])
def test_g4_one_block_calls_take_the_path_an_ordinary_bank_takes(mbf):
    paths = {}
    for name in ("ordinary", "reduced"):
        g = check(run_singles, name, mbf, lambda: GpuEngine(max_block_frames=mbf))
        paths[name] = g.cx.rt_path_stats()
        print("%s bank, one-block batches by path (resident, one launch, fused sequence, level executor): %s" % (name, paths[name]))
        assert sum(paths[name]) == 30
    assert int(np.argmax(paths["reduced"])) == int(np.argmax(paths["ordinary"])), paths


def run_glide(e, mbf):
    """0.5 -> 16 over three blocks and back, on a 17-frame and on a 529-frame loop, two steady voices beside them"""
    table = [voice(17, 0.5, True, "g"), voice(529, 0.5, True, "g"), voice(2000, 1.0, True, "g"), voice(2100, 1.5, False, "g", ch=1)]
    rig = build(e, table)
    outs = [np.asarray(e.process_blocks(2))]
    for s in rig.src[:2]:
        e.glide(s, 16.0, 3 * mbf, at_block=1)
        e.glide(s, 0.5, 3 * mbf + 7, at_block=5)
    outs.append(np.asarray(e.process_blocks(10)))
    outs.append(np.asarray(e.process_blocks(2)))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("mbf", [64, 256])
def test_g4_a_ratio_glide_across_the_gates(mbf):
    want = run_glide(gm.Tagged(gm.GlideRefEngine(max_block_frames=mbf)), mbf)
    g = GpuEngine(max_block_frames=mbf, max_batch=16)
    got = run_glide(gm.GpuGlide(g), mbf)
    assert g.cx.plan_kind() == 1 and g.cx.plan_fused_voices() == 4
    assert first_mismatch(want, got) is None, "call %s" % first_mismatch(want, got)
    assert np.any(want[1] != 0)
