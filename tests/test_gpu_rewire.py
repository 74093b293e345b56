"""In-place rewiring of voices that are already sounding (reference: any edge may be cut and made while audio runs, graph.rs:396-477,
and a re-plugged node keeps its smoother, biquad history, delay ring and playhead: processors persist across schedules).

The product answers an edit with a new plan and carries each voice's steady cache (VoiceCache) from the old plan to the new one when
the voice's chain is "the same" (fwgpu_types.h same_voice_chain).  Every test here takes voices that are sounding — steady, gliding,
muted and settled, paused, rendered by lazy calls — and moves, swaps, inserts or removes a stage or a filter INSIDE them, moves them to
another mixer port, or pushes them out of a fused plan's grammar and back, beside untouched voices whose caches must still travel.

GPU tier: bit for bit against the oracle (the first call after an edit carries no message: the call in which a wrongly carried
cache would be used).  CPU tier: the same scripts on the host-only harness (its adoption stub checks what travels) and on the oracle
alone (every edit must be audible there, or nothing is tested).

Shape tokens are test_chain_grammar's (v volume, p pan, c hard clip, B biquad, D delay, w width, leading m: mono sampler behind the
reference's adapter), plus s: a spatialiser as the last stage, and a leading r: a resampling source.
"""
import os

import numpy as np
import pytest

import fwapi
import scenarios
from fwapi import LOOP_FULL, GpuEngine, HostOnlyEngine, OracleEngine
from test_chain_grammar import ACCEPTED, DRY, FUZZ_SEEDS, REFUSED, assert_bits, build_voice


# ------------------------------------------------------------------------------------------------ voices whose wiring the test knows
class _Rec(object):
    """records the chain nodes test_chain_grammar.build_voice creates, in order (it returns them by kind only)"""

    def __init__(self, e, clip_db, vol0=False):
        self.e, self.log, self.adapter, self.clip_db, self.vol0 = e, [], None, clip_db, vol0

    def __getattr__(self, name):
        f = getattr(self.e, name)
        if name in ("pan", "biquad", "delay", "width"):
            def made(*a, **kw):
                n = f(*a, **kw)
                self.log.append(n)
                return n
            return made
        return f

    def volume(self, percent):
        n = self.e.volume(0.0 if self.vol0 else percent)  # (vol0: the voice's first volume is BORN at 0 %, see ROLES)
        self.vol0 = False
        self.log.append(n)
        return n

    def hard_clip(self, threshold_db):
        n = self.e.hard_clip(self.clip_db if self.clip_db is not None else threshold_db)  # (the catalogue's clips sit lower than build_voice's)
        self.log.append(n)
        return n

    def add_node(self, kind, n_in, n_out, params=()):
        n = self.e.add_node(kind, n_in, n_out, params)
        if kind == fwapi.MONO_TO_STEREO:
            self.adapter = n
        return n


def new_stage(e, tok, rng, delay_frames, clip_db=None):
    if tok == "v":
        return e.volume(float(rng.uniform(30, 100)))
    if tok == "p":
        return e.pan(float(rng.uniform(-1, 1)))
    if tok == "c":
        return e.hard_clip(-3.0 if clip_db is None else clip_db)
    if tok == "w":
        return e.width(1.3)
    if tok == "B":
        return e.biquad(int(rng.integers(0, 3)), float(rng.uniform(200, 8000)), float(rng.choice([0.707, 1.8])))
    if tok == "D":
        return e.delay(delay_frames / float(e.sample_rate), feedback=float(rng.choice([0.0, 0.45])), mix=0.5)
    if tok == "s":
        return e.spatial(float(rng.uniform(-5, 5)), float(rng.uniform(-1, 1)), float(rng.uniform(-5, 5)), n_in=2)
    raise ValueError(tok)


def make_voice(e, shape, rng, delay_frames, rs_sample=None, clip_db=None, vol0=False):
    """-> dict(sampler, src = the node that feeds the chain, chain = [[token, node], ...] in signal order, sink = None, kind = '', 'm', 'r')"""
    if shape.startswith("r"):
        s = e.resampler(rs_sample, ratio=float(rng.choice([0.5, 0.8, 1.25])), loop=True, playing=True)
        vc = dict(sampler=s, src=s, chain=[], sink=None, kind="r", rng=rng, delay=delay_frames, clip_db=clip_db)
        for t in shape[1:]:
            n = new_stage(e, t, rng, delay_frames, clip_db)
            e.connect_stereo(vc["chain"][-1][1] if vc["chain"] else s, n)
            vc["chain"].append([t, n])
        return vc
    rec = _Rec(e, clip_db, vol0)
    nodes = build_voice(rec, shape, rng, delay_frames)
    toks = shape[1:] if shape.startswith("m") else shape
    assert len(toks) == len(rec.log)
    return dict(sampler=nodes["sampler"], src=rec.adapter if rec.adapter is not None else nodes["sampler"],
                chain=[[t, n] for t, n in zip(toks, rec.log)], sink=None, kind="m" if shape.startswith("m") else "", rng=rng, delay=delay_frames, clip_db=clip_db)


def shape_of(vc):
    return vc["kind"] + "".join(t for t, _ in vc["chain"])


def of_kind(vc, tok):
    return [n for t, n in vc["chain"] if t == tok]


def _edges(vc):
    seq = [vc["src"]] + [n for _, n in vc["chain"]]
    for a, b in zip(seq[:-1], seq[1:]):
        yield a, 0, b, 0
        yield a, 1, b, 1
    if vc["sink"] is not None:
        m, p = vc["sink"]
        yield seq[-1], 0, m, 2 * p
        yield seq[-1], 1, m, 2 * p + 1


def unwire(e, vc):
    for a, ap, b, bp in _edges(vc):
        e.disconnect(a, ap, b, bp)


def wire(e, vc):
    for a, ap, b, bp in _edges(vc):
        e.connect(a, ap, b, bp)


def reshape(e, vc, new_shape, drop=()):
    """re-plug the voice's chain as `new_shape` (tokens only, no source prefix): a token takes the old chain's nodes of its kind in their
    old order — except the ones at the chain positions in `drop` —, what is left over is removed, what is missing is created"""
    unwire(e, vc)
    have = {}
    gone = []
    for i, (t, n) in enumerate(vc["chain"]):
        if i in drop:
            gone.append(n)
        else:
            have.setdefault(t, []).append(n)
    chain = []
    for t in new_shape:
        chain.append([t, have[t].pop(0) if have.get(t) else new_stage(e, t, vc["rng"], vc["delay"], vc["clip_db"])])
    for n in gone + [n for ns in have.values() for n in ns]:
        e.remove_node(n)
    vc["chain"] = chain
    wire(e, vc)


def move(e, vc, sink):
    unwire(e, vc)
    vc["sink"] = sink
    wire(e, vc)


def build_rewire_bank(e, shapes, radix, spare, seed, delays, fmts=None, frames=None, clip_db=None, spare_front=0, vol0=()):
    """voices under leaf sums of `radix` voices with `spare_front` open ports in front of them and `spare` behind, under one root sum.
    -> voices, free (sum, port) list"""
    mbf = e.max_block_frames
    rs_sample = None
    if any(sh.startswith("r") for sh in shapes):
        rs_sample = e.new_sample(fwapi.PLANAR_F32, 2, scenarios.voice_source(seed * 31 + 5, 5 * mbf + 17, 2))
    voices = [make_voice(e, sh, np.random.default_rng(seed * 977 + i), delays[i % len(delays)], rs_sample, clip_db, i in vol0) for i, sh in enumerate(shapes)]
    leaves, free = [], []
    for i in range(0, len(voices), radix):
        grp = voices[i:i + radix]
        m = e.sum(spare_front + len(grp) + spare)
        for p, vc in enumerate(grp, spare_front):
            vc["sink"] = (m, p)
            e.connect_stereo(vc["chain"][-1][1] if vc["chain"] else vc["src"], m, 2 * p)
        free += [(m, p) for p in list(range(spare_front)) + list(range(spare_front + len(grp), spare_front + len(grp) + spare))]
        leaves.append(m)
    assert len(leaves) >= 2
    root = e.sum(len(leaves))
    for p, m in enumerate(leaves):
        e.connect_stereo(m, root, 2 * p)
    e.connect_stereo(root, e.graph_out_node)
    e.update()
    for i, vc in enumerate(voices):
        if vc["kind"] == "r":
            continue
        fmt = fmts[i] if fmts else fwapi.PLANAR_F32
        n = frames[i] if frames else 6 * mbf
        ch = 2
        data = scenarios.voice_source(seed * 5000 + i, n, ch)
        if fmt in (fwapi.INTERLEAVED_I16, fwapi.PLANAR_I16):
            data = np.round(data * 32767).astype(np.int16)
        elif fmt == fwapi.INTERLEAVED_U16:
            data = np.round((data + 1.0) * 32767.5).astype(np.uint16)
        if fmt in (fwapi.INTERLEAVED_I16, fwapi.INTERLEAVED_U16, fwapi.INTERLEAVED_F32):
            data = data.T.copy()
        e.sampler_set_sample(vc["sampler"], e.new_sample(fmt, ch, data))
    return voices, free


# ------------------------------------------------------------------------------------------------ the catalogue
# edits: (shape before, shape after[, chain positions removed rather than re-plugged]) — five voices per entry, one per ROLE, are
# edited; `controls` are never touched.  plan: the plan kind before the first edit, after edit 1 (the steady / muted / paused voices),
# after edit 2 (the voices with a glide in flight) and after edit 3 (every edited voice back to what it was) — 1 voice bank, 2 chain,
# 3 hybrid, 0 level executor.  move: the edit is the voice's mixer port, not its chain.
# the state an edited voice is in when its edit lands.  muted: its volume glided to 0 % and settled — the reference's smoother then
# multiplies by 0.0 for good without ever reporting silence (checked on the oracle: 400 blocks on, the output is zeros and not flagged).
# silent: its volume was BORN at 0 % — a settled smoother at 0: that node reports silence, which is what the product's steady cache
# records as "silent" behind the filters and as the -1.0 sentinel between two of them (k_control.hip.h).
ROLES = ("steady", "muted", "silent", "paused", "glide_moved", "glide_stay")
QUIET_ROLES = ROLES[:4]


def _pair(a, b, controls=("vB", "BD", "v", "vp"), **kw):
    return dict(dict(name="%s<->%s" % (a, b), edits=[(a, b), (b, a)], controls=list(controls), plan=[2, 2, 2, 2]), **kw)


def _one(a, b, controls, plan, drop=(), roles=QUIET_ROLES, **kw):
    return dict(dict(name="%s->%s->%s" % (a, b, a) + ("" if not drop else " drop %d" % drop[0]), edits=[(a, b, drop)], controls=list(controls), plan=plan, roles=roles), **kw)


CATALOGUE = [
    # a gain stage moves across a filter, same nodes: n_pre / n_mid only
    _pair("BvD", "BDv"), _pair("vBD", "BvD"), _pair("BvB", "BBv"), _pair("DvB", "DBv"), _pair("BcD", "BDc"),
    # the filter order swaps, same nodes: fx_order
    _pair("BD", "DB"), _pair("BBD", "DBB"), _pair("vBDp", "vDBp"),
    # a stage is inserted or removed: n_stages, a new state slot
    _pair("BD", "BvD"), _pair("vB", "B"), _pair("vp", "vpc", controls=("v", "pv", "vp", ""), plan=[1, 1, 1, 1]),
    # a filter is inserted or removed: bq_state / bq2_state roles
    _pair("v", "vB"), _pair("vBD", "vD"),
    _one("BB", "B", ("vB", "BD", "v", "vBD"), [2, 2, 2, 2], drop=(0,), roles=ROLES),
    _one("BB", "B", ("vB", "BD", "v", "vBD"), [2, 2, 2, 2], drop=(1,), roles=ROLES),
    # two stages swap: stage_state[] / stage_kind[] / the stage program
    _pair("vp", "pv", controls=("v", "vp", "pc", ""), plan=[1, 1, 1, 1]), _pair("cv", "vc", controls=("v", "vp", "pc", ""), plan=[1, 1, 1, 1]),
    # the voice moves: voice index, summation order
    dict(name="BvD to another port", edits=[("BvD", "BvD"), ("vp", "vp")], controls=["vB", "BD", "v", "vp"], plan=[2, 2, 2, 2], move="port"),
    dict(name="BvD to another leaf", edits=[("BvD", "BvD"), ("vp", "vp")], controls=["vB", "BD", "v", "vp"], plan=[2, 2, 2, 2], move="leaf"),
    # accepted -> refused -> accepted
    _one("BD", "BDB", ("vB", "BD", "v", "vBD", "BvD", "vp"), [2, 3, 3, 2], roles=ROLES),
    _one("vB", "vBw", ("vB", "BD", "v", "vBD", "BvD", "vp"), [2, 3, 3, 2], roles=ROLES),
    # a spatialiser as the last stage of a dry voice comes and goes: sp_ext_off, its 64-frame history
    _one("v", "vs", ("v", "vp", "pc", "", "pv", "vp"), [1, 1, 1, 1], roles=ROLES),
    # a resampling source's gain is moved / removed: src_kind 1
    _pair("rvp", "rpv", controls=("v", "vp", "rv", "r"), plan=[1, 1, 1, 1]), _pair("rv", "r", controls=("v", "vp", "rvp", "pv"), plan=[1, 1, 1, 1]),
    # --- plans whose k_chain instantiation changes with the edit (every voice of a kind is edited at once: QUIET_ROLES, no glide group)
    # the edited voices are the only ones with a stage between two filters, and nobody holds a hard clip: stage sites on <-> off
    _one("BvD", "BDv", ("vB", "BD", "v", "vBD", "DBv", "vp"), [2, 2, 2, 2]),
    _one("BDv", "BvD", ("vB", "BD", "v", "vBD", "DBv", "vp"), [2, 2, 2, 2]),
    # the edited voices hold the plan's only second biquads
    _one("BBD", "BD", ("vB", "BD", "v", "vBD", "DBv", "vp"), [2, 2, 2, 2], drop=(1,)),
    # the edited voices get the plan's only delay shorter than a block of 128: the tile size changes
    _one("vB", "vBD", ("vB", "pBv", "v", "cB", "BB", "vp"), [2, 2, 2, 2], delays=(64,)),
    # the edited voices hold the plan's only filters: voice-bank plan <-> chain plan
    _one("v", "vB", ("v", "vp", "pc", "", "pv", "vp"), [1, 2, 2, 1]),
]
CASE_IDS = [c["name"].replace(" ", "_") + ("" if i < 24 else "_alone") for i, c in enumerate(CATALOGUE)]
SETTLE_FRAMES = 56 * 128  # a glide to 0 % takes about 45 blocks of 128 frames


def _gain_target(vc):
    """the stage the roles mute / glide: the voice's first volume — the stage every row of the catalogue moves, inserts or removes when
    it moves a volume — or the sampler's own gain"""
    v = of_kind(vc, "v")
    return v[0] if v else (vc["sampler"] if vc["kind"] != "r" else None)


def run_case(e, case, only=None, info=None):
    """only: None = every edit is made, -1 = none, i = voice i's alone (the oracle's "is this edit audible" runs).
    info (dict) receives: kinds (plan kind after each update), marks (sample offset of each edit), edited (voice index -> group),
    lazy (lazy_stats()[0] at four points)"""
    mbf = e.max_block_frames
    roles = case.get("roles", ROLES)
    plan = [(a, b, (rest[0] if rest else ()), r) for (a, b, *rest) in case["edits"] for r in roles] + [(c, None, (), None) for c in case["controls"]]
    order = np.random.default_rng(77).permutation(len(plan))
    plan = [plan[i] for i in order]
    n_edit = sum(1 for p in plan if p[3])
    voices, free = build_rewire_bank(e, [p[0] for p in plan], radix=(len(plan) + 1) // 2, spare=n_edit if case.get("move") else 1, spare_front=n_edit if case.get("move") else 0, seed=len(case["name"]) + 3,
                                     delays=case.get("delays", (300, 129, 700, 384, 1000)), clip_db=-30.0, vol0=[i for i, p in enumerate(plan) if p[3] == "silent"])  # (a clip low enough to bite behind a low-pass
    #                                                                                   filter: a clip that never clips cannot be heard moving)
    info = {} if info is None else info
    info.update(kinds=[], marks=[], lazy=[], edited={})
    out = []

    def call(k):
        out.append(np.asarray(e.process_blocks(k)))

    def lazy():
        info["lazy"].append(e.cx.lazy_stats()[0] if hasattr(e, "cx") else 0)

    def kind():
        info["kinds"].append(e.cx.plan_kind() if hasattr(e, "cx") else -1)

    def edit(group, back):
        n = 0
        for i, (vc, (a, b, drop, role)) in enumerate(zip(voices, plan)):
            if role is None or ((role in QUIET_ROLES) != (group == 0) and not back):
                continue
            info["edited"].setdefault(i, group)
            if only is not None and only != i:
                continue
            n += 1
            if case.get("move"):
                home = vc.setdefault("home", vc["sink"])
                if back:
                    dst = home
                else:
                    # (to the far side of its own leaf — behind the others if it sat in the front half, in front of them if not: a voice
                    #  that keeps its place in the order of summation has not moved audibly —, or to an open port of the other leaf)
                    mine = [s for s in free if (s[0] == home[0]) == (case["move"] == "port")]
                    if case["move"] == "port":
                        mine = [s for s in mine if (s[1] > home[1]) == (home[1] < n_edit + len(plan) // 4)]
                    dst = mine[0]
                    free.remove(dst)
                move(e, vc, dst)
            elif back:
                reshape(e, vc, a.lstrip("mr"))  # (what the first edit removed is created anew: the reference's nodes do not come back)
            else:
                reshape(e, vc, b.lstrip("mr"), drop)
        if n:
            e.update()
        kind()
        info["marks"].append(sum(x.size for x in out))
        call(3)  # no message at all: the call in which a cache that should not have travelled would be used
        for i, (vc, (a, b, drop, role)) in enumerate(zip(voices, plan)):
            if role is None or ((role in QUIET_ROLES) != (group == 0) and not back):
                continue
            t = _gain_target(vc)
            if role == "paused":
                if vc["kind"] != "r":
                    e.sampler_play(vc["sampler"], at_block=1)
            elif t is not None:
                e.set_param(t, 0, 70.0 if role in ("muted", "silent") else 55.0, at_block=1)
            for j, n in enumerate(of_kind(vc, "B")):
                e.set_param(n, 1, 700.0 + 900.0 * j + 60.0 * i, at_block=2)
        call(4)
        call(4)

    for vc in voices:
        if vc["kind"] != "r":
            e.sampler_set_loop_range(vc["sampler"], LOOP_FULL)
            e.sampler_play(vc["sampler"])
    call(3)
    for vc, p in zip(voices, plan):
        t = _gain_target(vc)
        if p[3] == "muted" and t is not None:
            e.set_param(t, 0, 0.0, at_block=0)
        if p[3] == "paused" and vc["kind"] != "r":
            e.sampler_pause(vc["sampler"], at_block=1)
    call(SETTLE_FRAMES // mbf)
    call(6)   # (quiet calls of 6 blocks: no batch size of the tests leaves a one-block batch behind, which on the voice-bank plan belongs
    lazy()    #  to the realtime kernels and spends the lazy records)
    call(6)
    call(6)
    lazy()
    kind()
    edit(0, False)                                   # --- edit 1: the steady, the muted-and-settled and the paused voices
    call(4)
    if any(r not in QUIET_ROLES for r in roles):
        for vc, p in zip(voices, plan):              # glides in flight across edit 2: on the stage that moves, on one that stays
            t = _gain_target(vc)
            if p[3] == "glide_moved" and t is not None:
                e.set_param(t, 0, 20.0, at_block=1)
            if p[3] == "glide_stay" and vc["kind"] != "r":
                e.set_param(vc["sampler"], 0, 35.0, at_block=1)
        call(2)
        edit(1, False)                               # --- edit 2
    else:
        kind()
        info["marks"].append(sum(x.size for x in out))
    call(SETTLE_FRAMES // mbf)
    call(6)   # (quiet calls of 6 blocks: no batch size of the tests leaves a one-block batch behind, which on the voice-bank plan belongs
    lazy()    #  to the realtime kernels and spends the lazy records)
    call(6)
    call(6)
    lazy()
    edit(0, True)                                    # --- edit 3: every edited voice back to its first shape, lazy calls behind it
    call(5)
    return np.concatenate(out)


_audible = {}


def oracle_case(case, mbf, per_voice=False):
    """the oracle's output of the case — after asserting that the edits are audible: behind every edit the run differs from the run
    of the same script without any edit.  per_voice (the CPU tier asks for it, for every case and both block sizes): the same for
    every edited voice on its own — the run in which that voice alone is edited differs from the run without edits between its edit
    and the edit that takes it back.  No case is exempt from either."""
    key = (case["name"], str(case["edits"]), mbf)
    if key not in _audible or (per_voice and not _audible[key][1]):
        info = {}
        full = run_case(scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf)), case, info=info)
        none = run_case(scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf)), case, only=-1)
        assert info["edited"] and full.shape == none.shape, case["name"]
        m = info["marks"] + [full.size]
        groups = sorted(set(info["edited"].values()))
        # (edit 3 takes every voice back: same nodes in their first order can be the run without edits again, bit for bit — both
        #  directions of a row are edits 1 and 2 of its two groups of voices)
        for lo, hi in [(m[g], m[g + 1]) for g in groups]:
            assert np.any(fwapi.bits(full[lo:hi]) != fwapi.bits(none[lo:hi])), "%s: the edit at sample %d cannot be heard in the oracle" % (case["name"], lo)
        for i, group in sorted(info["edited"].items()) if per_voice else ():
            solo = run_case(scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf)), case, only=i)
            assert solo.shape == none.shape
            lo, hi = m[group], m[2]  # (from its edit to the edit that takes it back)
            assert np.any(fwapi.bits(solo[lo:hi]) != fwapi.bits(none[lo:hi])), "%s: voice %d: its edit cannot be heard in the oracle" % (case["name"], i)
        _audible[key] = (full, per_voice)
    return _audible[key][0]


def _assert_lazy(case, info, max_batch, generic):
    """the quiet calls in front of edit 1 and the ones in front of edit 3 (behind edits 1 and 2) were rendered without a control kernel
    wherever the plan in force can do that: a chain plan; a voice-bank plan whose batches are longer than one block (one-block batches
    are the realtime kernels') and that holds no spatialiser (such banks keep their control kernel).  The hybrid plan and the level
    executor never do.  Banks with resampling sources are left out: whether such a voice is plain enough is the device's call."""
    if generic or os.environ.get("FWGPU_LAZY") == "0" or "r" in "".join(a + b for a, b, *_ in case["edits"]) + "".join(case["controls"]):
        return
    lz = info["lazy"]
    sp = any("s" in b for _, b, *_ in case["edits"])
    for kind, lo, hi, with_sp in ((case["plan"][0], lz[0], lz[1], False), (case["plan"][2], lz[2], lz[3], sp)):
        if kind == 2 or (kind == 1 and max_batch > 1 and not with_sp):
            assert hi > lo, (case["name"], lz)


# ------------------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("case", CATALOGUE, ids=CASE_IDS)
def test_every_catalogue_edit_is_audible_in_the_oracle(case):
    for mbf in (128, 64):
        out = oracle_case(case, mbf, per_voice=True)
        assert np.any(out != 0)


@pytest.mark.parametrize("case", CATALOGUE, ids=CASE_IDS)
def test_catalogue_on_the_host_harness(case):
    """the host half on the fake runtime: every table validated, the plan kinds of the table, and at every adoption the caches of the
    untouched voices travel while no cache travels between descriptors that differ (launch_stubs.cpp check_carry)"""
    for mbf, max_batch, generic in ((128, 8, False), (64, 3, False), (128, 1, True)):
        e = HostOnlyEngine(max_block_frames=mbf, max_batch=max_batch, force_generic=generic)
        fwapi.hostonly_lib().fwh_violation_reset()
        info = {}
        run_case(e, case, info=info)
        assert e.violation() == "", (case["name"], e.violation())
        assert info["kinds"] == ([0, 0, 0, 0] if generic else case["plan"]), (case["name"], info["kinds"])
        _assert_lazy(case, info, max_batch, generic)


# ------------------------------------------------------------------------------------------------ GPU tier
_COMBOS = [(64, 128), (3, 64), (1, 128), (64, 64), (3, 128), (1, 64)]  # (max_batch, max_block_frames)


def _case_params():
    """every case once on its fused plan and once as the level executor's twin, at one of the six (max_batch, max_block_frames)
    combinations each — taken in turn down the catalogue, so that every combination meets every class of edit on both executors (all
    six for every case cost several times what test_chain_grammar does; the twin shares its case's block size and so its oracle run)"""
    ps = []
    for i, (c, cid) in enumerate(zip(CATALOGUE, CASE_IDS)):
        mb, mbf = _COMBOS[i % 6]
        if c.get("delays") == (64,):
            mbf = 128  # (the case is about blocks of 128)
        for m, generic in ((mb, False), ([64, 3, 1][(i + 1) % 3], True)):
            ps.append(pytest.param(c, m, mbf, generic, id="%s-K%d-mbf%d%s" % (cid, m, mbf, "-levels" if generic else "")))
    return ps


@pytest.mark.gpu
@pytest.mark.parametrize("case,max_batch,mbf,generic", _case_params())
def test_rewired_voices_are_bit_exact(case, max_batch, mbf, generic):
    ro = oracle_case(case, mbf)
    g = GpuEngine(max_block_frames=mbf, max_batch=max_batch, force_generic=generic)
    info = {}
    rg = run_case(g, case, info=info)
    print("%s K<=%d mbf %d: plan kinds %r lazy %r" % (case["name"], max_batch, mbf, info["kinds"], info["lazy"]))
    m = info["marks"]
    a, b = np.asarray(ro), np.asarray(rg)
    bad = np.nonzero(fwapi.bits(a) != fwapi.bits(b))[0]
    where = "" if not bad.size else " (before the first edit)" if bad[0] < m[0] else " (%d blocks behind edit %d)" % ((bad[0] - [x for x in m if x <= bad[0]][-1]) // (2 * mbf), sum(1 for x in m if x <= bad[0]))
    assert_bits(ro, rg, "%s K<=%d mbf %d%s, plan kinds %r%s" % (case["name"], max_batch, mbf, " levels" if generic else "", info["kinds"], where))
    assert info["kinds"] == ([0, 0, 0, 0] if generic else case["plan"]), info["kinds"]
    for lo, hi in zip(m, m[1:] + [a.size]):
        assert np.any(a[lo:hi] != 0), "nothing sounded behind an edit"
    _assert_lazy(case, info, max_batch, generic)


# ------------------------------------------------------------------------------------------------ a seeded fuzz family for in-place edits
_GAINS = "vpc"


def _anagrams(toks, pool):
    key = sorted(toks)
    return [sh for sh in pool if sorted(sh) == key and sh != toks]


def fuzz_rewire(e, seed, log=None):
    """a bank of random shapes (accepted, dry, every third seed refused ones; mono and resampling sources among them), random formats
    and loop lengths; between calls of random length — long quiet stretches among them, so that steady caches and lazy records exist
    when an edit lands — 1-4 random in-place edits with probability one half, mixed with fuzz_grammar's kinds of message.  Every draw
    comes from one generator and the wiring is kept here, so every engine gets the same edits."""
    rng = np.random.default_rng(20_000 + seed)
    mbf = e.max_block_frames
    pool = ACCEPTED * 2 + DRY * 3 + ["rv", "rvp", "r"] + (REFUSED if seed % 3 == 0 else [])
    flat = [sh.lstrip("m") for sh in ACCEPTED + DRY] + ["pc", "vpc", "cv", "vc", "B", "BD", "D"]
    n = int(rng.integers(9, 36))
    shapes = [pool[int(rng.integers(0, len(pool)))] for _ in range(n)]
    radix = int(rng.choice([3, 5, 8, 16]))
    if n <= radix:
        radix = (n + 1) // 2
    delays = tuple(int(x) for x in rng.integers(64, 1300, size=7))
    fmts_all = [fwapi.PLANAR_F32] * 3 + [fwapi.INTERLEAVED_I16, fwapi.INTERLEAVED_U16, fwapi.PLANAR_I16, fwapi.INTERLEAVED_F32]
    whole = seed % 2 == 1  # odd seeds: planar f32 loops a whole number of blocks long — the quiet calls go lazy
    fmts = [fwapi.PLANAR_F32 if whole else fmts_all[int(rng.integers(0, len(fmts_all)))] for _ in range(n)]
    frames = [mbf * int(rng.integers(2, 7)) if whole else int(rng.integers(mbf + 40, 6 * mbf)) for _ in range(n)]
    voices, free = build_rewire_bank(e, shapes, radix=radix, spare=2, seed=seed + 100, delays=delays, fmts=fmts, frames=frames)
    for vc in voices:
        if vc["kind"] != "r":
            if rng.random() < 0.9:
                e.sampler_set_loop_range(vc["sampler"], LOOP_FULL)
            if rng.random() < 0.9:
                e.sampler_play(vc["sampler"])
    if log is not None:
        log.append(("shapes", shapes, "delays", delays, "radix", radix))
    out = []
    for call in range(int(rng.integers(8, 14))):
        quiet = rng.random() < 0.35
        k = int(rng.integers(20, 60)) if quiet and rng.random() < 0.5 else int(rng.integers(1, 9))
        if call > 1 and rng.random() < 0.5:
            for _ in range(int(rng.integers(1, 5))):
                vi = int(rng.integers(0, n))
                vc = voices[vi]
                toks = "".join(t for t, _ in vc["chain"])
                what = int(rng.integers(0, 6))
                dry = all(t in "vpcw" for t in toks)
                if what == 0:      # the same nodes in another order: a gain across a filter, the filters swapped, two stages swapped
                    cands = _anagrams(toks, flat)
                    new = cands[int(rng.integers(0, len(cands)))] if cands and rng.random() < 0.8 else "".join(rng.permutation(list(toks))) if toks else ""
                    if "s" in new:
                        new = new.replace("s", "") + "s"
                elif what == 1:    # to another shape altogether: stages and filters inserted and removed, the rest re-plugged
                    cand = DRY + ["pc", "vc"] if vc["kind"] == "r" or "s" in toks else flat + ([x for x in REFUSED] if seed % 3 == 0 else [])
                    new = cand[int(rng.integers(0, len(cand)))]
                elif what == 2:    # one stage or filter leaves
                    if not toks:
                        continue
                    d = int(rng.integers(0, len(toks)))
                    if log is not None:
                        log.append((call, vi, "drop", toks, d))
                    reshape(e, vc, toks[:d] + toks[d + 1:], drop=(d,))
                    continue
                elif what == 3:    # one gain stage arrives
                    if len(toks) >= 5 or "s" in toks:
                        continue
                    d = int(rng.integers(0, len(toks) + 1))
                    new = toks[:d] + _GAINS[int(rng.integers(0, 3))] + toks[d:]
                elif what == 4:    # a spatialiser as the last stage of a dry voice comes or goes
                    if "s" in toks:
                        new = toks.replace("s", "")
                    elif dry and vc["kind"] == "" and mbf % 64 == 0 and len(toks) < 5:
                        new = toks + "s"
                    else:
                        continue
                else:              # the voice moves to an open port, of its own leaf or of another
                    dst = free[int(rng.integers(0, len(free)))]
                    free.remove(dst)
                    free.append(vc["sink"])
                    if log is not None:
                        log.append((call, vi, "move", vc["sink"], dst))
                    move(e, vc, dst)
                    continue
                if log is not None:
                    log.append((call, vi, "reshape", toks, new))
                reshape(e, vc, new)
            e.update()
        if not quiet:
            msgs = sorted(((int(rng.integers(0, n)), int(rng.integers(0, k)), int(rng.integers(0, 7)), rng.random(4)) for _ in range(int(rng.integers(0, 1 + n // 2)))),
                          key=lambda m: m[1])
            for vi, at, what, u in msgs:
                vc = voices[vi]
                vols, pans, bqs, dls = of_kind(vc, "v"), of_kind(vc, "p"), of_kind(vc, "B"), of_kind(vc, "D")
                if log is not None:
                    log.append((call, k, vi, what, at))
                if what == 0 and vols:
                    e.set_param(vols[int(u[0] * len(vols))], 0, [0.0, 25.0, 60.0, 110.0][int(u[1] * 4)], at_block=at)
                elif what == 1 and pans:
                    e.set_param(pans[int(u[0] * len(pans))], 0, float(2.0 * u[1] - 1.0), at_block=at)
                elif what == 2 and bqs:
                    cut = u[2] < 0.5
                    e.set_param(bqs[int(u[0] * len(bqs))], 1 if cut else 2, float(150.0 + 8850.0 * u[1] if cut else 0.6 + 2.4 * u[1]), at_block=at)
                elif what == 3 and dls:
                    e.set_param(dls[0], 1 + int(u[0] * 2), float(0.7 * u[1]), at_block=at)
                elif vc["kind"] == "r":
                    continue
                elif what == 4:
                    e.sampler_pause(vc["sampler"], at_block=at)
                elif what == 5:
                    e.sampler_play(vc["sampler"], at_block=at)
                elif what == 6 and u[3] < 0.3:
                    e.sampler_stop(vc["sampler"], at_block=at)
        out.append(np.asarray(e.process_blocks(k)))
    return np.concatenate(out)


def _fuzz_cfg(seed):
    return [128, 64, 256][seed % 3], [64, 1, 3, 8][seed % 4]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_rewire_bit_exact(seed):
    mbf, max_batch = _fuzz_cfg(seed)
    o = scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf))
    g = GpuEngine(max_block_frames=mbf, max_batch=max_batch)
    ro, rg = fuzz_rewire(o, seed), fuzz_rewire(g, seed)
    a, b = np.asarray(ro), np.asarray(rg)
    bad = np.nonzero(fwapi.bits(a) != fwapi.bits(b))[0]
    assert bad.size == 0, "seed %d (plan %d, mbf %d, K<=%d): %d of %d samples differ, first at %d (block %d)" % (
        seed, g.cx.plan_kind(), mbf, max_batch, bad.size, a.size, bad[0], bad[0] // (2 * mbf))


def test_fuzz_rewire_on_the_host_harness():
    """the same edit and message streams through the host half on the fake runtime: every table the kernels would read is validated,
    and no steady cache travels between descriptors that differ"""
    for seed in range(12):
        mbf, max_batch = _fuzz_cfg(seed)
        e = HostOnlyEngine(max_block_frames=mbf, max_batch=max_batch)
        fwapi.hostonly_lib().fwh_violation_reset()
        fuzz_rewire(e, seed)
        assert e.violation() == "", (seed, e.violation())


def test_fuzz_rewire_is_deterministic_and_the_reference_takes_every_edit():
    """two oracles, one fed through TaggedOracle: the generator draws the same edits for every engine and never asks for an edge the
    reference rejects (AddEdgeError from connect fails the test: a generator bug, not a finding)"""
    for seed in range(12):
        mbf, _ = _fuzz_cfg(seed)
        la, lb = [], []
        a = fuzz_rewire(scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf)), seed, log=la)
        b = fuzz_rewire(scenarios.TaggedOracle(OracleEngine(max_block_frames=mbf)), seed, log=lb)
        assert repr(la) == repr(lb), seed
        assert np.array_equal(fwapi.bits(a), fwapi.bits(b)), seed
        assert np.any(a != 0), seed
