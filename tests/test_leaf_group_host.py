"""CPU tier: grouped calls (k_leaf_group_lazy), the host's side, on the host-only harness.

A grouped call changes NO launch the host makes: launch_leaf_sum_lazy gets a mark in its FusedView, launch_root_out one in its RootArgs,
and the launch stubs count both as before.  So for every graph below the launches() of a context created under FWGPU_LEAF_GROUP=1 equal
those of its twin created under FWGPU_LEAF_GROUP=0, violation() stays "", and group_stats() says which batches carried the mark: the
lazy ones of an eligible bank (tree = leaves -> root -> stereo out, K x pieces at or above the size rule), none anywhere else."""
import contextlib
import os

import numpy as np
import pytest

from fwapi import LOOP_FULL, PLANAR_F32, HostOnlyEngine

MBF, KB = 64, 8


@contextlib.contextmanager
def group_env(on, min_items=1):
    keys = {"FWGPU_LEAF_GROUP": "1" if on else "0", "FWGPU_LEAF_GROUP_MIN": str(min_items)}
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


def graph(e, kind):
    """12 voices (source -> volume -> pan) under 3 leaf mixers under a root; `kind` says what is different"""
    smp = e.new_sample(PLANAR_F32, 2, np.zeros((2, 4 * MBF), np.float32)) if kind == "resampler" else None
    ends, samplers = [], []
    for v in range(12):
        if kind == "resampler":
            cur = e.resampler(smp, 1.25, loop=True, playing=True)
        else:
            cur = e.sampler(90.0)
            samplers.append(cur)
        if kind == "chain":
            b = e.biquad(0, 1000.0 + 10 * v, 0.7)
            d = e.delay(0.01, feedback=0.2, mix=0.5)
            e.connect_stereo(cur, b)
            e.connect_stereo(b, d)
            cur = d
        vol, pan = e.volume(50.0 + v), e.pan(0.1 * (v % 5) - 0.2)
        e.connect_stereo(cur, vol)
        e.connect_stereo(vol, pan)
        ends.append(pan)

    def mixer(ins):
        m = e.sum(max(2, len(ins)))
        for p, n in enumerate(ins):
            e.connect_stereo(n, m, 2 * p)
        return m

    leaves = [mixer(ends[k:k + 4]) for k in range(0, 12, 4)]
    if kind == "third_level":
        top = mixer([mixer(leaves[:2]), leaves[2]])
    elif kind == "send":  # the leaves' buses are read twice: dry by the root and through a send bus with a filter on it
        bq = e.biquad(0, 2500.0)
        e.connect_stereo(mixer(leaves[:2]), bq)
        top = mixer(leaves + [bq])
    else:
        top = mixer(leaves)
    if kind == "master":
        mv = e.volume(80.0)
        e.connect_stereo(top, mv)
        top = mv
    e.connect_stereo(top, e.graph_out_node)
    e.update()
    for s in samplers:
        e.sampler_set_sample(s, e.new_sample(PLANAR_F32, 2, np.zeros((2, 4 * MBF), np.float32)))
        e.sampler_set_loop_range(s, LOOP_FULL)
        e.sampler_play(s)


def run(kind, on, min_items=1, k=KB):
    with group_env(on, min_items):
        e = HostOnlyEngine(max_block_frames=MBF, max_batch=KB)
    graph(e, kind)
    e.reset_launches()
    for _ in range(5):  # messages, the call behind them, then three quiet calls
        e.process_blocks(k)
    assert e.violation() == "", (kind, on, e.violation())
    return e.cx.plan_kind(), e.launches(), e.cx.lazy_stats(), e.cx.group_stats()


PLAN = dict(bank=1, master=1, third_level=1, send=3, resampler=1, chain=2)


@pytest.mark.parametrize("kind", list(PLAN))
def test_only_an_eligible_bank_is_grouped_and_the_launches_do_not_change(kind):
    plan_on, launches_on, lazy_on, grouped_on = run(kind, True)
    plan_off, launches_off, lazy_off, grouped_off = run(kind, False)
    assert plan_on == plan_off == PLAN[kind]
    assert launches_on == launches_off and lazy_on == lazy_off, (launches_on, launches_off, lazy_on, lazy_off)
    assert grouped_off == 0
    if os.environ.get("FWGPU_LAZY") == "0":
        assert grouped_on == 0
    elif kind == "bank":
        assert grouped_on == lazy_on[0] == 3 and launches_on["root_out"] == 5 and launches_on["leaf_sum"] == 5, (grouped_on, lazy_on, launches_on)
    else:
        assert grouped_on == 0, (kind, grouped_on)
    # the ineligible twins of the bank launch what the bank launches wherever they share the path (leaf_sum: once per batch)
    if kind in ("master", "third_level"):
        assert launches_on["leaf_sum"] == run("bank", True)[1]["leaf_sum"]


def test_the_size_rule():
    """K x pieces below the rule: today's two kernels (no mark), at the rule: grouped.  Blocks of 64 frames are one piece each."""
    if os.environ.get("FWGPU_LAZY") == "0":
        return  # (no lazy calls in this run: nothing to group)
    assert run("bank", True, min_items=KB + 1)[3] == 0
    assert run("bank", True, min_items=KB)[3] == 3
    assert run("bank", True, min_items=KB, k=KB - 1)[3] == 0
    assert run("bank", True, min_items=KB)[1] == run("bank", True, min_items=KB + 1)[1]


def test_the_switch_default_and_its_stats_entry():
    """a context created without the variable takes the library's default; the entry point tolerates a NULL result pointer"""
    saved = os.environ.pop("FWGPU_LEAF_GROUP", None)
    try:
        e = HostOnlyEngine(max_block_frames=MBF, max_batch=KB)
    finally:
        if saved is not None:
            os.environ["FWGPU_LEAF_GROUP"] = saved
    assert e.cx.group_stats() == 0
    assert e.cx.L.fwgpu_plan_group_stats(e.cx.c, None) == 0
