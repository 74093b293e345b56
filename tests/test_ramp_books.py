"""The host's three ramp books held together: biquad sweeps, spatialiser moves and gain rides each keep a
count of the frame behind which no ramp sent so far is in flight, and a flag that says whether the call just rendered could meet one.

CPU tier only, on the host-only harness: the books are a function of the messages and of the frames rendered, and of nothing on the
device.  Every figure below is worked out by hand from frames_done, at_block * F and N; the books are read through the three peek
functions of tests/test_bq_sweep.py, tests/test_sp_move.py and tests/test_gain_ride.py.

The graph: a voice bank (sampler -> spatialiser, sampler -> volume, a plain sampler) under one mixer, a biquad behind the mixer."""
import ctypes as C
import os

import numpy as np

import fwapi
import test_bq_sweep as t_sweep
import test_gain_ride as t_ride
import test_sp_move as t_move
from fwapi import LOOP_FULL, PLANAR_F32, HostOnlyEngine
from scenarios import voice_source

F, K = 64, 4
CALL = K * F
PIN = (1 << 64) - 1
ULL = C.c_ulonglong
LAZY = os.environ.get("FWGPU_LAZY") != "0"


class Bank(object):
    def __init__(self):
        e = self.e = HostOnlyEngine(max_block_frames=F, max_batch=K)
        self.samplers = [e.sampler(90.0 - 7 * v) for v in range(3)]
        self.sp = e.spatial(1.0, 0.0, -2.0, n_in=2)
        self.vol = e.volume(70.0)
        self.mixer = e.sum(3)
        self.bq = e.biquad(0, 1200.0, 2.0)
        e.connect_stereo(self.samplers[0], self.sp)
        e.connect_stereo(self.samplers[1], self.vol)
        for p, n in enumerate((self.sp, self.vol, self.samplers[2])):
            e.connect_stereo(n, self.mixer, 2 * p)
        e.connect_stereo(self.mixer, self.bq)
        e.connect_stereo(self.bq, e.graph_out_node)
        e.update()
        for v, s in enumerate(self.samplers):
            e.sampler_set_sample(s, e.new_sample(PLANAR_F32, 2, voice_source(5100 + v, 8 * F, 2)))
            e.sampler_set_loop_range(s, LOOP_FULL)
            e.sampler_play(s)
        assert e.cx.plan_kind() == 1 and e.cx.plan_fused_voices() == 3
        for _ in range(3):                                   # the set-up messages and their glides are behind us
            self.call()
        self.done = 3 * CALL
        assert self.books() == ([self.done, 0, 0], [self.done, 0, 0], [self.done, 0, 0, 0, 0])

    def call(self):
        """one process call of K blocks -> what it added to (lazy calls, control calls)"""
        a = self.e.cx.lazy_stats()
        self.e.process_blocks(K)
        b = self.e.cx.lazy_stats()
        return (b[0] - a[0], b[1] - a[1])

    def books(self):
        """(sweep: frames done, until, live), (move: the same), (ride: frames done, until, live, max_n, parked_n)"""
        c = self.e.cx.c
        s, m, r = (ULL * 3)(), (ULL * 3)(), (ULL * 5)()
        t_sweep._peek_lib().bsp_sweep_book(c, s)
        t_move.peek().spp_move_book(c, m)
        t_ride.peek().grp_ride_book(c, r)
        return list(s), list(m), list(r)

    def sweep(self, frames, at_block=0):
        assert self.e.cx.L.fwgpu_biquad_sweep(self.e.cx.c, self.bq, 5000.0, 3.0, frames, at_block) == 0

    def move(self, frames, at_block=0):
        assert self.e.cx.L.fwgpu_spatial_move(self.e.cx.c, self.sp, 4.0, 0.0, -0.5, frames, at_block) == 0

    def ride(self, frames, at_block=0, value=20.0):
        assert self.e.cx.L.fwgpu_gain_ride(self.e.cx.c, self.vol, value, frames, 1, 0.42, 0.0, 0.58, 1.0, at_block) == 0

    def node_block(self, node):
        """fwgpu_node_process: ONE node renders one block on its own"""
        self.e.node_process(node, F, [np.zeros(F, dtype=np.float32), np.zeros(F, dtype=np.float32)], 2)

    def close(self):
        assert self.e.violation() == ""


def _expect_lazy(got, live, sp_in_plan=True):
    """a bank that holds a spatialiser keeps its control kernel in every call (it makes no lazy records); without one, a call that may
    meet a ramp runs its control kernel and a quiet call behind a quiet call is lazy"""
    if LAZY:
        assert got == ((0, 1) if live or sp_in_plan else (1, 0)), (got, live, sp_in_plan)


def test_a_sweep_a_move_and_a_ride_sent_in_one_call_close_their_books_in_three_different_later_calls():
    b = Bank()
    D0 = b.done
    _expect_lazy(b.call(), False)                            # call 0: quiet
    D1 = D0 + CALL
    assert b.books() == ([D1, 0, 0], [D1, 0, 0], [D1, 0, 0, 0, 0])
    Ns, Nm, Nr = CALL + 5, 2 * CALL + 9, 3 * CALL + 7
    b.sweep(Ns, at_block=0)                                  # sent in front of call 1, which starts at frame D1
    b.move(Nm, at_block=1)
    b.ride(Nr, at_block=2)
    s_end, m_end, r_end = D1 + 0 * F + Ns, D1 + 1 * F + Nm, D1 + 2 * F + Nr
    # the calls' first frames are D1, D1 + CALL, ...: the sweep ends inside call 2, the move inside call 3, the ride inside call 4
    assert D1 + CALL < s_end < D1 + 2 * CALL < m_end < D1 + 3 * CALL < r_end < D1 + 4 * CALL
    for call in range(1, 8):
        start = D0 + call * CALL
        got = b.call()
        sl, ml, rl = int(start < s_end), int(start < m_end), int(start < r_end)
        assert (sl, ml, rl) == {1: (1, 1, 1), 2: (1, 1, 1), 3: (0, 1, 1), 4: (0, 0, 1)}.get(call, (0, 0, 0))
        assert b.books() == ([start + CALL, s_end, sl], [start + CALL, m_end, ml], [start + CALL, r_end, rl, Nr if rl else 0, 0]), call
        _expect_lazy(got, sl or ml or rl)
    b.close()


def test_a_ride_step_on_its_own_opens_the_ride_book_for_its_call_alone_and_the_other_books_stay_shut():
    b = Bank()
    D = b.done
    b.ride(0, at_block=1)                                    # 0 frames: a step, applied one block into the call
    until = D + 1 * F + 0
    _expect_lazy(b.call(), True)
    assert b.books() == ([D + CALL, 0, 0], [D + CALL, 0, 0], [D + CALL, until, 1, 0, 0])
    b.call()                                                 # (the call behind a message call renders its glides: not asserted lazy)
    assert b.books() == ([D + 2 * CALL, 0, 0], [D + 2 * CALL, 0, 0], [D + 2 * CALL, until, 0, 0, 0])
    _expect_lazy(b.call(), False)
    b.ride(0, at_block=0)                                    # at block 0 the bound is the call's first frame: the step alone opens the book
    until = D + 3 * CALL + 0 * F + 0
    _expect_lazy(b.call(), True)
    assert b.books()[2] == [D + 4 * CALL, until, 1, 0, 0]
    b.call()
    assert b.books()[2] == [D + 5 * CALL, until, 0, 0, 0]
    b.close()


def test_node_process_pins_the_book_of_its_kind_and_a_ride_step_pins_nothing():
    for kind in ("sweep", "move", "ride", "step"):
        b = Bank()
        D = b.done
        if kind == "sweep":
            b.sweep(100)
            b.node_block(b.bq)
        elif kind == "move":
            b.move(100)
            b.node_block(b.sp)
        else:
            b.ride(100 if kind == "ride" else 0)
            b.node_block(b.vol)
        # the ramp moves with that node's own calls from here on: no frame count bounds it (a step is over when it is applied)
        pin = {"sweep": (PIN, 0, 0), "move": (0, PIN, 0), "ride": (0, 0, PIN), "step": (0, 0, 0)}[kind]
        assert b.books() == ([D, pin[0], 0], [D, pin[1], 0], [D, pin[2], 0, 0, 0]), kind
        for call in range(1, 3):
            _expect_lazy(b.call(), kind != "step")
            live = [int(p == PIN) for p in pin]
            assert b.books() == ([D + call * CALL, pin[0], live[0]], [D + call * CALL, pin[1], live[1]],
                                 [D + call * CALL, pin[2], live[2], 0, 0]), (kind, call)
        b.close()


def test_a_spatialiser_and_a_volume_that_leave_in_mid_ramp_are_parked_and_open_their_books_again_when_they_return():
    b = Bank()
    e, D = b.e, b.done
    Nm, Nr = 10 * F, 11 * F
    b.move(Nm)
    b.ride(Nr)
    _expect_lazy(b.call(), True)
    D += CALL
    assert b.books() == ([D, 0, 0], [D, D - CALL + Nm, 1], [D, D - CALL + Nr, 1, Nr, 0])
    for port in (0, 1):
        e.disconnect(b.sp, port, b.mixer, 0 + port)
        e.disconnect(b.vol, port, b.mixer, 2 + port)
    e.update()                                               # both leave the plan with more than a call of their ramps to go
    # the install parks the longest ramp noted and counts its whole length from here: the node may come back where it stood
    m_until, r_until = D + Nm, D + Nr
    assert m_until > D - CALL + Nm and r_until > D - CALL + Nr
    for call in range(4):
        start = D + call * CALL
        got = b.call()
        ml, rl = int(start < m_until), int(start < r_until)
        assert (ml, rl) == [(1, 1), (1, 1), (1, 1), (0, 0)][call]
        assert b.books() == ([start + CALL, 0, 0], [start + CALL, m_until, ml], [start + CALL, r_until, rl, Nr if rl else 0, Nr]), call
        assert got[0] == 0 or not (ml or rl)                  # whatever plan the rest of the graph makes: no lazy call while a book is open
    D += 4 * CALL
    e.connect_stereo(b.sp, b.mixer, 0)
    e.connect_stereo(b.vol, b.mixer, 2)
    e.update()                                               # the install that brings them back opens both books again, for N frames each
    m_until, r_until = D + Nm, D + Nr
    for call in range(4):
        start = D + call * CALL
        b.call()
        ml, rl = int(start < m_until), int(start < r_until)
        assert (ml, rl) == [(1, 1), (1, 1), (1, 1), (0, 0)][call]
        assert b.books() == ([start + CALL, 0, 0], [start + CALL, m_until, ml], [start + CALL, r_until, rl, 0, Nr]), call
    _expect_lazy(b.call(), False)
    b.close()
