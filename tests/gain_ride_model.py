"""The gain ride of a volume or a pan node (fwgpu_gain_ride, CMD_GAIN_RIDE = 27; SPEC) restated over
tests/refmodel.py: `RideVolumeNode` and `RidePanNode` add the ride to the numpy VolumeNode / PanNode — `np.float32` operations one at a
time — and `RideRefEngine` is a RefEngine that builds them, with the message and with the graph-output silence flags of a run of blocks.
`Tagged` delivers messages tagged with a block, as scenarios.TaggedOracle does.  `curve_y` and `ride_values` are the SPEC's arithmetic
on plain arrays, for the tests that hold the g++ build of fwgpu_types.h gain_ride_* against them.  Everything else is refmodel's.
tests/test_gain_ride.py uses all of them."""
import numpy as np

import fwapi
import refmodel
import scenarios
from refmodel import ACTIVE, F0, INACTIVE, all_silent, clear_all_outputs, f32, pan_gains, percent_volume_to_raw_gain

FRAMES_MAX = 1 << 24
XF_ITERS = 24
CMD_SET_P0, CMD_SET_P1, CMD_GAIN_RIDE = 0, 1, 27
LINEAR, BEZIER = 0, 1
EASE = (0.42, 0.0, 0.58, 1.0)
OVERSHOOT = (0.3, -0.5, 0.7, 1.8)


def _bezier(t, a, d):
    """B(t; a, d) = ((q*t + b)*t + c)*t with c = 3*a; b = 3*(d - a) - c; q = (1 - c) - b: float32, one rounding per operation"""
    a, d = f32(a), f32(d)
    c = f32(3.0) * a
    b = f32(3.0) * (d - a) - c
    q = (f32(1.0) - c) - b
    return ((q * t + b) * t + c) * t


def curve_y(u, curve):
    """y(u) of the SPEC for a float32 array u: u itself for the linear shape (curve None), else the crossfader's solver"""
    u = np.asarray(u, dtype=f32)
    if curve is None:
        return u
    x1, y1, x2, y2 = curve
    lo, hi = np.zeros_like(u), np.ones_like(u)
    for _ in range(XF_ITERS):
        m = (lo + hi) * f32(0.5)
        below = _bezier(m, x1, x2) < u
        lo, hi = np.where(below, m, lo), np.where(below, hi, m)
    return np.where(u == 0, f32(0.0), _bezier((lo + hi) * f32(0.5), y1, y2)).astype(f32)


def ride_values(G0, G1, N, k, n, curve=None):
    """ride(0) .. ride(n - 1) of a ride G0 -> G1 over N frames of which k are rendered: a float32 array"""
    G0, G1 = f32(G0), f32(G1)
    out = np.full(n, G1, dtype=f32)
    t = k + np.arange(n, dtype=np.int64)
    live = (t < N) if N else np.zeros(n, dtype=bool)
    if not live.any():
        return out
    with np.errstate(all="ignore"):
        u = t[live].astype(f32) / f32(N)                  # both exact in f32 (<= 2^24)
        d = f32(G1 - G0)                                  # computed once
        v = (G0 + (d * curve_y(u, curve))).astype(f32)
    lo, hi = (G0, G1) if G0 < G1 else (G1, G0)
    out[live] = np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(f32)
    return out


def ride_value(G0, G1, N, k, curve=None):
    return ride_values(G0, G1, N, k, 1, curve)[0]


def _curve32(curve):
    return None if curve is None else tuple(f32(v) for v in curve)


class _Ride(object):
    """the SPEC's state of one node: the gains' smoothers and targets come from the node (`_gains`: [(smoother, target)], `_set_targets`)"""

    def _ride_init(self):
        self.N = self.k = 0
        self.G0 = [F0, F0]
        self.curve = None

    def _now(self):
        """per gain the value in force at the next block's first frame"""
        out = []
        for c, (sm, G1) in enumerate(self._gains()):
            if self.N:
                out.append(ride_value(self.G0[c], G1, self.N, self.k, self.curve))
            else:
                out.append(sm.last_output if sm.status == ACTIVE else sm.input)
        return out

    @staticmethod
    def _rest(sm, val):
        sm.status = INACTIVE
        sm.input = sm.last_output = f32(val)
        sm.output[:] = f32(val)

    def _end_ride(self):
        """param 0 in a ride: the smoothers are reset to the ride's current values and glide on from there"""
        if self.N == 0:
            return
        for (sm, _), g in zip(self._gains(), self._now()):
            self._rest(sm, g)
        self._ride_init()

    def ride(self, value, frames, curve=None):
        assert 0 <= frames <= FRAMES_MAX
        now = self._now()
        self._set_targets(value)
        for sm, G1 in self._gains():                       # at rest at the targets, coefficients untouched
            self._rest(sm, G1)
        self._ride_init()
        if frames == 0:                                    # a step: the hard set
            return
        self.G0 = [f32(g) for g in now] + [F0] * (2 - len(now))
        self.N, self.k, self.curve = int(frames), 0, _curve32(curve)

    def _block_gains(self, frames):
        """the gains of this block's frames, then k += frames"""
        g = [ride_values(self.G0[c], G1, self.N, self.k, frames, self.curve) for c, (_, G1) in enumerate(self._gains())]
        self.k += frames
        if self.k >= self.N:                               # at rest: a node set to the target whose smoother has settled
            self._ride_init()
        return g


class RideVolumeNode(refmodel.VolumeNode, _Ride):
    def __init__(self, eng, n_in, n_out, params):
        refmodel.VolumeNode.__init__(self, eng, n_in, n_out, params)
        self._ride_init()

    def _gains(self):
        return [(self.smoother, self.raw_gain)]

    def _set_targets(self, value):
        self.raw_gain = percent_volume_to_raw_gain(value)

    def set_param(self, param, value):
        self._end_ride()
        refmodel.VolumeNode.set_param(self, param, value)

    def process(self, frames, ins, outs, in_mask):
        if self.N == 0:
            return refmodel.VolumeNode.process(self, frames, ins, outs, in_mask)
        (g,) = self._block_gains(frames)                   # silent input or not
        if all_silent(in_mask, len(ins)):
            return clear_all_outputs(frames, outs)
        with np.errstate(all="ignore"):                    # (no mute test inside a ride)
            if len(ins) == 2 and len(outs) == 2:
                outs[0][:frames] = ins[0][:frames] * g
                outs[1][:frames] = ins[1][:frames] * g
                return in_mask
            for i in range(min(len(ins), len(outs))):
                outs[i][:frames] = F0 if (in_mask >> i) & 1 else ins[i][:frames] * g
        return in_mask


class RidePanNode(refmodel.PanNode, _Ride):
    def __init__(self, eng, n_in, n_out, params):
        refmodel.PanNode.__init__(self, eng, n_in, n_out, params)
        self._ride_init()

    def _gains(self):
        return [(self.sl, self.gl), (self.sr_, self.gr)]

    def _set_targets(self, value):
        self.gl, self.gr = pan_gains(value)

    def set_param(self, param, value):
        self._end_ride()
        refmodel.PanNode.set_param(self, param, value)

    def process(self, frames, ins, outs, in_mask):
        if self.N == 0:
            return refmodel.PanNode.process(self, frames, ins, outs, in_mask)
        gl, gr = self._block_gains(frames)
        if all_silent(in_mask, len(ins)):
            return clear_all_outputs(frames, outs)
        with np.errstate(all="ignore"):
            outs[0][:frames] = ins[0][:frames] * gl
            outs[1][:frames] = ins[1][:frames] * gr
        return in_mask


NODE_CLASSES = {fwapi.VOLUME: RideVolumeNode, fwapi.STEREO_PAN: RidePanNode}


class RideRefEngine(refmodel.RefEngine):
    def add_node(self, kind, n_in, n_out, params=()):
        if kind in NODE_CLASSES:
            return self._add(NODE_CLASSES[kind](self, n_in, n_out, [float(p) for p in params]))
        return refmodel.RefEngine.add_node(self, kind, n_in, n_out, params)

    def ride(self, node, value, frames, curve=None, at_block=0):
        assert at_block == 0
        self.nodes[node].ride(f32(value), int(frames), curve)

    def process_blocks_flags(self, k, n_out_ch=2):
        """(interleaved output, bool [k][n_out_ch]: the graph output channel is flagged silent in that block)"""
        mbf = self.max_block_frames
        out = np.zeros(k * mbf * n_out_ch, dtype=f32)
        fl = np.zeros((k, n_out_ch), dtype=bool)
        gout = [p for p in self.plan if p[0] == self.graph_out_node][0]
        for b in range(k):
            self._block(mbf, np.zeros(0, dtype=f32), 0, out[b * mbf * n_out_ch:(b + 1) * mbf * n_out_ch], n_out_ch)
            fl[b] = [bool(self.flags[gout[2][c]]) for c in range(n_out_ch)]
        return out, fl


class Tagged(scenarios.TaggedOracle):
    """messages tagged with a block of the next call, the ride among them"""

    def ride(self, node, value, frames, curve=None, at_block=0):
        self._defer(at_block, self.e.ride, node, value, frames, curve)

    def process_blocks_flags(self, k, n_out_ch=2):
        outs, fls = [], []
        for b in range(k):
            keep = []
            for at, fn, a in self.q:
                if at == b:
                    fn(*a)
                elif at > b:
                    keep.append((at, fn, a))
            self.q = keep
            o, f = self.e.process_blocks_flags(1, n_out_ch)
            outs.append(o)
            fls.append(f)
        self.q = [(at - k, fn, a) for at, fn, a in self.q]
        return np.concatenate(outs), np.concatenate(fls)


class GpuRide(object):
    """a GpuEngine (or the host-only harness engine) with the ride message under the same name"""

    def __init__(self, eng):
        self.e = eng

    def __getattr__(self, name):
        return getattr(self.e, name)

    def ride(self, node, value, frames, curve=None, at_block=0):
        shape, (x1, y1, x2, y2) = (LINEAR, (0.0, 0.0, 1.0, 1.0)) if curve is None else (BEZIER, curve)
        self.e._chk(self.e.cx.L.fwgpu_gain_ride(self.e.cx.c, node, value, frames, shape, x1, y1, x2, y2, at_block))
