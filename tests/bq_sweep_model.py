"""The biquad's coefficient sweep (fwgpu_biquad_sweep, CMD_BQ_SWEEP = 25; SPEC) restated in numpy: the state
machine (`Sweep`), c(j) in np.float32 operations — one separately rounded operation after the other, the division IEEE — and the
Direct-Form-I filter with `fma32` as tests/refmodel.py's BiquadNode writes it, each frame with its own five values
(`SweepBiquadNode`).  `SweepRefEngine` is a RefEngine that builds that node; `Tagged` delivers messages tagged with a block, as
scenarios.TaggedOracle does; `GpuSweep` adds `sweep` to a GpuEngine / HostOnlyEngine (tests/fwapi.py is not to change).  Nothing here
comes from the product.  tests/test_bq_sweep.py uses all of it."""
import numpy as np

import fwapi
import refmodel
import scenarios
from refmodel import f32, fma32, rbj_coefs

FRAMES_MAX = 1 << 24
CMD_SET_COEFS = 4
CMD_BQ_SWEEP = 25


def coef_values(A, T, N, k, js, rest):
    """c_i(j) of the SPEC for one coordinate and the frames `js` ahead (an integer array): rest, T, or the clamped interpolation.
    f32(k + j) and f32(N) are exact (both <= 2^24)."""
    js = np.asarray(js, dtype=np.int64)
    if N == 0:
        return np.full(js.shape, f32(rest), dtype=f32)
    A, T = f32(A), f32(T)
    t = k + js
    inside = t < N
    d = f32(T - A)
    with np.errstate(all="ignore"):
        u = (np.minimum(t, N).astype(f32) / f32(N)).astype(f32)
        v = (A + (d * u).astype(f32)).astype(f32)
    v = np.minimum(np.maximum(v, min(A, T)), max(A, T)).astype(f32)
    return np.where(inside, v, T).astype(f32)


class Sweep(object):
    """the SPEC's state and its moves: the message, CMD_SET_COEFS, "behind a rendered block" """

    def __init__(self, head):
        self.head = np.array(head, dtype=f32)      # the five at the head of the ext slice: the coefficients at rest
        self.A = np.zeros(5, dtype=f32)
        self.T = np.zeros(5, dtype=f32)
        self.N = self.k = 0

    def at_rest(self):
        return self.N == 0

    def values(self, frames):
        """[frames][5]: the five coefficients of each of the next `frames` frames"""
        js = np.arange(frames)
        return np.stack([coef_values(self.A[i], self.T[i], self.N, self.k, js, self.head[i]) for i in range(5)], axis=1)

    def start(self, T, frames):
        assert 0 <= frames <= FRAMES_MAX
        T = np.array(T, dtype=f32)
        if frames == 0:
            self.set_coefs(T)
            return
        self.A = self.values(1)[0]                 # a retarget in mid-sweep continues from where the sweep stands
        self.T, self.N, self.k = T, int(frames), 0

    def set_coefs(self, co):
        self.head = np.array(co, dtype=f32)
        self.N = self.k = 0

    def advance(self, frames):
        if self.N == 0:
            return
        self.k += frames
        if self.k >= self.N:
            self.head = self.T.copy()
            self.N = self.k = 0


def filter_rows(x, C, st):
    """rows of (node, channel): x [rows][frames], C [rows][frames][5], st [rows][4] = x1 x2 y1 y2 (updated in place) -> y.
    ff = ((b0*x) + (b1*x1)) + (b2*x2); y = fma(-a1, y1, fma(-a2, y2, ff)), frame n with C[:, n]; ONE time loop for all rows"""
    x = np.asarray(x, dtype=f32)
    frames = x.shape[1]
    xp1 = np.concatenate([st[:, 0:1], x[:, :-1]], axis=1)
    xp2 = np.concatenate([st[:, 1:2], st[:, 0:1], x[:, :-2]], axis=1) if frames >= 2 else st[:, 1:2].copy()
    ff = (((C[:, :, 0] * x).astype(f32) + (C[:, :, 1] * xp1).astype(f32)).astype(f32) + (C[:, :, 2] * xp2).astype(f32)).astype(f32)
    na1, na2 = (-C[:, :, 3]).astype(f32), (-C[:, :, 4]).astype(f32)
    y = np.empty_like(x)
    y1, y2 = st[:, 2].copy(), st[:, 3].copy()
    for i in range(frames):
        yi = fma32(na1[:, i], y1, fma32(na2[:, i], y2, ff[:, i]))
        y[:, i] = yi
        y2, y1 = y1, yi
    st[:, 1] = x[:, frames - 2] if frames >= 2 else st[:, 0]
    st[:, 0] = x[:, frames - 1]
    st[:, 2], st[:, 3] = y1, y2
    return y


class SweepBiquadNode(refmodel.BiquadNode):
    def __init__(self, eng, n_in, n_out, params):
        refmodel.BiquadNode.__init__(self, eng, n_in, n_out, params)
        self.sw = Sweep(self.co)

    def set_param(self, param, value):
        refmodel.BiquadNode.set_param(self, param, value)
        self.sw.set_coefs(self.co)   # CMD_SET_COEFS during a sweep ends it

    def sweep(self, cutoff_hz, q, frames):
        self.cutoff, self.q = f32(cutoff_hz), f32(q)   # a later set_param of Q alone starts from these
        self.co = rbj_coefs(self.ftype, self.cutoff, self.q, self.sr)
        self.sw.start(self.co, frames)

    @staticmethod
    def process_batch(items, frames):
        """items: [(node, ins, outs)] — every biquad of one schedule level, their channels side by side (RefEngine._block)"""
        rows = [(n, c, ins[c], outs[c]) for (n, ins, outs) in items for c in range(n.nch)]
        if not rows:
            return
        tabs = {id(n): n.sw.values(frames) for (n, _, _) in items}
        C = np.stack([tabs[id(r[0])] for r in rows])
        st = np.array([r[0].st[r[1]] for r in rows], dtype=f32)
        y = filter_rows(np.stack([r[2][:frames] for r in rows]), C, st)
        for k, (n, c, _, out) in enumerate(rows):
            out[:frames] = y[k]
            n.st[c] = st[k]
        for (n, _, _) in items:
            n.sw.advance(frames)

    def process(self, frames, ins, outs, in_mask):
        SweepBiquadNode.process_batch([(self, ins, outs)], frames)
        return 0


class SweepRefEngine(refmodel.RefEngine):
    def add_node(self, kind, n_in, n_out, params=()):
        if kind == fwapi.BIQUAD:
            return self._add(SweepBiquadNode(self, n_in, n_out, [float(p) for p in params]))
        return refmodel.RefEngine.add_node(self, kind, n_in, n_out, params)

    def sweep(self, node, cutoff_hz, q, frames, at_block=0):
        assert at_block == 0
        self.nodes[node].sweep(cutoff_hz, q, int(frames))

    def _block(self, *a):
        # (RefEngine._block hands a level's biquads to refmodel.BiquadNode.process_batch by name: for the length of a block that name
        #  is the sweeping one)
        saved = refmodel.BiquadNode.__dict__["process_batch"]
        refmodel.BiquadNode.process_batch = staticmethod(SweepBiquadNode.process_batch)
        try:
            return refmodel.RefEngine._block(self, *a)
        finally:
            refmodel.BiquadNode.process_batch = saved

    def node_process(self, node, frames, inputs, n_out):
        """one block of ONE node on the caller's buffers (fwgpu_node_process)"""
        n = self.nodes[node]
        outs = [np.zeros(frames, dtype=f32) for _ in range(n_out)]
        n.process(frames, [np.asarray(i, dtype=f32) for i in inputs], outs, 0)
        return np.stack(outs)


class Tagged(scenarios.TaggedOracle):
    """messages tagged with a block of the next call, the sweep among them"""

    def sweep(self, node, cutoff_hz, q, frames, at_block=0):
        self._defer(at_block, self.e.sweep, node, cutoff_hz, q, frames)


class GpuSweep(object):
    """a GpuEngine (or the host-only harness engine) with the sweep message under the same name"""

    def __init__(self, eng):
        self.e = eng

    def __getattr__(self, name):
        return getattr(self.e, name)

    def sweep(self, node, cutoff_hz, q, frames, at_block=0):
        self.e._chk(self.e.cx.L.fwgpu_biquad_sweep(self.e.cx.c, node, cutoff_hz, q, frames, at_block))
