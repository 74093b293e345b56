"""The spatialiser's move (fwgpu_spatial_move, CMD_SP_MOVE = 26; SPEC) restated over tests/refmodel.py:
`MoveSpatialNode` adds the move to the numpy SpatialNode — Python / int64 integers for the 32.32 delays D, `np.float32` operations one
at a time for the gains and the two-tap blend — and `MoveRefEngine` is a RefEngine that builds it, with the message and with the
graph-output silence flags of a run of blocks.  `Tagged` delivers messages tagged with a block, as scenarios.TaggedOracle does.
`start`, `gain_value`, `delay_value`, `iterate` and `tap` are the SPEC's arithmetic on plain numbers, for the tests that hold the closed
form against the iteration and the g++ build of fwgpu_types.h sp_move_* against both.  tests/test_sp_move.py uses all of them."""
import numpy as np

import fwapi
import refmodel
import scenarios
from refmodel import ACTIVE, F0, INACTIVE, SP_HIST, f32, spatial_params

M64 = (1 << 64) - 1
FRAMES_MAX = 1 << 24
CMD_SET_P0, CMD_SET_P1, CMD_SP_ITD, CMD_SP_MOVE = 0, 1, 22, 26
TWO_M24 = f32(2.0 ** -24)


def trunc_div(a, b):
    """C++ signed division: truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def start(D0, d1, N):
    """the message's integer half for one ear: the signed step per frame from the 32.32 delay D0 to d1 whole frames over N frames"""
    assert 0 < N <= FRAMES_MAX and 0 <= d1 <= 63 and 0 <= D0 <= 63 << 32
    return trunc_div((d1 << 32) - D0, N)


def gain_value(G0, G1, N, t):
    """the gain of frame t of a move G0 -> G1 over N frames: every operation a separately rounded f32 operation"""
    G0, G1 = f32(G0), f32(G1)
    if t >= N:
        return G1
    with np.errstate(all="ignore"):
        v = f32(G0 + f32(f32(G1 - G0) * f32(f32(t) / f32(N))))
    lo, hi = (G0, G1) if G0 < G1 else (G1, G0)
    return lo if v < lo else (hi if v > hi else v)


def delay_value(D0, inc, d1, N, t):
    """the 32.32 delay of frame t, in wrapping u64 arithmetic; behind the move exactly d1 << 32"""
    return d1 << 32 if t >= N else (D0 + t * inc) & M64


def iterate(D0, inc, d1, N, n):
    """n frames, one at a time -> the delays of the frames"""
    at, D, left = [], D0, N
    for _ in range(n):
        at.append(D)
        if left > 0:
            D = (D + inc) & M64
            left -= 1
            if left == 0:
                D = d1 << 32
    return at


def whole_frac(D):
    return D >> 32, f32((D & 0xffffffff) >> 8) * TWO_M24


def tap(a, b, D):
    """x of a frame whose first tap is a and whose second tap (the frame before it) is b"""
    _, f = whole_frac(D)
    if f == 0:
        return f32(a)
    with np.errstate(all="ignore"):
        return f32(f32(a) + f32(f32(f32(b) - f32(a)) * f))


class MoveSpatialNode(refmodel.SpatialNode):
    def __init__(self, eng, n_in, n_out, params):
        refmodel.SpatialNode.__init__(self, eng, n_in, n_out, params)
        self.N = self.k = 0
        self.G0 = [F0, F0]
        self.D = [0, 0]              # the 32.32 delays at the next block's first frame (in a move)
        self.inc = [0, 0]

    def _smoothers(self):
        return (self.sl, self.sr_)

    def _now(self):
        """per ear (gain in force, 32.32 delay) at the next block's first frame"""
        out = []
        for e, (sm, G1, d) in enumerate(zip(self._smoothers(), (self.gl, self.gr), (self.dl, self.dr))):
            if self.N:
                out.append((gain_value(self.G0[e], G1, self.N, self.k), self.D[e]))
            else:
                out.append((sm.last_output if sm.status == ACTIVE else sm.input, d << 32))
        return out

    def _end_move(self):
        """a plain set_position in a move: the smoothers continue from the move's current gains, the delays step"""
        if self.N == 0:
            return
        for sm, (g, _) in zip(self._smoothers(), self._now()):
            sm.last_output = f32(g)
        self.N = self.k = 0

    def set_param(self, param, value):
        self._end_move()
        refmodel.SpatialNode.set_param(self, param, value)

    def move(self, x, y, z, frames):
        self.xyz_target = [f32(x), f32(y), f32(z)]
        gl, gr, dl, dr = spatial_params(x, y, z, sample_rate=self.sr)
        if frames == 0:              # a step: params 0, 1 and 2
            self._end_move()
            self.xyz = list(self.xyz_target)
            self.gl, self.gr, self.dl, self.dr = gl, gr, dl, dr
            return
        assert 0 < frames <= FRAMES_MAX
        now = self._now()
        for sm, g in zip(self._smoothers(), (gl, gr)):       # at rest at the target, coefficients untouched
            sm.status = INACTIVE
            sm.input = sm.last_output = f32(g)
            sm.output[:] = f32(g)
        self.xyz = list(self.xyz_target)
        self.gl, self.gr, self.dl, self.dr = gl, gr, dl, dr
        self.G0 = [f32(now[0][0]), f32(now[1][0])]
        self.D = [now[0][1], now[1][1]]
        self.inc = [start(self.D[0], dl, frames), start(self.D[1], dr, frames)]
        self.N, self.k = frames, 0

    def process(self, frames, ins, outs, in_mask):
        if self.N == 0:
            return refmodel.SpatialNode.process(self, frames, ins, outs, in_mask)
        m = ins[0][:frames].copy() if self.n_in < 2 else (ins[0][:frames] + ins[1][:frames]) * f32(0.5)
        ext = np.concatenate([self.hist, m])                 # ext[SP_HIST + i] = m[i]
        i = np.arange(frames, dtype=np.int64)
        t = self.k + i
        inside = t < self.N
        with np.errstate(all="ignore"):
            pos = t.astype(f32) / f32(self.N)                # both exact in f32 (<= 2^24)
            for e, (G1, d1) in enumerate(((self.gl, self.dl), (self.gr, self.dr))):
                G0, G1 = f32(self.G0[e]), f32(G1)
                v = G0 + (f32(G1 - G0) * pos)
                lo, hi = (G0, G1) if G0 < G1 else (G1, G0)
                v = np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(f32)
                g = np.where(inside, v, G1).astype(f32)
                D = np.where(inside, np.int64(self.D[e]) + i * np.int64(self.inc[e]), np.int64(d1 << 32))
                lo_d, hi_d = sorted((self.D[e], d1 << 32))
                assert np.all((D >= lo_d) & (D <= hi_d)), "D left [D0, d1 << 32]"
                q = D >> 32
                f = ((D & 0xffffffff) >> 8).astype(f32) * TWO_M24
                assert np.all((f == 0) | (q <= SP_HIST - 2)), "a fractional delay needs q + 1 < SP_HIST"
                a = ext[SP_HIST + i - q]
                b = ext[np.where(f != 0, SP_HIST + i - q - 1, 0)]
                x = np.where(f == 0, a, a + ((b - a) * f)).astype(f32)
                outs[e][:frames] = x * g
        self.hist = ext[-SP_HIST:].copy()
        self.k += frames
        if self.k < self.N:
            self.D = [self.D[e] + frames * self.inc[e] for e in range(2)]
        else:                                                # at rest at the target
            self.N = self.k = 0
        return 0


class MoveRefEngine(refmodel.RefEngine):
    def add_node(self, kind, n_in, n_out, params=()):
        if kind == fwapi.SPATIAL:
            return self._add(MoveSpatialNode(self, n_in, n_out, [float(p) for p in params]))
        return refmodel.RefEngine.add_node(self, kind, n_in, n_out, params)

    def move(self, node, x, y, z, frames, at_block=0):
        assert at_block == 0
        self.nodes[node].move(f32(x), f32(y), f32(z), int(frames))

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
    """messages tagged with a block of the next call, the move among them"""

    def move(self, node, x, y, z, frames, at_block=0):
        self._defer(at_block, self.e.move, node, x, y, z, frames)

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


class GpuMove(object):
    """a GpuEngine (or the host-only harness engine) with the move message under the same name"""

    def __init__(self, eng):
        self.e = eng

    def __getattr__(self, name):
        return getattr(self.e, name)

    def move(self, node, x, y, z, frames, at_block=0):
        self.e._chk(self.e.cx.L.fwgpu_spatial_move(self.e.cx.c, node, x, y, z, frames, at_block))
