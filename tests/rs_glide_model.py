"""The resampler's ratio glide (fwgpu_resampler_glide, CMD_RS_GLIDE = 24; SPEC) restated over tests/refmodel.py:
`GlideResamplerNode` adds the glide to the numpy ResamplerNode — Python integers for pos / step / inc / left, the state moved frame
by frame, `fma32` for the taps — and `GlideRefEngine` is a RefEngine that builds it, with the message and with the graph-output
silence flags of a run of blocks.  `Tagged` delivers messages tagged with a block, as scenarios.TaggedOracle does.  `closed_form` is the
SPEC's closed form, for the tests that hold it against the iteration.  tests/test_rs_glide.py uses all of them."""
import numpy as np

import fwapi
import refmodel
import scenarios
from refmodel import F0, RS_PHASES, RS_TAPS, clear_all_outputs, f32, fma32, resampler_step

M64 = (1 << 64) - 1
FRAMES_MAX = 1 << 24
CMD_RS_STEP, CMD_RS_GLIDE = 20, 24


def trunc_div(a, b):
    """C++ signed division: truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def glide_start(step, S1, N):
    """the message, applied with the node's current step -> (inc, left, target)"""
    assert 0 < N <= FRAMES_MAX and abs(S1 - step) < 1 << 40
    return trunc_div(S1 - step, N), N, S1


def iterate(pos, step, inc, left, target, n):
    """n frames, one at a time -> (positions of the frames, pos, step, left) behind them"""
    at = []
    for _ in range(n):
        at.append(pos)
        pos = (pos + step) & M64
        if left > 0:
            step += inc
            left -= 1
            if left == 0:
                step = target
    return at, pos, step, left


def closed_form(pos0, step0, inc, i):
    """(pos_i, step_i) of frame i <= left of a run from (pos0, step0), in wrapping u64 arithmetic"""
    tri = i * (i - 1) // 2
    assert tri < 1 << 47
    return (pos0 + i * step0 + inc * tri) & M64, (step0 + i * inc) & M64


class GlideResamplerNode(refmodel.ResamplerNode):
    def __init__(self, eng, n_in, n_out, params):
        refmodel.ResamplerNode.__init__(self, eng, n_in, n_out, params)
        self.inc = self.left = self.target = 0

    def set_param(self, param, value):
        if param == 1:
            self.left = 0                      # a step ends a glide in flight
        refmodel.ResamplerNode.set_param(self, param, value)

    def glide(self, ratio, frames):
        if frames == 0:
            return self.set_param(1, ratio)
        self.inc, self.left, self.target = glide_start(self.step, resampler_step(ratio), frames)

    def process(self, frames, ins, outs, in_mask):
        if self.left == 0:
            return refmodel.ResamplerNode.process(self, frames, ins, outs, in_mask)
        if self.seek is not None:
            self.pos = (self.seek << 32) & M64
            self.seek = None
        n = self.src.frames
        if not self.playing_ctl or n == 0:     # renders nothing and advances nothing, the glide included
            return clear_all_outputs(frames, outs)
        sch = self.src.channels
        nfill = min(self.n_out, sch)
        p, self.pos, self.step, self.left = iterate(self.pos, self.step, self.inc, self.left, self.target, frames)
        idx = np.array([q >> 32 for q in p], dtype=np.int64)
        ph = np.array([(q >> 27) & (RS_PHASES - 1) for q in p], dtype=np.int64)
        mask = 0
        for c in range(nfill):
            acc = np.zeros(frames, dtype=f32)
            for k in range(RS_TAPS):
                j = idx - (RS_TAPS // 2 - 1) + k
                if self.loop:
                    x = self._channel(c, j % n)
                else:
                    inside = (j >= 0) & (j < n)
                    x = np.where(inside, self._channel(c, np.where(inside, j, 0)), F0).astype(f32)
                acc = fma32(self.h[ph, k], x, acc)
            outs[c][:frames] = acc
        if self.n_out > sch:
            if self.n_out == 2 and sch == 1:
                outs[1][:frames] = outs[0][:frames]
            else:
                for c in range(sch, self.n_out):
                    outs[c][:frames] = F0
                    mask |= 1 << c
        if self.loop:
            self.pos %= n << 32
        elif (self.pos >> 32) >= n + RS_TAPS // 2:
            self.playing_ctl = False
        return mask


class GlideRefEngine(refmodel.RefEngine):
    def add_node(self, kind, n_in, n_out, params=()):
        if kind == fwapi.RESAMPLER:
            return self._add(GlideResamplerNode(self, n_in, n_out, [float(p) for p in params]))
        return refmodel.RefEngine.add_node(self, kind, n_in, n_out, params)

    def glide(self, node, ratio, frames, at_block=0):
        assert at_block == 0
        self.nodes[node].glide(f32(ratio), int(frames))

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
    """messages tagged with a block of the next call, the glide among them"""

    def glide(self, node, ratio, frames, at_block=0):
        self._defer(at_block, self.e.glide, node, ratio, frames)

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


class GpuGlide(object):
    """a GpuEngine (or the host-only harness engine) with the glide message under the same name"""

    def __init__(self, eng):
        self.e = eng

    def __getattr__(self, name):
        return getattr(self.e, name)

    def glide(self, node, ratio, frames, at_block=0):
        self.e._chk(self.e.cx.L.fwgpu_resampler_glide(self.e.cx.c, node, ratio, frames, at_block))
