"""The sampler's gain envelope (fwgpu_sampler_fade, CMD_SMP_FADE = 16; SPEC) restated over tests/refmodel.py:
`FadeSamplerNode` adds the envelope to the numpy SamplerNode — E0, E1 as numpy f32, N, k as Python integers, the value of every frame
from `env_value`, one separately rounded f32 operation after the other, and the state moved frame by frame — and `FadeRefEngine` is a
RefEngine that builds it, with the message and with the graph-output silence flags of a run of blocks.  `Tagged` delivers messages
tagged with a block, as scenarios.TaggedOracle does; `GpuFade` adds `fade` to a GpuEngine / HostOnlyEngine (tests/fwapi.py is not to
change).  tests/test_sampler_fade.py uses all of them."""
import numpy as np

import fwapi
import refmodel
import scenarios
from refmodel import F0, clear_all_outputs, f32

FRAMES_MAX = 1 << 24
CMD_SMP_FADE = 16
NONE, PAUSE, STOP = 0, 1, 2
F1 = f32(1.0)


def env_value(E0, E1, N, k, j):
    """env(j) of the SPEC: every operation a separately rounded f32 operation; f32(k + j) and f32(N) are exact"""
    if N == 0 or k + j >= N:
        return f32(E1)
    E0, E1 = f32(E0), f32(E1)
    d = f32(E1 - E0)
    u = f32(f32(k + j) / f32(N))
    v = f32(E0 + f32(d * u))
    lo, hi = min(E0, E1), max(E0, E1)
    return f32(min(max(v, lo), hi))


class Envelope(object):
    """the SPEC's state and its three moves: the message, one frame, "the sampler no longer plays" """

    def __init__(self):
        self.E0, self.E1, self.N, self.k, self.then = F0, F1, 0, 0, NONE

    def state(self):
        return (fwapi.bits(np.array([self.E0, self.E1], dtype=f32)).tolist(), self.N, self.k, self.then)

    def at_rest(self):
        return self.N == 0

    def value(self, j=0):
        return env_value(self.E0, self.E1, self.N, self.k, j)

    def reset(self):
        self.E1, self.N, self.k, self.then = F1, 0, 0, NONE

    def start(self, target, frames, then):
        target = f32(target) + F0  # (-0.0 counts as +0.0)
        assert 0.0 <= target <= 1.0 and 0 <= frames <= FRAMES_MAX and then in (NONE, PAUSE, STOP) and (frames or then == NONE)
        if frames == 0:
            self.E1, self.N, self.k, self.then = target, 0, 0, NONE
            return
        self.E0 = self.value(0)
        self.E1, self.N, self.k, self.then = target, int(frames), 0, then

    def step(self):
        """one rendered frame -> the `then` that has just come due (NONE: nothing)"""
        if self.N == 0:
            return NONE
        self.k += 1
        if self.k < self.N:
            return NONE
        then = self.then
        self.N = self.k = 0
        self.then = NONE
        return then


class FadeSamplerNode(refmodel.SamplerNode):
    def __init__(self, eng, n_in, n_out, params):
        refmodel.SamplerNode.__init__(self, eng, n_in, n_out, params)
        self.env = Envelope()

    def _drain(self):
        """the messages, in order (refmodel.SamplerNode.process :331-414 with the envelope's rules)"""
        for m in self.msgs:
            what = m[0]
            if what == "fade":
                self.env.start(m[1], m[2], m[3])
                continue
            if what == "pause" or what == "stop" or (what == "sample" and m[2]):
                self.env.reset()  # the envelope is a transient
            self._apply_plain(m)
        self.msgs = []

    def _apply_plain(self, m):
        what = m[0]
        if what == "sample":
            self.sample = m[1]
            if self.loop_range is not None and self.loop_range[2]:
                self.loop_range[0], self.loop_range[1] = 0, self.sample.frames
            if m[2]:
                self.playhead = self.loop_range[0] if self.loop_range is not None else 0
                self.playing = False
        elif what == "play":
            self.playing = True
        elif what == "pause":
            self.playing = False
        elif what == "stop":
            self.playhead = self.loop_range[0] if self.loop_range is not None else 0
            self.playing = False
        elif what == "playhead":
            self.playhead = refmodel.rust_round_u64(m[1] * float(self.eng.sample_rate))
        elif what == "loop":
            self.loop_range = None if m[1] == 0 else self._loop_new(m[1], m[2], m[3])
            if self.loop_range is not None and self.loop_range[0] <= self.playhead < self.loop_range[1]:
                self.playhead = self.loop_range[0]

    def _behind(self, frames):
        """behind a block in which the smoother ran: the envelope moves on frame by frame; a `then` that came due takes effect now (the
        block was rendered whole); a sampler that no longer plays has its envelope back at rest at 1.0"""
        due = NONE
        for _ in range(frames):
            t = self.env.step()
            if t != NONE:
                due = t
        if due == PAUSE:
            self.playing = False
        elif due == STOP:
            self.playhead = self.loop_range[0] if self.loop_range is not None else 0
            self.playing = False
        if not self.playing:
            self.env.reset()

    def process(self, frames, ins, outs, in_mask):  # refmodel.SamplerNode.process with g[i] = s[i] * env(i)
        self._drain()
        if self.sample is None or not self.playing:
            return clear_all_outputs(frames, outs)
        sample = self.sample
        gain, smoothing = self.gain_smoother.set_and_process(self.raw_gain, frames)
        assert len(gain) == frames or (self.eng.short_blocks and len(gain) >= frames)
        e = self.env
        envv = np.array([env_value(e.E0, e.E1, e.N, e.k, j) for j in range(frames)], dtype=f32)
        if not smoothing and gain[0] < f32(0.00001):  # (a test on the smoother alone; the envelope runs on)
            self._behind(frames)
            return clear_all_outputs(frames, outs)
        out_mask = 0
        if self.loop_range is not None:
            start, end = self.loop_range[0], self.loop_range[1]
            if self.playhead >= end:
                self.playhead = start
            first = min(frames, end - self.playhead)
            sample.fill_buffers(outs, 0, first, self.playhead)
            if first < frames:
                self.playhead = start
                second = frames - first
                sample.fill_buffers(outs, first, frames, self.playhead)
                self.playhead += second
            else:
                self.playhead += frames
        else:
            if self.playhead >= sample.frames:
                self.playing = False
                self._behind(frames)
                return clear_all_outputs(frames, outs)
            copy = min(frames, sample.frames - self.playhead)
            sample.fill_buffers(outs, 0, copy, self.playhead)
            if copy < frames:
                self.playing = False
                self.playhead = 0
                for o in outs:
                    o[copy:frames] = F0
            else:
                self.playhead += frames
        sc = sample.channels
        g = (np.asarray(gain[:frames], dtype=f32) * envv).astype(f32)  # one f32 product
        if len(outs) >= 2 and sc == 2:
            outs[0][:frames] *= g
            outs[1][:frames] *= g
        else:
            for c in range(min(len(outs), sc)):
                outs[c][:frames] *= g
        if len(outs) > sc:
            if len(outs) == 2 and sc == 1:
                outs[1][:frames] = outs[0][:frames]
            else:
                for i in range(sc, len(outs)):
                    outs[i][:frames] = F0
                    out_mask |= 1 << i
        self._behind(frames)
        return out_mask


class FadeRefEngine(refmodel.RefEngine):
    def add_node(self, kind, n_in, n_out, params=()):
        if kind == fwapi.SAMPLER:
            return self._add(FadeSamplerNode(self, n_in, n_out, [float(p) for p in params]))
        return refmodel.RefEngine.add_node(self, kind, n_in, n_out, params)

    def fade(self, node, target, frames, then=NONE, at_block=0):
        assert at_block == 0
        self.nodes[node].msgs.append(("fade", f32(target), int(frames), int(then)))

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
    """messages tagged with a block of the next call, the fade among them"""

    def fade(self, node, target, frames, then=NONE, at_block=0):
        self._defer(at_block, self.e.fade, node, target, frames, then)

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


class GpuFade(object):
    """a GpuEngine (or the host-only harness engine) with the fade message under the same name"""

    def __init__(self, eng):
        self.e = eng

    def __getattr__(self, name):
        return getattr(self.e, name)

    def fade(self, node, target, frames, then=NONE, at_block=0):
        self.e._chk(self.e.cx.L.fwgpu_sampler_fade(self.e.cx.c, node, target, frames, then, at_block))
