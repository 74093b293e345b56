"""Streaming sample sources (fwgpu_sample_create_stream, CMD_SMP_STREAM = 17; SPEC) restated over tests/refmodel.py:
`StreamSamplerNode` adds the stream's four integers W, C, E, U to the numpy sampler (refmodel.SamplerNode by way of the fade model's
FadeSamplerNode, so the envelope is there too), `Ring` is the ring a writer fills — the model's twin of the control side's accounting —
and `StreamRefEngine` is a RefEngine that builds both.  tests/test_stream_source.py uses them."""
import numpy as np

import fwapi
import refmodel
import sampler_fade_model as sfm
from refmodel import clear_all_outputs

CMD_SMP_STREAM = 17
RING_MAX = 1 << 30
RING_MIN_BLOCKS = 4
DTYPE = {0: np.int16, 1: np.uint16, 2: np.float32, 3: np.int16, 4: np.uint16, 5: np.float32}


def layout(fmt, channels, frames_by_channel):
    """[frames][channels] values -> the flat array fwgpu_sample_create / fwgpu_sample_stream_write take for that format"""
    a = np.asarray(frames_by_channel, dtype=DTYPE[fmt]).reshape(-1, channels)
    return np.ascontiguousarray(a if fmt <= 2 else a.T).reshape(-1)


class Ring(object):
    """a stream as the control side sees it: R frames, zeroed; `write` appends at written % R and splits at the ring's end"""

    def __init__(self, fmt, channels, R, mbf):
        assert RING_MIN_BLOCKS * mbf <= R <= RING_MAX
        self.fmt, self.channels, self.R, self.mbf = fmt, channels, R, mbf
        self.sample = refmodel.Sample(fmt, channels, np.zeros(R * channels, dtype=DTYPE[fmt]))
        self.written = 0
        self.ended = False
        self.node = None  # the StreamSamplerNode it is bound to

    def consumed(self):
        return self.node.C if self.node is not None and self.node.stream is self else 0

    def free_frames(self, consumed_seen=None):
        return self.R - (self.written - (self.consumed() if consumed_seen is None else consumed_seen))

    def _put(self, rows):
        """rows: [n][channels] raw elements"""
        d = self.sample.data
        for i in range(len(rows)):
            p = (self.written + i) % self.R
            if self.sample.interleaved:
                d[p, :] = rows[i]
            else:
                d[:, p] = rows[i]
        self.written += len(rows)

    def write(self, frames_by_channel, consumed_seen=None):
        """-> frames accepted; the bound sampler is told the new W (seen at the top of its next block)"""
        assert not self.ended
        rows = np.asarray(frames_by_channel, dtype=DTYPE[self.fmt]).reshape(-1, self.channels)
        n = max(0, min(len(rows), self.free_frames(consumed_seen)))
        self._put(rows[:n])
        if self.node is not None and n:
            self.node.msgs.append(("stream", self.written, None))
        return n

    def end(self, consumed_seen=None):
        assert not self.ended
        if self.free_frames(consumed_seen) < self.mbf:
            return False
        E = self.written
        # (the padding: zero bytes; 0x8000 for the unsigned formats, which have no element that decodes to 0.0)
        self._put(np.full((self.mbf, self.channels), 0x8000 if self.fmt in (1, 4) else 0, dtype=DTYPE[self.fmt]))
        self.ended = True
        if self.node is not None:
            self.node.msgs.append(("stream", self.written, E))
        else:
            self.end_at = E
        return True


class StreamSamplerNode(sfm.FadeSamplerNode):
    def __init__(self, eng, n_in, n_out, params):
        sfm.FadeSamplerNode.__init__(self, eng, n_in, n_out, params)
        self.stream = None
        self.W = self.C = self.U = 0
        self.E = None
        self.finished = False

    def state(self):
        return dict(C=self.C, U=self.U, playing=bool(self.playing), finished=self.finished, playhead=self.playhead)

    def _drain(self):
        keep = []
        for m in self.msgs:
            what = m[0]
            if what == "stream_bind":  # set_sample with a stream: (ring, stop_playback, W)
                ring = m[1]
                self.stream, self.W, self.C, self.E, self.U, self.finished = ring, m[3], 0, None, 0, False
                self.msgs, saved = [("sample", ring.sample, False)], self.msgs
                sfm.FadeSamplerNode._drain(self)
                self.msgs = saved
                self.loop_range = [0, ring.R, False]
                self.playhead = 0
                if m[2]:
                    self.playing = False
                    self.env.reset()
                continue
            if what == "stream":
                if self.stream is not None:
                    self.W = max(self.W, m[1])
                    if m[2] is not None and self.E is None:
                        self.E = m[2]
                        if self.E <= self.C:  # a late end: every frame has been played — finished here, no block of padding
                            self.playing = False
                            self.env.reset()
                            self.finished = True
                continue
            if self.stream is not None:
                if what in ("playhead", "loop"):
                    continue  # a stream has no position to seek to and no range to loop
                if what == "play" and self.finished:
                    continue
                if what == "stop":
                    m = ("pause",)  # a stream does not rewind
                if what == "sample":  # another sample: a one-shot at frame 0 again
                    self.stream = None
                    self.loop_range = None
                    self.playhead = 0
            self.msgs, saved = [m], self.msgs
            sfm.FadeSamplerNode._drain(self)
            self.msgs = saved
        self.msgs = keep

    def _behind(self, frames):
        if self.stream is None:
            return sfm.FadeSamplerNode._behind(self, frames)
        ph = self.playhead
        sfm.FadeSamplerNode._behind(self, frames)
        self.playhead = ph  # (a fade's then = STOP acts as PAUSE)

    def process(self, frames, ins, outs, in_mask):
        self._drain()
        if self.stream is None:
            return sfm.FadeSamplerNode.process(self, frames, ins, outs, in_mask)
        if self.playing and self.sample is not None and self.W - self.C < frames:
            self.U += 1
            return clear_all_outputs(frames, outs)
        ph0 = self.playhead
        data = frames if self.E is None else max(0, min(frames, self.E - self.C))
        om = sfm.FadeSamplerNode.process(self, frames, ins, outs, in_mask)
        if self.playhead != ph0:
            # the block the end falls into is a one-shot's last block — frames behind the end are 0.0 — unless the ring's wrap falls in
            # front of the end inside the same block (a record holds one break): then they are read from the padding
            first = self.stream.R - (ph0 if ph0 < self.stream.R else 0)
            if data < frames and not (first < frames and first < data):
                for o in outs:
                    o[data:frames] = refmodel.F0
            self.C += frames
            if self.E is not None and self.C >= self.E:
                self.playing = False
                self.env.reset()
                self.finished = True
        return om


class StreamRefEngine(sfm.FadeRefEngine):
    def add_node(self, kind, n_in, n_out, params=()):
        if kind == fwapi.SAMPLER:
            return self._add(StreamSamplerNode(self, n_in, n_out, [float(p) for p in params]))
        return refmodel.RefEngine.add_node(self, kind, n_in, n_out, params)

    def new_stream(self, fmt, channels, R):
        return Ring(fmt, channels, R, self.max_block_frames)

    def sampler_set_stream(self, node, ring, stop_playback=False):
        assert ring.node is None
        ring.node = self.nodes[node]
        self.nodes[node].msgs.append(("stream_bind", ring, bool(stop_playback), ring.written))
        if ring.ended:
            self.nodes[node].msgs.append(("stream", ring.written, ring.end_at))
