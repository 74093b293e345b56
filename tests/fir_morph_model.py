"""The FIR morph (SPEC; include/fwgpu.h "FIR reverb morph") in numpy, for tests/test_fir_morph.py.

A morph-capable FirReverbNode is two plain FIR nodes on ONE input whose impulse responses are zero-padded to T taps (the slot sums),
blended by the crossfader's rule.  So the model is refmodel.FirNode twice (or, for a larger T, the oracle twice: two plain
one-parameter FIR graphs on padded samples) and the crossfader's curve, position and gains as tests/test_crossfade.py states them
(Segment, gains) — one statement of the curve for its three users here as in the library."""
import numpy as np

import fwapi
import refmodel
from fwapi import PLANAR_F32, OracleEngine
from test_crossfade import EQUAL_POWER, LINEAR_LAW, Segment, gains  # noqa: F401 (the laws are re-exported)

F32 = np.float32
MODE_A, MODE_B, MODE_BOTH = 1, 2, 3


def pad_ir(h, T):
    """h [C_h][len] -> [C_h][T], zero-padded in h's own number format (a zero of every sample format converts to 0.0f: exactly what
    k_ir_convert writes for a length of T)"""
    h = np.atleast_2d(np.asarray(h))
    if h.dtype not in (np.int16, np.uint16):
        h = h.astype(F32)
    assert h.shape[1] <= T, (h.shape, T)
    out = np.zeros((h.shape[0], T), dtype=h.dtype)
    if h.dtype == np.uint16:
        out[:] = 32768      # (the unsigned format's zero)
    out[:, :h.shape[1]] = h
    return out


class _Ir(object):
    """the part of refmodel's sample that FirNode reads"""

    def __init__(self, h):
        self.h = np.atleast_2d(np.asarray(h, dtype=F32))
        self.channels, self.frames = self.h.shape

    def fill_buffers(self, buffers, lo, hi, start_frame):
        for c in range(min(self.channels, len(buffers))):
            buffers[c][lo:hi] = self.h[c, start_frame:start_frame + (hi - lo)]


class _Eng(object):
    def __init__(self, h):
        self.samples = [_Ir(h)]


def blocks_of(calls, mbf):
    """the block lengths the executor renders for these calls (whole blocks, then a call's trailing short block)"""
    out = []
    for f in calls:
        out += [mbf] * (f // mbf) + ([f % mbf] if f % mbf else [])
    return out


def slot_sum_ref(h, T, x, blocks):
    """the slot sum of an impulse response h [C_h][len] padded to T over the input x [frames][ch], block by block, through
    refmodel.FirNode -> [frames][ch]"""
    ch = x.shape[1]
    node = refmodel.FirNode(_Eng(pad_ir(h, T)), ch, ch, [0.0])
    out = np.zeros(x.shape, dtype=F32)
    pos = 0
    for f in blocks:
        ins = [np.ascontiguousarray(x[pos:pos + f, c], dtype=F32) for c in range(ch)]
        outs = [np.zeros(f, dtype=F32) for _ in range(ch)]
        node.process(f, ins, outs, 0)
        for c in range(ch):
            out[pos:pos + f, c] = outs[c]
        pos += f
    assert pos == len(x)
    return out


def slot_sum_oracle(h, T, x, calls, mbf, fmt=PLANAR_F32):
    """... through the oracle: a plain one-parameter FIR graph on the padded sample (planar, format `fmt`), fed call by call"""
    ch = x.shape[1]
    hp = pad_ir(h, T)
    o = OracleEngine(max_block_frames=mbf, num_graph_inputs=ch, num_graph_outputs=ch)
    ir = o.new_sample(fmt, hp.shape[0], hp)
    f = o.fir(ir, ch=ch)
    for c in range(ch):
        o.connect(o.graph_in_node, c, f, c)
        o.connect(f, c, o.graph_out_node, c)
    o.update()
    out, pos = [], 0
    for n in calls:
        y = o.process_interleaved(n, ch, inp=np.ascontiguousarray(x[pos:pos + n]).reshape(-1), n_in_ch=ch)
        out.append(np.asarray(y, F32).reshape(-1, ch))
        pos += n
    return np.concatenate(out)


class Morph(object):
    """the blend of one morph-capable node since its activation: `to` is a message at the first frame of the next block, `block`
    renders one block from the two slot sums"""

    def __init__(self, position=0.0, law=EQUAL_POWER):
        self.law, self.T, self.seg = law, 0, Segment(position, position)

    def to(self, position, frames, curve=None):
        self.seg = Segment(self.seg.position([self.T])[0], position, self.T, frames, curve)

    def mode(self):
        """which slots run in the block that starts now"""
        s = self.seg
        rest = s.dur == 0 or self.T - s.t0 >= s.dur
        return MODE_A if rest and s.P1 == 0 else (MODE_B if rest and s.P1 == 1 else MODE_BOTH)

    def block(self, sa, sb):
        """sa, sb: [F][ch] slot sums of the block (sb None: an empty slot B, whose sum is +0.0) -> y [F][ch]"""
        sa = np.asarray(sa, dtype=F32)
        sb = np.zeros_like(sa) if sb is None else np.asarray(sb, dtype=F32)
        F = sa.shape[0]
        p = self.seg.position(self.T + np.arange(F, dtype=np.int64))
        a, b = gains(p, self.law)
        with np.errstate(invalid="ignore", over="ignore"):
            y = (sa * a[:, None]) + (sb * b[:, None])     # two products and a sum, each rounded to f32
        y = np.where((p == 0)[:, None], sa, np.where((p == 1)[:, None], sb, y)).astype(F32)
        self.T += F
        return y


def render(morph, sa, sb, blocks, messages=()):
    """sa, sb: [frames][ch] slot sums over the whole run; blocks: the block lengths; messages: {block index: [(position, frames,
    curve), ...]} applied, in order, at that block's first frame -> (y [frames][ch], the mode of every block)"""
    messages = dict(messages)
    out, modes, pos = [], [], 0
    for i, f in enumerate(blocks):
        for (position, frames, curve) in messages.get(i, ()):
            morph.to(position, frames, curve)
        modes.append(morph.mode())
        out.append(morph.block(sa[pos:pos + f], None if sb is None else sb[pos:pos + f]))
        pos += f
    return np.concatenate(out), modes


def gemm_workgroups(rows, T, mbf, frames=None):
    """GEMM workgroups per block for `rows` rows of one slot laid out in whole 32-row tiles: tiles x segments x column groups"""
    frames = mbf if frames is None else frames
    W = T - 1 + frames
    return ((rows + 31) // 32) * ((W + 4095) // 4096) * ((frames + 255) // 256)
