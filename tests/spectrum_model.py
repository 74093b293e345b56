"""The spectrum meter's numeric SPEC (include/fwgpu.h) restated in numpy: float32 after every operation, the tables
with math.cos / math.sin / math.pow — the libm the library calls — evaluated left to right as the SPEC writes them.  A restatement of
the SPEC's text, not of the kernel: whole stages at a time on arrays, no LDS, no threads."""
import math

import numpy as np

F32 = np.float32
FFT_SIZES = (256, 512, 1024, 2048, 4096)


def window(N):
    return np.array([F32(0.5 - 0.5 * math.cos(2.0 * math.pi * i / N)) for i in range(N)], dtype=F32)


def twiddles(N):
    wr = np.array([F32(math.cos(2.0 * math.pi * k / N)) for k in range(N // 2)], dtype=F32)
    wi = np.array([F32(-math.sin(2.0 * math.pi * k / N)) for k in range(N // 2)], dtype=F32)
    return wr, wi


def edges(N, bands):
    M = N // 2
    if bands == 0:
        return np.arange(M + 2, dtype=np.int64)
    e = [1]
    for b in range(1, bands):
        e.append(max(e[b - 1] + 1, min(M + 1 - (bands - b), int(math.floor(math.pow(float(M), float(b) / bands) + 0.5)))))
    return np.array(e + [M + 1], dtype=np.int64)


def record_len(N, bands):
    return bands if bands else N // 2 + 1


def bitrev(N):
    bits = N.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(N)], dtype=np.int64)


_tables = {}


def tables(N):
    if N not in _tables:
        _tables[N] = (window(N), twiddles(N), bitrev(N))
    return _tables[N]


def powers(frames, N):
    """frames [..., N] (the window's frames, oldest first) -> P [..., N/2 + 1]"""
    w, (wr, wi), rev = tables(N)
    v = (np.asarray(frames, dtype=F32) * w).astype(F32)
    re = np.ascontiguousarray(v[..., rev])
    im = np.zeros_like(re)
    lead = re.shape[:-1]
    h = 1
    while h < N:
        k = np.arange(h) * (N // (2 * h))
        cr, ci = wr[k], wi[k]
        re, im = re.reshape(lead + (-1, 2, h)), im.reshape(lead + (-1, 2, h))
        ar, ai, br, bi = re[..., 0, :], im[..., 0, :], re[..., 1, :], im[..., 1, :]
        tr = ((cr * br).astype(F32) - (ci * bi).astype(F32)).astype(F32)
        ti = ((cr * bi).astype(F32) + (ci * br).astype(F32)).astype(F32)
        re = np.stack([(ar + tr).astype(F32), (ar - tr).astype(F32)], axis=-2).reshape(lead + (N,))
        im = np.stack([(ai + ti).astype(F32), (ai - ti).astype(F32)], axis=-2).reshape(lead + (N,))
        h *= 2
    re, im = re[..., :N // 2 + 1], im[..., :N // 2 + 1]
    scale = F32(16.0) / F32(N * N)
    return ((((re * re).astype(F32) + (im * im).astype(F32)).astype(F32)) * scale).astype(F32)


def band_sums(P, N, bands):
    """P [..., N/2 + 1] -> [..., B]: one ascending chain of f32 adds per band"""
    e = edges(N, bands)
    B = record_len(N, bands)
    out = np.zeros(P.shape[:-1] + (B,), dtype=F32)
    width = int((e[1:] - e[:-1]).max())
    out[...] = P[..., e[:-1]]
    for j in range(1, width):
        sel = np.nonzero(e[:-1] + j < e[1:])[0]
        out[..., sel] = (out[..., sel] + P[..., e[sel] + j]).astype(F32)
    return out


def model(signal, block_frames, N, bands, silent=None, history=None):
    """signal [channels][frames]: a channel's frames since the node's activation (or since `history`, [channels][N] frames in front of
    them); block_frames: the length of every block in order, summing to the frame count; silent [blocks][channels] (bool): the channel
    is flagged silent for that block and counts as +0.0.  -> records [blocks][channels][B]"""
    signal = np.atleast_2d(np.asarray(signal, dtype=F32))
    ch, total = signal.shape
    assert sum(block_frames) == total
    x = signal.copy()
    ends = np.cumsum(block_frames)
    if silent is not None:
        for b, (a, z) in enumerate(zip(ends - np.asarray(block_frames), ends)):
            for c in range(ch):
                if silent[b][c]:
                    x[c, a:z] = F32(0.0)
    front = np.zeros((ch, N), dtype=F32) if history is None else np.asarray(history, dtype=F32)
    x = np.concatenate([front, x], axis=1)
    win = np.stack([x[:, z:z + N] for z in ends])  # block g's window ends with its last frame: x[z + N - N .. z + N)
    return band_sums(powers(win, N), N, bands)


def blocks_of(calls, mbf):
    """the block lengths of process calls of `calls` frames each: full blocks and a short last one"""
    out = []
    for f in calls:
        out += [mbf] * (f // mbf) + ([f % mbf] if f % mbf else [])
    return out
