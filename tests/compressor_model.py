"""The bus compressor's SPEC (FWGPU_COMPRESSOR = 21; include/fwgpu.h) in numpy: the table with math.log10 and
math.pow — the libm the library calls — `astype(float32)` after every f32 operation, cumsum for the two window sums.  `brute_gains` is
the twin that evaluates every window by a loop, as the SPEC's text reads."""
import math

import numpy as np

f32 = np.float32
KNOTS = 321


def knee_start(T, knee_db):
    return f32(float(f32(T)) * math.pow(10.0, -float(f32(knee_db)) / 40.0))


def exact_gr_db(over_t0_db, ratio, knee_db):
    """the curve itself: gain reduction in dB at a level `over_t0_db` decibels above T0"""
    over = over_t0_db - knee_db / 2.0
    slope = 1.0 / ratio - 1.0
    if knee_db > 0.0 and 2.0 * abs(over) <= knee_db:
        t = over + knee_db / 2.0
        return slope * (t * t) / (2.0 * knee_db)
    return slope * over if over > 0.0 else 0.0


def table(ratio, knee_db):
    ratio, knee_db = float(f32(ratio)), float(f32(knee_db))
    G = np.empty(KNOTS, dtype=f32)
    for i in range(KNOTS):
        u = math.ldexp(1.0 + (i % 16) / 16.0, i // 16)
        G[i] = f32(math.pow(10.0, exact_gr_db(20.0 * math.log10(u), ratio, knee_db) / 20.0))
    return G


def key_of(x):
    """x: [n][frames] -> key[frames]: fmaxf from +0.0 over |x_c|, a NaN sample is ignored"""
    x = np.asarray(x, dtype=f32)
    m = np.zeros(x.shape[1], dtype=f32)
    for c in range(x.shape[0]):
        m = np.fmax(m, np.abs(x[c]))
    return m


def target_t(key, T0, G):
    with np.errstate(over="ignore"):
        u = (key / f32(T0)).astype(f32)
    over = u > f32(1)
    d = np.where(over, u.view(np.uint32).astype(np.int64) - 0x3F800000, 0)
    i = d >> 19
    fr = (d & 0x7FFFF).astype(f32) * f32(2.0 ** -19)
    sat = i >= 320
    i = np.minimum(i, 319)
    t = (G[i] + ((G[i + 1] - G[i]).astype(f32) * fr).astype(f32)).astype(f32)
    return np.where(over, np.where(sat, G[320], t), f32(1)).astype(f32)


def target_q(key, T0, G):            # key: f32 array, NaN-free, >= 0
    t = target_t(key, T0, G)
    return ((t * f32(65535)).astype(f32) + f32(0.5)).astype(f32).astype(np.uint32)


def gains(q, A, R, H):               # q of every frame since activation
    W = max(A, R) + H
    pad = np.concatenate([np.full(W, 65535), q]).astype(np.int64)
    m = pad.copy()
    for k in range(1, H + 1):
        m[k:] = np.minimum(m[k:], pad[:-k])
    P = np.concatenate([[0], np.cumsum(m)])
    i = np.arange(W, W + len(q))
    a = (P[i + 1] - P[i + 1 - A]).astype(np.uint32).astype(f32) / f32(A * 65535)
    r = (P[i + 1] - P[i + 1 - R]).astype(np.uint32).astype(f32) / f32(R * 65535)
    return np.minimum(a, r)


def brute_gains(q, A, R, H, frames):
    """g at each frame of `frames`, one window at a time"""
    W = max(A, R) + H
    pad = np.concatenate([np.full(W, 65535), q]).astype(np.int64)
    m = np.array([pad[max(j - H, 0):j + 1].min() for j in range(len(pad))], dtype=np.int64)
    out = []
    for n in frames:
        j = n + W
        ca, cr = int(m[j - A + 1:j + 1].sum()), int(m[j - R + 1:j + 1].sum())
        a = f32(f32(np.uint32(ca)) / f32(A * 65535))
        r = f32(f32(np.uint32(cr)) / f32(R * 65535))
        out.append(min(a, r))
    return np.array(out, dtype=f32)


def model(x, T, ratio, knee_db, A, R, H, M, silent=None):
    """x: [n][frames] since the node's activation (silent: [n][frames] bool, a channel flagged silent there: it counts as +0.0 and
    gives zeros) -> y [n][frames]"""
    x = np.asarray(x, dtype=f32)
    seen = x if silent is None else np.where(silent, f32(0), x)
    g = gains(target_q(key_of(seen), knee_start(T, knee_db), table(ratio, knee_db)), A, R, H)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (seen * (g * f32(M)).astype(f32)).astype(f32)
    return y if silent is None else np.where(silent, f32(0), y).astype(f32)
