"""numpy models of the wave reductions of armour-dev_amd/csrc/wave.h and block_reduce.h: the butterfly
(wave_sum and the max / min forms: every lane computes every level) and the reduce-scatter
(scatter_sum: every tree node once), lane by lane as the device moves the values, and the block
reduction on top (waves in order). Shared by tests/test_reduce_model.py and
tests/test_gpu_block_reduce.py; doubles in, doubles out, compared through their bits."""
import numpy as np

LANES = 64
LEVELS = (1, 2, 4, 8, 16, 32)
PARTNER = {m: np.arange(LANES) ^ m for m in LEVELS}
OPS = {0: np.add, 1: np.fmax, 2: np.fmin}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def butterfly(v, kind=0, levels=LEVELS):
    """v [..., 64]: the butterfly's value on every lane, own (op) partner per level"""
    op = OPS[kind]
    with np.errstate(all="ignore"):
        for m in levels:
            v = op(v, v[..., PARTNER[m]])
    return v


def scatter_width(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def scatter_index(P, lane):
    idx, m, h = 0, 1, P >> 1
    while h >= 1:
        if lane & m:
            idx += h
        m, h = m << 1, h >> 1
    return idx


def scatter_sum(v, live=None):
    """v [..., 64 lanes, N]: wave.h scatter_sum. Returns (r [..., 64]: what each lane ends with, P); lane
    l's is the total of index scatter_index(P, l) where that index is live. live: N booleans (default all)."""
    N = v.shape[-1]
    P = scatter_width(N)
    live = [True] * N if live is None else list(live)
    live = live + [False] * (P - N)
    x = np.zeros(v.shape[:-1] + (P,))
    x[..., :N] = v
    lane = np.arange(LANES)
    m, h = 1, P >> 1
    with np.errstate(all="ignore"):
        while h >= 1:
            b = (lane & m) != 0
            for i in range(h):
                la, lb = live[i], live[i + h]
                if not la and not lb:
                    continue
                if la and lb:
                    keep = np.where(b, x[..., i + h], x[..., i])
                    send = np.where(b, x[..., i], x[..., i + h])
                    x[..., i] = keep + send[..., PARTNER[m]]
                else:
                    t = x[..., i] if la else x[..., i + h]
                    x[..., i] = t + t[..., PARTNER[m]]
            live = [live[i] or live[i + h] for i in range(h)]
            m, h = m << 1, h >> 1
        r = x[..., 0].copy()
        while m < LANES:
            r = r + r[..., PARTNER[m]]
            m <<= 1
    return r, P


def scatter_totals(v, live=None):
    """the N totals as block_reduce_get stores them: index idx from lane l < P with scatter_index(P, l) == idx"""
    N = v.shape[-1]
    r, P = scatter_sum(v, live)
    out = np.full(v.shape[:-2] + (N,), np.nan)
    for l in range(P):
        idx = scatter_index(P, l)
        if idx < N and (live is None or live[idx]):
            out[..., idx] = r[..., l]
    return out


def block_reduce(x, kinds, levels=LEVELS):
    """x [..., threads, N] -> [..., N]: per wave the butterfly's tree (levels in the given order), then the
    waves in order"""
    T, N = x.shape[-2:]
    kinds = np.asarray(kinds)
    out = np.empty(x.shape[:-2] + (N,))
    with np.errstate(all="ignore"):
        for kind in set(kinds.tolist()):
            sel = kinds == kind
            # [..., slots, waves, lanes]
            v = np.swapaxes(x[..., sel], -1, -2).reshape(x.shape[:-2] + (int(sel.sum()), T // LANES, LANES))
            w = butterfly(v, kind, levels)[..., 0]
            s = w[..., 0]
            for k in range(1, T // LANES):
                s = OPS[kind](s, w[..., k])
            out[..., sel] = s
    return out
