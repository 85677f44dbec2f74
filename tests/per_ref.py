"""Prioritised replay restated on the host (include/navenv.h, nav_per_*): Python integers for
every sum and comparison, oracle.philox for the random words, numpy fp64 for the two pow()s, and a
torch-fp64 weighted critic epoch from mlp_ref's pieces. Needs no GPU and no libnavenv.so."""
import bisect
import functools
import itertools

import numpy as np
import torch

import mlp_ref as R
from oracle import oracle as O

NAV_TAG_PER = 8
ONE = 65536              # priority 1.0 (16 fractional bits)
MAX_PRI = (1 << 31) - 1


@functools.lru_cache(maxsize=None)
def r64(b, seed, counter, actor):
    """(w.y << 32) | w.x of Philox at ctr = (b, 0, 8, 2*counter [+ 1]), key = the seed's words."""
    c3 = (2 * int(counter) + (1 if actor else 0)) & 0xFFFFFFFF
    w = O.philox((int(b), 0, NAV_TAG_PER, c3), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (int(w[1]) << 32) | int(w[0])


def prefix(pri, size):
    """P_k = sum_{j<=k} pri[j] over [0, size) as Python integers."""
    return list(itertools.accumulate(np.asarray(pri[:size]).astype(np.int64).tolist()))


def targets(S, B, seed, counter, actor):
    """t_b = floor(r64_b * S / 2^64)."""
    return [(r64(b, seed, counter, bool(actor)) * int(S)) >> 64 for b in range(B)]


def sample(pri, size, B, seed, counter, actor, P=None):
    """idx [B] int64: min{k : P_k > t_b} (P: prefix(pri, size) if the caller has it)."""
    P = prefix(pri, size) if P is None else P
    return np.array([min(bisect.bisect_right(P, t), size - 1)
                     for t in targets(P[-1], B, seed, counter, actor)], np.int64)


def weights(pri, size, idx, beta):
    """(float)pow((double)q_min / (double)pri[idx], (double)(float)beta), q_min over [0, size)."""
    p = np.asarray(pri[:size]).astype(np.uint32)
    q_min = np.float64(int(p.min()))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.power(q_min / p[np.asarray(idx)].astype(np.float64),
                        np.float64(np.float32(beta))).astype(np.float32)


def priority(td1, td2, alpha, eps):
    """q [B] int64 = clamp(floor(pow(0.5 (|td1| + |td2|) + eps, alpha) * 65536 + 0.5), 1, 2^31 - 1);
    NaN gives 1."""
    a, e = np.float64(np.float32(alpha)), np.float64(np.float32(eps))
    m = 0.5 * (np.abs(np.asarray(td1, np.float32).astype(np.float64)) +
               np.abs(np.asarray(td2, np.float32).astype(np.float64))) + e
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.floor(np.power(m, a) * 65536.0 + 0.5)
    q = np.where(v >= 1.0, np.minimum(v, float(MAX_PRI)), 1.0)  # NaN >= 1 is False
    return q.astype(np.int64)


def update(pri, idx, q):
    """The store after nav_per_update: every sampled row's old value replaced by the maximum of
    its new ones."""
    out = np.asarray(pri).astype(np.int64).copy()
    idx = np.asarray(idx)
    out[idx] = 0
    np.maximum.at(out, idx, np.asarray(q, np.int64))
    return out


def critic_epoch_w(ta, tc, cr, batch, eps, bits, w, dtype=torch.float64):
    """mlp_ref.critic_epoch with importance weights w [B]: dq[i] = (2 (q_i - y) / B) * w,
    loss[i] = mean(w (q_i - y)^2), grads[i] = the backward of the weighted dq; plus td[i] =
    |q_i - y|. y, q and zs are critic_epoch's own."""
    e = R.critic_epoch(ta, tc, cr, batch, eps, bits, dtype)
    B = batch.shape[0]
    x = batch.to(dtype)[:, :4]
    wv = w.to(dtype).reshape(B, 1)
    out = dict(y=e["y"], q=e["q"], zs=e["zs"], dq=[], loss=[], grads=[], td=[])
    for i in range(2):
        q, _, hs = R.mlp_forward(cr[i], x, dtype)
        err = q - e["y"].reshape(B, 1)
        dq = 2 * err / B * wv
        _, _, grads = R.mlp_backward(cr[i], hs, dq, bits[i], dtype)
        out["dq"].append(dq[:, 0])
        out["loss"].append((wv * err ** 2).mean())
        out["grads"].append(grads)
        out["td"].append(err[:, 0].abs())
    return out
