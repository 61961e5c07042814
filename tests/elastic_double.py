"""Float64 restatement of ElasticFace (Boutros et al., CVPR-W 2022) as the fused head applies it.  TEST-ONLY.

  draws     Philox4x32-10, key = (seed low 32 bits, seed high 32 bits), counter = (row, 0, step low 32, step high 32); one round is
            p0 = 0xD2511F53 c0, p1 = 0xCD9E8D57 c2 (64-bit products), c <- (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)),
            k0 += 0x9E3779B9, k1 += 0xBB67AE85.  u1 = (x0 + 0.5) 2^-32, u2 = (x1 + 0.5) 2^-32, z = sqrt(-2 ln u1) cos(2 pi u2),
            g = float32(m + sigma z); eval: g = float32(m)
  margins   kind "arc": m_ang = g, m_add = 0; kind "cos": m_ang = 0, m_add = g; the head's per-row rule is adaface_double.logits
  "+"       c_i = max over ranks of the row's target cosine (-2 where nobody owns it); rank r_i = #{j : c_j > c_i, or c_j == c_i and
            j < i}, here by a STABLE sort of -c; row i gets the r_i-th entry of the draws sorted ascending
"""
import math

import numpy as np
import torch

import adaface_double
from adaface_double import AdaHeadKernels

EPS = adaface_double.EPS
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
PRESETS = {"arc": (0.5, 0.05), "cos": (0.35, 0.05), "arc+": (0.5, 0.0175), "cos+": (0.35, 0.025)}      # (m, sigma) of the paper


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (values < 2^32) or ints, key: two ints -> the four output words after ten rounds (uint64 arrays)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    mask, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                # < 2^64: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def normals(n, seed, step):
    """z [n] float64: the Box-Muller value of rows 0 .. n - 1 at (seed, step)"""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    rows = np.arange(n, dtype=np.uint64)
    zero = np.zeros(n, dtype=np.uint64)
    x0, x1, _, _ = philox4x32_10((rows, zero, zero + np.uint64(step & MASK), zero + np.uint64(step >> 32)), (seed & MASK, seed >> 32))
    u1 = (x0.astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = (x1.astype(np.float64) + 0.5) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def draws(n, m, std, seed, step, update=True):
    """g [n] float32: the draws of one step; update False (eval): every entry float32(m)"""
    if not update:
        return torch.full((n,), float(np.float32(m)), dtype=torch.float32)
    return torch.from_numpy((m + std * normals(n, seed, step)).astype(np.float32))


def margins_of(g, kind):
    """-> (m_ang, m_add) float32"""
    zero = torch.zeros_like(g)
    return (g, zero) if kind in ("arc", 0) else (zero, g)


def ranks(tcos):
    """tcos [ws, n] or [n] -> (c [n]: maximum over ranks, r [n] int64: the number of rows before row i when the rows are ordered by
    descending c, equal values in row order)"""
    c = tcos.reshape(-1, tcos.shape[-1]).double().max(dim=0).values
    order = torch.sort(-c, stable=True).indices
    r = torch.empty_like(order)
    r[order] = torch.arange(order.numel())
    return c, r


def assign(tcos, g):
    """-> the draws handed out by difficulty [n]: row i gets the ranks(tcos)[i]-th smallest draw"""
    return torch.sort(g, stable=True).values[ranks(tcos)[1]]


def target_cos(ehat, what, labels, subcenters=1):
    """float64 target cosines [n] of one shard from its normalised operands: maximum over the class's centres (plane-major), -2 where the
    label is -1"""
    labels = labels.reshape(-1).long()
    n, c = ehat.shape[0], what.shape[0] // subcenters
    planes = (ehat.double() @ what.double().t()).view(n, subcenters, c).max(dim=1).values
    out = torch.full((n,), -2.0, dtype=torch.float64)
    rows = torch.nonzero(labels >= 0).flatten()
    out[rows] = planes[rows, labels[rows]]
    return out


def row_margins(n, m, std, kind, plus, seed, step, tcos=None, update=True):
    """the margins ElasticFace hands the head for one step -> (m_ang, m_add) float32"""
    g = draws(n, m, std, seed, step, update)
    if plus and update:
        g = assign(tcos, g)
    return margins_of(g, kind)


class ElasticHeadKernels(AdaHeadKernels):
    """adaface_double.AdaHeadKernels plus ElasticFace's three steps: the CPU stand-in for nets.PartialFC.HipHeadKernels on gloo"""

    def elastic_margins(self, n, mg, step, update, bare=False):
        g = draws(n, mg.m, mg.std, mg.seed, int(step), update)
        if update:
            with torch.no_grad():
                step += 1
        return g if bare else margins_of(g, mg.kind)

    def head_target_cos(self, ehat, what, labels_i32, subcenters=1):
        return target_cos(ehat, what, labels_i32, subcenters)

    def elastic_assign(self, tcos, g, mg):
        return margins_of(assign(tcos, g), mg.kind)


# ------------------------------------------------------------------------------------------------ shared inputs
SPECIAL_ROWS = dict(dup_a=0, dup_b=1, no_target=2, over_pi=3, clamp_hi=4)
BORDER_COLS = (0, 63, 64, 127, 128)            # + the last class
T_RANGE = (-0.3, 0.6)                          # the ordinary targets' cosines: an even grid over this range, in a seeded order
MIN_GAP = 1e-4                                 # between two distinct target cosines; the fp32 dot error is d 2^-24 (3.1e-5 at d = 512)


def case(n, classes, d, seed, specials=True):
    """Seeded inputs (float32 tensors; the double upcasts): targets in columns 0, 63, 64, 127, 128 and classes - 1, a duplicate label, a
    label -1 row, one target whose centre is minus the embedding (past pi - eps under an angular margin) and one whose centre is the
    embedding (raw cosine above 1 - eps).  Every other row is built FROM its class centre at a cosine of its own, the cosines an even grid
    over T_RANGE (step 0.9 / n >= 1e-3 for the sizes used), so that no rank is decided by rounding; those rows share a pool of 30 classes
    (a sampled head still draws negatives).  specials=False: the two boundary rows are ordinary rows too (a bf16 head, whose cosines
    must decide no branch).  -> emb [n, d], weight [classes, d], labels [n] int64"""
    g = torch.Generator().manual_seed(seed)
    sr = SPECIAL_ROWS
    wh = torch.randn((classes, d), generator=g, dtype=torch.float64)
    wh = wh / wh.norm(dim=1, keepdim=True)
    cols = list(BORDER_COLS) + [classes - 1]
    taken = set(cols + [10, 12, 20])
    free = [c for c in range(classes) if c not in taken]
    pool = free[::max(1, len(free) // 30)][:30]
    labels = torch.tensor([pool[int(torch.randint(0, len(pool), (1,), generator=g))] for _ in range(n)])
    labels[6:6 + len(cols)] = torch.tensor(cols)
    labels[sr["dup_a"]] = labels[sr["dup_b"]] = 20
    labels[sr["no_target"]] = -1
    labels[sr["over_pi"]], labels[sr["clamp_hi"]] = 10, 12
    emb = torch.randn((n, d), generator=g, dtype=torch.float64)
    emb = emb / emb.norm(dim=1, keepdim=True)
    ordinary = [i for i in range(n) if i != sr["no_target"] and (not specials or i not in (sr["over_pi"], sr["clamp_hi"]))]
    grid = torch.linspace(T_RANGE[0], T_RANGE[1], len(ordinary), dtype=torch.float64)[torch.randperm(len(ordinary), generator=g)]
    for t, i in zip(grid.tolist(), ordinary):
        c = wh[labels[i]]
        perp = emb[i] - (emb[i] @ c) * c
        emb[i] = t * c + math.sqrt(1.0 - t * t) * perp / perp.norm()
    if specials:
        emb[sr["over_pi"]] = -wh[10]
        emb[sr["clamp_hi"]] = wh[12]
    scale = 0.5 + 24.5 * torch.rand(n, generator=g, dtype=torch.float64)
    wscale = 0.2 + 0.2 * torch.rand(classes, generator=g, dtype=torch.float64)
    return (emb * scale[:, None]).float(), (wh * wscale[:, None]).float(), labels


def cosines(emb, weight):
    e, w = emb.double(), weight.double()
    return (e / e.norm(dim=1, keepdim=True)) @ (w / w.norm(dim=1, keepdim=True)).t()


def assert_gaps(tcos, min_gap=MIN_GAP):
    """no two DISTINCT target cosines closer than min_gap: no rank is decided by rounding"""
    gaps = tcos.double().flatten().sort().values.diff()
    gaps = gaps[gaps > 0]
    assert gaps.numel() == 0 or float(gaps.min()) >= min_gap, float(gaps.min())


def assert_case(emb, weight, labels, m, std, kind, eps=EPS, specials=True):
    """what the tests rely on, asserted on the DOUBLE: the special rows are what they claim, every other target stays >= 1e-3 from each
    boundary for margins from m - 5 sigma to m + 5 sigma, no non-target cosine is near the clamp, and the target cosines keep MIN_GAP.
    -> the float64 target cosines [n] (-2 for the row without a target)"""
    sr = SPECIAL_ROWS
    raw = cosines(emb, weight)
    own = torch.nonzero(labels >= 0).flatten()
    tcos = torch.full((labels.numel(),), -2.0, dtype=torch.float64)
    tcos[own] = raw[own, labels[own]]
    for c in list(BORDER_COLS) + [weight.shape[0] - 1]:
        assert int((labels == c).sum()) >= 1, c
    assert labels[sr["dup_a"]] == labels[sr["dup_b"]] and labels[sr["no_target"]] == -1
    lo, hi = m - 5 * std, m + 5 * std
    if specials:
        assert tcos[sr["clamp_hi"]] > 1 - eps
        if kind == "arc":
            assert math.acos(max(float(tcos[sr["over_pi"]]), -1 + eps)) + lo > math.pi - eps
    others = torch.tensor([i for i in own.tolist() if not specials or i not in (sr["over_pi"], sr["clamp_hi"])])
    t = tcos[others]
    assert float((1 - eps - t.abs()).min()) > 1e-3
    for a in ((lo, hi) if kind == "arc" else (0.0,)):
        u = t.acos() + a
        assert float((u - eps).min()) > 1e-3 and float((math.pi - eps - u).min()) > 1e-3
    off = raw.clone()
    off[own, labels[own]] = 0.0
    assert float(off.abs().max()) < 1 - eps - 1e-3
    assert_gaps(tcos)
    return tcos
