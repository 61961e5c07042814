"""Float64 restatement of CurricularFace (Huang et al., CVPR 2020; the official implementation's rule) as the fused head applies it.
TEST-ONLY.

  c_i      row i's target cosine: the maximum over the ranks' vectors (-2 where a rank does not own the row; a NaN counts as -2), owned
           where it is above -2, then clamped to [-1, 1]
  thr_i    c_i cos m - sqrt(1 - c_i^2) sin m = cos(theta_y + m), no fallback branch; +2 for a row nobody owns
  t        training: t <- alpha mean(c_i over the owned rows) + (1 - alpha) t BEFORE it is used (no owned row: unchanged); eval: only read
  logits   every cosine c = clamp(raw, -1, 1), gradient 0 where the clamp binds; the target by ArcFace's rule (cos(theta + m) above
           cos(pi - m), c - m sin(pi - m) below); a non-target with c > thr_i (strictly) becomes c (t + c); everything x s
  no gradient flows through thr or t; with K sub-centres the pooled cosine is what is compared and scaled (subcenter_double.pool)

Gradients come from torch autograd through the clamps and where() below; `logits` also returns the analytic slope the kernels use, which
tests/test_curricular_cpu.py holds against autograd."""
import math

import torch

from elastic_double import target_cos  # noqa: F401  (the target cosines of one shard, -2 where the label is -1)
from oracle import head_ref
from subcenter_double import SubcenterOracleKernels, cross_entropy, pool

ALPHA = 0.01


def merged(tcos):
    """tcos [ws, n] or [n] -> (c [n] float64 clamped to [-1, 1], owned [n] bool)"""
    t = tcos.detach().double().reshape(-1, tcos.shape[-1])
    t = torch.where(torch.isnan(t), torch.full_like(t, -2.0), t)
    c = t.max(dim=0).values.clamp_min(-2.0)
    return c.clamp(-1.0, 1.0), c > -2.0


def thresholds(tcos, m):
    """-> thr [n] float64"""
    c, owned = merged(tcos)
    thr = c * math.cos(m) - torch.sqrt((1.0 - c) * (1.0 + c)) * math.sin(m)
    return torch.where(owned, thr, torch.full_like(thr, 2.0))


def update_t(tcos, t, alpha=ALPHA):
    """-> the advanced t (float64 scalar tensor); unchanged when nobody owns a row"""
    c, owned = merged(tcos)
    t = (t.detach().double() if torch.is_tensor(t) else torch.tensor(float(t), dtype=torch.float64)).reshape(())
    if not bool(owned.any()):
        return t
    return alpha * c[owned].mean() + (1.0 - alpha) * t


def consts(m):
    return math.cos(m), math.sin(m), math.cos(math.pi - m), math.sin(math.pi - m) * m


def logits(cos, labels, thr, t, s, m):
    """cos [n, C] float64 raw cosines (may require grad), labels [n] (-1: no target), thr [n], t a scalar -> (z [n, C], slope [n, C] =
    the analytic dz / dcos, s included, 0 where the clamp binds)"""
    labels = labels.reshape(-1).long()
    cos_m, sin_m, theta, sinmm = consts(m)
    tt = float(t)
    thr = torch.as_tensor(thr).double().reshape(-1, 1)
    c = cos.clamp(-1.0, 1.0)
    onehot = torch.zeros(cos.shape, dtype=torch.bool)
    rows = torch.nonzero(labels >= 0).flatten()
    onehot[rows, labels[rows]] = True
    ct = torch.where(onehot, c, torch.zeros_like(c))                  # the arc branch is evaluated on the targets alone
    sin_t = torch.sqrt((1.0 - ct * ct).clamp_min(1e-300))
    above = ct.detach() > theta
    zt = torch.where(above, ct * cos_m - sin_t * sin_m, ct - sinmm)
    hard = ~onehot & (c.detach() > thr)
    zn = torch.where(hard, c * (tt + c), c)
    z = torch.where(onehot, zt, zn) * s
    cd = c.detach()
    slope_t = torch.where(above, cos_m + cd * sin_m / sin_t.detach(), torch.ones_like(cd))
    slope_n = torch.where(hard, tt + 2.0 * cd, torch.ones_like(cd))
    inside = (cos.detach() >= -1.0) & (cos.detach() <= 1.0)
    return z, torch.where(onehot, slope_t, slope_n) * s * inside


def hard_mask(cos, labels, thr):
    labels = labels.reshape(-1).long()
    onehot = torch.zeros(cos.shape, dtype=torch.bool)
    rows = torch.nonzero(labels >= 0).flatten()
    onehot[rows, labels[rows]] = True
    return ~onehot & (cos.detach().double().clamp(-1.0, 1.0) > torch.as_tensor(thr).double().reshape(-1, 1))


def head_reference(emb, weight, labels, s, m, thr, t, K=1):
    """the whole head from un-normalised embeddings [n, d] and class centres [K C, d] (plane-major) -> dict(loss, d_emb, d_w, raw [n, C]
    pooled cosines, z, win); float64, gradients by autograd"""
    labels = labels.reshape(-1).long()
    e = emb.detach().double().requires_grad_(True)
    w = weight.detach().double().requires_grad_(True)
    eh = e / e.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    wh = w / w.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    raw, win, _ = pool((eh @ wh.t()).view(e.shape[0], K, w.shape[0] // K))
    z, _ = logits(raw, labels, thr, t, s, m)
    loss = cross_entropy(z, labels)
    loss.backward()
    return dict(loss=loss.detach(), d_emb=e.grad, d_w=w.grad, raw=raw.detach(), z=z.detach(), win=win)


def is_curr(margin):
    return hasattr(margin, "thr")


class CurricularHeadKernels(SubcenterOracleKernels):
    """subcenter_double.SubcenterOracleKernels plus CurricularFace: the CPU stand-in for nets.PartialFC.HipHeadKernels on gloo.  t is the
    module's fp32 buffer, advanced in place like the kernel does (rounded to fp32 once)."""

    def head_target_cos(self, ehat, what, labels_i32, subcenters=1):
        return target_cos(ehat, what, labels_i32, subcenters)

    def curricular_rows(self, tcos, mg, t, update):
        if update:
            with torch.no_grad():
                t.copy_(update_t(tcos, t, mg.alpha).reshape(t.shape))
        return thresholds(tcos, mg.m)

    def _z(self, ehat, what, labels_i32, margin, subcenters):
        n, c = ehat.shape[0], what.shape[0] // subcenters
        raw, win, _ = pool((ehat @ what.t()).view(n, subcenters, c))
        return logits(raw, labels_i32, margin.thr, margin.t, margin.s, margin.m)[0], win

    def forward_stats(self, ehat, what, labels_i32, s, m, margin=None, subcenters=1):
        if not is_curr(margin):
            return super().forward_stats(ehat, what, labels_i32, s, m, margin=margin, subcenters=subcenters)
        z, win = self._z(ehat.double(), what.double(), labels_i32, margin, subcenters)
        n = z.shape[0]
        rmax = z.max(dim=1).values
        rsum = torch.exp(z - rmax[:, None]).sum(dim=1)
        zt = torch.zeros(n, dtype=torch.float64)
        tsub = torch.full((n,), -1, dtype=torch.int32)
        rows = torch.nonzero(labels_i32 >= 0).flatten()
        zt[rows] = z[rows, labels_i32[rows].long()]
        tsub[rows] = win[rows, labels_i32[rows].long()].to(torch.int32)
        return (zt, rmax, rsum, tsub) if subcenters > 1 else (zt, rmax, rsum)

    def backward(self, ehat, enorm, what, wnorm, labels_i32, s, m, rmax, rsum, n_global, upstream, e_scale=1.0, on_de=None,
                 margin=None, subcenters=1):
        if not is_curr(margin):
            return super().backward(ehat, enorm, what, wnorm, labels_i32, s, m, rmax, rsum, n_global, upstream, e_scale, on_de,
                                    margin=margin, subcenters=subcenters)
        with torch.enable_grad():
            eh = ehat.detach().double().requires_grad_(True)
            wh = what.detach().double().requires_grad_(True)
            z, _ = self._z(eh, wh, labels_i32, margin, subcenters)
            dz = torch.exp(z.detach() - rmax.double()[:, None]) / rsum.double()[:, None]      # softmax over ALL shards
            rows = torch.nonzero(labels_i32 >= 0).flatten()
            dz[rows, labels_i32[rows].long()] -= 1.0
            dz = dz / n_global * upstream.double()
            (z * dz).sum().backward()
        d_e = (head_ref.l2_normalize_bwd(eh.grad, ehat.double(), enorm.double()[:, None]) * e_scale).to(ehat.dtype)
        if on_de is not None:
            on_de(d_e)
        return d_e, head_ref.l2_normalize_bwd(wh.grad, what.double(), wnorm.double()[:, None]).to(what.dtype)


# ------------------------------------------------------------------------------------------------ shared inputs
ROWS = dict(dup_a=0, dup_b=1, no_target=2)
BORDER_COLS = (0, 63, 64, 127, 128)            # + the last class
T_RANGE = (-0.3, 0.9)                          # the targets' cosines: an even grid over this range, in a seeded order
BAND = 2e-4                                    # asserted: no non-target cosine closer than this to its row's threshold
BUILD_BAND = 3e-4                              # what the builder keeps clear (the bf16 head re-normalises on the device)
NUDGE, MAX_NUDGES = 3e-4, 40


def _row(t, c, perp):
    return t * c + math.sqrt(1.0 - t * t) * perp


def _round(x, dtype):
    """unit rows as the head's compute dtype holds them"""
    return x.float().to(dtype).double()


def case(n, classes, d, seed, m=0.5, dtype=torch.float32):
    """Seeded inputs (float32 tensors; the double upcasts) on which no branch of CurricularFace is decided by rounding.  Every row with a
    target is built FROM its class centre at a target cosine of its own, an even grid over T_RANGE in a seeded order: low targets make
    every negative hard, high ones none, those in between some.  Where a row has a non-target cosine within BUILD_BAND of its threshold,
    its target cosine is nudged by NUDGE until the row is clean.  Targets sit in columns 0, 63, 64, 127, 128 and classes - 1 (where there
    are that many classes), there is a duplicate label and a label -1 row; the other rows share a pool of 30 classes (a sampled head still
    draws negatives).  dtype: the compute dtype whose rounding of the unit rows the band is evaluated on.
    -> emb [n, d], weight [classes, d], labels [n] int64, nudges (the largest number a row needed)"""
    g = torch.Generator().manual_seed(seed)
    wh = torch.randn((classes, d), generator=g, dtype=torch.float64)
    wh = wh / wh.norm(dim=1, keepdim=True)
    cols = [c for c in BORDER_COLS if c < classes - 1] + [classes - 1]
    taken = set(cols + [20])
    free = [c for c in range(classes) if c not in taken]
    pool_ = free[::max(1, len(free) // 30)][:30]
    labels = torch.tensor([pool_[int(torch.randint(0, len(pool_), (1,), generator=g))] for _ in range(n)])
    k = min(len(cols), n - 3)
    labels[3:3 + k] = torch.tensor(cols[len(cols) - k:])
    labels[ROWS["dup_a"]] = labels[ROWS["dup_b"]] = 20
    labels[ROWS["no_target"]] = -1
    emb = torch.randn((n, d), generator=g, dtype=torch.float64)
    emb = emb / emb.norm(dim=1, keepdim=True)
    owned = [i for i in range(n) if i != ROWS["no_target"]]
    grid = torch.linspace(T_RANGE[0], T_RANGE[1], len(owned), dtype=torch.float64)[torch.randperm(len(owned), generator=g)]
    whr = _round(wh, dtype)
    cos_m, sin_m = math.cos(m), math.sin(m)
    worst = 0
    for t0, i in zip(grid.tolist(), owned):
        c = wh[labels[i]]
        perp = emb[i] - (emb[i] @ c) * c
        perp = perp / perp.norm()
        for tries in range(MAX_NUDGES + 1):
            row = _row(t0 + tries * NUDGE * (-1.0 if t0 > 0.3 else 1.0), c, perp)
            cs = whr @ _round(row, dtype)
            tc = float(cs[labels[i]])
            thr = tc * cos_m - math.sqrt(max(0.0, 1.0 - tc * tc)) * sin_m
            cs[labels[i]] = thr + 1.0
            if float((cs - thr).abs().min()) >= BUILD_BAND:
                break
        else:
            raise AssertionError("row %d: no target cosine within %d nudges keeps the band clear" % (i, MAX_NUDGES))
        worst = max(worst, tries)
        emb[i] = row
    scale = 0.5 + 24.5 * torch.rand(n, generator=g, dtype=torch.float64)
    wscale = 0.2 + 0.2 * torch.rand(classes, generator=g, dtype=torch.float64)
    return (emb * scale[:, None]).float(), (wh * wscale[:, None]).float(), labels, worst


def assert_case(raw, labels, m, need_kinds=True):
    """the condition the head tests rest on, asserted on the DOUBLE's cosines `raw` [n, C] (of the operands the head sees): every
    non-target cosine >= BAND from its row's threshold and >= 1e-3 from +-1, every target >= 1e-3 from theta and from +-1; rows whose
    negatives are all hard, rows with none, and mixed rows all occur.  -> (tcos [n] float64, -2 without a target; thr [n]; hard [n, C])"""
    labels = labels.reshape(-1).long()
    raw = raw.detach().double()
    own = torch.nonzero(labels >= 0).flatten()
    tcos = torch.full((labels.numel(),), -2.0, dtype=torch.float64)
    tcos[own] = raw[own, labels[own]]
    thr = thresholds(tcos, m)
    theta = math.cos(math.pi - m)
    assert float((tcos[own] - theta).abs().min()) >= 1e-3 and float((1.0 - tcos[own].abs()).min()) >= 1e-3
    off = raw.clone()
    off[own, labels[own]] = float("nan")
    gap = (off - thr[:, None]).abs()
    gap = gap[~torch.isnan(gap)]
    assert float(gap.min()) >= BAND, float(gap.min())
    edge = (1.0 - off.abs())
    assert float(edge[~torch.isnan(edge)].min()) >= 1e-3
    hard = hard_mask(raw, labels, thr)
    if need_kinds:
        per_row = hard[own].sum(dim=1)
        full = raw.shape[1] - 1
        assert int((per_row == full).sum()) >= 1 and int((per_row == 0).sum()) >= 1 and int(((per_row > 0) & (per_row < full)).sum()) >= 1
        assert int(hard[labels < 0].sum()) == 0                       # nobody owns the row: thr = +2, nothing in it is hard
    return tcos, thr, hard


def cosines(emb, weight):
    e, w = emb.double(), weight.double()
    return (e / e.norm(dim=1, keepdim=True)) @ (w / w.norm(dim=1, keepdim=True)).t()
