"""Float64 restatement of AdaFace's per-row margin (Kim et al., CVPR 2022) as the fused head applies it.  TEST-ONLY.

Everything is float64 and every gradient comes from torch autograd through the clamps, acos and cos below, never from the slope formula
the kernels use.

  sn = clip(norms, 0.001, 100); mean, std (unbiased) over the global batch
  training: batch_mean <- t_alpha mean + (1 - t_alpha) batch_mean, batch_std likewise, used in this same step; eval: only read
  k = clip(h (sn - batch_mean) / (batch_std + eps), -1, 1);  a = -m k;  b = m + m k
  t = clamp(raw, -1 + eps, 1 - eps);  non-target z = s t;  target z = s (cos(clip(acos(t) + a, eps, pi - eps)) - b)
  softmax cross-entropy over all classes exactly as the head computes it today: value -mean(log(max(q, 1e-30))), gradient
  softmax - onehot; a row without a target (label -1) therefore contributes -log(1e-30) and the gradient of its log-sum-exp.
"""
import math

import torch

from head_double import OracleHeadKernels
from oracle import head_ref

EPS = 1e-3
NO_TARGET = -math.log(1e-30)


def margins(norms, m, h, t_alpha, batch_mean, batch_std, update, eps=EPS):
    """-> dict(m_ang, m_add, k [n]; batch_mean, batch_std: the values used in this step, float64 scalars).  Changes no argument."""
    sn = norms.detach().double().reshape(-1).clamp(0.001, 100.0)
    mean, std = sn.mean(), sn.std(unbiased=True)
    bm, bs = torch.as_tensor(batch_mean).double().reshape(()), torch.as_tensor(batch_std).double().reshape(())
    if update:
        bm = t_alpha * mean + (1.0 - t_alpha) * bm
        bs = t_alpha * std + (1.0 - t_alpha) * bs
    k = (h * (sn - bm) / (bs + eps)).clamp(-1.0, 1.0)
    return dict(m_ang=-m * k, m_add=m + m * k, k=k, batch_mean=bm, batch_std=bs)


def target_angle(raw, labels, m_ang, eps=EPS):
    """u = acos(clamp(raw)) + a of every row's target (NaN for a row without one): what the tests assert the branches on"""
    labels = labels.reshape(-1).long()
    t = raw.detach().double().clamp(-1.0 + eps, 1.0 - eps)
    u = torch.full((raw.shape[0],), float("nan"), dtype=torch.float64)
    rows = torch.nonzero(labels >= 0).flatten()
    u[rows] = t[rows, labels[rows]].acos() + m_ang.double()[rows]
    return u


def logits(raw, labels, s, m_ang, m_add, eps=EPS):
    """raw [n, C] float64 cosines (may require grad), labels [n] (-1: no target) -> z [n, C]"""
    labels = labels.reshape(-1).long()
    t = raw.clamp(-1.0 + eps, 1.0 - eps)
    onehot = torch.zeros(raw.shape, dtype=torch.bool)
    rows = torch.nonzero(labels >= 0).flatten()
    onehot[rows, labels[rows]] = True
    u = t.acos() + m_ang.double()[:, None]
    zt = u.clamp(eps, math.pi - eps).cos() - m_add.double()[:, None]
    return torch.where(onehot, zt, t) * s


def head_loss(emb, weight, labels, s, m_ang, m_add, eps=EPS):
    """loss of the whole head from un-normalised embeddings [n, d] and class centres [C, d] (float64, may require grad)"""
    labels = labels.reshape(-1).long()
    eh = emb / emb.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    wh = weight / weight.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    z = logits(eh @ wh.t(), labels, s, m_ang, m_add, eps)
    lse = torch.logsumexp(z, dim=1)
    own = labels >= 0
    zt = z.gather(1, labels.clamp(min=0)[:, None]).flatten()
    per_row = torch.where(own, lse - zt, lse - lse.detach() + NO_TARGET)
    # the head's cross-entropy, as it is today: the VALUE is -log(max(q, 1e-30)), the gradient is softmax - onehot whether or not that
    # floor binds (the reference's DistCrossEntropyFunc, nets/PartialFC.py:441-484; a target pushed past pi - eps at s = 64 reaches it)
    value = per_row.detach().clamp(max=NO_TARGET)
    return (per_row + (value - per_row.detach())).mean()


def head_reference(emb, weight, labels, s, m_ang, m_add, eps=EPS):
    """-> (loss, d_emb, d_weight) float64 by autograd"""
    e = emb.detach().double().requires_grad_(True)
    w = weight.detach().double().requires_grad_(True)
    loss = head_loss(e, w, labels, s, m_ang, m_add, eps)
    loss.backward()
    return loss.detach(), e.grad, w.grad


class AdaHeadKernels(OracleHeadKernels):
    """tests/head_double.OracleHeadKernels plus the per-row margin: the CPU stand-in for nets.PartialFC.HipHeadKernels on gloo.
    Computes in float64 whatever it is given (autograd casts the gradient of an fp32 parameter back); gradients by autograd
    through `logits`."""

    def normalize(self, x):
        xh, n = head_ref.l2_normalize(x.detach().double())
        return xh, n.reshape(-1)

    def adaface_margins(self, norms, mg, batch_mean, batch_std, update):
        r = margins(norms, mg.m, mg.h, mg.t_alpha, batch_mean, batch_std, update, mg.eps)
        if update:
            with torch.no_grad():
                batch_mean.copy_(r["batch_mean"].reshape(batch_mean.shape))
                batch_std.copy_(r["batch_std"].reshape(batch_std.shape))
        return r["m_ang"], r["m_add"]

    def forward_stats(self, ehat, what, labels_i32, s, m, margin=None):
        if margin is None:
            return super().forward_stats(ehat, what, labels_i32, s, m)
        z = logits(ehat.double() @ what.double().t(), labels_i32, margin.s, margin.m_ang, margin.m_add, margin.eps)
        rmax = z.max(dim=1).values
        rsum = torch.exp(z - rmax[:, None]).sum(dim=1)
        zt = torch.zeros(z.shape[0], dtype=torch.float64)
        rows = torch.nonzero(labels_i32 >= 0).flatten()
        zt[rows] = z[rows, labels_i32[rows].long()]
        return zt, rmax, rsum

    def backward(self, ehat, enorm, what, wnorm, labels_i32, s, m, rmax, rsum, n_global, upstream, e_scale=1.0, on_de=None,
                 margin=None):
        if margin is None:
            return super().backward(ehat, enorm, what, wnorm, labels_i32, s, m, rmax, rsum, n_global, upstream, e_scale, on_de)
        with torch.enable_grad():
            eh = ehat.detach().double().requires_grad_(True)
            wh = what.detach().double().requires_grad_(True)
            z = logits(eh @ wh.t(), labels_i32, margin.s, margin.m_ang, margin.m_add, margin.eps)
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
SPECIAL_ROWS = dict(over_pi=3, under_eps=4, clamp_hi=5, dup_a=0, dup_b=1, no_target=2)
BUFFERS = (10.0, 2.0)        # batch_mean, batch_std the tests start from: the initial 20 / 100 never reach the clips of k


def branch_case(n, classes, d, seed):
    """Seeded inputs (float32 tensors; the double upcasts) on which the double itself takes every branch -- `assert_branches` checks it:
    norms from 0.5 to 25 (k at -1, inside, at +1 with BUFFERS), a target with u > pi - eps (centre = -embedding, smallest norms), one with
    u < eps (centre at cosine 0.97 of the embedding, largest norms), one with raw > 1 - eps (centre = embedding), a duplicate label, a
    label -1 row, and targets in columns 0, 63, 64, 127, 128 and classes - 1.  Every other target is a random direction: cosines of a few
    tenths at most, far from every boundary; they share a pool of 30 classes, so a sampled head (rate 0.3) still draws negatives.
    -> emb [n, d] (its row norms ARE the norms), weight [classes, d], labels [n] int64"""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn((n, d), generator=g, dtype=torch.float64)
    emb = emb / emb.norm(dim=1, keepdim=True)
    sr = SPECIAL_ROWS
    # the row that must have k = -1 gets the smallest norm, the one that must have k = +1 the largest, the clamp row the middle one;
    # the other norms go to the other rows in a seeded order
    values = torch.linspace(0.5, 25.0, n, dtype=torch.float64).tolist()
    fixed = {sr["over_pi"]: values[0], sr["under_eps"]: values[-1], sr["clamp_hi"]: values[n // 2]}
    rest = [v for i, v in enumerate(values) if i not in (0, n - 1, n // 2)]
    perm = torch.randperm(len(rest), generator=g).tolist()
    scale = torch.tensor([fixed[i] if i in fixed else rest[perm.pop()] for i in range(n)], dtype=torch.float64)
    weight = torch.randn((classes, d), generator=g, dtype=torch.float64) * 0.05
    labels = torch.randint(0, classes, (n,), generator=g)
    cols = [0, 63, 64, 127, 128, classes - 1]
    labels[6:6 + len(cols)] = torch.tensor(cols)
    labels[sr["over_pi"]], labels[sr["under_eps"]], labels[sr["clamp_hi"]] = 10, 11, 12
    labels[sr["dup_a"]] = labels[sr["dup_b"]] = 20
    labels[sr["no_target"]] = -1
    # no other row may share a class with a special row (its centre is about to be set), nor with another special column
    taken = set(cols + [10, 11, 12, 20])
    free = [c for c in range(classes) if c not in taken]
    pool = free[::max(1, len(free) // 30)][:30]
    for i in range(6 + len(cols), n):
        labels[i] = pool[int(torch.randint(0, len(pool), (1,), generator=g))]
    weight[10] = -emb[sr["over_pi"]] * 0.3
    r = torch.randn(d, generator=g, dtype=torch.float64)
    e = emb[sr["under_eps"]]
    perp = r - (r @ e) * e
    weight[11] = (0.97 * e + math.sqrt(1 - 0.97 ** 2) * perp / perp.norm()) * 0.3
    weight[12] = emb[sr["clamp_hi"]] * 0.3
    return (emb * scale[:, None]).float(), weight.float(), labels


def assert_branches(emb, weight, labels, norms, s, m, h, t_alpha, eps=EPS, update=True):
    """every branch of the definition is taken by the DOUBLE on these inputs, and nothing else sits within 1e-3 of a boundary"""
    mr = margins(norms, m, h, t_alpha, BUFFERS[0], BUFFERS[1], update, eps)
    k = mr["k"]
    assert int((k == -1).sum()) >= 2 and int((k == 1).sum()) >= 2 and int(((k > -0.9) & (k < 0.9)).sum()) >= 2
    e, w = emb.double(), weight.double()
    raw = (e / e.norm(dim=1, keepdim=True)) @ (w / w.norm(dim=1, keepdim=True)).t()
    u = target_angle(raw, labels, mr["m_ang"], eps)
    sr = SPECIAL_ROWS
    own = torch.nonzero(labels >= 0).flatten()
    traw = torch.full_like(u, float("nan"))
    traw[own] = raw[own, labels[own]]
    assert u[sr["over_pi"]] > math.pi - eps and k[sr["over_pi"]] == -1
    assert u[sr["under_eps"]] < eps and k[sr["under_eps"]] == 1 and traw[sr["under_eps"]] < 1 - eps
    assert traw[sr["clamp_hi"]] > 1 - eps
    assert labels[sr["dup_a"]] == labels[sr["dup_b"]] and labels[sr["no_target"]] == -1
    for c in (0, 63, 64, 127, 128, weight.shape[0] - 1):
        assert int((labels == c).sum()) >= 1, c
    others = torch.tensor([i for i in own.tolist() if i not in (sr["over_pi"], sr["under_eps"], sr["clamp_hi"])])
    assert float((1 - eps - traw[others].abs()).min()) > 1e-3
    assert float((u[others] - eps).min()) > 1e-3 and float((math.pi - eps - u[others]).min()) > 1e-3
    # no non-target cosine is anywhere near the clamp
    off = raw.clone()
    off[own, labels[own]] = 0.0
    assert float(off.abs().max()) < 1 - eps - 1e-3
    return mr
