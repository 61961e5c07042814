"""Float64 restatement of MagFace (Meng et al., CVPR 2021) as the fused head applies it.  TEST-ONLY.

Everything is float64 and every gradient comes from torch autograd through the clamps, acos and cos of tests/adaface_double.py and the
clamp of the norms below, never from the closed forms the kernels use.

  a = clamp(norm, l_a, u_a);  m_ang = l_m + (u_m - l_m) (a - l_a) / (u_a - l_a);  m_add = 0
  reg = mean over the global batch of a / u_a^2 + 1 / a
  logits: adaface_double.logits (every cosine clamped to [-1 + eps, 1 - eps], target s cos(clip(acos t + m_ang, eps, pi - eps)))
  loss = adaface_double.head_loss (the head's cross-entropy as it is today) + lambda_g reg
The margins are a function of the norms INSIDE the graph, the normalised rows a separate input: autograd yields the gradient along
the normalised rows (what the rows kernels give with the margins held fixed), the centres' gradient and d loss / d norm.
"""
import math

import torch

import adaface_double
from adaface_double import AdaHeadKernels

EPS = adaface_double.EPS
S, L_M, U_M, L_A, U_A, LAMBDA_G = 64.0, 0.45, 0.8, 10.0, 110.0, 35.0


def margins(norms, l_a=L_A, u_a=U_A, l_m=L_M, u_m=U_M):
    """-> m_ang [n], m_add [n] (zeros), reg (0-dim); float64, differentiable in `norms` where they require grad"""
    a = norms.double().reshape(-1).clamp(l_a, u_a)
    m_ang = l_m + (u_m - l_m) * (a - l_a) / (u_a - l_a)
    return m_ang, torch.zeros_like(m_ang), (a / (u_a * u_a) + 1.0 / a).mean()


def head_loss(emb, weight, labels, norms, s=S, l_a=L_A, u_a=U_A, l_m=L_M, u_m=U_M, lambda_g=LAMBDA_G, eps=EPS, head=None):
    """CE + lambda_g reg.  emb only feeds the normalised rows (adaface_double.head_loss divides by its own norm), `norms` feeds margins and
    regulariser: two inputs of the graph.  head: None, or a function with adaface_double.head_loss's signature that replaces it"""
    m_ang, m_add, reg = margins(norms, l_a, u_a, l_m, u_m)
    ce = (head or adaface_double.head_loss)(emb, weight, labels, s, m_ang, m_add, eps)
    return ce + lambda_g * reg


def head_reference(emb, weight, labels, head=None, **kw):
    """-> (loss, d_emb along the normalised rows, d_weight, d_norm), float64 by autograd; the gradient with respect to the un-normalised
    embeddings is d_emb + d_norm[:, None] * emb / |emb|.  head: replaces adaface_double.head_loss (sub-centres)"""
    e = emb.detach().double().requires_grad_(True)
    w = weight.detach().double().requires_grad_(True)
    n = emb.detach().double().norm(dim=1).requires_grad_(True)
    loss = head_loss(e, w, labels, n, head=head, **kw)
    loss.backward()
    return loss.detach(), e.grad, w.grad, n.grad


def target_angle(emb, weight, labels, **kw):
    """u = acos(clamp(raw)) + m_ang of every row's target (NaN without one), the raw cosines, and m_ang"""
    e, w = emb.detach().double(), weight.detach().double()
    raw = (e / e.norm(dim=1, keepdim=True)) @ (w / w.norm(dim=1, keepdim=True)).t()
    m_ang, _, _ = margins(e.norm(dim=1), **kw)
    return adaface_double.target_angle(raw, labels, m_ang, EPS), raw, m_ang


class MagHeadKernels(AdaHeadKernels):
    """adaface_double.AdaHeadKernels plus the two MagFace steps: the CPU stand-in for nets.PartialFC.HipHeadKernels on gloo"""

    def magface_margins(self, norms, mg):
        m_ang, m_add, reg = margins(norms.detach(), mg.l_a, mg.u_a, mg.m, mg.u_margin)
        return m_ang, m_add, reg.reshape(1)

    def magface_norm_grad(self, norms, packed, rmax, rsum, mg, gscale, upstream, out_scale=1.0):
        """By autograd through adaface_double.logits: the target logit as a function of the margin is s cos(clip(theta + m, eps, pi - eps))
        with theta recovered from the stored logit, theta = acos(z / s) - m.  That holds while the clip does not bind; where it binds the
        stored logit is s cos(eps) or its negative (told apart with a float64 guard) and the row's cross-entropy term is dropped."""
        packed = packed.double()
        zt = packed[:, :, 2].max(dim=0).values
        own = zt > float("-inf")
        with torch.enable_grad():
            n = norms.detach().double().requires_grad_(True)
            m_ang, m_add, reg = margins(n, mg.l_a, mg.u_a, mg.m, mg.u_margin)
            cu = torch.where(own, zt / mg.s, torch.zeros_like(zt))
            live = own & (cu.abs() < math.cos(mg.eps) - 1e-12)
            theta = cu.clamp(-1.0, 1.0).acos() - m_ang.detach()
            raw = theta.clamp(0.0, math.pi).cos()[:, None]
            lab = torch.where(own, torch.zeros_like(zt, dtype=torch.long), torch.full_like(zt, -1, dtype=torch.long))
            z = adaface_double.logits(raw, lab, mg.s, m_ang, m_add, mg.eps)[:, 0]
            q = torch.where(own, torch.exp(zt - rmax.double()) / rsum.double(), torch.zeros_like(zt))
            dz = torch.where(live, (q - 1.0) * gscale, torch.zeros_like(zt))
            ((z * dz).sum() + mg.lambda_g * reg).backward()
        return n.grad * float(upstream.double().reshape(-1)[0]) * out_scale


# ------------------------------------------------------------------------------------------------ shared inputs
SPECIAL_ROWS = dict(over_pi=3, clamp_hi=5, dup_a=0, dup_b=1, no_target=2)
COLUMNS = (0, 63, 64, 127, 128)                   # and the last class


def branch_case(n, classes, d, seed):
    """Seeded inputs (float32 tensors; the double upcasts) on which the double itself takes every branch -- `assert_branches` checks it:
    norms from 4 to 140 (several below l_a = 10, several above u_a = 110, the rest inside, none within 0.5 of either end), a target with
    u > pi - eps (centre = -embedding; norm inside the window, so only the regulariser reaches its norm), one with raw cosine above
    1 - eps (centre = embedding, norm inside the window), a duplicate label, a label -1 row, targets in columns 0, 63, 64, 127, 128 and
    classes - 1.  Every other target is a random direction, cosines of a few tenths at most; they share a pool of 30 classes, so a
    sampled head (rate 0.3) still draws negatives.
    -> emb [n, d] (its row norms ARE the norms), weight [classes, d], labels [n] int64"""
    assert n >= 16 and classes >= 140
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn((n, d), generator=g, dtype=torch.float64)
    emb = emb / emb.norm(dim=1, keepdim=True)
    sr = SPECIAL_ROWS
    values = torch.linspace(4.0, 140.0, n, dtype=torch.float64)
    # keep 0.5 clear of both ends of the window (linspace may land anywhere)
    values = torch.where((values - L_A).abs() < 0.5, torch.full_like(values, L_A + 0.75), values)
    values = torch.where((values - U_A).abs() < 0.5, torch.full_like(values, U_A - 0.75), values).tolist()
    fixed = {sr["over_pi"]: values[n // 3], sr["clamp_hi"]: values[n // 2]}      # both inside the window
    rest = [v for i, v in enumerate(values) if i not in (n // 3, n // 2)]
    perm = torch.randperm(len(rest), generator=g).tolist()
    scale = torch.tensor([fixed[i] if i in fixed else rest[perm.pop()] for i in range(n)], dtype=torch.float64)
    weight = torch.randn((classes, d), generator=g, dtype=torch.float64) * 0.05
    labels = torch.randint(0, classes, (n,), generator=g)
    cols = list(COLUMNS) + [classes - 1]
    labels[6:6 + len(cols)] = torch.tensor(cols)
    labels[sr["over_pi"]], labels[sr["clamp_hi"]] = 10, 12
    labels[sr["dup_a"]] = labels[sr["dup_b"]] = 20
    labels[sr["no_target"]] = -1
    taken = set(cols + [10, 12, 20])
    free = [c for c in range(classes) if c not in taken]
    pool = free[::max(1, len(free) // 30)][:30]
    for i in range(6 + len(cols), n):
        labels[i] = pool[int(torch.randint(0, len(pool), (1,), generator=g))]
    labels[4] = pool[0]
    weight[10] = -emb[sr["over_pi"]] * 0.3
    weight[12] = emb[sr["clamp_hi"]] * 0.3
    return (emb * scale[:, None]).float(), weight.float(), labels


def assert_branches(emb, weight, labels, eps=EPS):
    """every branch of the definition is taken by the DOUBLE on these inputs, and nothing else sits near a boundary"""
    norms = emb.double().norm(dim=1)
    assert float(norms.min()) >= 3.9 and float(norms.max()) <= 140.1
    assert int((norms < L_A).sum()) >= 2 and int((norms > U_A).sum()) >= 2 and int(((norms > L_A) & (norms < U_A)).sum()) >= 2
    assert float((norms - L_A).abs().min()) >= 0.5 and float((norms - U_A).abs().min()) >= 0.5
    u, raw, m_ang = target_angle(emb, weight, labels)
    sr = SPECIAL_ROWS
    own = torch.nonzero(labels >= 0).flatten()
    traw = torch.full_like(u, float("nan"))
    traw[own] = raw[own, labels[own]]
    # past pi - eps: d CE / d m is 0 there while the regulariser's term is not (the norm lies inside the window)
    assert u[sr["over_pi"]] > math.pi - eps and L_A < norms[sr["over_pi"]] < U_A
    # raw cosine above 1 - eps: d / d t is 0 (the clamp of the cosine binds) but u = acos(1 - eps) + m is inside its clip, d / d m is not 0
    assert traw[sr["clamp_hi"]] > 1 - eps and L_A < norms[sr["clamp_hi"]] < U_A
    assert eps + 1e-2 < u[sr["clamp_hi"]] < math.pi - eps - 1e-2
    assert labels[sr["dup_a"]] == labels[sr["dup_b"]] and labels[sr["no_target"]] == -1
    for c in list(COLUMNS) + [weight.shape[0] - 1]:
        assert int((labels == c).sum()) >= 1, c
    others = torch.tensor([i for i in own.tolist() if i != sr["over_pi"]])
    assert float((u[others] - eps).min()) >= 1e-2 and float((math.pi - eps - u[others]).min()) >= 1e-2
    off = raw.clone()
    off[own, labels[own]] = 0.0
    assert float(off.abs().max()) < 1 - eps - 1e-3
    return m_ang
