"""Float64 restatement of the sigmoid (binary cross-entropy) head, UniFace / SphereFace2 with t = 1, as the fused head applies it.
TEST-ONLY.

  c        every cosine clamp(raw, -1, 1), gradient 0 where the clamp binds (loss and bias terms still count); with K sub-centres the
           pooled cosine (subcenter_double.pool)
  target   a = s phi(c) - b; kind COS: phi = c - m; kind ARC: cos(theta + m) above cos(pi - m), c - m sin(pi - m) below;
           term w_pos softplus(-a), d/dc = -w_pos sigmoid(-a) s slope, d/db = +w_pos sigmoid(-a)
  other    a = s (c + m_neg) - b; term w_neg softplus(a), d/dc = w_neg sigmoid(a) s, d/db = -w_neg sigmoid(a)
  loss     (1 / N_global) sum of the terms over all rows and all classes of all shards; dbias the same sum of the d/db

`terms` is the rule written out with its analytic derivatives; `autograd_terms` is the same expression left to torch autograd
(softplus as -logsigmoid(-x) of torch.nn.functional).  tests/test_uniface_cpu.py holds one against the other."""
import math

import torch

from oracle import head_ref
from subcenter_double import SubcenterOracleKernels, pool

ARC, COS = 0, 1
KINDS = {"arc": ARC, "cos": COS}


def _onehot(shape, labels):
    labels = labels.reshape(-1).long()
    onehot = torch.zeros(shape, dtype=torch.bool)
    rows = torch.nonzero(labels >= 0).flatten()
    onehot[rows, labels[rows]] = True
    return onehot


def _softplus(x):
    return x.clamp_min(0.0) + torch.log1p(torch.exp(-x.abs()))


def _sigmoid(a):
    e = torch.exp(-a.abs())
    return torch.where(a >= 0, torch.ones_like(e), e) / (1.0 + e)


def phi(c, kind, m):
    """the target's margin on clamped cosines -> (value, slope)"""
    if kind == COS:
        return c - m, torch.ones_like(c)
    cos_m, sin_m, theta, sinmm = math.cos(m), math.sin(m), math.cos(math.pi - m), math.sin(math.pi - m) * m
    sin_t = torch.sqrt((1.0 - c * c).clamp_min(1e-300))
    above = c > theta
    return torch.where(above, c * cos_m - sin_t * sin_m, c - sinmm), torch.where(above, cos_m + c * sin_m / sin_t, torch.ones_like(c))


def terms(raw, labels, mg, b):
    """raw [n, C] float64 cosines, labels [n] (-1: no target), mg = (kind, s, m, m_neg, w_pos, w_neg), b a float
    -> (term [n, C], dcos [n, C] = d term / d raw, db [n, C] = d term / d b, a [n, C]); the rule written out, no autograd"""
    kind, s, m, m_neg, w_pos, w_neg = mg
    raw = raw.detach().double()
    onehot = _onehot(raw.shape, labels)
    c = raw.clamp(-1.0, 1.0)
    inside = ((raw >= -1.0) & (raw <= 1.0)).double()
    p, slope = phi(torch.where(onehot, c, torch.zeros_like(c)), int(kind), m)
    a_t, a_n = s * p - b, s * (c + m_neg) - b
    a = torch.where(onehot, a_t, a_n)
    term = torch.where(onehot, w_pos * _softplus(-a_t), w_neg * _softplus(a_n))
    db = torch.where(onehot, w_pos * _sigmoid(-a_t), -w_neg * _sigmoid(a_n))
    dcos = torch.where(onehot, -w_pos * _sigmoid(-a_t) * s * slope, w_neg * _sigmoid(a_n) * s) * inside
    return term, dcos, db, a


def autograd_terms(raw, labels, mg, b):
    """the same expression for torch autograd: raw and b (a 0-dim float64 tensor) may require grad -> term [n, C]"""
    kind, s, m, m_neg, w_pos, w_neg = mg
    onehot = _onehot(raw.shape, labels)
    c = raw.clamp(-1.0, 1.0)
    ct = torch.where(onehot, c, torch.zeros_like(c))            # the arc branch is evaluated on the targets alone
    if int(kind) == COS:
        p = ct - m
    else:
        above = ct.detach() > math.cos(math.pi - m)
        p = torch.where(above, torch.cos(torch.acos(ct.clamp(-1 + 1e-15, 1 - 1e-15)) + m), ct - math.sin(math.pi - m) * m)
    # softplus(x) = -logsigmoid(-x); F.softplus itself turns linear above its threshold of 20, an error of e^-20 = 2e-9 in the gradient
    sp = lambda x: -torch.nn.functional.logsigmoid(-x)      # noqa: E731
    return torch.where(onehot, w_pos * sp(-(s * p - b)), w_neg * sp(s * (c + m_neg) - b))


def head_reference(emb, weight, labels, mg, b, K=1, autograd=True):
    """the whole head from un-normalised embeddings [n, d] and class centres [K C, d] (plane-major) -> dict(loss, d_emb, d_w, dbias, raw
    [n, C] pooled cosines, win, a).  float64.  autograd=True: the gradients are torch's of autograd_terms; False: the written-out
    dcos / db of `terms` pushed back through the normalisations (what the kernels do)."""
    labels = labels.reshape(-1).long()
    n = emb.shape[0]
    e = emb.detach().double().requires_grad_(True)
    w = weight.detach().double().requires_grad_(True)
    bt = torch.tensor(float(b), dtype=torch.float64, requires_grad=True)
    eh = e / e.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    wh = w / w.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    raw, win, _ = pool((eh @ wh.t()).view(n, K, w.shape[0] // K))
    term, dcos, db, a = terms(raw, labels, mg, float(b))
    if autograd:
        loss = autograd_terms(raw, labels, mg, bt).sum() / n
        loss.backward()
        dbias = bt.grad
    else:
        loss = term.sum() / n
        (raw * (dcos / n)).sum().backward()
        dbias = db.sum() / n
    return dict(loss=loss.detach(), d_emb=e.grad, d_w=w.grad, dbias=dbias.detach(), raw=raw.detach(), win=win, a=a, term=term, db=db,
                dcos=dcos)


def is_bce(margin):
    return hasattr(margin, "bias")


def _mg(margin):
    return (margin.kind, margin.s, margin.m, margin.m_neg, margin.w_pos, margin.w_neg)


class UniHeadKernels(SubcenterOracleKernels):
    """subcenter_double.SubcenterOracleKernels plus the sigmoid head: the CPU stand-in for nets.PartialFC.HipHeadKernels on gloo"""

    def _terms(self, ehat, what, labels_i32, margin, subcenters):
        n, c = ehat.shape[0], what.shape[0] // subcenters
        raw, win, _ = pool((ehat @ what.t()).view(n, subcenters, c))
        return raw, win, terms(raw, labels_i32, _mg(margin), float(margin.bias))

    def forward_stats(self, ehat, what, labels_i32, s, m, margin=None, subcenters=1):
        if not is_bce(margin):
            return super().forward_stats(ehat, what, labels_i32, s, m, margin=margin, subcenters=subcenters)
        _, win, (term, _, db, a) = self._terms(ehat.double(), what.double(), labels_i32, margin, subcenters)
        n = term.shape[0]
        zt = torch.zeros(n, dtype=torch.float64)
        tsub = torch.full((n,), -1, dtype=torch.int32)
        rows = torch.nonzero(labels_i32 >= 0).flatten()
        zt[rows] = a[rows, labels_i32[rows].long()]
        tsub[rows] = win[rows, labels_i32[rows].long()].to(torch.int32)
        out = (zt, term.sum(dim=1), db.sum(dim=1))
        return out + (tsub,) if subcenters > 1 else out

    def bce_reduce(self, rowloss, rowdb):
        return torch.stack([rowloss.double().sum(), rowdb.double().sum()])

    def bce_merge(self, gathered, n_global):
        g = gathered.double().reshape(-1, 2)
        loss, db = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
        for r in range(g.shape[0]):                      # rank order
            loss, db = loss + g[r, 0], db + g[r, 1]
        return (loss / n_global).reshape(1), (db / n_global).reshape(1)

    def backward(self, ehat, enorm, what, wnorm, labels_i32, s, m, rmax, rsum, n_global, upstream, e_scale=1.0, on_de=None,
                 margin=None, subcenters=1):
        if not is_bce(margin):
            return super().backward(ehat, enorm, what, wnorm, labels_i32, s, m, rmax, rsum, n_global, upstream, e_scale, on_de,
                                    margin=margin, subcenters=subcenters)
        assert rmax is None and rsum is None                # the sigmoid head hands over no row statistics
        with torch.enable_grad():
            eh = ehat.detach().double().requires_grad_(True)
            wh = what.detach().double().requires_grad_(True)
            raw, _, (_, dcos, _, _) = self._terms(eh, wh, labels_i32, margin, subcenters)
            (raw * (dcos / n_global * upstream.double())).sum().backward()
        d_e = (head_ref.l2_normalize_bwd(eh.grad, ehat.double(), enorm.double()[:, None]) * e_scale).to(ehat.dtype)
        if on_de is not None:
            on_de(d_e)
        return d_e, head_ref.l2_normalize_bwd(wh.grad, what.double(), wnorm.double()[:, None]).to(what.dtype)


# ------------------------------------------------------------------------------------------------ shared inputs
ROWS = dict(dup_a=0, dup_b=1, no_target=2, low=3)
BORDER_COLS = (0, 63, 64, 127, 128)            # + the last class: the borders of the kernel's 64-column groups and 128-column tiles
T_RANGE = (-0.3, 0.9)                          # the targets' cosines: an even grid over this range, in a seeded order
T_LOW = -0.96                                  # row `low`: below cos(pi - m) for the margins the tests use: ArcFace's lower branch
_CASES = {}


def case(n, classes, d, seed):
    """Seeded inputs (float32 tensors; the double upcasts), built once per key and shared: never modify them.  Every row with a target is
    built FROM its class centre at a target cosine of its own (an even grid over T_RANGE in a seeded order; row `low` at T_LOW), so both
    branches of the arc rule and both tails of the sigmoid occur.  Targets sit in columns 0, 63, 64, 127, 128 and classes - 1 (where there
    are that many classes), there is a duplicate label and a label -1 row; the other rows share a pool of 30 classes (a sampled head
    still draws negatives).  -> emb [n, d], weight [classes, d], labels [n] int64"""
    key = (n, classes, d, seed)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(seed)
    wh = torch.randn((classes, d), generator=g, dtype=torch.float64)
    wh = wh / wh.norm(dim=1, keepdim=True)
    cols = [c for c in BORDER_COLS if c < classes - 1] + [classes - 1]
    taken = set(cols + [min(20, classes - 1)])
    free = [c for c in range(classes) if c not in taken] or [0]
    pool_ = free[::max(1, len(free) // 30)][:30]
    labels = torch.tensor([pool_[int(torch.randint(0, len(pool_), (1,), generator=g))] for _ in range(n)])
    k = max(0, min(len(cols), n - 4))
    if k:
        labels[4:4 + k] = torch.tensor(cols[len(cols) - k:])
    if n > ROWS["dup_b"]:
        labels[ROWS["dup_a"]] = labels[ROWS["dup_b"]] = min(20, classes - 1)
    if n > ROWS["no_target"]:
        labels[ROWS["no_target"]] = -1
    emb = torch.randn((n, d), generator=g, dtype=torch.float64)
    emb = emb / emb.norm(dim=1, keepdim=True)
    owned = [i for i in range(n) if int(labels[i]) >= 0]
    grid = torch.linspace(T_RANGE[0], T_RANGE[1], len(owned), dtype=torch.float64)[torch.randperm(len(owned), generator=g)]
    for t0, i in zip(grid.tolist(), owned):
        t0 = T_LOW if i == ROWS["low"] else t0
        c = wh[labels[i]]
        perp = emb[i] - (emb[i] @ c) * c
        perp = perp / perp.norm()
        emb[i] = t0 * c + math.sqrt(1.0 - t0 * t0) * perp
    scale = 0.5 + 24.5 * torch.rand(n, generator=g, dtype=torch.float64)
    wscale = 0.2 + 0.2 * torch.rand(classes, generator=g, dtype=torch.float64)
    _CASES[key] = ((emb * scale[:, None]).float(), (wh * wscale[:, None]).float(), labels)
    return _CASES[key]


def cosines(emb, weight):
    e, w = emb.double(), weight.double()
    return (e / e.norm(dim=1, keepdim=True)) @ (w / w.norm(dim=1, keepdim=True)).t()


def assert_case(raw, labels, kind, m, need_unowned=True):
    """the condition the tests rest on, asserted on the DOUBLE's cosines `raw` [n, C] (of the operands the head sees): every cosine >= 1e-3
    from +-1; for kind ARC every target >= 1e-3 from cos(pi - m); a label -1 row occurs"""
    labels = labels.reshape(-1).long()
    raw = raw.detach().double()
    assert float((1.0 - raw.abs()).min()) >= 1e-3, float((1.0 - raw.abs()).min())
    own = torch.nonzero(labels >= 0).flatten()
    if int(kind) == ARC and own.numel():
        gap = (raw[own, labels[own]] - math.cos(math.pi - m)).abs()
        assert float(gap.min()) >= 1e-3, float(gap.min())
    if need_unowned:
        assert int((labels < 0).sum()) >= 1
