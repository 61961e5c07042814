"""Float64 restatement of the sub-centre head (sub-center ArcFace, Deng et al., ECCV 2020) as the fused head applies it.  TEST-ONLY.

  K centres per class, plane-major: centre k of class c is row k * C + c of the table, each normalised on its own
  cos_c = max_k <xhat, what[k C + c]>, won by the FIRST index of the maximum (an exact tie goes to the lowest k)
  then everything the head does to a cosine today: clamp, the target's margin, interclass filtering, x s, softmax cross-entropy
  (value -mean(log(max(q, 1e-30))), gradient softmax - onehot; a label -1 row contributes -log(1e-30) and the gradient of its log-sum-exp)

The winner is computed explicitly and the pooled cosine is GATHERED at it, so autograd sends the gradient of a (row, class) to the winning
centre alone and an exact 0 to the others -- the definition, not torch.max's unspecified choice among equals.  Gradients come from autograd
through the margin restatements the other doubles use (tests/margin_formula.py, tests/adaface_double.py), never from the kernels' slope
formula.  At K = 1 it is tied to oracle.head_ref (tests/test_subcenter_cpu.py)."""
import math

import torch

import adaface_double
import margin_formula
from adaface_double import AdaHeadKernels
from oracle import head_ref

NO_TARGET = -math.log(1e-30)
GAP = 1e-5              # 2.6 x the worst-case fp32 error of a 64-term dot product of unit vectors (64 x 2^-24 = 3.8e-6)
TIE_CLASS = 10
BORDER_COLS = (0, 63, 64, 127, 128)      # + the last class: the borders of the kernel's 64-column groups and 128-column tiles


def is_rows(margin):
    return hasattr(margin, "m_ang")


def winners(planes):
    """planes [n, K, C] cosines -> (win [n, C] int64: first index of the maximum over K, gap [n, C]: best minus second best, inf at K = 1)"""
    n, k, c = planes.shape
    best = planes[:, 0].clone()
    win = torch.zeros((n, c), dtype=torch.int64)
    for j in range(1, k):
        better = planes[:, j] > best                   # strictly: an equal later plane never takes over
        best = torch.where(better, planes[:, j], best)
        win = torch.where(better, torch.full_like(win, j), win)
    if k == 1:
        return win, torch.full((n, c), float("inf"), dtype=planes.dtype)
    top = planes.sort(dim=1, descending=True).values
    return win, top[:, 0] - top[:, 1]


def pool(planes):
    """planes [n, K, C] (may require grad) -> (pooled [n, C] gathered at the winner, win, gap)"""
    win, gap = winners(planes.detach())
    return planes.gather(1, win[:, None, :]).squeeze(1), win, gap


def logits(raw, labels, s, m, margin=None):
    """pooled raw cosines [n, C] float64 -> scaled logits, by the head's margin: None = ArcFace(s, m); a (kind, easy, s, m, filter_thr)
    descriptor (nets.ArcFace.Margin); or per-row margins (s, eps, m_ang, m_add; nets.ArcFace.RowMargins)"""
    if margin is not None and is_rows(margin):
        return adaface_double.logits(raw, labels, margin.s, margin.m_ang, margin.m_add, margin.eps)
    kind, easy, s_, m_, thr = (0, 0, s, m, 0.0) if margin is None else margin
    return margin_formula.margin_logits(raw.clamp(-1.0, 1.0), labels, int(kind), bool(easy), float(s_), float(m_), float(thr))[0]


def cross_entropy(z, labels):
    labels = labels.reshape(-1).long()
    lse = torch.logsumexp(z, dim=1)
    own = labels >= 0
    zt = z.gather(1, labels.clamp(min=0)[:, None]).flatten()
    per_row = torch.where(own, lse - zt, lse - lse.detach() + NO_TARGET)
    value = per_row.detach().clamp(max=NO_TARGET)
    return (per_row + (value - per_row.detach())).mean()


def pooled_head(emb, weight, labels, K, s=30.0, m=0.35, margin=None):
    """emb [n, d], weight [K C, d] plane-major (un-normalised), labels [n] (-1: no target) -> dict(loss, d_emb, d_w [K C, d], win [n, C],
    gap [n, C], raw [n, C] pooled cosines, z [n, C], planes [n, K, C]); float64, gradients by autograd"""
    labels = labels.reshape(-1).long()
    e = emb.detach().double().requires_grad_(True)
    w = weight.detach().double().requires_grad_(True)
    assert w.shape[0] % K == 0
    c = w.shape[0] // K
    eh = e / e.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    wh = w / w.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    planes = (eh @ wh.t()).view(e.shape[0], K, c)
    raw, win, gap = pool(planes)
    z = logits(raw, labels, s, m, margin)
    loss = cross_entropy(z, labels)
    loss.backward()
    return dict(loss=loss.detach(), d_emb=e.grad, d_w=w.grad, win=win, gap=gap, raw=raw.detach(), z=z.detach(), planes=planes.detach())


class SubcenterOracleKernels(AdaHeadKernels):
    """the CPU stand-in for nets.PartialFC.HipHeadKernels on gloo, with `subcenters=`; float64, gradients by autograd through `pool`"""

    def forward_stats(self, ehat, what, labels_i32, s, m, margin=None, subcenters=1):
        n, c = ehat.shape[0], what.shape[0] // subcenters
        raw, win, _ = pool((ehat.double() @ what.double().t()).view(n, subcenters, c))
        z = logits(raw, labels_i32, s, m, margin)
        rmax = z.max(dim=1).values
        rsum = torch.exp(z - rmax[:, None]).sum(dim=1)
        zt = torch.zeros(n, dtype=torch.float64)
        tsub = torch.full((n,), -1, dtype=torch.int32)
        rows = torch.nonzero(labels_i32 >= 0).flatten()
        zt[rows] = z[rows, labels_i32[rows].long()]
        tsub[rows] = win[rows, labels_i32[rows].long()].to(torch.int32)
        return (zt, rmax, rsum, tsub) if subcenters > 1 else (zt, rmax, rsum)         # one centre: today's interface

    def backward(self, ehat, enorm, what, wnorm, labels_i32, s, m, rmax, rsum, n_global, upstream, e_scale=1.0, on_de=None,
                 margin=None, subcenters=1):
        n, c = ehat.shape[0], what.shape[0] // subcenters
        with torch.enable_grad():
            eh = ehat.detach().double().requires_grad_(True)
            wh = what.detach().double().requires_grad_(True)
            raw, _, _ = pool((eh @ wh.t()).view(n, subcenters, c))
            z = logits(raw, labels_i32, s, m, margin)
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
ROWS = dict(dup_a=0, dup_b=1, no_target=2, tie=3)        # rows 6 .. 11 carry the border columns


def _build(n, classes, d, K, seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn((n, d), generator=g, dtype=torch.float64)
    emb = emb / emb.norm(dim=1, keepdim=True) * (0.5 + 4.0 * torch.rand(n, generator=g, dtype=torch.float64))[:, None]
    weight = (torch.randn((K, classes, d), generator=g, dtype=torch.float64) * 0.05)
    labels = torch.randint(0, classes, (n,), generator=g)
    cols = list(BORDER_COLS) + [classes - 1]
    taken = set(cols + [TIE_CLASS, 20])
    free = [c for c in range(classes) if c not in taken]
    pool_ = free[::max(1, len(free) // 24)][:24]          # few distinct classes: a sampled head (rate 0.3) still draws negatives
    for i in range(n):
        labels[i] = pool_[int(torch.randint(0, len(pool_), (1,), generator=g))]
    labels[6:6 + len(cols)] = torch.tensor(cols)
    labels[ROWS["dup_a"]] = labels[ROWS["dup_b"]] = 20
    labels[ROWS["no_target"]] = -1
    labels[ROWS["tie"]] = TIE_CLASS
    # the exact-tie class: its first max(K - 1, 2) planes are bitwise copies of each other (all of them at K = 2) and, for the row whose
    # target it is, they are the winners by far (cosine 0.9) -- a tie rule other than "lowest k" reports another plane there
    e = emb[ROWS["tie"]] / emb[ROWS["tie"]].norm()
    centre = (e + torch.randn(d, generator=g, dtype=torch.float64) * (0.484 / math.sqrt(d))) * 0.3
    for k in range(min(K, max(K - 1, 2))):
        weight[k, TIE_CLASS] = centre
    return emb.float(), weight.reshape(K * classes, d).float(), labels


_CASES = {}


def case(n, classes, d, K, seed):
    """Seeded inputs (float32 tensors; the double upcasts) for the fp32-mode tests -> (emb [n, d], weight [K classes, d] plane-major,
    labels [n] int64, the double's result on them).  Apart from the exact-tie class, the double's top-two gap is >= GAP at every
    (row, class): no winner is decided by fp32 rounding.  Seeds are walked upwards from `seed` until that holds (at most 20).  Built once
    per key and shared: never modify the tensors."""
    key = (n, classes, d, K, seed)
    if key not in _CASES:
        for tries in range(20):
            emb, weight, labels = _build(n, classes, d, K, seed + tries)
            res = pooled_head(emb, weight, labels, K)
            gap = res["gap"].clone()
            gap[:, TIE_CLASS] = float("inf")
            if K == 1 or float(gap.min()) >= GAP:
                break
        else:
            raise AssertionError("no seed in [%d, %d) keeps every top-two gap above %g" % (seed, seed + 20, GAP))
        _CASES[key] = (emb, weight, labels, res)
    return _CASES[key]


def assert_case(emb, weight, labels, K, res):
    """what the tests rely on, asserted on the DOUBLE itself"""
    classes = weight.shape[0] // K
    win, gap = res["win"], res["gap"]
    for c in list(BORDER_COLS) + [classes - 1]:
        assert int((labels == c).sum()) >= 1, c
    assert labels[ROWS["tie"]] == TIE_CLASS and labels[ROWS["dup_a"]] == labels[ROWS["dup_b"]] and labels[ROWS["no_target"]] == -1
    planes = weight.view(K, classes, -1)
    for k in range(1, min(K, max(K - 1, 2))):
        assert torch.equal(planes[k, TIE_CLASS], planes[0, TIE_CLASS])
    if K > 1:
        assert bool((gap[:, TIE_CLASS] == 0).all() if K == 2 else True)
        assert float(gap[ROWS["tie"], TIE_CLASS]) == 0.0 and int(win[ROWS["tie"], TIE_CLASS]) == 0
        others = gap.clone()
        others[:, TIE_CLASS] = float("inf")
        assert float(others.min()) >= GAP
    own = torch.nonzero(labels >= 0).flatten()
    target = torch.zeros(win.shape, dtype=torch.bool)
    target[own, labels[own]] = True
    twin = win[own, labels[own]]
    for k in range(K):
        assert int((twin == k).sum()) >= 1, "plane %d wins no target" % k
        assert int(((win == k) & ~target).sum()) >= 1, "plane %d wins no non-target" % k
    assert float(res["raw"].abs().max()) < 0.999          # no cosine near the clamp
