"""Drop-in for the reference `nets/ArcFace.py` (margin modules).

`ArcFace(s, margin)`, `CosFace(s, m)` and `CombinedMarginLoss(s, m1, m2, m3)` keep the reference's constructors,
attribute names and `forward(logits, labels)` contract (/root/reference/nets/ArcFace.py:5-106): `logits` [N, C] fp32
cosines are modified IN PLACE at the target entries (labels [N,1] or [N] int64, -1 = no target on this shard) and the
scaled tensor is returned.  On the MI355X the work is one HIP row kernel (frhip_margin_fwd / _bwd) wrapped in an
autograd node.

`AdaFace(s, m, h, t_alpha)` (Kim et al., CVPR 2022; not in the reference) gives every row its own margin, derived from the norm of that
row's embedding before normalisation: `forward(logits, labels, norms)`.  It clamps EVERY cosine, so unlike the others it returns a new
tensor and leaves `logits` untouched.  `MagFace(s, m, u_margin, l_a, u_a, lambda_g)` (Meng et al., CVPR 2021; not in the reference) does the
same with a margin that grows with the norm; its regulariser and the gradient through the norms live in the fused head.
`ElasticFace(s, m, std, kind, plus, seed)` (Boutros et al., CVPR-W 2022; not in the reference) draws every row's margin from N(m, std) at
every step, and with `plus` hands the draws out by difficulty: `forward(logits, labels)`, a new tensor as well.
`CurricularFace(s, m, alpha)` (Huang et al., CVPR 2020; not in the reference) re-weights the hard NEGATIVES of every row by a running mean
of the target cosines: `forward(logits, labels)`, a new tensor as well.
`UniFace(s, m, kind, w_pos, w_neg, m_neg, bias_init, learn_bias)` (Zhou et al., ICCV 2023; SphereFace2 with t = 1; not in the reference) is
no softmax at all: every (row, class) pair is a sigmoid problem against one learnable threshold `bias`, and `forward(logits, labels)`
returns the 0-dim LOSS, not logits.

Inside PartialFC the margin is not applied through this `forward`: it lives in the epilogue of the fused cos-theta
MFMA kernel (frhip_head_fwd / frhip_head_fwd_ex), which only reads the module's constants through `margin_of`, so the
[N, C] logits this `forward` would overwrite never exist in HBM on the training hot path.
"""
import collections
import math

import torch

ARCFACE, COSFACE = 0, 1          # frhip_margin_t.kind

# What the HIP kernels implement, one record for every module below: kind ARCFACE (easy: the easy_margin switch) or COSFACE,
# scale s, margin m, interclass filtering threshold filter_thr (0 = off).
Margin = collections.namedtuple("Margin", "kind easy s m filter_thr")

# AdaFace: what margin_of returns for it (the constants of the module), and what the kernels take once frhip_adaface_margins has turned
# the batch's norms into margins: scale, clamp width and the device vectors [N] of angular / additive margins (frhip_margin_rows_t).
AdaMargin = collections.namedtuple("AdaMargin", "s m h t_alpha eps")
RowMargins = collections.namedtuple("RowMargins", "s eps m_ang m_add")
# MagFace: the constants of the module (m, u_margin: the margin at norms l_a and u_a; lambda_g: the weight of the regulariser); the kernels
# take RowMargins as well, filled by frhip_magface_margins
MagMargin = collections.namedtuple("MagMargin", "s m u_margin l_a u_a lambda_g eps")
# ElasticFace: the constants of the module (m, std: mean and deviation of the draws; kind "arc" / "cos"; plus: ranked assignment; seed:
# the key of the generator); the kernels take RowMargins, filled by frhip_elastic_margins or frhip_elastic_draws + frhip_elastic_assign
ElasticMargin = collections.namedtuple("ElasticMargin", "s m std kind plus seed eps")

# CurricularFace: the constants of the module (m: the margin, alpha: the momentum of t), and what the kernels take once
# frhip_curricular_rows has turned the batch's target cosines into thresholds: scale, margin, the device vector thr [N] and the device
# scalar t (frhip_margin_curr_t)
CurricularMargin = collections.namedtuple("CurricularMargin", "s m alpha")
CurrRows = collections.namedtuple("CurrRows", "s m thr t")

# The sigmoid (BCE) head: the constants of the UniFace module (kind ARCFACE / COSFACE: the target's rule; m_neg: additive margin of the
# negatives; w_pos, w_neg: the two weights), and what the kernels take: the same plus the device scalar bias (frhip_margin_bce_t)
UniMargin = collections.namedtuple("UniMargin", "kind s m m_neg w_pos w_neg")
BceMargin = collections.namedtuple("BceMargin", "kind s m m_neg w_pos w_neg bias")

SUPPORTED = ("ArcFace, CosFace, CombinedMarginLoss (ArcFace m1 == 1, m3 == 0 or CosFace m3 > 0), AdaFace, MagFace, ElasticFace, "
             "CurricularFace, UniFace")


def margin_of(module):
    """-> Margin of a margin module of this package, read from its attributes NOW (so a later `easy_margin = True` counts, as in
    the reference, whose modules read their attributes in forward); AdaMargin for AdaFace, MagMargin for MagFace, ElasticMargin for
    ElasticFace, CurricularMargin for CurricularFace, UniMargin for UniFace.  NotImplementedError for any other module."""
    if isinstance(module, UniFace):
        return UniMargin(UNIFACE_KINDS[module.kind], float(module.s), float(module.m), float(module.m_neg), float(module.w_pos),
                         float(module.w_neg))
    if isinstance(module, CurricularFace):
        return CurricularMargin(float(module.s), float(module.m), float(module.alpha))
    if isinstance(module, ElasticFace):
        return ElasticMargin(float(module.s), float(module.m), float(module.std), module.kind, bool(module.plus), int(module.seed),
                             float(module.eps))
    if isinstance(module, AdaFace):
        return AdaMargin(float(module.s), float(module.m), float(module.h), float(module.t_alpha), float(module.eps))
    if isinstance(module, MagFace):
        return MagMargin(float(module.s), float(module.m), float(module.u_margin), float(module.l_a), float(module.u_a),
                         float(module.lambda_g), float(module.eps))
    if isinstance(module, ArcFace):
        return Margin(ARCFACE, bool(module.easy_margin), float(module.scale), float(module.margin), 0.0)
    if isinstance(module, CosFace):
        return Margin(COSFACE, False, float(module.s), float(module.m), 0.0)
    if isinstance(module, CombinedMarginLoss):
        thr = float(module.interclass_filtering_threshold)
        thr = thr if thr > 0 else 0.0
        if module.m1 == 1.0 and module.m3 == 0.0:
            return Margin(ARCFACE, bool(module.easy_margin), float(module.s), float(module.m2), thr)
        if module.m3 > 0:                                       # m1, m2 are ignored, as in the reference
            return Margin(COSFACE, False, float(module.s), float(module.m3), thr)
        raise RuntimeError("CombinedMarginLoss(m1=%r, m2=%r, m3=%r): neither ArcFace (m1 == 1, m3 == 0) nor CosFace (m3 > 0); the "
                           "reference raises here too" % (module.m1, module.m2, module.m3))
    raise NotImplementedError("the fused head kernel implements the margin modules %s, not %s" % (SUPPORTED, type(module).__name__))


def is_plain_arcface(mg):
    return isinstance(mg, Margin) and mg.kind == ARCFACE and not mg.easy and mg.filter_thr == 0.0


class _MarginFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, mg):
        from frhip import ops
        if not logits.is_cuda:
            raise RuntimeError("nets.ArcFace (frhip): logits must live on the MI355X; there is no CPU path")
        lab = labels.reshape(-1).long().contiguous()
        buf = logits if (logits.is_contiguous() and logits.dtype == torch.float32) else logits.float().contiguous()
        if mg.easy or mg.filter_thr > 0:
            tsave, filt = ops.margin_fwd_ex(buf, lab, mg)
        else:
            tsave, filt = ops.margin_fwd(buf, lab, mg.s, mg.m, mg.kind), None
        ctx.mark_dirty(logits) if buf is logits else None
        ctx.save_for_backward(lab, tsave, filt)
        ctx.mg = mg
        return buf

    @staticmethod
    def backward(ctx, g):
        from frhip import ops
        lab, tsave, filt = ctx.saved_tensors
        mg = ctx.mg
        if mg.easy or mg.filter_thr > 0:
            return ops.margin_bwd_ex(g.contiguous().float(), lab, tsave, filt, mg), None, None
        return ops.margin_bwd(g.contiguous().float(), lab, tsave, mg.s, mg.m, mg.kind), None, None


class ArcFace(torch.nn.Module):
    """Additive angular margin: target logit cos(theta) -> cos(theta + m), everything x s.  easy_margin = True: only where
    cos(theta) > 0 (reference :82-84)."""
    kind = "arcface"

    def __init__(self, s=64.0, margin=0.5):
        super().__init__()
        self.scale = s
        self.margin = margin
        self.cos_m = math.cos(margin)
        self.sin_m = math.sin(margin)
        self.theta = math.cos(math.pi - margin)
        self.sinmm = math.sin(math.pi - margin) * margin
        self.easy_margin = False

    def forward(self, logits: torch.Tensor, labels: torch.Tensor):
        return _MarginFn.apply(logits, labels, margin_of(self))


class CosFace(torch.nn.Module):
    """Additive cosine margin: target logit t -> t - m, everything x s (reference :94-106)."""
    kind = "cosface"

    def __init__(self, s=64.0, m=0.40):
        super().__init__()
        self.s = s
        self.m = m
        self.scale, self.margin = s, m

    def forward(self, logits: torch.Tensor, labels: torch.Tensor):
        return _MarginFn.apply(logits, labels, margin_of(self))


class CombinedMarginLoss(torch.nn.Module):
    """(m1, m2, m3) front-end of the reference (:5-61): m1 == 1, m3 == 0 is ArcFace with margin m2; m3 > 0 is CosFace
    with margin m3; anything else raises like the reference.  interclass_filtering_threshold > 0: every non-target element
    whose cosine is above it becomes 0 (rows with label -1: every element above it), with zero gradient.  In place on
    `logits` like ArcFace / CosFace (the reference returns a new tensor when filtering; the values are the same)."""

    def __init__(self, s, m1, m2, m3, interclass_filtering_threshold=0):
        super().__init__()
        self.s, self.m1, self.m2, self.m3 = s, m1, m2, m3
        self.interclass_filtering_threshold = interclass_filtering_threshold
        self.cos_m, self.sin_m = math.cos(m2), math.sin(m2)
        self.theta = math.cos(math.pi - m2)
        self.sinmm = math.sin(math.pi - m2) * m2
        self.easy_margin = False

    def forward(self, logits, labels):
        return _MarginFn.apply(logits, labels, margin_of(self))


class _RowMarginFn(torch.autograd.Function):
    """per-row margins on explicit logits (frhip_margin_fwd_rows / _bwd_rows); no gradient to the margins"""

    @staticmethod
    def forward(ctx, logits, labels, rows):
        from frhip import ops
        if not logits.is_cuda:
            raise RuntimeError("nets.ArcFace (frhip): logits must live on the MI355X; there is no CPU path")
        lab = labels.reshape(-1).long().contiguous()
        ctx.save_for_backward(logits, lab, rows.m_ang, rows.m_add)        # the input itself: autograd then notices a later in-place write
        ctx.s, ctx.eps = rows.s, rows.eps
        return ops.margin_fwd_rows(logits.detach().float().contiguous(), lab, rows)

    @staticmethod
    def backward(ctx, g):
        from frhip import ops
        logits, lab, m_ang, m_add = ctx.saved_tensors
        return ops.margin_bwd_rows(g.contiguous().float(), logits.detach().float().contiguous(), lab,
                                   RowMargins(ctx.s, ctx.eps, m_ang, m_add)), None, None


class AdaFace(torch.nn.Module):
    """Quality-adaptive margin (AdaFace): with sn = clip(norm, 0.001, 100) and k = clip(h (sn - batch_mean) / (batch_std + eps), -1, 1),
    row i's target logit is s (cos(clip(theta + a_i, eps, pi - eps)) - b_i), a_i = -m k_i, b_i = m + m k_i; every cosine is clamped to
    [-1 + eps, 1 - eps] first and every logit is x s.  batch_mean / batch_std are running statistics of the GLOBAL batch's norms
    (momentum t_alpha, std unbiased), advanced in training mode before they are used and only read in eval mode.  No gradient flows
    through the norms.  needs_norms tells PartialFC / Model to hand the norms over."""
    kind = "adaface"
    needs_norms = True
    eps = 1e-3

    def __init__(self, s=64.0, m=0.4, h=0.333, t_alpha=0.01):
        super().__init__()
        self.s, self.m, self.h, self.t_alpha = s, m, h, t_alpha
        self.scale, self.margin = s, m
        self.register_buffer("batch_mean", torch.ones(1) * 20.0)
        self.register_buffer("batch_std", torch.ones(1) * 100.0)

    def row_margins(self, norms, kernels=None):
        """norms [N] of the global batch (fp32, detached) -> RowMargins; in training mode the running buffers are advanced first.
        ONE launch of frhip_adaface_margins, no host synchronisation.  kernels: PartialFC's kernel object (tests swap in a double)."""
        mg = margin_of(self)
        norms = norms.detach().reshape(-1).float().contiguous()
        fn = kernels.adaface_margins if kernels is not None else _hip_adaface_margins
        m_ang, m_add = fn(norms, mg, self.batch_mean, self.batch_std, self.training)
        return RowMargins(mg.s, mg.eps, m_ang, m_add)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor, norms: torch.Tensor):
        return _RowMarginFn.apply(logits, labels, self.row_margins(norms))


def _hip_adaface_margins(norms, mg, batch_mean, batch_std, update):
    from frhip import ops
    return ops.adaface_margins(norms, mg.m, mg.h, mg.t_alpha, mg.eps, batch_mean, batch_std, update)


class MagFace(torch.nn.Module):
    """Magnitude-aware margin (MagFace, Meng et al., CVPR 2021): with a = clip(norm, l_a, u_a), row i's target logit is
    s cos(clip(theta + m_i, eps, pi - eps)), m_i = m + (u_margin - m) (a_i - l_a) / (u_a - l_a); every cosine is clamped to
    [-1 + eps, 1 - eps] first and every logit is x s.  The loss gains lambda_g x the mean over the GLOBAL batch of g(a) = a / u_a^2 + 1 / a,
    and a gradient flows through the norms (margin and regulariser) while l_a < norm < u_a: the norm becomes a quality score.
    Where theta + m_i passes pi the angle is clipped (the per-row margin kernels' rule), where the official code switches to
    cos(theta) - m sin(m).  needs_norms / norms_need_grad tell PartialFC / Model to hand differentiable norms over.  No buffers."""
    kind = "magface"
    needs_norms = True
    norms_need_grad = True
    eps = 1e-3

    def __init__(self, s=64.0, m=0.45, u_margin=0.8, l_a=10.0, u_a=110.0, lambda_g=35.0):
        super().__init__()
        self.s, self.m, self.u_margin, self.l_a, self.u_a, self.lambda_g = s, m, u_margin, l_a, u_a, lambda_g
        self.scale, self.margin = s, m

    def row_margins(self, norms, kernels=None):
        """norms [N] of the global batch (detached) -> (RowMargins, reg): the per-row margins and the regulariser's value (a tensor of
        one element, not yet x lambda_g).  ONE launch of frhip_magface_margins, no host synchronisation.  kernels: PartialFC's kernel
        object (tests swap in a double)."""
        mg = margin_of(self)
        norms = norms.detach().reshape(-1).contiguous()
        fn = kernels.magface_margins if kernels is not None else _hip_magface_margins
        m_ang, m_add, reg = fn(norms, mg)
        return RowMargins(mg.s, mg.eps, m_ang, m_add), reg

    def forward(self, logits: torch.Tensor, labels: torch.Tensor, norms: torch.Tensor):
        """The margin alone, on explicit cosines: -> the scaled logits (a new tensor, like AdaFace.forward), differentiable in `logits`
        only.  The regulariser and the gradient through the norms live in the fused head (nets.PartialFC); `row_margins` returns the
        regulariser's value."""
        return _RowMarginFn.apply(logits, labels, self.row_margins(norms)[0])


def _hip_magface_margins(norms, mg):
    from frhip import ops
    return ops.magface_margins(norms.float(), mg.l_a, mg.u_a, mg.m, mg.u_margin)


class ElasticFace(torch.nn.Module):
    """Elastic margin (ElasticFace, Boutros et al., CVPR-W 2022): at every training step row i of the GLOBAL batch draws g_i from N(m, std);
    kind "arc": target logit s cos(clip(theta + g_i, eps, pi - eps)), kind "cos": s (cos(clip(theta, eps, pi - eps)) - g_i); every cosine
    is clamped to [-1 + eps, 1 - eps] first and every logit is x s (the per-row margin kernels' rule: the clip of the angle at pi - eps
    stands where the official code has none).  The published presets (m, std): Arc (0.5, 0.05), Cos (0.35, 0.05), Arc+ (0.5, 0.0175),
    Cos+ (0.35, 0.025).

    Draws: Philox4x32-10 keyed by `seed`, counter (row, step), Box-Muller in float64 (include/frhip.h, frhip_elastic_margins): a draw
    depends on (seed, step, row) alone, so every rank derives the whole batch's margins with no collective.  `step` is a device buffer
    (int64, checkpointed), advanced by the kernel itself in training mode; in eval mode every margin is m and `step` stands still.

    plus=True (ElasticFace-Arc+ / -Cos+): the draws are handed out by difficulty.  With c_i the row's target cosine (the maximum over
    sub-centres and over the ranks' shards, -2 where nobody owns the row) and r_i = #{j : c_j > c_i, or c_j == c_i and j < i}, row i gets
    the r_i-th smallest draw: the largest cosine gets the smallest margin.  This is the paper's stated rule; the official code indexes
    the sorted margins with the sort permutation itself instead of the rank.  No gradient flows through the ranking or the margins."""
    eps = 1e-3
    KINDS = ("arc", "cos")

    def __init__(self, s=64.0, m=0.5, std=0.05, kind="arc", plus=False, seed=0):
        super().__init__()
        if kind not in self.KINDS:
            raise ValueError("ElasticFace: kind must be 'arc' or 'cos', got %r" % (kind,))
        if not std >= 0:
            raise ValueError("ElasticFace: std must be >= 0, got %r" % (std,))
        self.s, self.m, self.std, self.kind, self.plus, self.seed = s, m, std, kind, bool(plus), int(seed)
        self.scale, self.margin = s, m
        self.register_buffer("step", torch.zeros(1, dtype=torch.int64))

    def row_margins(self, kernels=None, tcos=None, n=None):
        """-> RowMargins of the n rows of the global batch; in training mode `step` is advanced.  tcos ([world_size, n] or [n], detached):
        the target cosines `plus` ranks by, required in training mode with plus (n is then read off it); eval mode never looks at it.
        ONE launch without plus, three with it; no host synchronisation.  kernels: PartialFC's kernel object (tests swap in a double)."""
        mg = margin_of(self)
        kern = kernels if kernels is not None else _HipElastic
        ranked = mg.plus and self.training
        if ranked:
            if tcos is None:
                raise ValueError("ElasticFace(plus=True) ranks the draws by the rows' target cosines: pass tcos")
            tcos = tcos.detach()
            tcos = tcos.reshape(1, -1) if tcos.dim() == 1 else tcos
            n = tcos.shape[1]
        elif n is None:
            if tcos is None:
                raise ValueError("ElasticFace.row_margins: the number of rows n is needed")
            n = tcos.shape[-1]
        if ranked:
            m_ang, m_add = kern.elastic_assign(tcos, kern.elastic_margins(n, mg, self.step, True, bare=True), mg)
        else:
            m_ang, m_add = kern.elastic_margins(n, mg, self.step, self.training)
        return RowMargins(mg.s, mg.eps, m_ang, m_add)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor):
        """The margin on explicit cosines [N, C] (labels [N] or [N, 1], -1 = no target): -> the scaled logits, a new tensor like
        AdaFace.forward, differentiable in `logits`.  With plus the target cosines are read off `logits`."""
        lab = labels.reshape(-1).long()
        tcos = None
        if self.plus and self.training:
            picked = logits.detach().float().gather(1, lab.clamp(min=0).view(-1, 1)).view(-1)
            tcos = torch.where(lab >= 0, picked, torch.full_like(picked, -2.0)).contiguous()
        if self.step.device != logits.device:
            raise RuntimeError("nets.ArcFace (frhip): ElasticFace's step buffer must live on the logits' device: module.to(device)")
        return _RowMarginFn.apply(logits, labels, self.row_margins(None, tcos, n=logits.shape[0]))


class _HipElastic:
    """ElasticFace's launches for the stand-alone module: the three methods nets.PartialFC.HipHeadKernels has under the same names"""

    @staticmethod
    def elastic_margins(n, mg, step, update, bare=False):
        from frhip import ops
        if bare:
            return ops.elastic_draws(n, mg.m, mg.std, mg.seed, step, update)
        return ops.elastic_margins(n, mg.kind, mg.m, mg.std, mg.seed, step, update)

    @staticmethod
    def elastic_assign(tcos, g, mg):
        from frhip import ops
        return ops.elastic_assign(tcos.float().contiguous(), g, mg.kind)


class _CurrFn(torch.autograd.Function):
    """CurricularFace on explicit logits (frhip_margin_fwd_curr / _bwd_curr); no gradient to the thresholds or t"""

    @staticmethod
    def forward(ctx, logits, labels, rows):
        from frhip import ops
        if not logits.is_cuda:
            raise RuntimeError("nets.ArcFace (frhip): logits must live on the MI355X; there is no CPU path")
        lab = labels.reshape(-1).long().contiguous()
        # t is kept by value: the module advances its buffer in place at the next call, and the mask is rebuilt from this step's
        ctx.save_for_backward(logits, lab, rows.thr, rows.t.clone())
        ctx.s, ctx.m = rows.s, rows.m
        return ops.margin_fwd_curr(logits.detach().float().contiguous(), lab, rows)

    @staticmethod
    def backward(ctx, g):
        from frhip import ops
        logits, lab, thr, t = ctx.saved_tensors
        return ops.margin_bwd_curr(g.contiguous().float(), logits.detach().float().contiguous(), lab, CurrRows(ctx.s, ctx.m, thr, t)), None, None


class CurricularFace(torch.nn.Module):
    """Adaptive curriculum (CurricularFace, Huang et al., CVPR 2020; the official implementation's rule): the target logit is ArcFace's,
    s cos(theta_y + m) above cos(pi - m) and s (cos(theta_y) - m sin(pi - m)) below; a NON-target cosine c of row i that is above the row's
    own cos(theta_y + m) -- a hard negative -- becomes s c (t + c), every other one s c.  t is a running mean of the GLOBAL batch's target
    cosines (momentum alpha; a device buffer, checkpointed, starts at 0), advanced in training mode BEFORE it is used and only read in
    eval mode: hard negatives weigh little early in training and more later.  Every cosine is clamped to [-1, 1] first; no gradient
    flows through the thresholds or t."""
    kind = "curricularface"

    def __init__(self, s=64.0, m=0.5, alpha=0.01):
        super().__init__()
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("CurricularFace: alpha must lie in [0, 1], got %r" % (alpha,))
        if not 0.0 <= m < math.pi:
            raise ValueError("CurricularFace: m must lie in [0, pi), got %r" % (m,))
        self.s, self.m, self.alpha = s, m, alpha
        self.scale, self.margin = s, m
        self.register_buffer("t", torch.zeros(1))

    def row_thresholds(self, tcos, kernels=None):
        """tcos ([world_size, n] or [n], detached; -2 where a rank does not own the row): the rows' target cosines -> CurrRows; in
        training mode t is advanced first.  ONE launch of frhip_curricular_rows, no host synchronisation.  kernels: PartialFC's kernel
        object (tests swap in a double)."""
        mg = margin_of(self)
        tcos = tcos.detach()
        tcos = tcos.reshape(1, -1) if tcos.dim() == 1 else tcos
        fn = kernels.curricular_rows if kernels is not None else _hip_curricular_rows
        return CurrRows(mg.s, mg.m, fn(tcos, mg, self.t, self.training), self.t)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor):
        """The loss's logits from explicit cosines [N, C] (labels [N] or [N, 1], -1 = no target): -> the scaled logits, a new tensor like
        AdaFace.forward, differentiable in `logits`.  The target cosines are read off `logits`."""
        lab = labels.reshape(-1).long()
        if self.t.device != logits.device:
            raise RuntimeError("nets.ArcFace (frhip): CurricularFace's t buffer must live on the logits' device: module.to(device)")
        picked = logits.detach().float().gather(1, lab.clamp(min=0).view(-1, 1)).view(-1)
        tcos = torch.where(lab >= 0, picked, torch.full_like(picked, -2.0)).contiguous()
        return _CurrFn.apply(logits, labels, self.row_thresholds(tcos))


def _hip_curricular_rows(tcos, mg, t, update):
    from frhip import ops
    return ops.curricular_rows(tcos.float().contiguous(), mg.m, mg.alpha, t, update)


UNIFACE_KINDS = {"arc": ARCFACE, "cos": COSFACE}


class _UniFaceFn(torch.autograd.Function):
    """the sigmoid head on explicit cosines (frhip_bce_fwd -> _reduce -> _merge; frhip_bce_bwd): -> the 0-dim loss, with gradients to the
    logits and to the bias"""

    @staticmethod
    def forward(ctx, logits, bias, labels, mg):
        from frhip import ops
        if not logits.is_cuda:
            raise RuntimeError("nets.ArcFace (frhip): logits must live on the MI355X; there is no CPU path")
        lab = labels.reshape(-1).long().contiguous()
        cos = logits.detach().float().contiguous()
        b = bias.detach().clone()                         # by value: the optimizer moves the parameter on
        bm = BceMargin(*mg, b)
        n = cos.shape[0]
        loss, dbias = ops.bce_merge(ops.bce_reduce(*ops.bce_fwd(cos, lab, bm)), n)
        ctx.save_for_backward(cos, lab, b, dbias)
        ctx.mg, ctx.shapes = mg, (logits.dtype, bias.shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        from frhip import ops
        cos, lab, b, dbias = ctx.saved_tensors
        up = g.reshape(1).float().contiguous()
        gin = ops.bce_bwd(cos, lab, BceMargin(*ctx.mg, b), 1.0 / cos.shape[0], up)
        return gin.to(ctx.shapes[0]), (up * dbias).reshape(ctx.shapes[1]), None, None


class UniFace(torch.nn.Module):
    """Unified cross-entropy (UniFace, Zhou et al., ICCV 2023): every class is a binary sigmoid problem against ONE threshold b.  With
    c the cosine clamped to [-1, 1]: the target contributes w_pos softplus(-(s phi(c) - b)), phi(c) = c - m (kind "cos") or ArcFace's
    cos(theta + m) / c - m sin(pi - m) (kind "arc"); every other class w_neg softplus(s (c + m_neg) - b); the loss is their sum over
    all rows and all classes (of all shards; with sampling the activated ones) divided by the global batch size.  An element's gradient
    depends on nothing outside the element, so a class-sharded backward pass needs nothing from the other shards.
    `bias` is a [1] fp32 Parameter (a buffer with learn_bias=False); bias_init=None means log(10 x num_classes), set by
    reset_bias(num_classes) -- PartialFC calls it at construction, the stand-alone user once the class count is known.
    SphereFace2 (Wen et al., ICLR 2022) with its similarity adjustment g(z) = 2 ((z + 1) / 2)^t - 1 at t = 1 is this module with
    s = r, m_neg = m, w_pos = lambda / r, w_neg = (1 - lambda) / r; t != 1 is not built."""
    def __init__(self, s=64.0, m=0.4, kind="cos", w_pos=1.0, w_neg=1.0, m_neg=0.0, bias_init=None, learn_bias=True):
        super().__init__()
        if kind not in UNIFACE_KINDS:
            raise ValueError("UniFace: kind must be 'arc' or 'cos', got %r" % (kind,))
        if not (s > 0 and math.isfinite(s)):
            raise ValueError("UniFace: s must be positive and finite, got %r" % (s,))
        if not (math.isfinite(m) and math.isfinite(m_neg)):
            raise ValueError("UniFace: m and m_neg must be finite, got %r, %r" % (m, m_neg))
        if kind == "arc" and not 0.0 <= m < math.pi:
            raise ValueError("UniFace: kind 'arc' needs m in [0, pi), got %r" % (m,))
        if not (w_pos >= 0 and w_neg >= 0 and math.isfinite(w_pos) and math.isfinite(w_neg)) or (w_pos == 0 and w_neg == 0):
            raise ValueError("UniFace: w_pos and w_neg must be finite, >= 0 and not both 0, got %r, %r" % (w_pos, w_neg))
        if bias_init is not None and not math.isfinite(bias_init):
            raise ValueError("UniFace: bias_init must be finite, got %r" % (bias_init,))
        self.s, self.m, self.kind = s, m, kind
        self.w_pos, self.w_neg, self.m_neg = w_pos, w_neg, m_neg
        self.scale, self.margin = s, m
        self.bias_init, self.learn_bias = bias_init, bool(learn_bias)
        b = torch.full((1,), float(bias_init) if bias_init is not None else 0.0, dtype=torch.float32)
        if self.learn_bias:
            self.bias = torch.nn.Parameter(b)
        else:
            self.register_buffer("bias", b)

    @torch.no_grad()
    def reset_bias(self, num_classes):
        """bias <- bias_init, or log(10 x num_classes) (the GLOBAL class count) when bias_init is None"""
        if num_classes < 1:
            raise ValueError("UniFace.reset_bias: num_classes must be >= 1, got %r" % (num_classes,))
        self.bias.fill_(float(self.bias_init) if self.bias_init is not None else math.log(10.0 * num_classes))

    def forward(self, logits: torch.Tensor, labels: torch.Tensor):
        """explicit cosines [N, C] (labels [N] or [N, 1], -1 = no target) -> the 0-dim loss (mean over the N rows of the rows' sums),
        differentiable in `logits` and in `bias`.  It is NOT a logit tensor: nothing downstream is a softmax."""
        if self.bias.device != logits.device:
            raise RuntimeError("nets.ArcFace (frhip): UniFace's bias must live on the logits' device: module.to(device)")
        return _UniFaceFn.apply(logits, self.bias, labels, margin_of(self))
