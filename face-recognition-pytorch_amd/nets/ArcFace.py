"""Drop-in for the reference `nets/ArcFace.py` (margin modules).

`ArcFace(s, margin)`, `CosFace(s, m)` and `CombinedMarginLoss(s, m1, m2, m3)` keep the reference's constructors,
attribute names and `forward(logits, labels)` contract (/root/reference/nets/ArcFace.py:5-106): `logits` [N, C] fp32
cosines are modified IN PLACE at the target entries (labels [N,1] or [N] int64, -1 = no target on this shard) and the
scaled tensor is returned.  On the MI355X the work is one HIP row kernel (frhip_margin_fwd / _bwd) wrapped in an
autograd node.

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

SUPPORTED = "ArcFace, CosFace, CombinedMarginLoss (ArcFace m1 == 1, m3 == 0 or CosFace m3 > 0)"


def margin_of(module):
    """-> Margin of a margin module of this package, read from its attributes NOW (so a later `easy_margin = True` counts, as in
    the reference, whose modules read their attributes in forward).  NotImplementedError for any other module."""
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
    return mg.kind == ARCFACE and not mg.easy and mg.filter_thr == 0.0


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
