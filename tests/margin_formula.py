"""fp32 torch restatement of the reference margin modules (nets/ArcFace.py:5-106) on explicit logits, for the margin tests:
z = s * margin(t) with interclass filtering, and d z / d t (the slope, 0 where an element is filtered).  TEST-ONLY."""
import math

import torch


def margin_logits(t, labels, kind, easy, s, m, thr):
    """t [N, C] clamped cosines, labels [N] (-1 = no target on this shard) -> (z, dz/dt / s)"""
    t = t.clone()
    slope = torch.ones_like(t)
    lab = labels.long().view(-1)
    pos = torch.nonzero(lab >= 0).flatten()
    if thr > 0:
        dirty = t > thr
        dirty[pos, lab[pos]] = False
        t[dirty] = 0.0
        slope[dirty] = 0.0
    tt = t[pos, lab[pos]]
    if kind == 0:
        sin_t = torch.sqrt(1.0 - tt * tt)
        cos_tm = tt * math.cos(m) - sin_t * math.sin(m)
        d_tm = math.cos(m) + tt * math.sin(m) / sin_t
        if easy:
            big = tt > 0
            new, sl = torch.where(big, cos_tm, tt), torch.where(big, d_tm, torch.ones_like(tt))
        else:
            big = tt > math.cos(math.pi - m)
            new = torch.where(big, cos_tm, tt - math.sin(math.pi - m) * m)
            sl = torch.where(big, d_tm, torch.ones_like(tt))
    else:
        new, sl = tt - m, torch.ones_like(tt)
    t[pos, lab[pos]] = new
    slope[pos, lab[pos]] = sl
    return t * s, slope
