"""CPU double of the 1:N search (frhip_gallery_topk, utils.eval.identify).  TEST-ONLY, numpy.

Scores are summed SEQUENTIALLY over the columns, one column at a time in a Python loop, because that is the order the kernels
add in: np.sum(axis=...) adds pairwise and differs in the last bits of most scores at d = 512.  Every step is the kernels' own:
the float32 difference gallery - probe, its exact square in float64, the running float64 sum, score = 1 - sum / 4.
Cost: P * G * d; 257 x 5 000 x 512 takes some 10 s."""
import numpy as np


def scores(probe, gallery):
    """[P, G] float64 scores of every probe / gallery pair"""
    p, g = np.asarray(probe, dtype=np.float32), np.asarray(gallery, dtype=np.float32)
    s = np.zeros((p.shape[0], g.shape[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(p.shape[1]):
            s += (g[None, :, c] - p[:, None, c]).astype(np.float64) ** 2
        return 1.0 - s / 4.0


def topk_from_scores(score, k, exclude=None):
    """the lists of a [P, G] score matrix: NaN and excluded entries dropped, score descending then index ascending, -inf / -1 padding"""
    n_p, n_g = score.shape
    top_score = np.full((n_p, k), -np.inf, dtype=np.float64)
    top_index = np.full((n_p, k), -1, dtype=np.int64)
    for i in range(n_p):
        idx = np.arange(n_g, dtype=np.int64)
        keep = ~np.isnan(score[i])
        if exclude is not None and exclude[i] >= 0:
            keep &= idx != exclude[i]
        idx, s = idx[keep], score[i][keep]
        order = np.lexsort((idx, -s))[:k]
        top_score[i, :order.size], top_index[i, :order.size] = s[order], idx[order]
    return top_score, top_index


def topk(probe, gallery, k, exclude=None):
    return topk_from_scores(scores(probe, gallery), k, exclude)
