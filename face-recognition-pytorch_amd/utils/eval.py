"""Drop-in for the reference verification metrics `utils/eval.py`.

Same functions / return shapes as /root/reference/utils/eval.py: `pair_score(embedding_1, embedding_2, labels)` ->
(hist_genuine[100001], hist_imposter[100001], score_list), `performance_roc(hist_genuine, hist_imposter, min_level,
max_level)` -> (roc report string, eer_threshold), `performance_acc(score_list, label_list, th)` -> accuracy in %,
`cross_score(embeddings, labels)` -> (hist_genuine, hist_imposter, score_list, label_list) over all pairs j < i (:102-137).
`cross_histograms(embeddings, labels)` and `cross_accuracy(embeddings, labels, th)` (not in the reference) give the same
histograms and the same accuracy as cross_score + performance_acc from one pass over the pairs that keeps no pair list
(frhip_cross_hist), so the cross test runs at any N.
`identify(probe, gallery, k)` and `identification_rates(...)` (not in the reference) are the 1:N side: the k best gallery entries of
every probe under the same scores, to the bit, as cross_score's (frhip_gallery_topk; the P x G scores are never written), and
the closed-set CMC / open-set TPIR @ FPIR figures from those lists (host logic, numpy).
pair_score runs on the MI355X (frhip_pair_score: float64 accumulation of float32 differences in the reference's
order, so `int(99999*score)` is bit-exact); the ROC scan and accuracy are host logic on 100 001-bin histograms
(the reference runs them on the host too) restated with numpy cumulative sums instead of Python loops.
"""
import numpy as np
import torch


def pair_score(embedding_1, embedding_2, labels, metric="euclidean", min_level=3, max_level=9):
    assert metric in ["euclidean", "cosine"], "Invalid metric !!!"
    from frhip import ops
    if not torch.cuda.is_available():
        raise RuntimeError("utils.eval.pair_score (frhip) needs the MI355X; there is no CPU path")
    e1 = torch.as_tensor(np.asarray(embedding_1), dtype=torch.float32).cuda().contiguous() if not torch.is_tensor(embedding_1) else embedding_1.float().cuda().contiguous()
    e2 = torch.as_tensor(np.asarray(embedding_2), dtype=torch.float32).cuda().contiguous() if not torch.is_tensor(embedding_2) else embedding_2.float().cuda().contiguous()
    lab = torch.as_tensor(np.asarray(labels)).long().cuda().contiguous() if not torch.is_tensor(labels) else labels.long().cuda().contiguous()
    scores, _, hg, hi = ops.pair_score(e1, e2, lab)
    return hg.cpu().numpy().astype(np.float64), hi.cpu().numpy().astype(np.float64), scores.cpu().numpy()


def _dev(x, dtype):
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    return t.to(dtype).cuda().contiguous()


def cross_score(embeddings, labels, metric="euclidean"):
    """Cross-matching scores of ONE embedding set (reference utils/eval.py:102-137): every pair j < i in the reference's
    order l = i(i-1)/2 + j -> (hist_genuine[100001], hist_imposter[100001], score_list[P], label_list[P]), label 1 where the
    two identities agree.  frhip_cross_score: the reference's float64-of-float32-differences arithmetic, so the histogram
    bins are bit-exact."""
    assert metric in ["euclidean", "cosine"], "Invalid metric !!!"
    from frhip import ops
    if not torch.cuda.is_available():
        raise RuntimeError("utils.eval.cross_score (frhip) needs the MI355X; there is no CPU path")
    scores, plab, _, hg, hi = ops.cross_score(_dev(embeddings, torch.float32), _dev(labels, torch.int64).view(-1))
    return hg.cpu().numpy().astype(np.float64), hi.cpu().numpy().astype(np.float64), scores.cpu().numpy(), plab.cpu().numpy()


def performance_roc(hist_genuine, hist_imposter, min_level=3, max_level=9):
    th = np.arange(int(1e5), 0, -1)
    total_genuine, total_imposter = int(sum(hist_genuine)), int(sum(hist_imposter))
    hg, hi = np.asarray(hist_genuine, dtype=np.float64)[th], np.asarray(hist_imposter, dtype=np.float64)[th]
    cum_g = np.concatenate([[0.0], np.cumsum(hg)[:-1]])
    cum_i = np.concatenate([[0.0], np.cumsum(hi)[:-1]])
    far = (cum_i + hi) / total_imposter
    frr = (total_genuine - cum_g) / total_genuine
    diff = np.abs(far - frr)
    eer, eer_threshold = None, 1e5
    if diff.min() < 1:
        j = int(np.argmax(diff == diff.min()))
        eer, eer_threshold = (far[j] + frr[j]) / 2, int(th[j])
    roc_result = "\n"
    for level in range(min_level, max_level + 1):
        ok = far <= float(f"1e-{level}")
        j = int(np.argmin(np.where(ok, frr, np.inf)))
        roc_result += f"- FRR @ FAR{level} {100 * frr[j]:6.3f}%, (Threshold = {th[j] / 1e5:.5f})  \n"
    roc_result += "- EER {0:6.3f}%, (Threshold = {1:.5f})\n".format(100 * eer, eer_threshold / 1e5)
    roc_result += "- Total count = {:,}\n".format(total_genuine + total_imposter)
    roc_result += "- Total genuine count = {:,}\n".format(total_genuine)
    roc_result += "- Total imposter count = {:,}\n".format(total_imposter)
    return roc_result, eer_threshold


def performance_acc(score_list, label_list, th):
    score_list, label_list = np.asarray(score_list), np.asarray(label_list)
    fr = int(np.sum((score_list <= th / 1e5) & (label_list == 1)))
    fa = int(np.sum((score_list > th / 1e5) & (label_list == 0)))
    return (1 - (fa + fr) / (len(score_list))) * 100


# one-entry cache of the last cross_hist pass: cross_histograms and cross_accuracy on the same inputs share it
_CROSS_CACHE = {}


def _cross_counts(embeddings, labels):
    """-> (hist_genuine, hist_imposter, thr_genuine, thr_imposter) int64 numpy, n, from one frhip_cross_hist pass (cached)"""
    from frhip import ops
    if not torch.cuda.is_available():
        raise RuntimeError("utils.eval cross histograms (frhip) need the MI355X; there is no CPU path")
    e, lab = _dev(embeddings, torch.float32), _dev(labels, torch.int64).view(-1)
    if e.dim() != 2 or lab.numel() != e.shape[0]:
        raise ValueError("cross histograms: embeddings [n, d] and n labels expected, got %s and %d" % (tuple(e.shape), lab.numel()))
    c = _CROSS_CACHE.get("last")
    if c is not None and c[0].shape == e.shape and torch.equal(c[0], e) and torch.equal(c[1], lab):
        return c[2], e.shape[0]
    counts = tuple(h.cpu().numpy() for h in ops.cross_hist(e, lab))
    own = lambda t, src: t.clone() if torch.is_tensor(src) and t.data_ptr() == src.data_ptr() else t   # noqa: E731
    _CROSS_CACHE["last"] = (own(e, embeddings), own(lab, labels), counts)
    return counts, e.shape[0]


def cross_histograms(embeddings, labels, metric="euclidean"):
    """(hist_genuine[100001], hist_imposter[100001]) float64 of every pair j < i: element for element those of cross_score, without
    the pair list; they go straight into performance_roc"""
    assert metric in ["euclidean", "cosine"], "Invalid metric !!!"
    (hg, hi, _, _), _ = _cross_counts(embeddings, labels)
    return hg.astype(np.float64), hi.astype(np.float64)


def cross_accuracy(embeddings, labels, th, metric="euclidean"):
    """performance_acc(score_list, label_list, th) of cross_score's lists, exactly, from the threshold-slot histograms:
    fr = genuine pairs with score <= th / 1e5, fa = imposter pairs with score > th / 1e5.  th: an integer in [0, 100000]
    (performance_roc's eer_threshold is one)."""
    assert metric in ["euclidean", "cosine"], "Invalid metric !!!"
    if not (float(th).is_integer() and 0 <= th <= 100000):
        raise ValueError("cross_accuracy: th = %r is not an integer in [0, 100000]" % (th,))
    t = int(th)
    (_, _, tg, ti), n = _cross_counts(embeddings, labels)
    if n < 2:
        raise ValueError("cross_accuracy: %d embeddings make no pair" % n)
    fr = int(tg[:t + 1].sum())
    fa = int(ti[t + 1:].sum())
    return (1 - (fa + fr) / (n * (n - 1) // 2)) * 100


def identify(probe, gallery, k=10, exclude_self=False):
    """1:N search: for every probe row the k best gallery rows -> (top_score float64 [P,k], top_index int64 [P,k]) numpy, score
    descending then gallery index ascending; the scores are cross_score's to the bit; fewer than k candidates leave -inf / -1 at the
    end.  exclude_self: probe and gallery are the same set (same length) and row i is not a candidate for probe i (leave-one-out)."""
    from frhip import ops
    if not torch.cuda.is_available():
        raise RuntimeError("utils.eval.identify (frhip) needs the MI355X; there is no CPU path")
    p, g = _dev(probe, torch.float32), _dev(gallery, torch.float32)
    if p.dim() != 2 or g.dim() != 2 or p.shape[1] != g.shape[1]:
        raise ValueError("identify: probe [P, d] and gallery [G, d] expected, got %s and %s" % (tuple(p.shape), tuple(g.shape)))
    excl = None
    if exclude_self:
        if p.shape[0] != g.shape[0]:
            raise ValueError("identify: exclude_self needs probe and gallery of the same length, got %d and %d" % (p.shape[0], g.shape[0]))
        excl = torch.arange(p.shape[0], dtype=torch.int64, device=p.device)
    top_score, top_index = ops.gallery_topk(p, g, int(k), excl)
    return top_score.cpu().numpy(), top_index.cpu().numpy()


def identification_rates(top_score, top_index, probe_labels, gallery_labels, ranks=(1, 5, 10), fpirs=(1e-1, 1e-2, 1e-3),
                         exclude_self=False):
    """Closed-set CMC and open-set TPIR @ FPIR from the lists of identify().  Host logic, no GPU.
    A probe is mated if its label occurs among the gallery labels (under exclude_self: in a row other than its own).
      cmc[r]  : share of the mated probes with a same-label entry among the first r list positions (r <= k)
      open set: s = the top-1 scores of the non-mated probes, descending; for an FPIR f the threshold is tau = s[floor(f len(s))]
                and a score is accepted if > tau, so the realised FPIR never exceeds f; tpir[f] = share of the mated probes whose
                rank-1 entry has their label and a score > tau.
    -> {"cmc": {r: rate}, "tpir": {f: rate}, "threshold": {f: tau}, "fpir": {f: realised}, "n_probe", "n_mated", "n_nonmated",
    "report"}; without mated probes the cmc / tpir entries are None, without non-mated ones the tpir / threshold / fpir entries."""
    top_score, top_index = np.asarray(top_score, dtype=np.float64), np.asarray(top_index, dtype=np.int64)
    pl, gl = np.asarray(probe_labels).reshape(-1), np.asarray(gallery_labels).reshape(-1)
    if top_score.ndim != 2 or top_score.shape != top_index.shape or top_score.shape[0] != pl.size:
        raise ValueError("identification_rates: top_score / top_index [P, k] and P probe labels expected, got %s, %s and %d"
                         % (top_score.shape, top_index.shape, pl.size))
    n, k = top_index.shape
    if any(int(r) != r or r < 1 or r > k for r in ranks):
        raise ValueError("identification_rates: ranks %r outside 1..k = %d" % (tuple(ranks), k))
    if exclude_self and gl.size != n:
        raise ValueError("identification_rates: exclude_self needs as many gallery labels as probes, got %d and %d" % (gl.size, n))
    if top_index.size and top_index.max() >= gl.size:
        raise ValueError("identification_rates: index %d outside the %d gallery labels" % (top_index.max(), gl.size))
    values, counts = np.unique(gl, return_counts=True)
    if values.size:
        at = np.minimum(np.searchsorted(values, pl), values.size - 1)
        occurs = np.where(values[at] == pl, counts[at], 0)
    else:
        occurs = np.zeros(n, dtype=np.int64)
    if exclude_self:
        occurs = occurs - 1                                    # the probe's own row carries its label
    mated = occurs > 0
    valid = top_index >= 0
    hit = valid & (gl[np.where(valid, top_index, 0)] == pl[:, None]) if gl.size else np.zeros((n, k), dtype=bool)
    n_mated, n_non = int(mated.sum()), int((~mated).sum())
    first_hit = np.where(hit.any(axis=1), hit.argmax(axis=1), k)        # list position of the first same-label entry, k: none
    cmc = {int(r): (float(np.mean(first_hit[mated] < r)) if n_mated else None) for r in ranks}
    tpir, threshold, realised = {}, {}, {}
    top1 = top_score[:, 0] if k else np.full(n, -np.inf)
    s = np.sort(top1[~mated])[::-1]
    for f in fpirs:
        if n_non == 0:
            tpir[f], threshold[f], realised[f] = None, None, None
            continue
        tau = float(s[min(int(np.floor(f * n_non)), n_non - 1)])
        threshold[f] = tau
        realised[f] = float(np.mean(s > tau))
        tpir[f] = float(np.mean(hit[mated, 0] & (top1[mated] > tau))) if n_mated else None
    pct = lambda v: "   n/a " if v is None else "%6.3f%%" % (100 * v)       # noqa: E731
    report = "\n"
    for r in ranks:
        report += "- Rank-%d rate %s  \n" % (r, pct(cmc[int(r)]))
    for f in fpirs:
        th = "n/a" if threshold[f] is None else "%.5f" % threshold[f]
        report += "- TPIR @ FPIR %g %s, (Threshold = %s, realised FPIR %s)  \n" % (f, pct(tpir[f]), th, pct(realised[f]).strip())
    report += "- Total probe count = {:,}\n".format(n)
    report += "- Mated probe count = {:,}\n".format(n_mated)
    report += "- Non-mated probe count = {:,}\n".format(n_non)
    return {"cmc": cmc, "tpir": tpir, "threshold": threshold, "fpir": realised, "n_probe": n, "n_mated": n_mated,
            "n_nonmated": n_non, "report": report}
