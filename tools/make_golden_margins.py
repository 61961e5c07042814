#!/usr/bin/env python3
"""Generate the margin-variant fixtures tests/golden/{head_margin_*, margin_*, train_step_*_cosface_*}.npz by running the REAL
reference modules (build container only), the same way tools/make_golden.py does for ArcFace (whose fixtures this script
leaves alone).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_margins.py [--only NAME]

Margin variants (reference nets/ArcFace.py), each built with the PartialFC arguments (conf.loss_s, conf.loss_m):
  cosface    CosFace(s, m)
  arc_filt   CombinedMarginLoss(s, 1.0, m, 0.0, THR)      ArcFace + interclass filtering
  cos_filt   CombinedMarginLoss(s, 1.0, 0.0, m, THR)      CosFace + interclass filtering
  arc_easy   ArcFace(s, m) with easy_margin = True set after construction
THR = 0.1: at D = 128 the random cosines have a standard deviation of about 0.09, so roughly 13 % of the elements are filtered; the
head fixtures store the count (n_filtered of n_elements, per rank).
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

from make_golden import TRAIN_PROBED, _init_pg, _ref, save  # noqa: E402
from oracle import recipe, resnet_ref  # noqa: E402

THR = 0.1
KINDS = ("cosface", "arc_filt", "cos_filt", "arc_easy")


def _margin_factory(A, kind):
    if kind == "cosface":
        return A.CosFace
    if kind == "arc_filt":
        return lambda s, m: A.CombinedMarginLoss(s, 1.0, m, 0.0, THR)
    if kind == "cos_filt":
        return lambda s, m: A.CombinedMarginLoss(s, 1.0, 0.0, m, THR)
    if kind == "arc_easy":
        return A.ArcFace
    raise ValueError(kind)


def _build_margin(A, kind, s, m):
    mod = _margin_factory(A, kind)(s, m)
    if kind == "arc_easy":
        mod.easy_margin = True
    return mod


def _count_filtered(logits, labels):
    """elements the reference's interclass filter zeroes (nets/ArcFace.py:28-39), from the clamped cosines it is given"""
    dirty = logits > THR
    pos = torch.where(labels.view(-1) != -1)[0]
    dirty[pos, labels.view(-1)[pos]] = False
    return int(dirty.sum())


# ----------------------------------------------------------------------------- head, any world size
def _head_worker(rank, ws, path, cfg, ret):
    A, P, _ = _ref()
    _init_pg(rank, ws, path)
    C, B, D, rate, s, m, kind = cfg["C"], cfg["B"], cfg["D"], cfg["rate"], cfg["s"], cfg["m"], cfg["kind"]
    conf = types.SimpleNamespace(emd_size=D, sample_rate=rate, mixed_precision=False, loss_s=s, loss_m=m)
    pfc = P.PartialFC(conf, C, margin_loss=_margin_factory(A, kind))
    if kind == "arc_easy":
        pfc.margin_softmax.easy_margin = True
    counts = []
    inner = pfc.margin_softmax.forward

    def counting(logits, labels):
        counts.append((_count_filtered(logits, labels), logits.numel()))
        return inner(logits, labels)

    pfc.margin_softmax.forward = counting
    W = recipe.normal(500 + rank, (pfc.num_local, D), 0.05)
    with torch.no_grad():
        if rate < 1:
            pfc.weight.copy_(W)
        else:
            pfc.weight_activated.data.copy_(W)
    dummy = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": pfc.parameters()}], lr=0.1, momentum=0.9)
    emb = recipe.normal(100 + rank, (B, D)).requires_grad_(True)
    lab = recipe.labels(200 + rank, B, C)
    lab[0] = 3
    lab[1] = 3
    torch.manual_seed(1000 + rank)
    loss = pfc(emb, lab.clone(), opt)
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    ret[rank] = dict(loss=loss.detach().clone(), d_emb=emb.grad.clone(), d_w_act=pfc.weight_activated.grad.clone(),
                     index=idx.clone().long(), n_filtered=counts[0][0], n_elements=counts[0][1])
    import torch.distributed as dist
    dist.destroy_process_group()


def gen_head(kind, ws, rate, C=1003, B=6, D=128, s=30.0, m=0.35):
    cfg = dict(C=C, B=B, D=D, rate=rate, s=s, m=m, kind=kind)
    mgr = mp.Manager()
    ret = mgr.dict()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "pg")
        if ws == 1:
            _head_worker(0, 1, path, cfg, ret)
        else:
            mp.spawn(_head_worker, args=(ws, path, cfg, ret), nprocs=ws, join=True)
    arrs = dict(C=C, B=B, D=D, rate=rate, s=s, m=m, ws=ws, dup=1, kind=kind, thr=THR if kind.endswith("filt") else 0.0)
    for r in range(ws):
        for k, v in ret[r].items():
            arrs["r%d_%s" % (r, k)] = v
    if kind.endswith("filt"):
        frac = sum(ret[r]["n_filtered"] for r in range(ws)) / sum(ret[r]["n_elements"] for r in range(ws))
        assert frac >= 0.05, frac
    save("head_margin_%s_ws%d_rate%s" % (kind, ws, str(rate).replace(".", "")), **arrs)


# ----------------------------------------------------------------------------- stand-alone margin module, edge cosines
def gen_margin(kind, s=30.0, m=0.35):
    A, _, _ = _ref()
    theta = np.cos(np.pi - m)
    thr32 = np.float32(THR)
    # target cosines: both sides of the ArcFace branch point cos(pi - m), of the easy-margin branch point 0 and of the threshold
    # (targets are never filtered); +-1 stay off the target (the reference's own gradient is not finite there)
    t = [0.3, -0.2, 0.999, -0.999, theta, np.nextafter(np.float32(theta), np.float32(1)), np.nextafter(np.float32(theta), np.float32(-1)),
         0.0, 1e-7, -1e-7, thr32, np.nextafter(thr32, np.float32(1)), 0.5]
    n, c = len(t) + 3, 130                                    # three rows without a target on this shard; c spans three mask words
    logits = recipe.normal(78, (n, c), 0.3).clamp_(-1, 1)
    labels = torch.full((n, 1), -1, dtype=torch.int64)
    for i in range(len(t)):
        labels[i, 0] = (i * 7) % c
        logits[i, labels[i, 0]] = float(t[i])
    # non-target edges: the threshold itself (kept), the next float above it (filtered), the clamp ends
    for i in range(n):
        for j, v in ((1, thr32), (2, np.nextafter(thr32, np.float32(1))), (3, 1.0), (4, -1.0), (129, np.nextafter(thr32, np.float32(-1)))):
            if labels[i, 0] != j:
                logits[i, j] = float(v)
    up = recipe.normal(79, (n, c))
    leaf = logits.clone().requires_grad_(True)
    mod = _build_margin(A, kind, s, m)
    out = mod(leaf.clone(), labels)
    out.backward(up)
    save("margin_%s" % kind, kind=kind, s=s, m=m, thr=THR if kind.endswith("filt") else 0.0, logits_in=logits, labels=labels,
         logits_out=out.detach(), upstream=up, grad=leaf.grad, n_filtered=_count_filtered(logits, labels) if kind.endswith("filt") else 0)


# ----------------------------------------------------------------------------- three SGD steps, ResNet-18, CosFace
def gen_train_cosface(rate=0.3):
    """tools/make_golden.py gen_train_steps(fresh=True) at rate 0.3 with margin_loss=CosFace"""
    A, P, R = _ref()
    import torch.distributed as dist
    import torch.nn.functional as F
    with tempfile.TemporaryDirectory() as td:
        _init_pg(0, 1, os.path.join(td, "pg"))
        C, B, steps = 256, 16, 3
        conf = types.SimpleNamespace(network="ResNet18", emd_size=512, sample_rate=rate, mixed_precision=False, loss_s=30.0, loss_m=0.35)
        enc = R.ResNet18(conf)
        spec = resnet_ref.resnet_spec(resnet_ref.BLOCKS["ResNet18"])
        sd = recipe.fill_state(spec, 777)
        for k, _, kd in spec:
            if kd == "bn_w" or kd == "bn_rv":
                sd[k].fill_(1.0)
            elif kd in ("bn_b", "bn_rm"):
                sd[k].zero_()
        enc.load_state_dict(sd, strict=True)
        pfc = P.PartialFC(conf, C, margin_loss=A.CosFace)
        W = recipe.normal(778, (C, 512), 0.01)
        with torch.no_grad():
            (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(W)
        opt = torch.optim.SGD([{"params": enc.parameters()}, {"params": pfc.parameters()}], lr=0.1, momentum=0.9, weight_decay=5e-4)
        arrs = dict(C=C, B=B, steps=steps, rate=rate, lr=0.1, momentum=0.9, wd=5e-4)
        losses, gnorms = [], []
        for st in range(steps):
            img, ids = recipe.images(779 + 10 * st, B), recipe.labels(780 + 10 * st, B, C)
            opt.zero_grad()
            enc.train()
            feat = F.normalize(enc(img))
            torch.manual_seed(3000 + st)
            loss = pfc(feat, ids.clone(), opt)
            loss.backward()
            gn = torch.nn.utils.clip_grad_norm_(enc.parameters(), 5)
            opt.step()
            losses.append(loss.detach().clone())
            gnorms.append(gn.detach().clone())
            if rate < 1:
                arrs["index_step%d" % st] = pfc.weight_index.clone()
        pfc.update() if rate < 1 else None
        arrs.update(losses=torch.stack(losses), grad_norms=torch.stack(gnorms))
        wfin = pfc.weight if rate < 1 else pfc.weight_activated.data
        for k in TRAIN_PROBED:
            arrs["probe." + k] = recipe.probe(enc.state_dict()[k].float())
        arrs["probe.head_weight"] = recipe.probe(wfin, 4096)
        save("train_step_resnet18_c256_fresh_cosface_rate%s" % str(rate).replace(".", "")[:2], **arrs)
        dist.destroy_process_group()


GENS = {
    "head_cosface_ws1_rate10": lambda: gen_head("cosface", 1, 1.0),
    "head_cosface_ws1_rate03": lambda: gen_head("cosface", 1, 0.3),
    "head_cosface_ws2_rate03": lambda: gen_head("cosface", 2, 0.3),
    "head_arc_filt_ws1_rate10": lambda: gen_head("arc_filt", 1, 1.0),
    "head_arc_filt_ws2_rate03": lambda: gen_head("arc_filt", 2, 0.3),
    "head_cos_filt_ws1_rate03": lambda: gen_head("cos_filt", 1, 0.3),
    "head_arc_easy_ws1_rate10": lambda: gen_head("arc_easy", 1, 1.0),
    **{"margin_" + k: (lambda k=k: gen_margin(k)) for k in KINDS},
    "train_cosface": gen_train_cosface,
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.set_num_threads(8)
    for name, fn in GENS.items():
        if a.only is None or a.only == name:
            fn()
