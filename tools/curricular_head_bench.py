#!/usr/bin/env python3
"""Cost of the CurricularFace head step beside the ArcFace and the ElasticFace-Arc+ head steps at the cfg-2 head shape
(512 x 122 000 x 512, bf16, one rank): the whole head through nets.PartialFC._MarginSoftmaxFn -- normalise, fused forward, loss, dT, dE,
dW -- forward + backward.  CurricularFace adds the target-cosine pass ElasticFace-Arc+ has (frhip_head_target_cos), ONE small launch
(frhip_curricular_rows, against the three of the ranking) and a one-element copy of t; its two big kernels read two more floats per row
and spend one compare and two multiplies per element.

The three margins alternate A B C A B C ... inside one process on the same inputs, `--rounds` times, `--iters` steps per round between
two device events (tools/elastic_head_bench.py's scheme); reports each margin's median and spread over the rounds, then the two big
kernels alone (forward statistics and dT recompute, ArcFace and CurricularFace alternating) and the added launches alone.

Usage:  python tools/curricular_head_bench.py [--rounds 7] [--iters 20]      prints one JSON line"""
import argparse
import functools
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "face-recognition-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from elastic_head_bench import timed  # noqa: E402


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def kernels_alone(head, emb, labels, rounds, iters):
    """the two big kernels with the ArcFace and the CurricularFace epilogue, alternating, and CurricularFace's added launches"""
    from frhip import ops
    from nets.ArcFace import CurrRows, margin_of
    n = emb.shape[0]
    ehat, _ = ops.l2norm_rows(emb.contiguous(), torch.bfloat16)
    what, _ = ops.l2norm_rows(head.weight_activated.detach(), torch.bfloat16)
    lab = labels.to(torch.int32)
    mg = margin_of(head.margin_softmax)
    t = torch.full((1,), 0.3, device="cuda")
    tcos = ops.head_target_cos(ehat, what, lab)
    rows = CurrRows(mg.s, mg.m, ops.curricular_rows(tcos, mg.m, mg.alpha, t, False), t)
    _, rmax, rsum = ops.head_fwd(ehat, what, lab, mg.s, mg.m)
    calls = {"fwd_arcface": lambda: ops.head_fwd(ehat, what, lab, mg.s, mg.m),
             "fwd_curricular": lambda: ops.head_fwd(ehat, what, lab, mg.s, mg.m, margin=rows),
             "bwd_dt_arcface": lambda: ops.head_bwd_dt(ehat, what, lab, mg.s, mg.m, rmax, rsum, 1.0 / n, transposed=True),
             "bwd_dt_curricular": lambda: ops.head_bwd_dt(ehat, what, lab, mg.s, mg.m, rmax, rsum, 1.0 / n, transposed=True, margin=rows)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            ms[name] += timed(fn, 1, iters)
    out = {name: _stats(v) for name, v in ms.items()}
    small = {"head_target_cos": lambda: ops.head_target_cos(ehat, what, lab),
             "curricular_rows": lambda: ops.curricular_rows(tcos, mg.m, mg.alpha, t, True)}
    for name, fn in small.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        v = timed(fn, rounds, iters * 5)
        out[name + "_us"] = round(v[len(v) // 2] * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--classes", type=int, default=122000)
    a = ap.parse_args()
    import nets.PartialFC as P
    from nets.ArcFace import ArcFace, CurricularFace, ElasticFace
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(tempfile.mkdtemp(), "pg"), rank=0, world_size=1)
    n, classes, d = a.n, a.classes, 512
    gen = torch.Generator(device="cuda").manual_seed(1)
    emb = (torch.randn((n, d), device="cuda", generator=gen) * (0.2 + 2.0 * torch.rand((n, 1), device="cuda", generator=gen)))
    emb.requires_grad_(True)
    labels = torch.randint(0, classes, (n,), device="cuda", generator=gen)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=1.0, mixed_precision=True, loss_s=64.0, loss_m=0.5, frhip_dtype="bf16")
    factories = (("arcface", ArcFace), ("elastic_arc_plus", functools.partial(ElasticFace, std=0.0175, plus=True)),
                 ("curricular", CurricularFace))
    heads = {}
    for name, factory in factories:
        torch.manual_seed(2)
        heads[name] = P.PartialFC(conf, classes, margin_loss=factory).cuda()

    def step(name):
        head = heads[name]
        emb.grad = None
        head.weight_activated.grad = None
        head(emb, labels.clone(), None).backward()

    for name in heads:                                   # warm every shape and code object the timed window uses
        for _ in range(3):
            step(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in heads}
    for _ in range(a.rounds):
        for name in heads:
            ms[name] += timed(functools.partial(step, name), 1, a.iters)
    out = {"shape": [n, classes, d], "dtype": "bf16", "rounds": a.rounds, "iters": a.iters}
    for name, v in ms.items():
        out[name] = _stats(v)
    for name in ("elastic_arc_plus", "curricular"):
        out[name + "_over_arcface"] = round(out[name]["median_ms"] / out["arcface"]["median_ms"], 4)
    out["kernels"] = kernels_alone(heads["curricular"], emb.detach(), labels, a.rounds, a.iters)
    out["t_after"] = float(heads["curricular"].margin_softmax.t)
    print(json.dumps(out))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
