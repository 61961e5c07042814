#!/usr/bin/env python3
"""Cost of the ElasticFace head step beside the ArcFace head step at the cfg-2 head shape (512 x 122 000 x 512, bf16, one rank): the
whole head through nets.PartialFC._MarginSoftmaxFn -- normalise, fused forward, loss, dT, dE, dW -- forward + backward.
ElasticFace-Arc adds one launch (frhip_elastic_margins) and two floats per row in the head kernels; ElasticFace-Arc+ adds four
(frhip_elastic_draws, frhip_head_target_cos, the two of frhip_elastic_assign).

The three margins alternate A B C A B C ... inside one process on the same inputs, `--rounds` times, `--iters` steps per round between
two device events; reports each margin's median and spread over the rounds, and the added launches alone (device events around
`--iters` back-to-back calls, so a figure near the launch floor is the launch floor).

Usage:  python tools/elastic_head_bench.py [--rounds 7] [--iters 20]      prints one JSON line"""
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

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def timed(fn, rounds, iters):
    """-> sorted per-call times in ms of `rounds` windows of `iters` calls"""
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return sorted(out)


def added_launches(head, emb, labels, rounds, iters):
    """the launches ElasticFace puts in front of the head kernels, each alone, in microseconds (median over the rounds)"""
    from frhip import ops
    from nets.ArcFace import margin_of
    n = emb.shape[0]
    ehat, _ = ops.l2norm_rows(emb.contiguous(), torch.bfloat16)
    what, _ = ops.l2norm_rows(head.weight_activated.detach(), torch.bfloat16)
    lab = labels.to(torch.int32)
    mg = margin_of(head.margin_softmax)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = ops.elastic_draws(n, mg.m, mg.std, mg.seed, step, True)
    tcos = ops.head_target_cos(ehat, what, lab)
    calls = {"elastic_margins": lambda: ops.elastic_margins(n, mg.kind, mg.m, mg.std, mg.seed, step, True),
             "elastic_draws": lambda: ops.elastic_draws(n, mg.m, mg.std, mg.seed, step, True),
             "head_target_cos": lambda: ops.head_target_cos(ehat, what, lab),
             "elastic_assign": lambda: ops.elastic_assign(tcos, g, mg.kind)}
    out = {}
    for name, fn in calls.items():
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
    from nets.ArcFace import ArcFace, ElasticFace
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(tempfile.mkdtemp(), "pg"), rank=0, world_size=1)
    n, classes, d = a.n, a.classes, 512
    gen = torch.Generator(device="cuda").manual_seed(1)
    emb = (torch.randn((n, d), device="cuda", generator=gen) * (0.2 + 2.0 * torch.rand((n, 1), device="cuda", generator=gen)))
    emb.requires_grad_(True)
    labels = torch.randint(0, classes, (n,), device="cuda", generator=gen)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=1.0, mixed_precision=True, loss_s=64.0, loss_m=0.5, frhip_dtype="bf16")
    factories = (("arcface", ArcFace), ("elastic_arc", functools.partial(ElasticFace, std=0.05)),
                 ("elastic_arc_plus", functools.partial(ElasticFace, std=0.0175, plus=True)))
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
        v = sorted(v)
        out[name] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    for name in ("elastic_arc", "elastic_arc_plus"):
        out[name + "_over_arcface"] = round(out[name]["median_ms"] / out["arcface"]["median_ms"], 4)
    out["added_launches"] = added_launches(heads["elastic_arc_plus"], emb.detach(), labels, a.rounds, a.iters)
    print(json.dumps(out))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
