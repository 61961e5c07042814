#!/usr/bin/env python3
"""Cost of the UniFace (sigmoid / BCE) head step beside the plain ArcFace head step at the cfg-2 head shape (512 x 122 000 x 512, bf16,
one rank): the whole head through nets.PartialFC -- normalise, fused forward, loss, dT, dE, dW -- forward + backward.  Both heads run
the same two GEMM passes; the BCE epilogue spends an exp and a log1p per element in the forward and an exp and a division in the
recompute where the softmax epilogue spends one exp, and it reads no row statistics.

The two heads alternate A B A B ... inside one process on the same inputs, `--rounds` times, `--iters` steps per round between two
device events (tools/elastic_head_bench.py's scheme); reports each head's median and spread over the rounds and their ratio, then the two
big kernels alone (forward and dT recompute, ArcFace and BCE alternating) and the three small launches behind the BCE forward.

Usage:  python tools/uniface_head_bench.py [--rounds 7] [--iters 20]      prints one JSON line"""
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
    """the two big kernels with the ArcFace and the BCE epilogue, alternating, and the small launches behind the BCE forward"""
    from frhip import ops
    from nets.ArcFace import BceMargin, margin_of
    n = emb.shape[0]
    ehat, _ = ops.l2norm_rows(emb.contiguous(), torch.bfloat16)
    what, _ = ops.l2norm_rows(head.weight_activated.detach(), torch.bfloat16)
    lab = labels.to(torch.int32)
    mg = margin_of(head.margin_softmax)
    bce = BceMargin(*mg, head.margin_softmax.bias.detach().clone())
    _, rmax, rsum = ops.head_fwd(ehat, what, lab, mg.s, 0.5)
    _, rowloss, rowdb = ops.head_fwd(ehat, what, lab, mg.s, mg.m, margin=bce)
    calls = {"fwd_arcface": lambda: ops.head_fwd(ehat, what, lab, mg.s, 0.5),
             "fwd_bce": lambda: ops.head_fwd(ehat, what, lab, mg.s, mg.m, margin=bce),
             "bwd_dt_arcface": lambda: ops.head_bwd_dt(ehat, what, lab, mg.s, 0.5, rmax, rsum, 1.0 / n, transposed=True),
             "bwd_dt_bce": lambda: ops.head_bwd_dt(ehat, what, lab, mg.s, mg.m, None, None, 1.0 / n, transposed=True, margin=bce)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            ms[name] += timed(fn, 1, iters)
    out = {name: _stats(v) for name, v in ms.items()}
    pair = ops.bce_reduce(rowloss, rowdb)
    small = {"bce_reduce": lambda: ops.bce_reduce(rowloss, rowdb), "bce_merge": lambda: ops.bce_merge(pair, n)}
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
    from nets.ArcFace import ArcFace, UniFace
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(tempfile.mkdtemp(), "pg"), rank=0, world_size=1)
    n, classes, d = a.n, a.classes, 512
    gen = torch.Generator(device="cuda").manual_seed(1)
    emb = (torch.randn((n, d), device="cuda", generator=gen) * (0.2 + 2.0 * torch.rand((n, 1), device="cuda", generator=gen)))
    emb.requires_grad_(True)
    labels = torch.randint(0, classes, (n,), device="cuda", generator=gen)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=1.0, mixed_precision=True, loss_s=64.0, loss_m=0.5, frhip_dtype="bf16")
    factories = (("arcface", ArcFace), ("uniface", lambda s, m: UniFace(s, 0.4)))
    heads = {}
    for name, factory in factories:
        torch.manual_seed(2)
        heads[name] = P.PartialFC(conf, classes, margin_loss=factory).cuda()

    def step(name):
        head = heads[name]
        emb.grad = None
        for p in head.parameters():
            p.grad = None
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
    out["uniface_over_arcface"] = round(out["uniface"]["median_ms"] / out["arcface"]["median_ms"], 4)
    out["kernels"] = kernels_alone(heads["uniface"], emb.detach(), labels, a.rounds, a.iters)
    out["bias"] = float(heads["uniface"].margin_softmax.bias.detach())
    print(json.dumps(out))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
