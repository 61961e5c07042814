#!/usr/bin/env python3
"""Cost of K sub-centres per class in the fused head, bf16, one rank: head forward (normalise embeddings and centres, fused forward,
target probability, loss) and head backward (dT recompute, dE GEMM, normalise-backward, dW) through nets.PartialFC.HipHeadKernels, at
K = 1, 2, 3 for the cfg 2 head shape (512 x 122 000 x 512, rate 1.0) and the cfg 3 shard shape (4 096 x 1 525 x 512).

K = 1 makes the calls the head made before sub-centres existed; K > 1 runs head_sub_kernel and, by the dense-zero choice, K times the
GEMM work in the backward pass.  The K values alternate 1 2 3 1 2 3 ... inside one process on the same inputs, `--rounds` times,
`--iters` calls per round between two device events; reports each median and spread over the rounds, and K = 3 over 3 x K = 1.
To compare K = 1 with another build of the library, run this tool alternately with FRHIP_LIB_PATH pointing at either (tools/ab_libs.sh
does the same for bench.py).

Usage:  python tools/subcenter_bench.py [--rounds 7] [--iters 10]      prints one JSON line per shape.  GPU box only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd")]

import torch  # noqa: E402

S, M = 64.0, 0.4
KS = (1, 2, 3)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def bench(n, classes, rounds, iters):
    from nets.PartialFC import HipHeadKernels
    kern = HipHeadKernels(torch.bfloat16)
    gen = torch.Generator(device="cuda").manual_seed(1)
    emb = torch.randn((n, 512), device="cuda", generator=gen)
    labels = torch.randint(0, classes, (n,), device="cuda", generator=gen).to(torch.int32)
    table = torch.randn((max(KS) * classes, 512), device="cuda", generator=gen) * 0.01
    up = torch.ones(1, device="cuda")
    state = {}

    def fwd(k):
        sub = {"subcenters": k} if k > 1 else {}
        ehat, enorm = kern.normalize(emb)
        what, wnorm = kern.normalize(table[:k * classes])
        zt, rmax, rsum = kern.forward_stats(ehat, what, labels, S, M, **sub)[:3]
        kern.loss(kern.target_prob(zt, labels, rmax, rsum))
        state[k] = (ehat, enorm, what, wnorm, rmax, rsum, sub)

    def bwd(k):
        ehat, enorm, what, wnorm, rmax, rsum, sub = state[k]
        kern.backward(ehat, enorm, what, wnorm, labels, S, M, rmax, rsum, n, up, **sub)

    for k in KS:
        for _ in range(3):
            fwd(k)
            bwd(k)
    torch.cuda.synchronize()
    us = {(p, k): [] for p in ("fwd", "bwd") for k in KS}
    for _ in range(rounds):
        for k in KS:
            us[("fwd", k)].append(timed(lambda: fwd(k), iters))
            us[("bwd", k)].append(timed(lambda: bwd(k), iters))
    out = {"shape": [n, classes, 512], "dtype": "bf16", "rounds": rounds, "iters": iters}
    for (p, k), v in us.items():
        v = sorted(v)
        out["%s_K%d_us" % (p, k)] = {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
    for p in ("fwd", "bwd"):
        out["%s_K3_over_3xK1" % p] = round(out["%s_K3_us" % p]["median"] / (3 * out["%s_K1_us" % p]["median"]), 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for n, classes in ((512, 122000), (4096, 1525)):
        bench(n, classes, a.rounds, a.iters)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
