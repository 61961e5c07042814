#!/usr/bin/env python3
"""Fused head forward + dT time per margin variant at 512 x 122 000 x 512 bf16 (the cfg-2 shard): ArcFace (the headline kernel),
CosFace, ArcFace + interclass filtering.  Same process, the variants alternate round by round so drift hits all of them alike;
prints the median of the per-round medians in microseconds as one JSON line.

Usage:  python tools/head_margin_bench.py [--rounds 7] [--iters 30]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "face-recognition-pytorch_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    from frhip import ops
    from nets.ArcFace import ARCFACE, COSFACE, Margin
    n, classes, d, s, m = 512, 122000, 512, 64.0, 0.5
    gen = torch.Generator(device="cuda").manual_seed(0)
    ehat, _ = ops.l2norm_rows(torch.randn((n, d), device="cuda", generator=gen), torch.bfloat16)
    what, _ = ops.l2norm_rows(torch.randn((classes, d), device="cuda", generator=gen), torch.bfloat16)
    lab = torch.randint(0, classes, (n,), device="cuda", generator=gen).to(torch.int32)
    variants = {"arcface": None, "cosface": Margin(COSFACE, False, s, 0.4, 0.0), "arcface_filter": Margin(ARCFACE, False, s, m, 0.05)}

    def step(mg):
        zt, rmax, rsum = ops.head_fwd(ehat, what, lab, s, m, margin=mg)
        ops.head_bwd_dt(ehat, what, lab, s, m, rmax, rsum, 1.0 / n, transposed=True, margin=mg)

    for mg in variants.values():
        for _ in range(5):
            step(mg)
    torch.cuda.synchronize()
    per = {k: [] for k in variants}
    for r in range(a.rounds):
        for k, mg in variants.items():
            ts = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(mg)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            per[k].append(sorted(ts)[len(ts) // 2])
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    out = {"shape": [n, classes, d], "dtype": "bf16", "us_median": {k: round(v, 1) for k, v in med.items()},
           "rounds_us": {k: [round(x, 1) for x in v] for k, v in per.items()},
           "rel_to_arcface": {k: round(v / med["arcface"], 4) for k, v in med.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
