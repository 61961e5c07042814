#!/usr/bin/env python3
"""Image-gradient costs at bench shape, one JSON line (median of per-round medians, microseconds / milliseconds):
  stem_dx_train / stem_dx_eval : frhip_stem_dx at B = 512, 112 x 112 (training coefficients: conv recompute; eval: sparse form only)
  stem_dx_s2                   : frhip_stem_dx_s2 at B = 256, 192 x 192
  pgd_ms                       : one PGD iteration on ResNet50, B = 512: eval-mode forward + input-only backward (net.requires_grad_(False))
  train_ms                     : beside it, the encoder's training forward + backward (parameter gradients, x not differentiated)
The memory floors the kernels are compared against: ~0.67 GB / ~0.11 ms (stride 1), ~0.42 GB / ~0.07 ms (stride 2).

Usage:  python tools/input_grad_bench.py [--dtype bf16|fp32] [--rounds 5] [--iters 20]"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "face-recognition-pytorch_amd"))

import torch  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from frhip import ops
    import nets.resnet as R
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(0)
    # ---- stride-1 kernel operands at bench shape
    b, h, w = 512, 112, 112
    x = torch.randn(b, 3, h, w, device="cuda", generator=gen)
    wp = ops.pack_stem(torch.randn(64, 27, device="cuda", generator=gen) * 0.2, dt, kp=32)
    one = torch.ones(64, device="cuda")
    st = ops.bn_eval_affine(one, torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda"), one)
    pooled, arg = ops.stem_fwd(x, wp, st)
    dpool = torch.randn(pooled.shape, device="cuda", generator=gen).to(dt)
    coef = torch.randn(3, 64, device="cuda", generator=gen)
    # ---- stride-2 operands
    b2, h2 = 256, 192
    dy0 = torch.randn(b2, 96, 96, 64, device="cuda", generator=gen).to(dt)
    wp2 = ops.pack_stem(torch.randn(64, 27, device="cuda", generator=gen) * 0.2, dt)
    # ---- ResNet50 at B = 512
    conf = types.SimpleNamespace(network="ResNet50", emd_size=512, frhip_dtype=a.dtype)
    net = R.Encoder(conf).cuda()
    xi = torch.randn(b, 3, h, w, device="cuda", generator=gen)
    target = torch.nn.functional.normalize(torch.randn(b, 512, device="cuda", generator=gen), dim=1)

    def pgd():
        net.eval()
        net.requires_grad_(False)
        xa = xi.clone().requires_grad_(True)
        (1.0 - torch.nn.functional.cosine_similarity(net(xa), target, dim=1)).mean().backward()
        xi.sub_(1e-3 * xa.grad.sign())

    def train():
        net.train()
        net.requires_grad_(True)
        for p in net.parameters():
            p.grad = None
        net(xi).backward(target)

    cases = {"stem_dx_train_us": lambda: ops.stem_dx(x, wp, dpool, arg, pooled, coef),
             "stem_dx_eval_us": lambda: ops.stem_dx(x, wp, dpool, arg, pooled, coef, eval_mode=True),
             "stem_dx_s2_us": lambda: ops.stem_dx_s2(dy0, wp2, h2, h2),
             "pgd_ms": pgd, "train_ms": train}
    res = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, fn in cases.items():
            iters = a.iters if k.endswith("_us") else max(2, a.iters // 5)
            t = timed(fn, iters)
            res[k].append(t * 1000.0 if k.endswith("_us") else t)
    out = {"dtype": a.dtype}
    out.update({k: round(median(v), 2) for k, v in res.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
