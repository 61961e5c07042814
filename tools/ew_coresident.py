"""Bandwidth of the element-wise BatchNorm passes ALONE and BESIDE a resident matrix kernel, per ResNet50 shape at B = 512 (bf16):
    python tools/ew_coresident.py [--fwd]
The backward pass never offers these kernels an empty chip: a weight-gradient workgroup of the side stream sits on every CU while they
run.  "beside" therefore times the pass on the current stream while a second stream runs the library's weight gradient of a
14 x 14 x 256 layer (frhip_conv_wgrad, 3 x 3) back to back; the timed window lies inside that stream's busy time (checked).  Each launch
takes another buffer set from a rotation of > 1.2 GB, so nothing is served by the 256-MB last-level cache.  Both forms of
frhip_set_ew_batch are timed: 0 = the row-at-a-time kernels, 1 = the batched kernels (the default)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd")]

import torch  # noqa: E402

from frhip import ops  # noqa: E402
from frhip._abi import check, lib  # noqa: E402

B = 512
SHAPES = [(56, 64), (28, 128), (14, 256), (7, 512)]


def launcher(fwd, rows, c, sets):
    p, s = ops._p, ops._s
    coef = torch.full((5, c), 0.5, dtype=torch.float32, device="cuda")
    if fwd:           # residual form: out = relu(y * scale + shift + res)
        def go(i):
            a, b, o = sets[i % len(sets)]
            check(lib().frhip_bn_apply(0, p(a), p(coef[0]), p(coef[1]), p(b), None, None, 1, p(o), rows, c, s()), "frhip_bn_apply")
    else:
        def go(i):
            a, b, o = sets[i % len(sets)]
            check(lib().frhip_bn_bwd_apply(0, p(a), p(b), p(coef[0]), p(coef[1]), p(coef[2]), p(coef[3]), p(coef[4]), p(o), rows, c,
                                           s()), "frhip_bn_bwd_apply")
    return go


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fwd", action="store_true", help="time frhip_bn_apply (residual form) instead of frhip_bn_bwd_apply")
    ap.add_argument("--reps", type=int, default=24)
    args = ap.parse_args()
    side = torch.cuda.Stream()
    # the resident matrix kernel: weight gradient of a 14 x 14 x 256 layer
    wx = torch.randn((B, 14, 14, 256), device="cuda").to(torch.bfloat16)
    wdy = torch.randn((B, 14, 14, 256), device="cuda").to(torch.bfloat16)
    dw = torch.zeros((256, 3, 3, 256), dtype=torch.float32, device="cuda")
    with torch.cuda.stream(side):
        ops.conv_wgrad(wdy, wx, dw, 3, 3, 1, 1)
    torch.cuda.synchronize()
    old = lib().frhip_set_ew_batch(-1)
    print("%s, B = %d, bf16" % ("bn_apply (residual, relu)" if args.fwd else "bn_bwd_apply (relu mask)", B))
    for h, c in SHAPES:
        rows = B * h * h
        nbytes = rows * c * 2
        nset = (1200 << 20) // (3 * nbytes) + 2
        sets = [(torch.randn((rows, c), device="cuda").to(torch.bfloat16), torch.randn((rows, c), device="cuda").to(torch.bfloat16),
                 torch.empty((rows, c), dtype=torch.bfloat16, device="cuda")) for _ in range(nset)]
        go = launcher(args.fwd, rows, c, sets)
        print("%d x %d x %d: %.0f MB per launch, %d buffer sets" % (h, h, c, 3 * nbytes / 1e6, nset))
        for form in (0, 1):
            lib().frhip_set_ew_batch(form)
            res = []
            for beside in (False, True):
                for i in range(nset):
                    go(i)
                torch.cuda.synchronize()
                e0, e1, es = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                if beside:
                    started = torch.cuda.Event()
                    with torch.cuda.stream(side):
                        ops.conv_wgrad(wdy, wx, dw, 3, 3, 1, 1)
                        started.record()
                        # enough launches to outlast the timed window (about 160 us each)
                        for _ in range(int(args.reps * (3 * nbytes / 2.0e12) / 120e-6) + 12):
                            ops.conv_wgrad(wdy, wx, dw, 3, 3, 1, 1)
                        es.record()
                    torch.cuda.current_stream().wait_event(started)
                e0.record()
                for i in range(args.reps):
                    go(i)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / args.reps * 1e3
                covered = (not beside) or e1.elapsed_time(es) > 0
                res.append((us, 3 * nbytes / us / 1e6, covered))
            print("  %-14s alone %7.1f us %5.2f TB/s   beside %7.1f us %5.2f TB/s%s"
                  % ("batched" if form else "row at a time", res[0][0], res[0][1], res[1][0], res[1][1], "" if res[1][2] else "   (side stream ran out early)"))
        del sets, go
        torch.cuda.empty_cache()
    lib().frhip_set_ew_batch(old)


if __name__ == "__main__":
    main()
