#!/usr/bin/env python3
"""How far do AlterNet50's whole-net gradients move when the tail ReLU decides a few elements the other way?  (CPU, oracle only.)

tests/wholenet.check_whole_net_train holds everything upstream of bn2 -> ReLU to `kink_rtol` because an implementation whose bn2 output
differs from the reference's by fp32 round-off (1e-4 after 50 blocks) flips the pre-ReLU values that lie that close to zero.  This
script repeats the measurement behind that bound for a whole-net fixture: it runs the oracle twice, with the ReLU threshold at 0 and at
--shift, and prints the number of flipped elements (those a tail dropout mask zeroes do not count) and every gradient's movement as a
fraction of its rms.

Usage:  python tools/kink_shift.py [--fixture alternet50_b8_train_stochastic] [--shift 1e-4]
"""
import argparse
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import alternet_ref, recipe  # noqa: E402
from wholenet import stochastic_draws  # noqa: E402


TAIL = ("fc.", "bn3.", "bn2.", "layer4.3.norm2.", "layer4.3.attn.proj.")        # check_whole_net_train's kink_free of the AlterNet tests
NOISE = ("proj.bias", "v_bias")


def run(g, keeps, mask, kink):
    """-> (every parameter gradient, the input of bn2)"""
    spec = alternet_ref.alter_spec("AlterNet50")
    sd = alternet_ref.fill_special(recipe.fill_state(spec, int(g["seed"])), spec)
    names = [k for k, _, kind in spec if kind in ("conv", "linear_w", "linear_b", "bn_w", "bn_b", "logit_scale")]
    for k in names:
        sd[k].requires_grad_(True)
    seen = []
    orig = alternet_ref.tail

    def tail(sd_, y, training, dropout_mask=None):
        seen.append(y.detach())
        return orig(sd_, y, training, dropout_mask, kink=kink)
    alternet_ref.tail = tail
    try:
        y = alternet_ref.alter_forward(sd, recipe.images(int(g["seed"]) + 1, int(g["batch"]), 192, 192), "AlterNet50", True,
                                       keeps=keeps, dropout_mask=mask)
    finally:
        alternet_ref.tail = orig
    y.backward(recipe.normal(int(g["seed"]) + 2, tuple(y.shape), 0.05))
    return {k: sd[k].grad.double() for k in names}, seen[0], sd


def needed_rtol(want, got, full):
    """the smallest `t` at which check_whole_net_train's element test |got - want| <= t |want| + 2 t rms accepts the movement, over the
    elements the check reads: the 256 probe positions, or the whole tensor where the fixture stores it"""
    rms = float(want.pow(2).mean().sqrt())
    if not full:
        pos = torch.from_numpy(recipe.probe_positions(want.numel()))
        want, got = want.reshape(-1)[pos], got.reshape(-1)[pos]
    return float(((got - want).abs() / (want.abs() + 2 * rms + 1e-30)).max())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="alternet50_b8_train_stochastic")
    ap.add_argument("--shift", type=float, default=1e-4)
    a = ap.parse_args()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", a.fixture + ".npz")))
    keeps, mask = stochastic_draws(g) if "dropout_seed" in g else (None, None)
    g0, x4, sd = run(g, keeps, mask, 0.0)
    g1, _, _ = run(g, keeps, mask, a.shift)
    mu, var = x4.mean((0, 2, 3), keepdim=True), x4.var((0, 2, 3), unbiased=False, keepdim=True)         # training-mode bn2
    z = (x4 - mu) / torch.sqrt(var + 1e-5) * sd["bn2.weight"].detach().view(1, -1, 1, 1) + sd["bn2.bias"].detach().view(1, -1, 1, 1)
    live = torch.ones_like(z, dtype=torch.bool) if mask is None else mask != 0
    print("pre-ReLU values: %d, within %.0e of zero: %d (of them not zeroed by the dropout mask: %d), flipped by the shift: %d"
          % (z.numel(), a.shift, int((z.abs() < a.shift).sum()), int(((z.abs() < a.shift) & live).sum()),
             int(((z > 0) & (z <= a.shift) & live).sum())))
    rows = []
    for k in g0:
        if float(g0[k].pow(2).mean().sqrt()) > 1e-7 and not k.endswith(NOISE) and k != "fc.bias":
            rows.append((needed_rtol(g0[k], g1[k], ("gfull." + k) in g), k))
    rows.sort(reverse=True)
    up, tl = [r for r in rows if not r[1].startswith(TAIL)], [r for r in rows if r[1].startswith(TAIL)]
    print("movement in the check's terms (|d| / (|want| + 2 rms) over the elements it reads; the bound is kink_rtol):")
    for r in up[:6]:
        print("  upstream  %.3e  %s" % r)
    print("  layer4.3.attn.qkv.weight  %.3e" % [r[0] for r in rows if r[1] == "layer4.3.attn.qkv.weight"][0])
    for r in tl[:3]:
        print("  tail (kink_free, bound rtol)  %.3e  %s" % r)
