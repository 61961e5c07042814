#!/usr/bin/env python3
"""1:N identification cost: the exact top-k gallery search (frhip_gallery_topk, ops.gallery_topk) at (P, G) = (128, 10^6),
(10 000, 10^5) and (20 000, 20 000), d = 512, k = 10, random unit embeddings with repeated identities; and frhip_cross_hist at
N = 20 000 from the same process, whose pair rate is the yardstick (the same K loop, two 64-bit atomics per pair where the search
has one compare).  Reports kernel time (median of --reps), pairs/s, fp64 rate, the launches per search, the longest single launch
and peak device memory over inputs and outputs; also a d = 32 search at (10 000, 10^5), whose time is the part that does not scale
with d (epilogue, list inserts, merge), and the k = 64 search at (20 000, 20 000).

fp64 accounting as tools/cross_hist_bench.py: 2 FLOP per pair-k against AMD's published 78.6 TFLOP/s FP64 vector (not measured).

Usage:  python tools/identify_bench.py [--reps 3]      prints one JSON line"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "face-recognition-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from cross_hist_bench import FP64_VECTOR_PEAK_FLOPS, embeddings, peak_of, timed  # noqa: E402

SHAPES = ((128, 1_000_000), (10_000, 100_000), (20_000, 20_000))


def longest_launch(probe, gallery, k):
    """ms of the slowest single band launch (search + merge) of the default split, and the number of launches"""
    from frhip import ops
    from frhip._abi import check, lib
    p, d = probe.shape
    g = gallery.shape[0]
    ts = torch.full((p, k), float("-inf"), dtype=torch.float64, device="cuda")
    ti = torch.full((p, k), -1, dtype=torch.int64, device="cuda")
    ws = ops.gallery_topk_workspace(p, k, "cuda")
    b = ops.gallery_topk_bands(p, g)
    worst = 0.0
    for g0, g1 in zip(b, b[1:]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib().frhip_gallery_topk(probe.data_ptr(), gallery.data_ptr(), None, p, g, d, k, g0, g1, ts.data_ptr(), ti.data_ptr(),
                                       ws.data_ptr(), ws.numel() * 8, ops._s()), "gallery_topk")
        e1.record()
        e1.synchronize()
        worst = max(worst, e0.elapsed_time(e1))
    return worst, len(b) - 1


def search_row(p, g, d, k, reps):
    from frhip import ops
    gallery, _ = embeddings(g, d, g + 1)
    probe, _ = embeddings(p, d, p + 2)
    sec = timed(lambda: ops.gallery_topk(probe, gallery, k), reps)
    worst_ms, launches = longest_launch(probe, gallery, k)
    peak = peak_of(lambda: ops.gallery_topk(probe, gallery, k))
    pairs = p * g
    row = {"p": p, "g": g, "d": d, "k": k, "pairs": pairs, "kernel_s": round(sec, 4), "pairs_per_s": float("%.4g" % (pairs / sec)),
           "fp64_flops": float("%.4g" % (2 * pairs * d / sec)), "fp64_fraction_of_peak": round(2 * pairs * d / sec / FP64_VECTOR_PEAK_FLOPS, 4),
           "launches": launches, "longest_launch_ms": round(worst_ms, 2), "peak_device_bytes_over_inputs": peak,
           "output_bytes": p * k * 16}
    del probe, gallery
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from frhip import ops
    out = {"d": 512, "k": 10, "fp64_vector_peak_flops": FP64_VECTOR_PEAK_FLOPS,
           "fp64_peak_source": "AMD MI355X specification, FP64 vector 78.6 TFLOP/s; not measured", "search": {}}
    warm_e, warm_l = embeddings(2048, 512, 1)
    ops.cross_hist(warm_e, warm_l)
    ops.gallery_topk(warm_e, warm_e, 10)
    torch.cuda.synchronize()
    for p, g in SHAPES:
        out["search"]["%dx%d" % (p, g)] = search_row(p, g, 512, 10, a.reps)
    # the yardstick: cross_hist at N = 20 000 in the same process
    n = 20000
    e, lab = embeddings(n, 512, n)
    pairs = n * (n - 1) // 2
    sec = timed(lambda: ops.cross_hist(e, lab), a.reps)
    out["cross_hist_n20000"] = {"pairs": pairs, "kernel_s": round(sec, 4), "pairs_per_s": float("%.4g" % (pairs / sec))}
    del e, lab
    torch.cuda.empty_cache()
    rate = {key: row["pairs_per_s"] for key, row in out["search"].items()}
    out["rate_over_cross_hist"] = {key: round(v / out["cross_hist_n20000"]["pairs_per_s"], 3) for key, v in rate.items()}
    out["small_p_rate_over_large_p_rate"] = round(rate["128x1000000"] / max(rate["10000x100000"], rate["20000x20000"]), 3)
    # what does not scale with d, and the longest lists
    d32 = search_row(10_000, 100_000, 32, 10, a.reps)
    out["d32_10000x100000"] = {"kernel_s": d32["kernel_s"], "ns_per_pair": round(d32["kernel_s"] / d32["pairs"] * 1e9, 4)}
    out["d32_over_d512_10000x100000"] = round(d32["kernel_s"] / out["search"]["10000x100000"]["kernel_s"], 3)
    out["k64_20000x20000"] = search_row(20_000, 20_000, 512, 64, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
