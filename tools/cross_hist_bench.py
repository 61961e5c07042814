#!/usr/bin/env python3
"""Cross-matching test cost: the histogram route (frhip_cross_hist, utils.eval.cross_histograms + cross_accuracy) at N = 20 000,
50 000 and 100 000, d = 512, random unit embeddings with repeated identities; at N = 20 000 also the pair-list route (cross_score +
performance_acc).  Reports kernel time, pairs/s, fp64 rate, the longest single launch, peak device memory of each route, and a d = 32
run at N = 50 000 whose time per pair is the part that does not scale with d (epilogue, the four 64-bit histogram atomics).

fp64 accounting: each pair-k is one v_cvt_f64_f32 and one v_fma_f64 (2 FLOP).  Peak used: 78.6 TFLOP/s FP64 vector, AMD's
published MI355X specification (not measured here); 39.3 T fp64 FMA/s.

Usage:  python tools/cross_hist_bench.py [--reps 3]      prints one JSON line"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "face-recognition-pytorch_amd"))

import torch  # noqa: E402

FP64_VECTOR_PEAK_FLOPS = 78.6e12      # AMD MI355X specification sheet, FP64 vector; not measured


def embeddings(n, d, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ids = max(1, n // 20)
    centres = torch.randn((ids, d), device="cuda", generator=gen)
    lab = torch.randint(0, ids, (n,), device="cuda", generator=gen)
    e = torch.nn.functional.normalize(centres[lab] * 0.6 + torch.randn((n, d), device="cuda", generator=gen))
    return e.contiguous(), lab.contiguous()


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def longest_launch(e, lab):
    """ms of the slowest single band launch of the default split"""
    from frhip import ops
    from frhip._abi import check, lib
    n, d = e.shape
    hs = [torch.zeros((100002,), dtype=torch.int64, device="cuda") for _ in range(4)]
    b = ops.cross_hist_bands(n)
    worst = 0.0
    for i0, i1 in zip(b, b[1:]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib().frhip_cross_hist(e.data_ptr(), lab.data_ptr(), n, d, i0, i1, *[h.data_ptr() for h in hs], ops._s()), "cross_hist")
        e1.record()
        e1.synchronize()
        worst = max(worst, e0.elapsed_time(e1))
    return worst, len(b) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from frhip import ops
    from utils import eval as ev
    out = {"d": 512, "fp64_vector_peak_flops": FP64_VECTOR_PEAK_FLOPS,
           "fp64_peak_source": "AMD MI355X specification, FP64 vector 78.6 TFLOP/s; not measured", "hist": {}}
    warm_e, warm_l = embeddings(2048, 512, 1)
    ops.cross_hist(warm_e, warm_l)
    torch.cuda.synchronize()
    for n in (20000, 50000, 100000):
        e, lab = embeddings(n, 512, n)
        pairs = n * (n - 1) // 2
        sec = timed(lambda: ops.cross_hist(e, lab), a.reps)
        worst_ms, bands = longest_launch(e, lab)

        def route():
            ev._CROSS_CACHE.clear()
            hg, hi = ev.cross_histograms(e, lab)
            _, th = ev.performance_roc(hg, hi)
            ev.cross_accuracy(e, lab, th)
        route_sec = timed(route, 1)
        ev._CROSS_CACHE.clear()
        peak = peak_of(lambda: ops.cross_hist(e, lab))
        out["hist"][str(n)] = {"pairs": pairs, "kernel_s": round(sec, 4), "pairs_per_s": float("%.4g" % (pairs / sec)),
                               "fp64_flops": float("%.4g" % (2 * pairs * 512 / sec)),
                               "fp64_fraction_of_peak": round(2 * pairs * 512 / sec / FP64_VECTOR_PEAK_FLOPS, 4),
                               "bands": bands, "longest_launch_ms": round(worst_ms, 2), "route_with_roc_and_acc_s": round(route_sec, 3),
                               "peak_device_bytes_over_inputs": peak}
        del e, lab
        torch.cuda.empty_cache()
    # the part of the per-pair cost that does not scale with d
    n = 50000
    e, lab = embeddings(n, 32, 7)
    pairs = n * (n - 1) // 2
    sec32 = timed(lambda: ops.cross_hist(e, lab), a.reps)
    out["d32_n50000"] = {"kernel_s": round(sec32, 4), "ns_per_pair": round(sec32 / pairs * 1e9, 4)}
    out["d32_over_d512_n50000"] = round(sec32 / out["hist"]["50000"]["kernel_s"], 3)     # near 1: the k loop is not the bound
    del e, lab
    torch.cuda.empty_cache()
    # the pair-list route at N = 20 000
    n = 20000
    e, lab = embeddings(n, 512, n)
    list_kernel = timed(lambda: ops.cross_score(e, lab), a.reps)
    list_peak = peak_of(lambda: ops.cross_score(e, lab))

    def list_route():
        hg, hi, scores, plab = ev.cross_score(e, lab)
        _, th = ev.performance_roc(hg, hi)
        ev.performance_acc(scores, plab, th)
    out["list_n20000"] = {"kernel_s": round(list_kernel, 4), "route_with_roc_and_acc_s": round(timed(list_route, 1), 3),
                          "peak_device_bytes_over_inputs": list_peak}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
