"""Dense CRF (ops.dense_crf: method "exact", csrc/dense_crf.hip, and "permutohedral", csrc/dense_crf_permutohedral.hip): one JSON
line per method and case.  Cases: 224^2 and 448^2; K = 27, and 27 + 27 (the
linear and the cluster CRF of one frame in one shared pass); B = 1 and 8.  Fields: ms per mean-field iteration (the difference of a
T = 10 and a T = 1 call over 9, per frame), ms per frame at T = 10 (everything: normaliser pass, unary, ten updates), and pixel
pairs per second of the update passes against the exp-issue bound (one v_exp_f32 per pair at 8 cycles per wave: 256 CUs x 4 SIMDs
x 64 lanes / 8 cycles x 2.4 GHz = 1.97e13 / s; exact method only).  With several methods, every case runs under each of them in
turn, and the lattice lines carry the exact method's T = 10 time of the same case and the ratio.

    python scripts/bench_dense_crf.py [--cases 224x1:27,448x8:27+27] [--iters N] [--method exact,permutohedral]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd import ops  # noqa: E402

EXP_BOUND = 256 * 4 * 64 / 8 * 2.4e9


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def run_case(dev, size, B, ks, iters, method="exact"):
    gen = torch.Generator().manual_seed(0)
    # piecewise-constant colour with noise (the kernel is exact: the time does not depend on the content)
    base = torch.randint(0, 256, (8, 3), generator=gen)
    ids = torch.randint(0, 8, (B, size // 32 + 1, size // 32 + 1), generator=gen).repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :size, :size]
    img = (base[ids] + torch.randint(-4, 5, (B, size, size, 3), generator=gen)).clamp(0, 255).to(torch.uint8).to(dev)
    logits = [torch.randn(B, k, size, size, generator=gen).to(dev) for k in ks]
    arg = tuple(logits) if len(logits) == 2 else logits[0]
    t10 = timed(lambda: ops.dense_crf(arg, img, iterations=10, method=method), iters)
    t1 = timed(lambda: ops.dense_crf(arg, img, iterations=1, method=method), iters)
    it_ms = (t10 - t1) / 9 / B
    out = {"method": method, "frame": f"{size}x{size}", "batch": B, "K": "+".join(str(k) for k in ks), "ms_per_iteration": round(it_ms, 4),
           "ms_per_frame_T10": round(t10 / B, 3)}
    if method == "exact":
        rate = float(size * size) ** 2 / (it_ms * 1e-3)
        out.update({"pixel_pairs_per_s": f"{rate:.3e}", "exp_issue_bound_per_s": f"{EXP_BOUND:.3e}", "fraction_of_exp_bound": round(rate / EXP_BOUND, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="224x1:27,224x8:27,224x1:27+27,224x8:27+27,448x1:27,448x8:27,448x1:27+27,448x8:27+27")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--method", default="exact", help="comma-separated: exact, permutohedral")
    a = ap.parse_args()
    methods = a.method.split(",")
    if any(m not in ("exact", "permutohedral") for m in methods):
        ap.error(f"--method: exact and / or permutohedral, not {a.method!r}")
    dev = torch.device("cuda:0")
    exact_ms = {}
    for m in methods:
        for c in a.cases.split(","):
            geo, ks = c.split(":")
            size, B = (int(v) for v in geo.split("x"))
            r = run_case(dev, size, B, [int(k) for k in ks.split("+")], a.iters, m)
            if m == "exact":
                exact_ms[c] = r["ms_per_frame_T10"]
            elif c in exact_ms:
                r["exact_ms_per_frame_T10"] = exact_ms[c]
                r["fraction_of_exact"] = round(r["ms_per_frame_T10"] / exact_ms[c], 4)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
