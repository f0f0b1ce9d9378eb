"""Kernel benchmark: the 64-row-tile fp8-weight kernel behind ops.linear_w8
(with its split-K reduce) against the composition such calls ran before it,
F.linear(x, dequantize_weight_fp8(q, scale)), at the five Llama-3-8B weight
shapes and M = 64 .. 4096. The table sets ops.W8_WIDE_MAX_ROWS.

    python tests/bench_linear_w8_wide.py [--out FILE] [--sweep]

Timing as in bench_linear_w8.py: device events around `iters` back-to-back
eager calls, rotating over enough weight copies that repeats miss the 256 MiB
Infinity Cache; the two paths alternate, three runs each; µs per call, launch
gaps, the reduce launch and the composition's temporary included. The kernel
is called through the extension, so rows above the current cap are measured
too. "wins" is true where the composition's median exceeds the kernel's by
more than the two ranges together. --sweep adds one timing per num_splits.
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

from bench_linear_w8 import ROTATE_BYTES, SHAPES, timed
from kubetorch_amd import ops

MS = (64, 128, 256, 512, 1024, 2048, 4096)


def stats(v):
    return {"median": round(statistics.median(v), 1),
            "range": round(max(v) - min(v), 1),
            "runs": [round(t, 1) for t in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_linear_w8_wide needs a GPU")
    dev = torch.device("cuda")
    wide = ops._ext().linear_w8_wide
    rows = []
    for name, N, K in SHAPES:
        torch.manual_seed(0)
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02
        q, s = ops.quantize_weight_fp8(w)
        del w
        copies = [(q.clone(), s)
                  for _ in range(max(2, -(-ROTATE_BYTES // (N * K))))]
        plan = ops.linear_w8_splits(N, K)
        for M in MS:
            iters = 30 if M <= 512 else 10
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)

            def kern(c, S=0):
                return wide(x, c[0], c[1], S)

            def comp(c):
                return F.linear(x, ops.dequantize_weight_fp8(c[0], c[1]))
            err = (kern(copies[0]).float()
                   - comp(copies[0]).float()).abs().max().item()
            rk, rc = [], []
            for _ in range(3):
                rk.append(timed(kern, copies, iters))
                rc.append(timed(comp, copies, iters))
            a, b = stats(rk), stats(rc)
            row = {"shape": name, "N": N, "K": K, "M": M, "splits": plan,
                   "kernel_us": a, "composition_us": b,
                   "kernel_over_composition": round(
                       a["median"] / b["median"], 3),
                   "wins": b["median"] - a["median"]
                   > a["range"] + b["range"],
                   "max_abs_diff": err}
            if args.sweep:
                row["sweep_us"] = {
                    str(S): round(timed(lambda c: kern(c, S), copies, iters),
                                  1)
                    for S in (1, 2, 4, 8)
                    if S <= K // 128 and S * M * N * 4 <= 2 << 30}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del copies, q
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"kernel": rows}, f, indent=1)


if __name__ == "__main__":
    main()
