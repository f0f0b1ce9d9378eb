"""Kernel benchmark: FusedMoEMLP with FP8 expert weights (the W8A16 routed
GEMMs) against FusedMoEMLP holding the same represented weights in bf16.

    python tests/bench_moe_w8.py [--out FILE] [--dim D --inter I]

D = 4096, I = 14336, E = 8, top-2, T in 1, 8, 32. Device events around
`iters` back-to-back eager calls, rotating over enough weight copies that
repeats miss the 256 MiB Infinity Cache; the two modes alternate, three runs
each; µs per call with launch gaps included. TB/s is the weight bytes of the
experts that were actually picked (3 D I per expert for fp8, 6 D I for bf16)
over the mean time.
"""
import argparse
import json
import sys

import torch

from kubetorch_amd import ops
from kubetorch_amd.models import dequantize_weights, quantize_weights_fp8
from kubetorch_amd.models.moe import FusedMoEMLP

from bench_linear_w8 import stats, timed

ROTATE_BYTES = 320 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--inter", type=int, default=14336)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_w8 needs a GPU")
    dev = torch.device("cuda")
    D, I, E, k = args.dim, args.inter, args.experts, args.top_k
    n = max(2, -(-ROTATE_BYTES // (3 * D * I * E)))
    pairs = []  # (fp8 module, bf16 module with the represented weights)
    for c in range(n):
        torch.manual_seed(c)
        q = FusedMoEMLP(D, I, E, k, device=dev, dtype=torch.bfloat16)
        for p in q.parameters():
            p.data.normal_(0.0, 0.02)
        q = quantize_weights_fp8(torch.nn.Sequential(q), inplace=True)
        pairs.append((q[0], dequantize_weights(q)[0]))
    rows = []
    with torch.no_grad():
        for T in (1, 8, 32):
            x = torch.randn(T, 1, D, device=dev, dtype=torch.bfloat16)
            q0, b0 = pairs[0]
            assert ops._moe_kernel_ok(x, q0.router(x), q0.w_gate_up, q0.w_down,
                                      k, q0.w_gate_up_scale, q0.w_down_scale)
            assert ops._moe_kernel_ok(x, b0.router(x), b0.w_gate_up, b0.w_down,
                                      k)
            err = (q0(x).float() - b0(x).float()).abs().max().item()
            picked = sum(int(ops.moe_route(q.router(x), k)[0].unique().numel())
                         for q, _ in pairs) / n
            fp8, bf16 = [], []
            for _ in range(3):
                fp8.append(timed(lambda c: c[0](x), pairs, args.iters))
                bf16.append(timed(lambda c: c[1](x), pairs, args.iters))
            a, b = stats(fp8), stats(bf16)
            row = {"D": D, "I": I, "E": E, "top_k": k, "T": T,
                   "splits": ops.moe_down_splits(D, I, E, k),
                   "experts_picked": round(picked, 2),
                   "fp8_us": a, "bf16_us": b,
                   "fp8_TBps": round(picked * 3 * D * I / a["mean"] / 1e6, 3),
                   "bf16_TBps": round(picked * 6 * D * I / b["mean"] / 1e6, 3),
                   "fp8_over_bf16": round(a["mean"] / b["mean"], 3),
                   "max_abs_diff": err}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"kernel": rows}, f, indent=1)


if __name__ == "__main__":
    main()
