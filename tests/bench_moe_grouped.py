"""Kernel benchmark: ops.moe_mlp above 32 tokens through the grouped GEMM
kernels against the torch composition (ops._moe_mlp_ref, the path such calls
took before the kernels existed) on the same inputs, in the same process.

    python tests/bench_moe_grouped.py [--out FILE] [--dim D --inter I]

D = 4096, I = 14336, E = 8, top-2, T in 64, 256, 1024, 4096, bf16 and e4m3
expert weights. Device events around `iters` back-to-back eager calls (the
composition's host syncs included: that is what a caller waits for), rotating
over enough weight copies that repeats miss the 256 MiB Infinity Cache; the
two paths alternate, five runs each; µs per call, median and min..max. TB/s
is the weight bytes of all E experts (every expert is picked at these T) and
TFLOP/s is 2 * T * k * 3 * D * I, both over the median time of the call, so
they include routing, alignment, combine and the launch gaps.
"""
import argparse
import json
import statistics
import sys

import torch

from kubetorch_amd import ops
from kubetorch_amd.models import quantize_weights_fp8
from kubetorch_amd.models.moe import FusedMoEMLP

from bench_linear_w8 import timed

ROTATE_BYTES = 320 << 20


def stats(v):
    return {"median": round(statistics.median(v), 1),
            "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ref-iters", type=int, default=4)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--inter", type=int, default=14336)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=2)
    ap.add_argument("--tokens", type=int, nargs="+",
                    default=[64, 256, 1024, 4096])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_grouped needs a GPU")
    dev = torch.device("cuda")
    D, I, E, k = args.dim, args.inter, args.experts, args.top_k
    rows = []
    for wt, wbytes in (("bf16", 2), ("e4m3", 1)):
        n = max(2, -(-ROTATE_BYTES // (3 * D * I * E * wbytes)))
        mods = []
        for c in range(n):
            torch.manual_seed(c)
            m = FusedMoEMLP(D, I, E, k, device=dev, dtype=torch.bfloat16)
            for p in m.parameters():
                p.data.normal_(0.0, 0.02)
            if wt == "e4m3":
                m = quantize_weights_fp8(torch.nn.Sequential(m),
                                         inplace=True)[0]
            mods.append(m)

        def call(fn, x):
            def run(m):
                sc = (m.w_gate_up_scale, m.w_down_scale) if m.is_fp8 \
                    else (None, None)
                return fn(x, m.router(x), m.w_gate_up, m.w_down, k, *sc)
            return run

        def grouped(x, lg, wgu, wd, k, sgu, sd):
            assert ops._moe_grouped_kernel_ok(x, lg, wgu, wd, k, sgu, sd)
            return ops.moe_mlp(x, lg, wgu, wd, k, w_gate_up_scale=sgu,
                               w_down_scale=sd)

        with torch.no_grad():
            for T in args.tokens:
                x = torch.randn(T, D, device=dev, dtype=torch.bfloat16)
                new, old = call(grouped, x), call(ops._moe_mlp_ref, x)
                diff = (new(mods[0]).float() - old(mods[0]).float()).abs()
                kern, comp = [], []
                for _ in range(5):
                    kern.append(timed(new, mods, args.iters))
                    comp.append(timed(old, mods, args.ref_iters))
                a, b = stats(kern), stats(comp)
                row = {"weights": wt, "D": D, "I": I, "E": E, "top_k": k,
                       "T": T, "grouped_us": a, "composition_us": b,
                       "speedup": round(b["median"] / a["median"], 2),
                       "weight_TBps": round(
                           E * 3 * D * I * wbytes / a["median"] / 1e6, 3),
                       "TFLOPs": round(
                           2 * T * k * 3 * D * I / a["median"] / 1e6, 1),
                       "max_abs_diff": diff.max().item()}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del mods
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"kernel": rows}, f, indent=1)


if __name__ == "__main__":
    main()
