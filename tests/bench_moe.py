"""Kernel benchmark: ops.moe_mlp (routing, the two routed GEMMs and the
combine: four launches) against MoEMLP._dispatch_local (the per-expert Python
loop with its host syncs) on the same weights.

    python tests/bench_moe.py [--out FILE] [--dim D --inter I]

D = 4096, I = 14336, E = 8, top-2, T in 1, 8, 32. Device events around
`iters` back-to-back eager calls, rotating over enough weight copies that
repeats miss the 256 MiB Infinity Cache; the two modes alternate, three runs
each; µs per call with launch gaps and the loop's syncs included. TB/s is the
weight bytes of the experts that were actually picked (6 D I per expert)
over the mean time.
"""
import argparse
import json
import sys

import torch

from kubetorch_amd import ops
from kubetorch_amd.models.moe import FusedMoEMLP, MoEMLP

from bench_linear_w8 import stats, timed

ROTATE_BYTES = 320 << 20


class _Cfg:
    def __init__(self, dim, intermediate):
        self.dim, self.intermediate = dim, intermediate


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
        sys.exit("bench_moe needs a GPU")
    dev = torch.device("cuda")
    D, I, E, k = args.dim, args.inter, args.experts, args.top_k
    n = max(2, -(-ROTATE_BYTES // (6 * D * I * E)))
    pairs = []
    for c in range(n):
        torch.manual_seed(c)
        with torch.device(dev):
            moe = MoEMLP(_Cfg(D, I), n_experts=E, top_k=k).to(torch.bfloat16)
        for p in moe.parameters():
            p.data.normal_(0.0, 0.02)
        pairs.append((moe, FusedMoEMLP.from_moe(moe)))
    rows = []
    with torch.no_grad():
        for T in (1, 8, 32):
            x = torch.randn(T, 1, D, device=dev, dtype=torch.bfloat16)
            m0, f0 = pairs[0]
            assert ops._moe_kernel_ok(x, f0.router(x), f0.w_gate_up, f0.w_down,
                                      k)
            err = (f0(x).float() - m0(x).float()).abs().max().item()
            picked = sum(int(ops.moe_route(f.router(x), k)[0].unique().numel())
                         for _, f in pairs) / n
            fused, loop = [], []
            for _ in range(3):
                fused.append(timed(lambda c: c[1](x), pairs, args.iters))
                loop.append(timed(lambda c: c[0](x), pairs, args.iters))
            a, b = stats(fused), stats(loop)
            nbytes = picked * 6 * D * I
            row = {"D": D, "I": I, "E": E, "top_k": k, "T": T,
                   "splits": ops.moe_down_splits(D, I, E, k),
                   "experts_picked": round(picked, 2),
                   "fused_us": a, "loop_us": b,
                   "fused_TBps": round(nbytes / a["mean"] / 1e6, 3),
                   "loop_TBps": round(nbytes / b["mean"] / 1e6, 3),
                   "fused_over_loop": round(a["mean"] / b["mean"], 3),
                   "max_abs_diff": err}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"kernel": rows}, f, indent=1)


if __name__ == "__main__":
    main()
