"""Operand-layout microbench for the backward GEMMs of the Llama-3-8B step
(profiles/kcontig_backward.md). At T tokens, for every Linear class:

  wgrad  dW[out,in] = dY[T,out]^T @ X[T,in]
    a  dY.t() @ X               today: neither operand K(=T)-contiguous
    b  dY.t() @ (X^T).t()       X^T pre-transposed
    c  (dY^T) @ X               dY^T pre-transposed
    d  (dY^T) @ (X^T).t()       both
    each timed as the GEMM alone and with the ops.transpose_bf16 calls that
    produce its operands.
  dgrad  dX[T,in] = dY @ W      the model's layout (W is [out,in])
         dX = dY @ (W^T).t()    the FlatDDP shadow layout

and the two transpose kernels in isolation (GB/s = read + write bytes over
time) next to the fused AdamW kernel.

Run on the box: PYTHONPATH=. python tests/bench_gemm_layouts.py
"""
import argparse
import json

import torch

from kubetorch_amd import ops

# (name, in, out) of y[T,out] = x[T,in] @ W[out,in]^T
LAYERS = [
    ("qkv", 4096, 6144),
    ("wo", 4096, 4096),
    ("w13", 4096, 28672),
    ("w2", 14336, 4096),
    ("lm_head", 4096, 128256),
]
TRANSPOSE_SHAPES = [(16384, 4096), (16384, 28672), (28672, 4096),
                    (128256, 4096)]


def timed(fn, iters, warmup=3):
    """Mean milliseconds per call by device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_layer(name, T, in_f, out_f, iters):
    dev = "cuda"
    x = torch.randn(T, in_f, dtype=torch.bfloat16, device=dev)
    dy = torch.randn(T, out_f, dtype=torch.bfloat16, device=dev)
    w = torch.randn(out_f, in_f, dtype=torch.bfloat16, device=dev)
    xt = ops.transpose_bf16(x)
    dyt = ops.transpose_bf16(dy)
    wt = ops.transpose_bf16(w)
    tflop = 2.0 * T * in_f * out_f / 1e12
    row = {"layer": name, "T": T, "in": in_f, "out": out_f, "tflop": tflop}

    gemm = {
        "a": lambda: dy.t() @ x,
        "b": lambda: dy.t() @ xt.t(),
        "c": lambda: dyt @ x,
        "d": lambda: dyt @ xt.t(),
    }
    full = {
        "a": gemm["a"],
        "b": lambda: dy.t() @ ops.transpose_bf16(x).t(),
        "c": lambda: ops.transpose_bf16(dy) @ x,
        "d": lambda: ops.transpose_bf16(dy) @ ops.transpose_bf16(x).t(),
    }
    for v in "abcd":
        row[f"wgrad_{v}_gemm_ms"] = timed(gemm[v], iters)
        row[f"wgrad_{v}_total_ms"] = timed(full[v], iters)
    row["dgrad_model_ms"] = timed(lambda: dy @ w, iters)
    row["dgrad_shadow_ms"] = timed(lambda: dy @ wt.t(), iters)
    row["fwd_ms"] = timed(lambda: torch.nn.functional.linear(x, w), iters)
    best = min("abcd", key=lambda v: row[f"wgrad_{v}_total_ms"])
    row["wgrad_best_total"] = best
    print(json.dumps(row), flush=True)
    parts = " ".join(
        f"{v}={row[f'wgrad_{v}_gemm_ms']:.3f}/{row[f'wgrad_{v}_total_ms']:.3f}"
        for v in "abcd")
    print(f"# {name:8s} wgrad gemm/total ms: {parts} best={best} | dgrad "
          f"model={row['dgrad_model_ms']:.3f} shadow="
          f"{row['dgrad_shadow_ms']:.3f} | fwd={row['fwd_ms']:.3f} "
          f"({tflop / row['fwd_ms'] * 1e3:.0f} TF)", flush=True)
    return row


def bench_transposes(iters):
    dev = "cuda"
    for R, C in TRANSPOSE_SHAPES:
        src = torch.randn(R, C, dtype=torch.bfloat16, device=dev)
        dst = torch.empty(R * C, dtype=torch.bfloat16, device=dev)
        table, max_tiles = ops.transpose_table([(0, 0, R, C)], R * C, R * C,
                                               dev)
        flat = src.view(-1)
        gb = 2 * 2.0 * R * C / 1e9
        ms_one = timed(lambda: ops.transpose_bf16(src), iters)
        ms_seg = timed(lambda: ops.transpose_segments_bf16(
            flat, dst, table, max_tiles), iters)
        ms_torch = timed(lambda: src.t().contiguous(), iters)
        row = {"transpose": [R, C], "transpose_bf16_ms": ms_one,
               "transpose_bf16_gbps": gb / ms_one * 1e3,
               "transpose_segments_ms": ms_seg,
               "transpose_segments_gbps": gb / ms_seg * 1e3,
               "torch_t_contiguous_ms": ms_torch,
               "torch_t_contiguous_gbps": gb / ms_torch * 1e3}
        print(json.dumps(row), flush=True)
        del src, dst
    n = 128 * 1024 * 1024
    p = torch.randn(n, device=dev).bfloat16()
    g = torch.randn(n, device=dev).bfloat16()
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    ms = timed(lambda: ops.adamw_(p, g, m, v, 1e-4, 0.9, 0.95, 1e-8, 0.1, 1),
               iters)
    # p, m, v read and written, g read: 2+2 + 4+4 + 4+4 + 2 = 22 B/param
    print(json.dumps({"adamw_numel": n, "adamw_ms": ms,
                      "adamw_gbps": 22.0 * n / 1e9 / ms * 1e3}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layers", nargs="*", default=None)
    ap.add_argument("--skip-transposes", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemm_layouts needs a GPU")
    if not args.skip_transposes:
        bench_transposes(args.iters)
    for name, in_f, out_f in LAYERS:
        if args.layers and name not in args.layers:
            continue
        bench_layer(name, args.tokens, in_f, out_f, args.iters)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
