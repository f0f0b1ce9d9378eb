"""Kernel benchmark: ops.linear_w8 (fp8 weights, gfx950 skinny-M kernel)
against F.linear on bf16 weights, at the five Llama-3-8B weight shapes.

    python tests/bench_linear_w8.py [--out FILE] [--sweep]

Device events around `iters` back-to-back eager calls, rotating over enough
weight copies that repeats miss the 256 MiB Infinity Cache; the two modes
alternate, three runs each; µs per call with launch gaps (and, for fp8, the
split-K reduce launch) included. TB/s is weight bytes (N*K for fp8, 2*N*K
for bf16) over the mean time. --sweep adds num_splits 1..16 at M = 8.

--engine measures bench_decode.py's engine instead: one Llama-3-8B build and
a quantised copy of it in one process, --kv paged with the
captured decode graph; per configuration one untimed warm-up run of each
model, then bf16 and fp8 weights alternated, three timed runs each.
"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

from kubetorch_amd import ops

SHAPES = [("wqkv", 6144, 4096), ("wo", 4096, 4096),
          ("w_gate_up", 28672, 4096), ("w_down", 4096, 14336),
          ("lm_head", 128256, 4096)]
MS = (1, 8, 32)
ROTATE_BYTES = 320 << 20


def timed(fn, copies, iters):
    for i in range(min(len(copies), 4) + 2):  # warm up
        fn(copies[i % len(copies)])
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(copies[i % len(copies)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters  # µs


def stats(v):
    return {"mean": round(sum(v) / len(v), 2),
            "spread": round(max(v) - min(v), 2),
            "runs": [round(x, 2) for x in v]}


ENGINE_CONFIGS = [(8, 128, 128), (32, 128, 128), (8, 4096, 128)]


def engine(model_name, out):
    import bench_decode as bd
    from kubetorch_amd.models import quantize_weights_fp8

    dev = torch.device("cuda")
    model, cfg = bd.build_model(model_name, dev)
    models = {"bf16": model, "fp8": quantize_weights_fp8(model)}
    rows = []
    for batch, prompt, new in ENGINE_CONFIGS:
        if prompt + new + 8 > cfg.max_seq_len:
            continue
        res = {k: {"tok_s": [], "ttft_ms": []} for k in models}
        for timed_pass in (False, True, True, True):
            for k, m in models.items():
                toks, dt, ttft = bd.timed_run(dev, m, cfg, batch, prompt, new,
                                              kv="paged")
                if timed_pass:
                    res[k]["tok_s"].append(toks / dt)
                    res[k]["ttft_ms"].append(ttft * 1e3)
        row = {"batch": batch, "prompt": prompt, "new": new, "kv": "paged",
               "model": model_name}
        for k in models:
            row[k] = {n: stats(v) for n, v in res[k].items()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump({"engine": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--model", default="llama3-8b",
                    choices=["llama3-8b", "tiny"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_linear_w8 needs a GPU")
    if args.engine:
        return engine(args.model, args.out)
    dev = torch.device("cuda")
    rows = []
    for name, N, K in SHAPES:
        n = max(2, -(-ROTATE_BYTES // (N * K)))
        torch.manual_seed(0)
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02
        q, s = ops.quantize_weight_fp8(w)
        wq = ops.dequantize_weight_fp8(q, s)
        fp8 = [(q.clone(), s) for _ in range(n)]
        bf16 = [wq.clone() for _ in range(max(2, n // 2))]
        del w
        plan = ops.linear_w8_splits(N, K)
        for M in MS:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            assert ops._linear_w8_kernel_ok(x, q, s)
            err = (ops.linear_w8(x, q, s).float()
                   - F.linear(x, wq).float()).abs().max().item()
            r8, r16 = [], []
            for _ in range(3):
                r8.append(timed(lambda c: ops.linear_w8(x, c[0], c[1]),
                                fp8, args.iters))
                r16.append(timed(lambda c: F.linear(x, c), bf16, args.iters))
            a, b = stats(r8), stats(r16)
            row = {"shape": name, "N": N, "K": K, "M": M, "tile_n": 128,
                   "splits": plan, "fp8_us": a, "bf16_us": b,
                   "fp8_TBps": round(N * K / a["mean"] / 1e6, 3),
                   "bf16_TBps": round(2 * N * K / b["mean"] / 1e6, 3),
                   "fp8_over_bf16": round(a["mean"] / b["mean"], 3),
                   "max_abs_diff": err}
            if args.sweep and M == 8:
                row["sweep_us"] = {
                    str(S): round(timed(
                        lambda c: ops.linear_w8(x, c[0], c[1], num_splits=S),
                        fp8, args.iters), 2)
                    for S in (1, 2, 3, 4, 6, 8, 12, 16) if S <= K // 128}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del fp8, bf16, q, wq
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"kernel": rows}, f, indent=1)


if __name__ == "__main__":
    main()
