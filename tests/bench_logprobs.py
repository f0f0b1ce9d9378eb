"""Stage benchmark: ops.token_logprobs (gfx950 kernel) against the torch
composition it replaces, on bf16 [8 | 32, 128256] logits with top_n 0 / 5 /
20.

    python tests/bench_logprobs.py [--out FILE] [--iters 50]

The composition is what a caller would write: log_softmax(logits.float() /
T) over the whole row, a gather for the token, a comparison and a sum for
its rank, topk for the alternatives. "kernel" is `iters` back-to-back calls
between device events, no host copy; "call" is wall clock per call including
the copy of the outputs to the host (the kernel's four packed into one
tensor, as the engine does; the composition's likewise). The two modes
alternate, three runs each; µs per call.

--engine measures bench_decode.py's engine instead: one Llama-3-8B build in
one process, --kv paged with the captured decode graph, sampler="fused"
without logprobs and with logprobs 0 and 5 (every request asking),
alternated, one untimed warm-up run of each and three timed runs each, at
batch 8 and 32.
"""
import argparse
import json
import sys
import time

import torch

from kubetorch_amd import ops

V = 128256
BATCHES = (8, 32)
TOP_NS = (0, 5, 20)


def composition(logits, token, T, top_n):
    B = logits.shape[0]
    lp = torch.log_softmax(logits.float() / T.view(B, 1), -1)
    tok = token.view(B, 1)
    rank = (logits > logits.gather(1, tok)).sum(1) + 1
    out = [lp.gather(1, tok).view(B), rank.to(torch.int32)]
    if top_n:
        top = lp.topk(top_n, dim=1)
        out += [top.indices.to(torch.int32), top.values]
    return out


def packed(outs):
    B = outs[0].shape[0]
    return torch.cat([t.double().view(B, -1) for t in outs], dim=1)


def device_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def wall_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) * 1e6 / iters


def stats(v):
    return {"mean": round(sum(v) / len(v), 2),
            "spread": round(max(v) - min(v), 2),
            "runs": [round(x, 2) for x in v]}


ENGINE_CONFIGS = [(8, 128, 128), (32, 128, 128)]


def engine(model_name, out):
    import bench_decode as bd

    dev = torch.device("cuda")
    model, cfg = bd.build_model(model_name, dev)
    modes = {"fused": None, "logprobs0": 0, "logprobs5": 5}
    rows = []
    for batch, prompt, new in ENGINE_CONFIGS:
        res = {k: {"tok_s": [], "ttft_ms": []} for k in modes}
        for timed_pass in (False, True, True, True):
            for k, n in modes.items():
                kw = dict(kv="paged", sampler="fused",
                          sampling=dict(temperature=0.8))
                if n is not None:
                    kw.update(logprobs=n)
                    kw["sampling"].update(logprobs=n)
                toks, dt, ttft = bd.timed_run(dev, model, cfg, batch, prompt,
                                              new, **kw)
                if timed_pass:
                    res[k]["tok_s"].append(toks / dt)
                    res[k]["ttft_ms"].append(ttft * 1e3)
        row = {"batch": batch, "prompt": prompt, "new": new, "kv": "paged",
               "model": model_name, "temperature": 0.8}
        for k in modes:
            row[k] = {n: stats(v) for n, v in res[k].items()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump({"engine": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--model", default="llama3-8b",
                    choices=["llama3-8b", "tiny"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_logprobs needs a GPU")
    if args.engine:
        return engine(args.model, args.out)
    dev = torch.device("cuda")
    rows = []
    for B in BATCHES:
        gen = torch.Generator().manual_seed(B)
        logits = (torch.randn(B, V, generator=gen) * 3).to(torch.bfloat16) \
            .to(dev)
        assert ops._sampler_kernel_ok(logits)
        token = torch.randint(0, V, (B,), generator=gen).to(dev)
        T = torch.full((B,), 0.8, device=dev)
        for n in TOP_NS:
            def kern():
                return ops.token_logprobs(logits, token, T, n)

            def comp():
                return composition(logits, token, T, n)

            got, want = kern(), comp()
            err = (got[0] - want[0]).abs().max().item()
            assert got[1].tolist() == want[1].tolist()
            res = {k: [] for k in ("kernel", "torch", "kernel_call",
                                   "torch_call")}
            for _ in range(3):
                res["kernel"].append(device_us(kern, args.iters))
                res["torch"].append(device_us(comp, args.iters))
                res["kernel_call"].append(wall_us(
                    lambda: packed(kern()).tolist(), args.iters))
                res["torch_call"].append(wall_us(
                    lambda: packed(comp()).tolist(), args.iters))
            row = {"batch": B, "V": V, "top_n": n,
                   **{k + "_us": stats(v) for k, v in res.items()},
                   "max_abs_diff_logprob": err}
            row["torch_over_kernel"] = round(
                row["torch_us"]["mean"] / row["kernel_us"]["mean"], 2)
            row["torch_over_kernel_call"] = round(
                row["torch_call_us"]["mean"] / row["kernel_call_us"]["mean"],
                2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"stage": rows}, f, indent=1)


if __name__ == "__main__":
    main()
