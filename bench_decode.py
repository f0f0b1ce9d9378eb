"""Serving benchmark: continuous-batching decode throughput (tokens/s).

Not the driver's headline bench (that is bench.py's training step) — this
measures the serving half: N concurrent requests through BatchedGenerator
on one GPU. Usage:

    python bench_decode.py --model llama3-8b --batch 8 --prompt 128 --new 128
    python bench_decode.py ... --kv paged [--page-size 16] [--num-splits 0]

--kv slot (default) is the padded slot cache; --kv paged the block-table
page pools with the fused decode-attention kernel. --num-splits 0 lets the
engine choose the split-KV factor.
"""
import argparse
import json
import sys
import time

import torch


def build_model(name, dev):
    from kubetorch_amd.models import Llama, llama3_8b, llama_tiny

    cfg = (llama3_8b() if name == "llama3-8b" else llama_tiny())
    torch.manual_seed(0)
    prev = torch.get_default_dtype()
    if dev.type == "cuda":
        torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            model = Llama(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    return model, cfg


def run_once(model, cfg, batch, prompt, new, kv="slot", page_size=16,
             num_splits=0):
    """One full engine run; returns the number of generated tokens."""
    from kubetorch_amd.models import BatchedGenerator

    kw = {}
    if kv != "slot":  # the slot run is the constructor's default call
        kw = dict(kv=kv, page_size=page_size, num_splits=num_splits or None)
    eng = BatchedGenerator(model, max_batch=batch, max_len=prompt + new + 8,
                           **kw)
    for i in range(batch):
        p = torch.randint(0, cfg.vocab_size, (prompt,))
        eng.submit(p.tolist(), max_new_tokens=new)
    out = eng.run()
    return sum(len(v) - prompt for v in out.values())


def timed_run(dev, *args, **kw):
    """(generated tokens, seconds) of one run_once, device-synchronised."""
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    new_toks = run_once(*args, **kw)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return new_toks, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b",
                    choices=["llama3-8b", "tiny"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kv", default="slot", choices=["slot", "paged"])
    ap.add_argument("--page-size", type=int, default=16)
    ap.add_argument("--num-splits", type=int, default=0,
                    help="paged split-KV factor; 0 = engine's choice")
    args = ap.parse_args()

    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model, cfg = build_model(args.model, dev)
    run = (model, cfg, args.batch, args.prompt, args.new)
    mode = dict(kv=args.kv, page_size=args.page_size,
                num_splits=args.num_splits)

    for _ in range(args.warmup):
        run_once(*run, **mode)
    new_toks, dt = timed_run(dev, *run, **mode)

    print(json.dumps({
        "metric": "decode_tokens_per_sec",
        "value": round(new_toks / dt, 2),
        "unit": "tokens/s",
        "batch": args.batch,
        "prompt_len": args.prompt,
        "new_tokens": args.new,
        "model": args.model,
        "device": dev.type,
        "kv": args.kv,
    }), flush=True)
    print(f"[decode] {new_toks} tokens in {dt:.2f}s", file=sys.stderr)


if __name__ == "__main__":
    main()
