"""Serving benchmark: continuous-batching decode throughput (tokens/s).

Not the driver's headline bench (that is bench.py's training step) — this
measures the serving half: N concurrent requests through BatchedGenerator
on one GPU. Usage:

    python bench_decode.py --model llama3-8b --batch 8 --prompt 128 --new 128
    python bench_decode.py ... --kv paged [--page-size 16] [--num-splits 0]
    python bench_decode.py ... --kv paged --prefill paged
    python bench_decode.py ... --kv paged --kv-dtype fp8
    python bench_decode.py ... --kv paged --prefix-cache --shared-prefix 2048
    python bench_decode.py ... --sampler fused --temperature 0.8 --top-k 50 \
        --top-p 0.9
    python bench_decode.py ... --sampler fused --logprobs 5
    python bench_decode.py ... --weight-dtype fp8

--kv slot (default) is the padded slot cache; --kv paged the block-table
page pools with the fused decode-attention kernel. --num-splits 0 lets the
engine choose the split-KV factor. --prefill paged prefills straight into
the pages with the paged prefill kernel; --prefix-cache shares prompt pages
between requests. --kv-dtype fp8 stores the pages as e4m3 bytes (unit
scales: random weights, nothing to calibrate on). --shared-prefix N makes the first N prompt tokens the
same for every request and every run; one engine then serves the warm-up
and the timed runs, so with --prefix-cache the timed run hits the pages the
warm-up left. ttft_ms is the wall time of the first step() (all prefills
plus one decode step), device-synchronised. --sampler fused picks each
step's tokens with ops.sample_tokens (one call and one host copy per step);
--top-k and --top-p need it. --temperature applies to either sampler.
--logprobs N (needs --sampler fused) makes every request record each token's
log-probability, rank and N alternatives (ops.token_logprobs after every
sampler call, one more host copy per step).
--weight-dtype fp8 quantises the model's linear weights in place after it is
built (models.quantize_weights_fp8: e4m3 bytes, the skinny-M decode kernel);
every other flag combines with it.
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


def make_engine(model, batch, prompt, new, kv="slot", page_size=16,
                num_splits=0, prefill="cache", prefix_cache=False,
                kv_dtype="bf16", sampler="torch", logprobs=None):
    from kubetorch_amd.models import BatchedGenerator

    kw = {}
    if kv != "slot":  # the slot run is the constructor's default call
        kw = dict(kv=kv, page_size=page_size, num_splits=num_splits or None)
    if prefill != "cache" or prefix_cache:
        kw.update(prefill=prefill, prefix_cache=prefix_cache)
    if kv_dtype == "fp8":
        kw.update(kv_dtype="fp8")
    if sampler != "torch":
        kw.update(sampler=sampler)
    if logprobs is not None:
        kw.update(logprobs=logprobs)
    return BatchedGenerator(model, max_batch=batch, max_len=prompt + new + 8,
                            **kw)


def run_once(dev, model, cfg, batch, prompt, new, eng=None, shared=None,
             sampling=None, **mode):
    """One full engine run: (generated tokens, seconds of the first step).
    `shared`: the prompt tokens every request starts with; `sampling`:
    submit()'s temperature / top_k / top_p, if any."""
    if eng is None:
        eng = make_engine(model, batch, prompt, new, **mode)
    shared = shared or []
    for i in range(batch):
        p = torch.randint(0, cfg.vocab_size, (prompt - len(shared),))
        eng.submit(shared + p.tolist(), max_new_tokens=new,
                   **(sampling or {}))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.step()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    ttft = time.perf_counter() - t0
    out = eng.run()
    eng.logprobs.clear()
    return sum(len(v) - prompt for v in out.values()), ttft


def timed_run(dev, *args, **kw):
    """(generated tokens, seconds, first-step seconds) of one run_once,
    device-synchronised."""
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    new_toks, ttft = run_once(dev, *args, **kw)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return new_toks, time.perf_counter() - t0, ttft


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
    ap.add_argument("--prefill", default="cache", choices=["cache", "paged"],
                    help="paged: prefill into the pages (needs --kv paged)")
    ap.add_argument("--prefix-cache", action="store_true",
                    help="share prompt pages between requests (--kv paged)")
    ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: e4m3 page pools (needs --kv paged)")
    ap.add_argument("--shared-prefix", type=int, default=0,
                    help="first N prompt tokens equal across requests and "
                         "runs; one engine serves all runs")
    ap.add_argument("--sampler", default="torch", choices=["torch", "fused"],
                    help="fused: one ops.sample_tokens call per step")
    ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: e4m3 weight-only linears (W8A16)")
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--top-k", type=int, default=0,
                    help="needs --sampler fused")
    ap.add_argument("--top-p", type=float, default=1.0,
                    help="needs --sampler fused")
    ap.add_argument("--logprobs", type=int, default=None,
                    help="record N alternatives per token (0..32); needs "
                         "--sampler fused")
    args = ap.parse_args()
    if args.sampler != "fused" and (args.top_k != 0 or args.top_p != 1.0):
        ap.error("--top-k and --top-p need --sampler fused")
    if args.logprobs is not None and (args.sampler != "fused"
                                      or not 0 <= args.logprobs <= 32):
        ap.error("--logprobs needs --sampler fused and a value in [0, 32]")
    if not 0 <= args.shared_prefix <= args.prompt:
        ap.error("--shared-prefix must be in [0, --prompt]")
    if args.kv_dtype == "fp8" and args.kv != "paged":
        ap.error("--kv-dtype fp8 needs --kv paged")

    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model, cfg = build_model(args.model, dev)
    if args.weight_dtype == "fp8":
        from kubetorch_amd.models import quantize_weights_fp8

        model = quantize_weights_fp8(model, inplace=True)
    run = (model, cfg, args.batch, args.prompt, args.new)
    mode = dict(kv=args.kv, page_size=args.page_size,
                num_splits=args.num_splits)
    if args.prefill != "cache" or args.prefix_cache:
        mode.update(prefill=args.prefill, prefix_cache=args.prefix_cache)
    if args.kv_dtype == "fp8":
        mode.update(kv_dtype="fp8")
    extra = {}
    if args.sampler != "torch":
        mode.update(sampler=args.sampler)
    if args.temperature != 0.0:
        extra["sampling"] = dict(temperature=args.temperature)
    if args.top_k != 0 or args.top_p != 1.0:
        extra.setdefault("sampling", {}).update(top_k=args.top_k,
                                                top_p=args.top_p)
    if args.logprobs is not None:
        mode.update(logprobs=args.logprobs)
        extra.setdefault("sampling", {}).update(logprobs=args.logprobs)
    eng = None
    if args.shared_prefix:
        gen = torch.Generator().manual_seed(1)
        extra["shared"] = torch.randint(
            0, cfg.vocab_size, (args.shared_prefix,), generator=gen).tolist()
        eng = extra["eng"] = make_engine(model, args.batch, args.prompt,
                                         args.new, **mode)

    for _ in range(args.warmup):
        run_once(dev, *run, **extra, **mode)
    hit0 = eng.prefix_stats["hit_tokens"] if eng is not None else 0
    new_toks, dt, ttft = timed_run(dev, *run, **extra, **mode)

    more = {}
    if args.prefill != "cache" or args.prefix_cache or args.shared_prefix:
        more = {"prefill": "paged" if args.prefix_cache else args.prefill,
                "prefix_cache": args.prefix_cache,
                "shared_prefix": args.shared_prefix}
        if eng is not None:
            more["hit_tokens"] = eng.prefix_stats["hit_tokens"] - hit0
    if args.kv_dtype == "fp8":
        more["kv_dtype"] = "fp8"
    if args.weight_dtype == "fp8":
        more["weight_dtype"] = "fp8"
    if args.sampler != "torch" or "sampling" in extra:
        more.update(sampler=args.sampler, temperature=args.temperature,
                    top_k=args.top_k, top_p=args.top_p)
    if args.logprobs is not None:
        more["logprobs"] = args.logprobs
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
        "ttft_ms": round(ttft * 1e3, 3),
        **more,
    }), flush=True)
    print(f"[decode] {new_toks} tokens in {dt:.2f}s", file=sys.stderr)


if __name__ == "__main__":
    main()
